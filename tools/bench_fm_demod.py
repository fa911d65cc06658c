#!/usr/bin/env python3
"""bench_fm_demod.py -- FM demodulation (cordic_fm_demod) against the converter
alone and against what a caller did before it: cordic_r2p into a phase array,
then a difference of that array.

For bench.py's two r2p workloads (cfg3, natr2p24; parameters from its workload
table, tools/bench_common.py) and, for the record, one core of the fallback
(r2p35: WW 35), in ONE process, on 2^28 samples of random 24-bit I/Q:

  (a) fm_demod   the call under test (read 8, write 8 B per sample)
  (b) r2p        cordic_r2p alone on the same arrays (read 8, write 8 B)
  (c) r2p+diff   cordic_r2p, then torch.sub(ph[1:], ph[:-1]) into a third array
                 (8 + 8, then 8 + 4 B; every core here has PW 32, so the
                 32-bit subtraction wraps where the difference has to)

Before any timing the outputs of (a) are checked on every sample against (c)
(with the phase in front of sample 0 equal to 0, freq[0] = ph[0]).  Timing: HIP
events around 10 calls, the legs alternated within every repetition, one
warm-up repetition, then --reps (>= 5) timed ones; min / median / max over the
repetitions.  cordic_fm_demod_info says which path (a) took.

  python tools/bench_fm_demod.py --out profiles/r11/fm_demod.txt
"""
import argparse
import os
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
STEPS = 10
R2P35 = ("r2p", 27, 27, 2, 32, 20)      # tests/test_jobset_fused.py: WW 35


def measure(name, cli, desc, n, reps, bufs):
    import bench_common as B
    import torch
    import cordic_amd as ca

    cfg = ca.Config.from_cli(B.MODE[cli[0]], *cli[1:])
    if cfg.pw != 32:
        raise SystemExit("%s: PW %d: leg (c) needs a sign extension" % (name, cfg.pw))
    fused, tile = ca.fm_demod_info(cfg)
    x, y, mag, freq, ph, ref, work = bufs

    # ---- the outputs first
    ca.r2p(cfg, x, y, mag, ph)
    ref[0] = ph[0]
    torch.sub(ph[1:], ph[:-1], out=ref[1:])
    mref = mag.clone()
    mag.fill_(-1); freq.fill_(-1)
    ca.fm_demod(cfg, x, y, mag, freq, work)
    if not torch.equal(freq, ref) or not torch.equal(mag, mref):
        raise SystemExit("%s: fm_demod differs from r2p + difference" % name)
    del mref
    torch.cuda.synchronize()

    def pair():
        ca.r2p(cfg, x, y, mag, ph)
        torch.sub(ph[1:], ph[:-1], out=ref[1:])

    legs = [("fm_demod", 16, lambda: ca.fm_demod(cfg, x, y, mag, freq, work)),
            ("r2p", 16, lambda: ca.r2p(cfg, x, y, mag, ph)),
            ("r2p+diff", 28, pair)]
    rates = {k: [] for k, _, _ in legs}
    for rep in range(reps + 1):         # rep 0: warm-up of every leg
        for k, _, run in legs:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(STEPS):
                run()
            e1.record()
            e1.synchronize()
            if rep:
                rates[k].append(n * STEPS / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    lines = ["%s  %s  [%s]" % (name, desc, ("fused kernel, tile %d samples" % tile)
                               if fused else "fallback")]
    stat = {}
    for k, b, _ in legs:
        v = sorted(rates[k])
        med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
        stat[k] = (v[0], med, v[-1])
        lines.append("    %-9s %2d B/sample  min %7.1f  median %7.1f  max %7.1f "
                     "Gsample/s  (%5.2f TB/s)" % (k, b, v[0], med, v[-1], med * b / 1e3))
    f, r, p = stat["fm_demod"], stat["r2p"], stat["r2p+diff"]
    ratio = "    fm_demod / r2p = %.3f (minima), %.3f (medians)" % (f[0] / r[0],
                                                                    f[1] / r[1])
    if fused:       # (the fallback's rates are for the record: no floor)
        spread = max(f[2] - f[0], r[2] - r[0])
        floor = 0.95 * r[0] - spread
        ratio += ("; 0.95 x r2p's minimum less the larger min-max spread = %.1f: "
                  "fm_demod's minimum %.1f is %s"
                  % (floor, f[0], "above it" if f[0] >= floor else "** BELOW it **"))
    lines.append(ratio)
    lines.append("    fm_demod / (r2p+diff) = %.2fx (medians; the bytes allow "
                 "28/16 = 1.75x); slowest fm_demod repetition %s fastest r2p+diff "
                 "repetition" % (f[1] / p[1], ">" if f[0] > p[2] else "<="))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--log2-samples", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if not 10 <= a.log2_samples <= 28:
        ap.error("--log2-samples: 10 .. 28")
    sys.path.insert(0, TOOLS)
    import bench_common as B
    import torch
    import cordic_amd as ca
    import build_stamp

    n = 1 << a.log2_samples
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    x = torch.randint(-(1 << 23), 1 << 23, (n,), dtype=torch.int32, device=dev,
                      generator=gen)
    y = torch.randint(-(1 << 23), 1 << 23, (n,), dtype=torch.int32, device=dev,
                      generator=gen)
    bufs = [x, y] + [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
    bufs.append(torch.zeros(max(16, ca.fm_demod_workspace(n)), dtype=torch.uint8,
                            device=dev))
    st = build_stamp.stamp()
    lines = ["%s, commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
        torch.cuda.get_device_name(0), st["git_head"],
        " + uncommitted changes" if st["git_dirty"] else "",
        st["kernel_sources_sha256"], st["lib_sha256"]),
        "2^%d samples, random 24-bit I/Q; HIP events around %d calls, legs "
        "alternated, %d repetitions after one warm-up of every leg; one process; "
        "fm_demod checked against r2p + difference on every sample first"
        % (a.log2_samples, STEPS, a.reps)]
    print("\n".join(lines), flush=True)
    cores = [(k, B.WORKLOADS[k]["cli"], B.WORKLOADS[k]["desc"])
             for k in ("cfg3", "natr2p24")]
    cores.append(("r2p35", R2P35, "topolar 20-stage, 27-bit ports, WW 35 (the "
                  "left-justified wide kernel): the fallback, for the record"))
    for name, cli, desc in cores:
        part = measure(name, cli, desc, n, a.reps, bufs)
        print("\n".join(part), flush=True)
        lines += part
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
