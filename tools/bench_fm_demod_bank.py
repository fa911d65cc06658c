#!/usr/bin/env python3
"""bench_fm_demod_bank.py -- an FM demodulation bank (cordic_demodbank_run)
against what a caller did before it, one cordic_fm_demod call per block, and
against ONE cordic_fm_demod call over the same samples.

For bench.py's two r2p workloads (cfg3, natr2p24; parameters from its workload
table, tools/bench_common.py) and, for the record, one core of the one-by-one
path (r2p35: WW 35), in ONE process: 1024 blocks x 2^16 samples of random
24-bit I/Q, back to back in four arrays, each block with a d_last word:

  (a) bank       one cordic_demodbank_run over all blocks
  (b) per block  one cordic_fm_demod call per block, on the same arrays and
                 d_last words (the C entry point through ctypes with the
                 arguments converted beforehand)
  (c) one call   ONE cordic_fm_demod call of 2^26 samples on the same arrays

All three read 8 and write 8 B per sample.  Before any timing the outputs and
d_last words of (a) are checked on every sample against those of (b).  Timing:
HIP events around `steps` runs of a leg (10 for (a) and (c), 1 pass over the
blocks for (b)), the legs alternated within every repetition, one warm-up
repetition, then --reps (>= 5) timed ones; min - max over the repetitions.

The one gate: on the fused cores the bank's slowest repetition must be faster
than the per-block loop's fastest.  The ratio to one long call is recorded.

  python tools/bench_fm_demod_bank.py --out profiles/r13/fm_demod_bank.txt
"""
import argparse
import os
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
R2P35 = ("r2p", 27, 27, 2, 32, 20)      # tests/test_jobset_fused.py: WW 35


def measure(name, cli, desc, blocks, length, reps, bufs):
    import bench_common as B
    import torch
    import cordic_amd as ca

    cfg = ca.Config.from_cli(B.MODE[cli[0]], *cli[1:])
    x, y, mag, freq, lasts, work = bufs
    n = blocks * length
    view = lambda t, k: t[k * length:(k + 1) * length]
    jobs = [(view(x, k), view(y, k), view(mag, k), view(freq, k), length, 0,
             lasts[k:]) for k in range(blocks)]
    bank = ca.DemodBank(cfg, jobs)
    info = bank.info()
    st = torch.cuda.current_stream().cuda_stream
    fn = ca.lib().cordic_fm_demod
    calls = [(cfg.ref, length, j[0].data_ptr(), j[1].data_ptr(), 0, j[6].data_ptr(),
              j[2].data_ptr(), j[3].data_ptr(), work.data_ptr(), st) for j in jobs]

    def loop():
        for a in calls:
            if fn(*a):
                raise SystemExit("%s: cordic_fm_demod failed" % name)

    def long_call():
        ca.fm_demod(cfg, x, y, mag, freq, work, n=n, last=lasts)

    # ---- the outputs first
    lasts.zero_(); mag.fill_(-1); freq.fill_(-1)
    loop()
    torch.cuda.synchronize()
    mref, fref, lref = mag.clone(), freq.clone(), lasts.clone()
    lasts.zero_(); mag.fill_(-1); freq.fill_(-1)
    bank.run()
    torch.cuda.synchronize()
    if not (torch.equal(mag, mref) and torch.equal(freq, fref)
            and torch.equal(lasts, lref)):
        raise SystemExit("%s: the bank differs from one call per block" % name)
    del mref, fref, lref

    legs = [("bank", 10, bank.run), ("per block", 1, loop), ("one call", 10, long_call)]
    rates = {k: [] for k, _, _ in legs}
    for rep in range(reps + 1):         # rep 0: warm-up of every leg
        for k, steps, run in legs:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                run()
            e1.record()
            e1.synchronize()
            if rep:
                rates[k].append(n * steps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    bank.close()
    path = ("fused: %d tiles of %d samples, %d tail jobs, two launches"
            % (info["tiles"], info["tile"], info["tail_jobs"])) if info["fused"] \
        else "one by one"
    lines = ["%s  %s  [%s]" % (name, desc, path)]
    stat = {}
    for k, _, _ in legs:
        v = sorted(rates[k])
        stat[k] = (v[0], v[-1])
        lines.append("    %-9s  min %7.1f  max %7.1f Gsample/s" % (k, v[0], v[-1]))
    b, p, o = stat["bank"], stat["per block"], stat["one call"]
    lines.append("    bank / per block = %.1fx .. %.1fx; bank / one call = %.2f .. %.2f"
                 % (b[0] / p[1], b[1] / p[0], b[0] / o[1], b[1] / o[0]))
    ok = True
    if info["fused"]:
        ok = b[0] > p[1]
        lines.append("    gate: the bank's slowest repetition %.1f is %s the per-block "
                     "loop's fastest %.1f" % (b[0], "above" if ok else "** NOT above **",
                                              p[1]))
    return lines, ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--log2-block", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if not 1 <= a.blocks <= 65536 or not 2 <= a.log2_block <= 24 \
            or a.blocks << a.log2_block > 1 << 28:
        ap.error("--blocks 1 .. 65536, --log2-block 2 .. 24, at most 2^28 samples")
    sys.path.insert(0, TOOLS)
    import bench_common as B
    import torch
    import cordic_amd as ca
    import build_stamp

    length = 1 << a.log2_block
    n = a.blocks * length
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    x = torch.randint(-(1 << 23), 1 << 23, (n,), dtype=torch.int32, device=dev,
                      generator=gen)
    y = torch.randint(-(1 << 23), 1 << 23, (n,), dtype=torch.int32, device=dev,
                      generator=gen)
    bufs = [x, y] + [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
    bufs.append(torch.zeros(a.blocks, dtype=torch.int32, device=dev))
    bufs.append(torch.zeros(max(16, ca.fm_demod_workspace(n)), dtype=torch.uint8,
                            device=dev))
    st = build_stamp.stamp()
    lines = ["%s, commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
        torch.cuda.get_device_name(0), st["git_head"],
        " + uncommitted changes" if st["git_dirty"] else "",
        st["kernel_sources_sha256"], st["lib_sha256"]),
        "%d blocks x 2^%d samples, random 24-bit I/Q, a d_last word per block; HIP "
        "events around 10 bank runs / one pass of per-block calls / 10 long calls, "
        "legs alternated, min - max of %d repetitions after one warm-up of every leg; "
        "one process; the bank checked against the per-block calls on every sample "
        "first" % (a.blocks, a.log2_block, a.reps)]
    print("\n".join(lines), flush=True)
    cores = [(k, B.WORKLOADS[k]["cli"], B.WORKLOADS[k]["desc"])
             for k in ("cfg3", "natr2p24")]
    cores.append(("r2p35", R2P35, "topolar 20-stage, 27-bit ports, WW 35 (the "
                  "left-justified wide kernel): one by one, for the record"))
    ok = True
    for name, cli, desc in cores:
        part, good = measure(name, cli, desc, a.blocks, length, a.reps, bufs)
        print("\n".join(part), flush=True)
        lines += part
        ok = ok and good
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
