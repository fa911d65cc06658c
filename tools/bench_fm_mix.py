#!/usr/bin/env python3
"""bench_fm_mix.py -- the FM mixer (cordic_plan_fm_mix) against what a caller
did before it: cordic_phase_accumulate into a phase array, then cordic_plan_p2r
on that array; and, for scale, against the constant-tone mixer.

For the `ddc` workload's core (cfg2), a 20-stage core (n20) and nat24
(parameters from bench.py's workload table, tools/bench_common.py) and, for the
record, one core of the fallback (ww38: WW 38), in ONE process, on 2^28 samples
of random tuning words and random full-scale I/Q:

  (a) fm_mix      the call under test (fcw read twice, x, y read, two outputs
                  written: 24 B per sample; the fallback 32)
  (b) acc+p2r     cordic_phase_accumulate (4 B read twice, 4 B written), then
                  cordic_plan_p2r (12 B read, 8 B written): 32 B per sample
  (c) mix         cordic_plan_mix with one tuning word for the call: the
                  constant-tone ceiling (8 B read, 8 B written)

Before any timing the outputs of (a) are checked on every sample against (b).
Timing: HIP events around 10 calls, the legs alternated within every
repetition, one warm-up repetition, then --reps (>= 5) timed ones; min / median
/ max over the repetitions.  cordic_plan_fm_mix_info says which path (a) took.

  python tools/bench_fm_mix.py --out profiles/r12/fm_mix.txt
"""
import argparse
import os
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
STEPS = 10
N20 = ("p2r", 32, 32, 2, 32, 20)
WW38 = ("p2r", 32, 32, 5, 32, 24)       # tests/test_jobset_fused.py: WW 38


def measure(name, cli, desc, n, reps, bufs, gen):
    import bench_common as B
    import torch
    import cordic_amd as ca

    cfg = ca.Config.from_cli(B.MODE[cli[0]], *cli[1:])
    plan = ca.Plan(cfg)
    fused, tile = plan.fm_mix_info()
    fcw, x, y, ox, oy, ph, rx, ry = bufs
    half = 1 << (cfg.iw - 1)
    for t in (x, y):                    # full scale of this core's ports
        torch.randint(-half, half, (n,), dtype=torch.int32, device=t.device,
                      generator=gen, out=t)
    work = torch.zeros(max(16, plan.fm_mix_workspace(n)), dtype=torch.uint8,
                       device=x.device)
    awork = torch.zeros(ca.fm_workspace(n), dtype=torch.uint8, device=x.device)
    phase0 = 0x9e3779b1

    def pair():
        ca.phase_accumulate(fcw, ph, phase0=phase0, work=awork)
        plan.p2r(x, y, ph, rx, ry)

    # ---- the outputs first
    pair()
    ox.fill_(-1); oy.fill_(-1)
    plan.fm_mix(fcw, x, y, ox, oy, work, phase0=phase0)
    if not torch.equal(ox, rx) or not torch.equal(oy, ry):
        raise SystemExit("%s: fm_mix differs from phase_accumulate + plan p2r" % name)
    torch.cuda.synchronize()

    ba = 24 if fused else 32
    legs = [("fm_mix", ba, lambda: plan.fm_mix(fcw, x, y, ox, oy, work, phase0=phase0)),
            ("acc+p2r", 32, pair),
            ("mix", 16, lambda: plan.mix(phase0, 0x01234567, 0, x, y, rx, ry))]
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
    lines = ["%s  %s  [%s]" % (name, desc, ("fused kernel, %d samples per pass" % tile)
                               if fused else "fallback")]
    stat = {}
    for k, b, _ in legs:
        v = sorted(rates[k])
        med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
        stat[k] = (v[0], med, v[-1])
        lines.append("    %-8s %2d B/sample  min %7.1f  median %7.1f  max %7.1f "
                     "Gsample/s  (%5.2f TB/s)" % (k, b, v[0], med, v[-1], med * b / 1e3))
    f, p, m = stat["fm_mix"], stat["acc+p2r"], stat["mix"]
    lines.append("    fm_mix / (acc+p2r) = %.2fx (medians; the bytes allow %d/%d = "
                 "%.2fx); slowest fm_mix repetition %s fastest acc+p2r repetition"
                 % (f[1] / p[1], 32, ba, 32 / ba, ">" if f[0] > p[2] else "<="))
    lines.append("    fm_mix / mix = %.2f (medians; the bytes allow 16/%d = %.2f)"
                 % (f[1] / m[1], ba, 16 / ba))
    plan.close()
    return lines, bool(fused), f[0] > p[2]


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
    import build_stamp

    n = 1 << a.log2_samples
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    fcw = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device=dev,
                        generator=gen)
    bufs = [fcw] + [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(7)]
    st = build_stamp.stamp()
    lines = ["%s, commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
        torch.cuda.get_device_name(0), st["git_head"],
        " + uncommitted changes" if st["git_dirty"] else "",
        st["kernel_sources_sha256"], st["lib_sha256"]),
        "2^%d samples, random tuning words, random full-scale I/Q; HIP events "
        "around %d calls, legs alternated, %d repetitions after one warm-up of "
        "every leg; one process; fm_mix checked against phase_accumulate + plan "
        "p2r on every sample first" % (a.log2_samples, STEPS, a.reps)]
    print("\n".join(lines), flush=True)
    table = {
        "cfg2": (B.WORKLOADS["cfg2"]["cli"], "basiccordic 16-stage, 32-bit: the "
                 "core of the `ddc` workload"),
        "n20": (N20, "basiccordic 20-stage, 32-bit"),
        "nat24": (B.WORKLOADS["nat24"]["cli"], "gencordic -t p2r -i 24 -o 24: WW27 "
                  "PW31, 27 stages"),
        "ww38": (WW38, "basiccordic 24-stage, 32-bit, 5 extra bits: WW 38, the "
                 "fallback, for the record"),
    }
    lost = []
    for name, (cli, desc) in table.items():
        part, fused, won = measure(name, cli, desc, n, a.reps, bufs, gen)
        print("\n".join(part), flush=True)
        lines += part
        if fused and not won:
            lost.append(name)
    lines.append("acceptance (every fused core: slowest fm_mix repetition above the "
                 "fastest acc+p2r repetition): %s"
                 % ("met" if not lost else "** NOT met on %s **" % ", ".join(lost)))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
