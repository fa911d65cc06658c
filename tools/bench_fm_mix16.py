#!/usr/bin/env python3
"""bench_fm_mix16.py -- the FM mixer and its banks on int16 I/Q arrays
(cordic_plan_fm_mix16, cordic_mixbank_create16) against the 32-bit forms on
widened copies of the same data: what a caller with samples in shorts did
before them, less the widening and narrowing passes themselves.

For cfg1's core (p2r 16 16 2 16 16, 13 live stages), nat16 (19 live stages) and a
16-stage 16-bit core with PW 32 (p2r 16 16 2 32 16; only if
cordic_plan_fm_mix_info says it is fused), each in a child process of its own
under its own time limit, on 2^28 samples of random tuning words and random
full-scale 16-bit I/Q:

  (a) fm_mix16     one cordic_plan_fm_mix16 call: fcw read twice, x, y read and
                   two outputs written as shorts, 16 B per sample
  (b) fm_mix       one cordic_plan_fm_mix call on the widened copies, 24 B
  (c) bank16       cordic_mixbank_run on a 16-bit bank of 1024 blocks x 2^16
                   samples, a d_acc word per block
  (d) bank         the 32-bit bank on the widened copies of those blocks
  (e) per block    one cordic_plan_fm_mix16 call per block (the C entry point
                   through ctypes with the arguments converted beforehand)

Before any timing the outputs of (a) are checked on every sample against those
of (b), and the outputs and d_acc words of (c) against those of (d) and of (e).
Timing: HIP events around `steps` runs of a leg (10; 1 pass over the blocks for
(e)), every window behind one untimed run of the same leg; (a) .. (d) alternated
within every repetition, one warm-up repetition, then --reps (>= 5, 7 by default)
timed ones; then (e) in repetitions of its own; min - max over the repetitions.
(e) is kept out of the alternation because it is a launch-bound loop that leaves
the device nearly idle, and the windows are some ten milliseconds long: with (e)
among the others, the leg timed behind it read a tenth low on pw32 (185 - 189
Gsample/s for (a) where every order without (e) in front of it gives 204 - 214),
one untimed run in between notwithstanding.

Requirement: the 16-bit forms move fewer bytes through the same arithmetic, so
(a) >= 0.97 x (b) and (c) >= 0.97 x (d), best repetition against best
repetition (3 % is the run-to-run spread of the FM rows within one process).
The byte counts are read off the code, not profiled; the report states rates
and ratios and no memory-bandwidth fraction.

  python tools/bench_fm_mix16.py --out profiles/r17/fm_mix16.txt
"""
import argparse
import os
import subprocess
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
STEPS = 10
CORES = {
    "cfg1": (("p2r", 16, 16, 2, 16, 16), "basiccordic 16-bit: WW19 PW16, 13 live "
             "stages"),
    "nat16": (("p2r", 16, 16, 2, -1, -1), "gencordic -t p2r -i 16 -o 16: WW19 PW23, "
              "19 stages"),
    "pw32": (("p2r", 16, 16, 2, 32, 16), "basiccordic 16-bit ports, PW 32, 16 "
             "stages"),
}
BOUND = 0.97


def measure(name, log2_samples, blocks, log2_block, reps):
    """the child: one core, the report lines on stdout"""
    sys.path.insert(0, TOOLS)
    import bench_common as B
    import torch
    import cordic_amd as ca

    cli, desc = CORES[name]
    cfg = ca.Config.from_cli(B.MODE[cli[0]], *cli[1:])
    plan = ca.Plan(cfg)
    fused, tile = plan.fm_mix_info()
    if not fused:
        print("%s  %s  [not fused (cordic_plan_fm_mix_info): not measured]"
              % (name, desc))
        plan.close()
        return 0
    n, length = 1 << log2_samples, 1 << log2_block
    nb = blocks * length
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    fcw = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device=dev,
                        generator=gen)
    x16 = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int16, device=dev,
                        generator=gen)
    y16 = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int16, device=dev,
                        generator=gen)
    x32, y32 = x16.to(torch.int32), y16.to(torch.int32)
    ox16, oy16 = torch.empty_like(x16), torch.empty_like(x16)
    ox32, oy32 = torch.empty_like(x32), torch.empty_like(x32)
    acc16 = torch.zeros(blocks, dtype=torch.int32, device=dev)
    acc32 = torch.zeros(blocks, dtype=torch.int32, device=dev)
    work16 = torch.zeros(max(16, plan.fm_mix16_workspace(n)), dtype=torch.uint8,
                         device=dev)
    work32 = torch.zeros(max(16, plan.fm_mix_workspace(n)), dtype=torch.uint8,
                         device=dev)
    phase0 = 0x9e3779b1
    view = lambda t, k: t[k * length:(k + 1) * length]

    def jobs(x, y, ox, oy, accs):
        return [(view(fcw, k), None, view(x, k), view(y, k), view(ox, k), view(oy, k),
                 length, 0, accs[k:]) for k in range(blocks)]

    j16 = jobs(x16, y16, ox16, oy16, acc16)
    bank16 = ca.MixBank16(plan, j16)
    bank32 = ca.MixBank(plan, jobs(x32, y32, ox32, oy32, acc32))
    i16, i32 = bank16.info(), bank32.info()
    st = torch.cuda.current_stream().cuda_stream
    fn = ca.lib().cordic_plan_fm_mix16
    calls = [(plan._h, length, j[0].data_ptr(), None, 0, j[8].data_ptr(),
              j[2].data_ptr(), j[3].data_ptr(), j[4].data_ptr(), j[5].data_ptr(),
              work16.data_ptr(), st) for j in j16]

    def call16():
        plan.fm_mix16(fcw, x16, y16, ox16, oy16, work16, phase0=phase0)

    def call32():
        plan.fm_mix(fcw, x32, y32, ox32, oy32, work32, phase0=phase0)

    def loop():
        for a in calls:
            if fn(*a):
                raise SystemExit("%s: cordic_plan_fm_mix16 failed" % name)

    def same(a16, a32):
        return torch.equal(a16.to(torch.int32), a32)

    # ---- the outputs first
    for t in (ox16, oy16, ox32, oy32):
        t.fill_(-1)
    call16()
    call32()
    torch.cuda.synchronize()
    if not (same(ox16, ox32) and same(oy16, oy32)):
        raise SystemExit("%s: fm_mix16 differs from fm_mix on widened copies" % name)
    for t in (ox16, oy16, ox32, oy32):
        t.fill_(-1)
    bank16.run()
    bank32.run()
    torch.cuda.synchronize()
    if not (same(ox16[:nb], ox32[:nb]) and same(oy16[:nb], oy32[:nb])
            and torch.equal(acc16, acc32)):
        raise SystemExit("%s: the 16-bit bank differs from the 32-bit bank" % name)
    xref, yref, aref = ox16[:nb].clone(), oy16[:nb].clone(), acc16.clone()
    acc16.zero_(); ox16.fill_(-1); oy16.fill_(-1)
    loop()
    torch.cuda.synchronize()
    if not (torch.equal(ox16[:nb], xref) and torch.equal(oy16[:nb], yref)
            and torch.equal(acc16, aref)):
        raise SystemExit("%s: the 16-bit bank differs from one call per block" % name)
    del xref, yref, aref

    legs = [("fm_mix16", n, STEPS, call16), ("fm_mix", n, STEPS, call32),
            ("bank16", nb, STEPS, bank16.run), ("bank", nb, STEPS, bank32.run),
            ("per block", nb, 1, loop)]
    rates = {k: [] for k, _, _, _ in legs}
    # (a) .. (d) alternated, then (e) on its own (see the head of this file)
    rounds = [legs[:4]] * (reps + 1) + [legs[4:]] * (reps + 1)
    for at, group in enumerate(rounds):
        rep = at % (reps + 1)           # rep 0: warm-up of every leg
        for k, count, steps, run in group:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            run()                       # untimed: the window starts behind its own leg
            e0.record()
            for _ in range(steps):
                run()
            e1.record()
            e1.synchronize()
            if rep:
                rates[k].append(count * steps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    bank16.close()
    bank32.close()
    plan.close()
    print("%s  %s  [%s; fused, %d samples per pass; banks: %d / %d spans of %d / %d "
          "samples]" % (name, desc, torch.cuda.get_device_name(0), tile, i16["spans"],
                        i32["spans"], i16["tile"], i32["tile"]))
    notes = {"fm_mix16": "(a) 16 B/sample, 2^%d" % log2_samples,
             "fm_mix": "(b) 24 B/sample, widened copies",
             "bank16": "(c) 16 B/sample, %d x 2^%d" % (blocks, log2_block),
             "bank": "(d) 24 B/sample, widened copies",
             "per block": "(e) %d cordic_plan_fm_mix16 calls" % blocks}
    best = {}
    for k, _, _, _ in legs:
        v = sorted(rates[k])
        best[k] = v[-1]
        print("    %-9s  min %7.1f  max %7.1f Gsample/s   %s"
              % (k, v[0], v[-1], notes[k]))
    ra, rc = best["fm_mix16"] / best["fm_mix"], best["bank16"] / best["bank"]
    print("    (a) / (b) = %.3f, (c) / (d) = %.3f, best of %d against best of %d "
          "(required: >= %.2f each): %s; (c) / (e) = %.1fx"
          % (ra, rc, reps, reps, BOUND,
             "met" if ra >= BOUND and rc >= BOUND else "** NOT met **",
             best["bank16"] / best["per block"]))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--log2-samples", type=int, default=28)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--log2-block", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240,
                    help="seconds a core's child process may take")
    ap.add_argument("--core", default=None, choices=sorted(CORES),
                    help="(the child: measure this core and print its lines)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if not 10 <= a.log2_samples <= 28:
        ap.error("--log2-samples: 10 .. 28")
    if not 1 <= a.blocks <= 65536 or not 2 <= a.log2_block <= 24 \
            or a.blocks << a.log2_block > 1 << a.log2_samples:
        ap.error("--blocks 1 .. 65536, --log2-block 2 .. 24, the blocks within the "
                 "samples")
    if a.core:
        return measure(a.core, a.log2_samples, a.blocks, a.log2_block, a.reps)
    sys.path.insert(0, TOOLS)
    import build_stamp

    st = build_stamp.stamp()
    lines = ["commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
                 st["git_head"], " + uncommitted changes" if st["git_dirty"] else "",
                 st["kernel_sources_sha256"], st["lib_sha256"]),
             "2^%d samples and %d blocks x 2^%d of them, random tuning words, random "
             "full-scale 16-bit I/Q, the 32-bit legs on widened copies; HIP events "
             "around %d runs of a leg (one pass of per-block calls) behind one untimed "
             "run of it, legs (a) .. (d) alternated, (e) behind them on its own, min - max of %d repetitions after one warm-up of every leg; one process "
             "per core; outputs compared on every sample first.  Bytes per sample are "
             "read off the code, not profiled."
             % (a.log2_samples, a.blocks, a.log2_block, STEPS, a.reps)]
    print("\n".join(lines), flush=True)
    failed = []
    for name in ("cfg1", "nat16", "pw32"):
        cmd = [sys.executable, os.path.abspath(__file__), "--core", name,
               "--log2-samples", str(a.log2_samples), "--blocks", str(a.blocks),
               "--log2-block", str(a.log2_block), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            part = r.stdout.rstrip("\n").split("\n") if r.stdout.strip() else []
            if r.returncode:
                part.append("%s: the child ended with status %d: %s"
                            % (name, r.returncode, r.stderr.strip()[-400:]))
                failed.append(name)
        except subprocess.TimeoutExpired:
            part = ["%s: the child ran into its time limit of %d s" % (name, a.timeout)]
            failed.append(name)
        print("\n".join(part), flush=True)
        lines += part
        if failed:          # nothing more on the device after a failure
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
