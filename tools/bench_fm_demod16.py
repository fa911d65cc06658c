#!/usr/bin/env python3
"""bench_fm_demod16.py -- FM demodulation and its banks on int16 I/Q arrays
(cordic_fm_demod16 on its fused kernel, cordic_demodbank_create16) against the
path the 16-bit call took before it had one, and against the 32-bit forms on
widened copies of the same data: what a caller with samples in shorts did
before them, less the widening and narrowing passes themselves.

For io16 (r2p 16 16 2 16 -1: WW 24, 13 live stages) and ww34 (r2p 16 16 7 16
-1: the widest fused core with 16-bit ports), each in a child process of its
own under its own time limit, on 2^28 samples of random full-scale 16-bit I/Q:

  (a) fm_demod16   one cordic_fm_demod16 call: the fused kernel, 8 B per sample
                   in two launches
  (b) no_lj        the same call with CORDIC_FLAG_NO_LJ on the configuration:
                   the fallback -- the unrolled converter on shorts, fmd_save,
                   fmd_diff, about 12 B per sample in three launches.
                   launch_topolar ignores the flag for 16-bit arrays, so this
                   is, launch for launch, what cordic_fm_demod16 ran before the
                   fused kernel took shorts: the earlier path in the same
                   process and build
  (c) fm_demod     one cordic_fm_demod call on the widened copies, 16 B
  (d) bank16       cordic_demodbank_run on a 16-bit bank of 1024 blocks x 2^16
                   samples, a d_last word per block
  (e) bank         the 32-bit bank on the widened copies of those blocks
  (f) per block    one cordic_fm_demod16 call per block (the C entry point
                   through ctypes with the arguments converted beforehand)

Every call has a d_last word.  Before any timing the outputs and the word of
(a) are checked on every sample against those of (b) and (c), and the outputs
and words of (d) against those of (e) and of (f).
Timing: HIP events around `steps` runs of a leg (10; 1 pass over the blocks for
(f)), every window behind one untimed run of the same leg; (a) .. (e) alternated
within every repetition, one warm-up repetition, then --reps (>= 5, 7 by default)
timed ones; then (f) in repetitions of its own, because it is a launch-bound
loop that leaves the device nearly idle and the leg timed behind it reads low
(profiles/r17/fm_mix16_leg_order.txt); min - max over the repetitions.

Requirement: (a) >= 0.97 x (b), (a) >= 0.97 x (c) and (d) >= 0.97 x (e), best
repetition against best repetition (3 % is the run-to-run spread of the FM rows
within one process).  (d) / (f) and (d) / (a) are reported without a bound.
The byte counts are read off the code, not profiled; the report states rates
and ratios and no memory-bandwidth fraction.

  python tools/bench_fm_demod16.py --out profiles/r18/fm_demod16.txt
"""
import argparse
import os
import subprocess
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
STEPS = 10
CORES = {
    "io16": (("r2p", 16, 16, 2, 16, -1), "gencordic -t r2p -i 16 -o 16 -p 16: WW24, "
             "13 live stages"),
    "ww34": (("r2p", 16, 16, 7, 16, -1), "the same with 7 extra bits: WW34, stage 1 "
             "on 64 bits"),
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
    slow = cfg.with_flags(ca.FLAG_NO_LJ)
    fused, tile = ca.fm_demod16_info(cfg)
    if not fused or ca.fm_demod16_info(slow)[0]:
        raise SystemExit("%s: cordic_fm_demod16_info does not name the paths" % name)
    n, length = 1 << log2_samples, 1 << log2_block
    nb = blocks * length
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    x16 = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int16, device=dev,
                        generator=gen)
    y16 = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int16, device=dev,
                        generator=gen)
    x32, y32 = x16.to(torch.int32), y16.to(torch.int32)
    m16, f16 = torch.empty_like(x16), torch.empty_like(x16)
    m32, f32 = torch.empty_like(x32), torch.empty_like(x32)
    # one word per call on a 16-byte slot: [0] (a), [4] (b), [8] (c)
    words = torch.zeros(12, dtype=torch.int32, device=dev)
    last16 = torch.zeros(blocks, dtype=torch.int32, device=dev)
    last32 = torch.zeros(blocks, dtype=torch.int32, device=dev)
    work = torch.zeros(max(16, ca.fm_demod_workspace(n)), dtype=torch.uint8, device=dev)
    phase0 = 0x9e3779b1
    view = lambda t, k: t[k * length:(k + 1) * length]

    def jobs(x, y, m, f, lasts):
        return [(view(x, k), view(y, k), view(m, k), view(f, k), length, 0, lasts[k:])
                for k in range(blocks)]

    j16 = jobs(x16, y16, m16, f16, last16)
    bank16 = ca.DemodBank16(cfg, j16)
    bank32 = ca.DemodBank(cfg, jobs(x32, y32, m32, f32, last32))
    i16, i32 = bank16.info(), bank32.info()
    if not (i16["fused"] and i32["fused"]):
        raise SystemExit("%s: a bank is not fused" % name)
    st = torch.cuda.current_stream().cuda_stream
    fn = ca.lib().cordic_fm_demod16
    calls = [(cfg.ref, length, j[0].data_ptr(), j[1].data_ptr(), 0, j[6].data_ptr(),
              j[2].data_ptr(), j[3].data_ptr(), work.data_ptr(), st) for j in j16]

    def call16():
        ca.fm_demod(cfg, x16, y16, m16, f16, work, phase0=phase0, last=words)

    def call_no_lj():
        ca.fm_demod(slow, x16, y16, m16, f16, work, phase0=phase0, last=words[4:])

    def call32():
        ca.fm_demod(cfg, x32, y32, m32, f32, work, phase0=phase0, last=words[8:])

    def loop():
        for a in calls:
            if fn(*a):
                raise SystemExit("%s: cordic_fm_demod16 failed" % name)

    def same(a16, a32):
        return torch.equal(a16.to(torch.int32), a32)

    # ---- the outputs first
    for t in (m16, f16, m32, f32):
        t.fill_(-1)
    call16()
    call32()
    torch.cuda.synchronize()
    if not (same(m16, m32) and same(f16, f32) and words[0].item() == words[8].item()):
        raise SystemExit("%s: fm_demod16 differs from fm_demod on widened copies" % name)
    mref, fref = m16.clone(), f16.clone()
    m16.fill_(-1); f16.fill_(-1)
    call_no_lj()
    torch.cuda.synchronize()
    if not (torch.equal(m16, mref) and torch.equal(f16, fref)
            and words[0].item() == words[4].item()):
        raise SystemExit("%s: fm_demod16 differs from its fallback" % name)
    del mref, fref
    for t in (m16, f16, m32, f32):
        t.fill_(-1)
    bank16.run()
    bank32.run()
    torch.cuda.synchronize()
    if not (same(m16[:nb], m32[:nb]) and same(f16[:nb], f32[:nb])
            and torch.equal(last16, last32)):
        raise SystemExit("%s: the 16-bit bank differs from the 32-bit bank" % name)
    mref, fref, lref = m16[:nb].clone(), f16[:nb].clone(), last16.clone()
    last16.zero_(); m16.fill_(-1); f16.fill_(-1)
    loop()
    torch.cuda.synchronize()
    if not (torch.equal(m16[:nb], mref) and torch.equal(f16[:nb], fref)
            and torch.equal(last16, lref)):
        raise SystemExit("%s: the 16-bit bank differs from one call per block" % name)
    del mref, fref, lref

    legs = [("fm_demod16", n, STEPS, call16), ("no_lj", n, STEPS, call_no_lj),
            ("fm_demod", n, STEPS, call32), ("bank16", nb, STEPS, bank16.run),
            ("bank", nb, STEPS, bank32.run), ("per block", nb, 1, loop)]
    rates = {k: [] for k, _, _, _ in legs}
    # (a) .. (e) alternated, then (f) on its own (see the head of this file)
    rounds = [legs[:5]] * (reps + 1) + [legs[5:]] * (reps + 1)
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
    print("%s  %s  [%s; fused, tiles of %d samples; banks: %d / %d tiles of %d / %d "
          "samples, %d / %d tails]"
          % (name, desc, torch.cuda.get_device_name(0), tile, i16["tiles"], i32["tiles"],
             i16["tile"], i32["tile"], i16["tail_jobs"], i32["tail_jobs"]))
    notes = {"fm_demod16": "(a) 8 B/sample, 2 launches, 2^%d" % log2_samples,
             "no_lj": "(b) CORDIC_FLAG_NO_LJ: ~12 B/sample, 3 launches",
             "fm_demod": "(c) 16 B/sample, widened copies",
             "bank16": "(d) 8 B/sample, %d x 2^%d" % (blocks, log2_block),
             "bank": "(e) 16 B/sample, widened copies",
             "per block": "(f) %d cordic_fm_demod16 calls" % blocks}
    best = {}
    for k, _, _, _ in legs:
        v = sorted(rates[k])
        best[k] = v[-1]
        print("    %-10s  min %7.1f  max %7.1f Gsample/s   %s"
              % (k, v[0], v[-1], notes[k]))
    rb = best["fm_demod16"] / best["no_lj"]
    rc = best["fm_demod16"] / best["fm_demod"]
    re_ = best["bank16"] / best["bank"]
    print("    (a) / (b) = %.3f, (a) / (c) = %.3f, (d) / (e) = %.3f, best of %d against "
          "best of %d (required: >= %.2f each): %s; (d) / (f) = %.1fx, (d) / (a) = %.3f"
          % (rb, rc, re_, reps, reps, BOUND,
             "met" if min(rb, rc, re_) >= BOUND else "** NOT met **",
             best["bank16"] / best["per block"], best["bank16"] / best["fm_demod16"]))
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
             "2^%d samples and %d blocks x 2^%d of them, random full-scale 16-bit I/Q, "
             "the 32-bit legs on widened copies, a d_last word per call and per block; "
             "HIP events around %d runs of a leg (one pass of per-block calls) behind "
             "one untimed run of it, legs (a) .. (e) alternated, (f) behind them on its "
             "own, min - max of %d repetitions after one warm-up of every leg; one "
             "process per core; outputs compared on every sample first.  Bytes per "
             "sample are read off the code, not profiled."
             % (a.log2_samples, a.blocks, a.log2_block, STEPS, a.reps)]
    print("\n".join(lines), flush=True)
    failed = []
    for name in ("io16", "ww34"):
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
