#!/usr/bin/env python3
"""bench_fm_mix_bank.py -- an FM mixer bank (cordic_mixbank_run) against what a
caller did before it, one cordic_plan_fm_mix call per block, and against ONE
cordic_plan_fm_mix call over the same samples.

For cfg2's core, the 20-stage core and nat24 (the cores of tools/bench_fm_mix.py)
and, for the record, one core of the one-by-one path (ww38: WW 38), in ONE
process: 1024 blocks x 2^16 samples of random tuning words and random
full-scale I/Q, back to back in five arrays, each block with a d_acc word:

  (a) bank       one cordic_mixbank_run over all blocks
  (b) per block  one cordic_plan_fm_mix call per block, on the same arrays and
                 d_acc words (the C entry point through ctypes with the
                 arguments converted beforehand)
  (c) one call   ONE cordic_plan_fm_mix call of 2^26 samples on the same arrays

On a fused core all three read 16 and write 8 B per sample.  Before any timing
the outputs and d_acc words of (a) are checked on every sample against those of
(b).  Timing: HIP events around `steps` runs of a leg (10 for (a) and (c), 1
pass over the blocks for (b)), the legs alternated within every repetition, one
warm-up repetition, then --reps (>= 5) timed ones; min - max over the
repetitions.  (b) and (c) are code the bank does not add.

No threshold is fixed in advance; the ratios are recorded.

  python tools/bench_fm_mix_bank.py --out profiles/r15/fm_mix_bank.txt
"""
import argparse
import os
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
N20 = ("p2r", 32, 32, 2, 32, 20)
WW38 = ("p2r", 32, 32, 5, 32, 24)       # tests/test_jobset_fused.py: WW 38


def measure(name, cli, desc, blocks, length, reps, bufs, gen):
    import bench_common as B
    import torch
    import cordic_amd as ca

    cfg = ca.Config.from_cli(B.MODE[cli[0]], *cli[1:])
    plan = ca.Plan(cfg)
    fcw, x, y, ox, oy, accs = bufs
    n = blocks * length
    half = 1 << (cfg.iw - 1)
    for t in (x, y):                    # full scale of this core's ports
        torch.randint(-half, half, (n,), dtype=torch.int32, device=t.device,
                      generator=gen, out=t)
    work = torch.zeros(max(16, plan.fm_mix_workspace(n)), dtype=torch.uint8,
                       device=x.device)
    view = lambda t, k: t[k * length:(k + 1) * length]
    jobs = [(view(fcw, k), None, view(x, k), view(y, k), view(ox, k), view(oy, k),
             length, 0, accs[k:]) for k in range(blocks)]
    bank = ca.MixBank(plan, jobs)
    info = bank.info()
    st = torch.cuda.current_stream().cuda_stream
    fn = ca.lib().cordic_plan_fm_mix
    calls = [(plan._h, length, j[0].data_ptr(), None, 0, j[8].data_ptr(),
              j[2].data_ptr(), j[3].data_ptr(), j[4].data_ptr(), j[5].data_ptr(),
              work.data_ptr(), st) for j in jobs]

    def loop():
        for a in calls:
            if fn(*a):
                raise SystemExit("%s: cordic_plan_fm_mix failed" % name)

    def long_call():
        plan.fm_mix(fcw, x, y, ox, oy, work, n=n, acc=accs)

    # ---- the outputs first
    accs.zero_(); ox.fill_(-1); oy.fill_(-1)
    loop()
    torch.cuda.synchronize()
    xref, yref, aref = ox.clone(), oy.clone(), accs.clone()
    accs.zero_(); ox.fill_(-1); oy.fill_(-1)
    bank.run()
    torch.cuda.synchronize()
    if not (torch.equal(ox, xref) and torch.equal(oy, yref)
            and torch.equal(accs, aref)):
        raise SystemExit("%s: the bank differs from one call per block" % name)
    del xref, yref, aref

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
    plan.close()
    path = ("fused: %d spans of %d samples, two launches"
            % (info["spans"], info["tile"])) if info["fused"] else "one by one"
    lines = ["%s  %s  [%s]" % (name, desc, path)]
    stat = {}
    for k, _, _ in legs:
        v = sorted(rates[k])
        stat[k] = (v[0], v[-1])
        lines.append("    %-9s  min %7.1f  max %7.1f Gsample/s" % (k, v[0], v[-1]))
    b, p, o = stat["bank"], stat["per block"], stat["one call"]
    lines.append("    bank / per block = %.1fx .. %.1fx; bank / one call = %.2f .. %.2f"
                 % (b[0] / p[1], b[1] / p[0], b[0] / o[1], b[1] / o[0]))
    return lines


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
    import build_stamp

    length = 1 << a.log2_block
    n = a.blocks * length
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    fcw = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device=dev,
                        generator=gen)
    bufs = [fcw] + [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
    bufs.append(torch.zeros(a.blocks, dtype=torch.int32, device=dev))
    st = build_stamp.stamp()
    lines = ["%s, commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
        torch.cuda.get_device_name(0), st["git_head"],
        " + uncommitted changes" if st["git_dirty"] else "",
        st["kernel_sources_sha256"], st["lib_sha256"]),
        "%d blocks x 2^%d samples, random tuning words, random full-scale I/Q, a "
        "d_acc word per block; HIP events around 10 bank runs / one pass of "
        "per-block calls / 10 long calls, legs alternated, min - max of %d "
        "repetitions after one warm-up of every leg; one process; the bank checked "
        "against the per-block calls on every sample first"
        % (a.blocks, a.log2_block, a.reps)]
    print("\n".join(lines), flush=True)
    cores = [
        ("cfg2", B.WORKLOADS["cfg2"]["cli"], "basiccordic 16-stage, 32-bit: the core "
         "of the `ddc` workload"),
        ("n20", N20, "basiccordic 20-stage, 32-bit"),
        ("nat24", B.WORKLOADS["nat24"]["cli"], "gencordic -t p2r -i 24 -o 24: WW27 "
         "PW31, 27 stages"),
        ("ww38", WW38, "basiccordic 24-stage, 32-bit, 5 extra bits: WW 38, one by "
         "one, for the record"),
    ]
    for name, cli, desc in cores:
        part = measure(name, cli, desc, a.blocks, length, a.reps, bufs, gen)
        print("\n".join(part), flush=True)
        lines += part
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
