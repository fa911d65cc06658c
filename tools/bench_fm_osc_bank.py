#!/usr/bin/env python3
"""bench_fm_osc_bank.py -- an FM oscillator bank (cordic_fmbank_run) against what
a caller did before it, one cordic_table_fm / cordic_quad_fm call per block, and
against ONE such call over the same samples.

For sintbl, qtrtbl16, qtrtbl (the L2 gather) and quadtbl (parameters from
bench.py's workload table, tools/bench_common.py), sine only and quadrature,
and for the int16 sine-only form on sintbl, in ONE process: 1024 blocks x 2^16
samples of random full-range tuning words, back to back in one array, the
outputs back to back as well, each block with a d_acc word:

  (a) bank       one cordic_fmbank_run over all blocks: two launches
  (b) per block  one single call per block, on the same arrays and d_acc words
                 (the C entry point through ctypes with the arguments converted
                 beforehand): two launches per block
  (c) one call   ONE single call of 2^26 samples on the same arrays

All three read 8 B per sample (the tuning words twice) and write 4 per output
(2 in the int16 form).  Before any timing the outputs and d_acc words of (a)
are checked on every sample against those of (b).  Timing: HIP events around
`steps` runs of a leg (10 for (a) and (c), 1 pass over the blocks for (b)), the
legs alternated within every repetition, one warm-up repetition, then --reps
(>= 5) timed ones; min - max over the repetitions.  (b) and (c) are code the
bank does not add.

The bank has to beat the per-block calls, best against best, on every core: the
exit status is 2 where it does not.  The ratio to the one long call is recorded.

  python tools/bench_fm_osc_bank.py --out profiles/r19/fm_osc_bank.txt
"""
import argparse
import os
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
# (workload, quadrature, int16)
CASES = [(w, iq, False) for w in ("sintbl", "qtrtbl16", "qtrtbl", "quadtbl")
         for iq in (False, True)] + [("sintbl", False, True)]


def measure(name, iq, i16, blocks, length, reps, bufs):
    import bench_common as B
    import torch
    import cordic_amd as ca

    w = B.WORKLOADS[name]
    is_table = "table" in w
    core = ca.Table(*w["table"]) if is_table else ca.Quad(*w["quad"])
    layout = ("lds mode %d" % core.lds_mode) if is_table else "quad, lds"
    fcw, s32, c32, accs = bufs
    n = blocks * length
    s, c = (s32.view(torch.int16)[:n], c32.view(torch.int16)[:n]) if i16 else (s32, c32)
    if not iq:
        c = None
    work = torch.zeros(max(16, ca.fm_workspace(n)), dtype=torch.uint8, device=fcw.device)
    view = lambda t, k: None if t is None else t[k * length:(k + 1) * length]
    jobs = [(view(fcw, k), None, view(s, k), view(c, k), length, 0, accs[k:])
            for k in range(blocks)]
    bank = core.fm_bank(jobs, i16=i16)
    info = bank.info()
    st = torch.cuda.current_stream().cuda_stream
    fn = getattr(ca.lib(), ("cordic_table_fm" if is_table else "cordic_quad_fm")
                 + ("16" if i16 else ""))
    calls = [(core._h, length, j[0].data_ptr(), None, 0, j[6].data_ptr(),
              j[2].data_ptr(), None if j[3] is None else j[3].data_ptr(),
              work.data_ptr(), st) for j in jobs]

    def loop():
        for a in calls:
            if fn(*a):
                raise SystemExit("%s: the single call failed" % name)

    def long_call():
        core.fm(fcw, s, c, n=n, acc=accs, work=work)

    # ---- the outputs first
    outs = [t for t in (s, c) if t is not None]
    accs.zero_()
    for t in outs:
        t.fill_(-1)
    loop()
    torch.cuda.synchronize()
    refs, aref = [t.clone() for t in outs], accs.clone()
    accs.zero_()
    for t in outs:
        t.fill_(-1)
    bank.run()
    torch.cuda.synchronize()
    if not (all(torch.equal(t, r) for t, r in zip(outs, refs))
            and torch.equal(accs, aref)):
        raise SystemExit("%s: the bank differs from one call per block" % name)
    del refs, aref

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
    core.close()
    form = "%s, %s" % ("int16" if i16 else "int32", "sine and cosine" if iq else "sine only")
    lines = ["%s  %s  [%s; %s; %d spans of %d samples, two launches]"
             % (name, w["desc"], layout, form, info["spans"], info["tile"])]
    stat = {}
    for k, _, _ in legs:
        v = sorted(rates[k])
        stat[k] = (v[0], v[-1])
        lines.append("    %-9s  min %7.1f  max %7.1f Gsample/s" % (k, v[0], v[-1]))
    b, p, o = stat["bank"], stat["per block"], stat["one call"]
    beats = b[1] > p[1]
    lines.append("    bank / per block = %.1fx .. %.1fx, best against best %.1fx (%s); "
                 "bank / one call = %.2f .. %.2f, best against best %.2f"
                 % (b[0] / p[1], b[1] / p[0], b[1] / p[1],
                    "the bank beats the per-block calls" if beats
                    else "** THE BANK DOES NOT BEAT THE PER-BLOCK CALLS **",
                    b[0] / o[1], b[1] / o[0], b[1] / o[1]))
    return lines, beats


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
    import torch
    import build_stamp

    length = 1 << a.log2_block
    n = a.blocks * length
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    fcw = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device=dev,
                        generator=gen)
    bufs = [fcw] + [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
    bufs.append(torch.zeros(a.blocks, dtype=torch.int32, device=dev))
    st = build_stamp.stamp()
    lines = ["%s, commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
        torch.cuda.get_device_name(0), st["git_head"],
        " + uncommitted changes" if st["git_dirty"] else "",
        st["kernel_sources_sha256"], st["lib_sha256"]),
        "%d blocks x 2^%d samples, random tuning words, a d_acc word per block; HIP "
        "events around 10 bank runs / one pass of per-block calls / 10 long calls, "
        "legs alternated, min - max of %d repetitions after one warm-up of every "
        "leg; one process; the bank checked against the per-block calls on every "
        "sample first" % (a.blocks, a.log2_block, a.reps)]
    print("\n".join(lines), flush=True)
    slow = []
    for name, iq, i16 in CASES:
        part, beats = measure(name, iq, i16, a.blocks, length, a.reps, bufs)
        print("\n".join(part), flush=True)
        lines += part
        if not beats:
            slow.append(part[0].split("  ")[0])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if slow:
        sys.stderr.write("the bank does not beat the per-block calls on: %s\n"
                         % ", ".join(slow))
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
