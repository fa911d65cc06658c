#!/usr/bin/env python3
"""bench_fm_mix_c16.py -- the FM mixer family on INTERLEAVED int16 I/Q, in and
out (cordic_plan_fm_mix_c16, cordic_plan_fm_mix_decim_c16,
cordic_mixbank_create_decim_c16) against the *16 forms on split arrays, and
against what a caller with a capture buffer did before them: a splitting pass
in front of the *16 form and an interleaving pass behind it.

cfg1's core and nat16, ONE process, random tuning words, random full-scale I/Q,
a d_acc word:

  (a) fm_mix_c16     one cordic_plan_fm_mix_c16 call on 2^28 complex samples
  (b) fm_mix16       cordic_plan_fm_mix16 on split copies of the same data
  (c) split + (b) + interleave   the fallback's two elementwise kernels around
                     (b), timed together

  (d) fm_mix_decim_c16 at k = 2 and k = 6, (e) the _decim16 twin, (f) split +
      (e) + interleave

  (g) c16 bank       a cordic_mixbank_create_decim_c16 bank of 256 x 1536 at k =
                     3, 200 rounds back to back, time per round
  (h) 16 bank        the cordic_mixbank_create_decim16 bank on split copies
  (i) split + (h) + interleave   ONE split launch over the round's buffer, (h),
                     ONE interleave launch over the round's output

  (j) a c16 bank of 1024 x 2^16 at k = 3, (k) its *16 twin

Before any timing every output short and the d_acc words of an interleaved leg
and of a leg with the two passes around it are compared with the *16 leg's.
Timing: HIP events around `steps` runs of a leg, the legs alternated within
every repetition, one warm-up repetition, then --reps (>= 5) timed ones; min -
max over the repetitions; INPUT samples per second.  Required, best against
best: every interleaved form >= 0.97 of its *16 twin ((a)/(b), (d)/(e),
(g)/(h), (j)/(k): the same bytes through the same arithmetic) and > 1.00 of the
twin with the two conversion launches around it ((a)/(c), (d)/(f), (g)/(i)).
A miss is reported as MISSED with its numbers.

The two elementwise kernels are not part of the C ABI; the tool calls the
library's own launchers of them by their C++ symbols, so that (c), (f) and (i)
time the kernels the fallback runs and not copies.

  python tools/bench_fm_mix_c16.py --out profiles/r26/fm_mix_c16.txt
"""
import argparse
import ctypes as C
import os
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
CORES = (("cfg1", ("p2r", 16, 16, 2, 16, 16)), ("nat16", ("p2r", 16, 16, 2, -1, -1)))
SPLIT = "_ZN10cordic_amd21launch_fmrx_split_c16EmPKsPsS2_Pv"
INTERLEAVE = "_ZN10cordic_amd25launch_fmx_interleave_c16EmPKsS1_PsPv"


def verdict(ratio, need, strict):
    ok = ratio > need if strict else ratio >= need
    return "ok" if ok else "MISSED (required %s %.2f)" % (">" if strict else ">=", need)


def ratios(lines, top, name, bot, bname, need, strict):
    q = top[-1] / bot[-1]
    lines.append("    %s / %s: best against best %.2f, range %.2f .. %.2f: %s"
                 % (name, bname, q, top[0] / bot[-1], top[-1] / bot[0],
                    verdict(q, need, strict)))


def measure(core, args, n, reps, steps, rounds, big_rounds):
    import bench_common as B
    import torch
    import cordic_amd as ca

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    plan = ca.Plan(ca.Config.from_cli(B.MODE[args[0]], *args[1:]))
    fused = plan.fm_mix_c16_info()[0]
    fns = []
    for sym in (SPLIT, INTERLEAVE):
        try:
            fn = getattr(ca.lib(), sym)
        except AttributeError:
            raise SystemExit("the library does not export %s" % sym)
        fn.restype = C.c_int
        fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        fns.append(fn)
    split_fn, inter_fn = fns

    fcw = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device=dev,
                        generator=gen)
    # the capture buffer and the output, one complex sample off the 16-byte grid
    buf = torch.randint(-(1 << 15), 1 << 15, (2 * n + 2,), dtype=torch.int32, device=dev,
                        generator=gen).to(torch.int16)
    iq = buf[2:]
    x, y = iq[0::2].contiguous(), iq[1::2].contiguous()
    sx, sy = torch.empty_like(x), torch.empty_like(y)      # what the split pass writes
    obuf = torch.empty(2 * n + 2, dtype=torch.int16, device=dev)
    oiq = obuf[2:]
    ox, oy = (torch.empty(n, dtype=torch.int16, device=dev) for _ in range(2))
    words = torch.zeros(4, dtype=torch.int32, device=dev)
    z = lambda b: torch.zeros(max(16, b), dtype=torch.uint8, device=dev)

    def split(count):
        if split_fn(count, iq.data_ptr(), sx.data_ptr(), sy.data_ptr(), None):
            raise SystemExit("the split launch failed")

    def inter(count):
        if inter_fn(count, ox.data_ptr(), oy.data_ptr(), oiq.data_ptr(), None):
            raise SystemExit("the interleave launch failed")

    def timed(legs, count, samples):
        """per leg the sorted rates (Gsample/s, input samples)"""
        rates = {k: [] for k, _ in legs}
        for rep in range(reps + 1):     # rep 0: warm-up of every leg
            for k, run in legs:
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(count):
                    run()
                e1.record()
                e1.synchronize()
                if rep:
                    rates[k].append(samples * count / (e0.elapsed_time(e1) * 1e-3) / 1e9)
        return {k: sorted(v) for k, v in rates.items()}

    lines = ["%s  %s, int16  [%s]" % (core, " ".join(map(str, args)),
                                      "fused, two launches" if fused else "fallback")]

    # ---- the single calls: k = 0 is (a) / (b) / (c), k = 2 and 6 are (d) / (e) / (f)
    for k in (0, 2, 6):
        m = n >> k
        wc = z(plan.fm_mix_decim_c16_workspace(n, k))
        w16 = z(plan.fm_mix_decim16_workspace(n, k))

        def leg_c16():
            plan.fm_mix_decim_c16(k, fcw, iq, oiq, wc, n=n, acc=words)

        def leg_16(px=x, py=y):
            plan.fm_mix_decim16(k, fcw, px, py, ox, oy, w16, n=n, acc=words)

        def leg_conv():
            split(n)
            leg_16(sx, sy)
            inter(m)

        def checked(run, interleaved, what, ref=None):
            words.zero_(); oiq[:2 * m].fill_(-1); ox[:m].fill_(-1); oy[:m].fill_(-1)
            run()
            torch.cuda.synchronize()
            got = (oiq[0:2 * m:2].clone(), oiq[1:2 * m:2].clone()) if interleaved \
                else (ox[:m].clone(), oy[:m].clone())
            got += (words.clone(),)
            if ref is not None and not all(torch.equal(g, r) for g, r in zip(got, ref)):
                raise SystemExit("%s differs from the 16-bit form on split copies" % what)
            return got

        ref = checked(leg_16, False, "the twin")
        checked(leg_c16, True, "the interleaved call at k = %d" % k, ref)
        checked(leg_conv, True, "split + the twin + interleave at k = %d" % k, ref)
        if not (torch.equal(sx, x) and torch.equal(sy, y)):
            raise SystemExit("the split kernel's arrays differ from the halves")
        del ref
        r = timed([("c16", leg_c16), ("16", leg_16), ("conv", leg_conv)], steps, n)
        a, b, c = r["c16"], r["16"], r["conv"]
        la, lb, lc = ("(a)", "(b)", "(c)") if k == 0 else ("(d)", "(e)", "(f)")
        lines.append("    2^%d complex samples, k = %d: %s c16 %.1f .. %.1f, %s the *16 twin "
                     "%.1f .. %.1f, %s split + twin + interleave %.1f .. %.1f Gsample/s"
                     % (n.bit_length() - 1, k, la, a[0], a[-1], lb, b[0], b[-1], lc, c[0],
                        c[-1]))
        ratios(lines, a, la, b, lb, 0.97, False)
        ratios(lines, a, la, c, lc, 1.0, True)

    # ---- the banks at k = 3: (g) / (h) / (i) the small round, (j) / (k) the large
    k = 3
    for blocks, length, count, conv in ((256, 1536, rounds, True),
                                        (min(1024, n >> 16), 1 << 16, big_rounds, False)):
        tot, dl = blocks * length, length >> k
        md = tot >> k
        view = lambda t, j, ln: t[j * ln:(j + 1) * ln]
        wds = torch.zeros(4 * blocks, dtype=torch.int32, device=dev)
        cj = [(view(fcw, j, length), None, iq[2 * j * length:], oiq[2 * j * dl:], length, 0,
               wds[4 * j:]) for j in range(blocks)]

        def jobs16(px, py):
            return [(view(fcw, j, length), None, view(px, j, length), view(py, j, length),
                     view(ox, j, dl), view(oy, j, dl), length, 0, wds[4 * j:])
                    for j in range(blocks)]
        cbank = ca.MixBankC16(plan, cj, log2r=k)
        hbank = ca.MixBank16(plan, jobs16(x, y), log2r=k)
        ibank = ca.MixBank16(plan, jobs16(sx, sy), log2r=k)

        def leg_i():
            split(tot)
            ibank.run()
            inter(md)

        def checked_bank(run, interleaved, what, ref=None):
            wds.zero_(); oiq[:2 * md].fill_(-1); ox[:md].fill_(-1); oy[:md].fill_(-1)
            run()
            torch.cuda.synchronize()
            got = (oiq[0:2 * md:2].clone(), oiq[1:2 * md:2].clone()) if interleaved \
                else (ox[:md].clone(), oy[:md].clone())
            got += (wds.clone(),)
            if ref is not None and not all(torch.equal(g, r) for g, r in zip(got, ref)):
                raise SystemExit("%s differs from the 16-bit bank on split copies" % what)
            return got

        sx.fill_(0); sy.fill_(0)
        ref = checked_bank(hbank.run, False, "the twin")
        checked_bank(cbank.run, True, "the c16 bank of %d x %d" % (blocks, length), ref)
        legs = [("c16", cbank.run), ("16", hbank.run)]
        if conv:
            checked_bank(leg_i, True, "split + the 16-bit bank + interleave", ref)
            legs.append(("conv", leg_i))
        del ref
        info = cbank.info()
        r = timed(legs, count, tot)
        cbank.close(); hbank.close(); ibank.close()
        us = lambda v: tot / (v * 1e9) * 1e6            # a round's time from its rate
        g, h = r["c16"], r["16"]
        lg, lh, li = ("(g)", "(h)", "(i)") if conv else ("(j)", "(k)", None)
        text = ("    %d blocks x %d at k = 3, %d rounds back to back [%d spans, fused %d]: %s "
                "c16 bank %.1f .. %.1f us a round (%.1f .. %.1f Gsample/s), %s 16-bit bank "
                "%.1f .. %.1f us (%.1f .. %.1f)"
                % (blocks, length, count, info["spans"], info["fused"], lg, us(g[-1]),
                   us(g[0]), g[0], g[-1], lh, us(h[-1]), us(h[0]), h[0], h[-1]))
        if conv:
            i = r["conv"]
            text += ", %s split + 16-bit bank + interleave %.1f .. %.1f us" % (
                li, us(i[-1]), us(i[0]))
        lines.append(text)
        ratios(lines, g, lg, h, lh, 0.97, False)
        if conv:
            ratios(lines, g, lg, r["conv"], li, 1.0, True)
    plan.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--log2-n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--big-rounds", type=int, default=8)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if not 19 <= a.log2_n <= 28:
        ap.error("--log2-n 19 .. 28")
    sys.path.insert(0, TOOLS)
    sys.path.insert(0, os.path.dirname(TOOLS))
    import torch
    import build_stamp

    st = build_stamp.stamp()
    lines = ["%s, commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
        torch.cuda.get_device_name(0), st["git_head"],
        " + uncommitted changes" if st["git_dirty"] else "",
        st["kernel_sources_sha256"], st["lib_sha256"]),
        "random tuning words, random full-scale int16 I/Q, input and output one complex "
        "sample off the 16-byte grid, a d_acc word; HIP events around %d runs of a leg (%d "
        "rounds of the small bank, %d of the large), legs alternated, min - max of %d "
        "repetitions after one warm-up of every leg; one process; INPUT samples per second; "
        "every output short and all words compared with the 16-bit form on split copies "
        "first" % (a.steps, a.rounds, a.big_rounds, a.reps)]
    for core, args in CORES:
        lines += measure(core, args, 1 << a.log2_n, a.reps, a.steps, a.rounds, a.big_rounds)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
