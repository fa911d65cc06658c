#!/usr/bin/env python3
"""bench_fm_rx_c16.py -- the tuned FM receiver on INTERLEAVED int16 I/Q
(cordic_plan_fm_rx_c16, cordic_rxbank_create_decim_c16) against the *16 forms
on split arrays, and against what a caller with a capture buffer did before
them: a splitting pass of their own in front of the *16 form.

The 16-bit pair of profiles/r23/fm_rx_decim.txt (cfg1's core into io16), ONE
process, random tuning words, random full-scale I/Q, a d_acc and a d_last word:

  (a) fm_rx_c16    one cordic_plan_fm_rx_c16 call on 2^28 complex samples
  (b) fm_rx16      cordic_plan_fm_rx16 on split copies of the same data
  (c) split + (b)  the fallback's split kernel (fm_rx_split_c16, one 16-byte load
                   and two 8-byte stores per lane) over the buffer, then (b),
                   timed together

  (d) c16 bank     a cordic_rxbank_create_decim_c16 bank of 256 x 1536 at k = 3,
                   200 rounds back to back, time per round
  (e) 16 bank      the cordic_rxbank_create_decim16 bank on split copies
  (f) split + (e)  ONE split launch over the whole round's buffer, then (e)

Before any timing every output sample and both words of (a), (c) are compared
with (b)'s, and those of (d), (f) with (e)'s.  Timing: HIP events around
`steps` runs of a leg, the legs alternated within every repetition, one warm-up
repetition, then --reps (>= 5) timed ones; min - max over the repetitions.
Required, best against best: (a) / (b) and (d) / (e) >= 0.97 (the same chains
behind another container, the same 12 bytes a sample); (a) / (c) and (d) / (f)
> 1.00 (a launch and 8 bytes a sample saved).  A miss is reported as MISSED
with its numbers.

The split kernel is not part of the C ABI; the tool calls the library's own
launcher of it by its C++ symbol, so that (c) and (f) time the kernel the
fallback runs and not a copy.

  python tools/bench_fm_rx_c16.py --out profiles/r24/fm_rx_c16.txt
"""
import argparse
import ctypes as C
import os
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
CFG1 = ("p2r", 16, 16, 2, 16, 16)
IO16 = ("r2p", 16, 16, 2, 16, -1)
SPLIT = "_ZN10cordic_amd21launch_fmrx_split_c16EmPKsPsS2_Pv"


def verdict(ratio, need, strict):
    ok = ratio > need if strict else ratio >= need
    return "ok" if ok else "MISSED (required %s %.2f)" % (">" if strict else ">=", need)


def measure(n, reps, steps, rounds):
    import bench_common as B
    import torch
    import cordic_amd as ca

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    mcfg = ca.Config.from_cli(B.MODE[CFG1[0]], *CFG1[1:])
    ccfg = ca.Config.from_cli(B.MODE[IO16[0]], *IO16[1:])
    plan = ca.Plan(mcfg)
    fused = plan.fm_rx_c16_info(ccfg)[0]
    try:
        split_fn = getattr(ca.lib(), SPLIT)
    except AttributeError:
        raise SystemExit("the library does not export %s" % SPLIT)
    split_fn.restype = C.c_int
    split_fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    fcw = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device=dev,
                        generator=gen)
    # the capture buffer, one complex sample off the 16-byte grid, and its halves
    buf = torch.randint(-(1 << 15), 1 << 15, (2 * n + 2,), dtype=torch.int32, device=dev,
                        generator=gen).to(torch.int16)
    iq = buf[2:]
    x, y = iq[0::2].contiguous(), iq[1::2].contiguous()
    sx, sy = torch.empty_like(x), torch.empty_like(y)      # what the split pass writes
    mag, freq = (torch.empty(n, dtype=torch.int16, device=dev) for _ in range(2))
    words = torch.zeros(8, dtype=torch.int32, device=dev)
    acc, last = words[0:], words[4:]
    z = lambda b: torch.zeros(max(16, b), dtype=torch.uint8, device=dev)

    def split(count):
        if split_fn(count, iq.data_ptr(), sx.data_ptr(), sy.data_ptr(), None):
            raise SystemExit("the split launch failed")

    def timed(legs, count, samples):
        """per leg the sorted rates (Gsample/s)"""
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

    lines = ["cfg1-io16  %s -> %s, int16  [%s]" % (
        " ".join(map(str, CFG1)), " ".join(map(str, IO16)),
        "fused, two launches" if fused else "fallback")]

    # ---- (a) / (b) / (c): the single call
    wc16, w16 = z(plan.fm_rx_c16_workspace(ccfg, n)), z(plan.fm_rx16_workspace(ccfg, n))

    def leg_a():
        plan.fm_rx_c16(ccfg, fcw, iq, mag, freq, wc16, n=n, acc=acc, last=last)

    def leg_b():
        plan.fm_rx16(ccfg, fcw, x, y, mag, freq, w16, n=n, acc=acc, last=last)

    def leg_c():
        split(n)
        plan.fm_rx16(ccfg, fcw, sx, sy, mag, freq, w16, n=n, acc=acc, last=last)

    def checked(run, what, ref=None, upto=n):
        words.zero_(); mag.fill_(-1); freq.fill_(-1)
        run()
        torch.cuda.synchronize()
        got = (mag[:upto].clone(), freq[:upto].clone(), words.clone())
        if ref is not None and not all(torch.equal(g, r) for g, r in zip(got, ref)):
            raise SystemExit("%s differs from the 16-bit form on split copies" % what)
        return got

    ref = checked(leg_b, "(b)")
    checked(leg_a, "(a) fm_rx_c16", ref)
    checked(leg_c, "(c) the split in front of fm_rx16", ref)
    if not (torch.equal(sx, x) and torch.equal(sy, y)):
        raise SystemExit("the split kernel's arrays differ from the halves")
    del ref
    r = timed([("a", leg_a), ("b", leg_b), ("c", leg_c)], steps, n)
    a, b, c = r["a"], r["b"], r["c"]
    lines.append("    2^%d complex samples: (a) fm_rx_c16 %.1f .. %.1f, (b) fm_rx16 %.1f .. "
                 "%.1f, (c) split + fm_rx16 %.1f .. %.1f Gsample/s"
                 % (n.bit_length() - 1, a[0], a[-1], b[0], b[-1], c[0], c[-1]))
    q = a[-1] / b[-1]
    lines.append("    (a) / (b): best against best %.2f, range %.2f .. %.2f: %s"
                 % (q, a[0] / b[-1], a[-1] / b[0], verdict(q, 0.97, False)))
    q = a[-1] / c[-1]
    lines.append("    (a) / (c): best against best %.2f, range %.2f .. %.2f: %s"
                 % (q, a[0] / c[-1], a[-1] / c[0], verdict(q, 1.0, True)))

    # ---- (d) / (e) / (f): the small round at k = 3
    k, blocks, length = 3, 256, 1536
    tot, dl = blocks * length, length >> 3
    md = tot >> k
    view = lambda t, j, ln=length: t[j * ln:(j + 1) * ln]
    wds = torch.zeros(8 * blocks, dtype=torch.int32, device=dev)
    cj = [(view(fcw, j), None, iq[2 * j * length:], view(mag, j, dl), view(freq, j, dl), length,
           0, wds[8 * j:], 0, wds[8 * j + 4:]) for j in range(blocks)]

    def jobs16(px, py):
        return [(view(fcw, j), None, view(px, j), view(py, j), view(mag, j, dl),
                 view(freq, j, dl), length, 0, wds[8 * j:], 0, wds[8 * j + 4:])
                for j in range(blocks)]
    cbank = ca.RxBankC16(plan, ccfg, cj, log2r=k)
    ebank = ca.RxBank16(plan, ccfg, jobs16(x, y), log2r=k)
    fbank = ca.RxBank16(plan, ccfg, jobs16(sx, sy), log2r=k)

    def leg_f():
        split(tot)
        fbank.run()

    def checked_bank(run, what, ref=None):
        wds.zero_(); mag[:md].fill_(-1); freq[:md].fill_(-1)
        run()
        torch.cuda.synchronize()
        got = (mag[:md].clone(), freq[:md].clone(), wds.clone())
        if ref is not None and not all(torch.equal(g, r) for g, r in zip(got, ref)):
            raise SystemExit("%s differs from the 16-bit bank on split copies" % what)
        return got

    sx.fill_(0); sy.fill_(0)
    ref = checked_bank(ebank.run, "(e)")
    checked_bank(cbank.run, "(d) the c16 bank", ref)
    checked_bank(leg_f, "(f) the split in front of the 16-bit bank", ref)
    info = cbank.info()
    r = timed([("d", cbank.run), ("e", ebank.run), ("f", leg_f)], rounds, tot)
    cbank.close(); ebank.close(); fbank.close()
    plan.close()
    us = lambda v: tot / (v * 1e9) * 1e6            # a round's time from its rate
    d, e, f = r["d"], r["e"], r["f"]
    lines.append("    256 blocks x 1536 at k = 3, %d rounds back to back [%d spans, fused %d]: "
                 "(d) c16 bank %.1f .. %.1f us a round, (e) 16-bit bank %.1f .. %.1f, (f) "
                 "split + 16-bit bank %.1f .. %.1f"
                 % (rounds, info["spans"], info["fused"], us(d[-1]), us(d[0]), us(e[-1]),
                    us(e[0]), us(f[-1]), us(f[0])))
    q = d[-1] / e[-1]
    lines.append("    (d) / (e): best against best %.2f, range %.2f .. %.2f: %s"
                 % (q, d[0] / e[-1], d[-1] / e[0], verdict(q, 0.97, False)))
    q = d[-1] / f[-1]
    lines.append("    (d) / (f): best against best %.2f, range %.2f .. %.2f: %s"
                 % (q, d[0] / f[-1], d[-1] / f[0], verdict(q, 1.0, True)))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--log2-n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=200)
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
        "random tuning words, random full-scale int16 I/Q one complex sample off the "
        "16-byte grid, a d_acc and a d_last word; HIP events around %d runs of a leg (%d "
        "rounds of a bank), legs alternated, min - max of %d repetitions after one warm-up "
        "of every leg; one process; every output sample and all words compared with the "
        "16-bit form on split copies first" % (a.steps, a.rounds, a.reps)]
    lines += measure(1 << a.log2_n, a.reps, a.steps, a.rounds)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
