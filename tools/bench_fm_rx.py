#!/usr/bin/env python3
"""bench_fm_rx.py -- the tuned FM receiver (cordic_plan_fm_rx, cordic_plan_fm_rx16)
and the receiver banks (cordic_rxbank_run) against what a caller did before
them: the mixer into two arrays and the discriminator from them.

Per core pair, in ONE process, on 2^28 samples (--log2-n) of random tuning
words and random full-scale I/Q, with a d_acc and a d_last word:

  (a) receiver   one cordic_plan_fm_rx call
  (b) two calls  cordic_plan_fm_mix + cordic_fm_demod on the same inputs, the
                 tuned I/Q in two arrays of their own

  (c) rx bank    1024 blocks x 2^16 samples, each with both words, one
                 cordic_rxbank_run
  (d) two banks  a cordic_mixbank_run and a cordic_demodbank_run over the same
                 blocks
  (e) rx bank    256 blocks x 1500 samples (examples/afc_receiver.c's round),
                 200 runs back to back, time per round
  (f) two banks  the same round through the two banks

On int32 (a) moves 20 B per sample and (b) 40; on int16 12 and 24.  Before any
timing the outputs and all words of (a), (c), (e) are checked on every sample
against those of (b), (d), (f).  Timing: HIP events around `steps` runs of a leg, the legs
alternated within every repetition, one warm-up repetition, then --reps (>= 5)
timed ones; min - max over the repetitions.  (b), (d), (f) are code the
receiver does not add.  Required: best against best >= 1.00 for (a) / (b), (c) /
(d) and (e) / (f) on every pair.

  python tools/bench_fm_rx.py --out profiles/r20/fm_rx.txt
"""
import argparse
import os
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
CFG3 = ("r2p", 24, 24, 2, -1, 20)
NATR2P24 = ("r2p", 24, 24, 2, -1, -1)
CFG1 = ("p2r", 16, 16, 2, 16, 16)
IO16 = ("r2p", 16, 16, 2, 16, -1)


def measure(name, mcli, ccli, i16, n, reps, steps, gen):
    import bench_common as B
    import torch
    import cordic_amd as ca

    dev = torch.device("cuda:0")
    mcfg = ca.Config.from_cli(B.MODE[mcli[0]], *mcli[1:])
    ccfg = ca.Config.from_cli(B.MODE[ccli[0]], *ccli[1:])
    plan = ca.Plan(mcfg)
    dt = torch.int16 if i16 else torch.int32
    half = 1 << (mcfg.iw - 1)
    fcw = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device=dev,
                        generator=gen)
    x, y = (torch.randint(-half, half, (n,), dtype=torch.int32, device=dev,
                          generator=gen).to(dt) for _ in range(2))
    mag, freq, tx, ty = (torch.empty(n, dtype=dt, device=dev) for _ in range(4))
    words = torch.zeros(8, dtype=torch.int32, device=dev)
    acc, last = words[0:], words[4:]
    z = lambda b: torch.zeros(max(16, b), dtype=torch.uint8, device=dev)
    rx, mix = (plan.fm_rx16, plan.fm_mix16) if i16 else (plan.fm_rx, plan.fm_mix)
    wrx = z((plan.fm_rx16_workspace if i16 else plan.fm_rx_workspace)(ccfg, n))
    wmix = z((plan.fm_mix16_workspace if i16 else plan.fm_mix_workspace)(n))
    wdem = z(ca.fm_demod_workspace(n))
    fused = (plan.fm_rx16_info if i16 else plan.fm_rx_info)(ccfg)[0]

    def receiver():
        rx(ccfg, fcw, x, y, mag, freq, wrx, n=n, acc=acc, last=last)

    def two_calls():
        mix(fcw, x, y, tx, ty, wmix, n=n, acc=acc)
        ca.fm_demod(ccfg, tx, ty, mag, freq, wdem, n=n, last=last)

    # ---- the outputs first
    words.zero_(); mag.fill_(-1); freq.fill_(-1)
    two_calls()
    torch.cuda.synchronize()
    mref, fref, wref = mag.clone(), freq.clone(), words.clone()
    words.zero_(); mag.fill_(-1); freq.fill_(-1)
    receiver()
    torch.cuda.synchronize()
    if not (torch.equal(mag, mref) and torch.equal(freq, fref)
            and torch.equal(words, wref)):
        raise SystemExit("%s: the receiver differs from the two calls" % name)
    del mref, fref, wref

    def timed(legs, count, samples):
        """per leg the sorted rates (Gsample/s) and times per run (us)"""
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

    legs = [("receiver", receiver), ("two calls", two_calls)]
    rates = timed(legs, steps, n)

    # ---- the banks: (c) / (d) on `blocks` x `length`, (e) / (f) on 256 x 1500
    def banks(blocks, length, count, what):
        m = blocks * length
        view = lambda t, k: t[k * length:(k + 1) * length]
        wds = torch.zeros(8 * blocks, dtype=torch.int32, device=dev)
        rxj = [(view(fcw, k), None, view(x, k), view(y, k), view(mag, k), view(freq, k),
                length, 0, wds[8 * k:], 0, wds[8 * k + 4:]) for k in range(blocks)]
        mxj = [(view(fcw, k), None, view(x, k), view(y, k), view(tx, k), view(ty, k),
                length, 0, wds[8 * k:]) for k in range(blocks)]
        dmj = [(view(tx, k), view(ty, k), view(mag, k), view(freq, k), length, 0,
                wds[8 * k + 4:]) for k in range(blocks)]
        rxb = (ca.RxBank16 if i16 else ca.RxBank)(plan, ccfg, rxj)
        mxb = (ca.MixBank16 if i16 else ca.MixBank)(plan, mxj)
        dmb = (ca.DemodBank16 if i16 else ca.DemodBank)(ccfg, dmj)

        def two_banks():
            mxb.run()
            dmb.run()

        wds.zero_(); mag[:m].fill_(-1); freq[:m].fill_(-1)
        two_banks()
        torch.cuda.synchronize()
        ref = (mag[:m].clone(), freq[:m].clone(), wds.clone())
        wds.zero_(); mag[:m].fill_(-1); freq[:m].fill_(-1)
        rxb.run()
        torch.cuda.synchronize()
        if not (torch.equal(mag[:m], ref[0]) and torch.equal(freq[:m], ref[1])
                and torch.equal(wds, ref[2])):
            raise SystemExit("%s: the rx bank differs from the two banks (%s)"
                             % (name, what))
        info = rxb.info()
        r = timed([("rx bank", rxb.run), ("two banks", two_banks)], count, m)
        rxb.close(); mxb.close(); dmb.close()
        return r, info

    big, big_info = banks(1024, min(1 << 16, n // 1024), 10, "1024 blocks")
    small, small_info = banks(256, 1500, 200, "256 x 1500")
    plan.close()
    lines = ["%s  %s -> %s, %s  [%s]" % (name, " ".join(map(str, mcli)),
                                         " ".join(map(str, ccli)),
                                         "int16" if i16 else "int32",
                                         "fused, two launches" if fused else "fallback")]
    stat = {}
    for k, _ in legs:
        v = rates[k]
        stat[k] = (v[0], v[-1])
        lines.append("    %-9s  min %7.1f  max %7.1f Gsample/s" % (k, v[0], v[-1]))
    a, b = stat["receiver"], stat["two calls"]
    lines.append("    (a) / (b): best against best %.2f, range %.2f .. %.2f"
                 % (a[1] / b[1], a[0] / b[1], a[1] / b[0]))
    c, d = big["rx bank"], big["two banks"]
    lines.append("    1024 blocks x 2^16 [%d spans, fused %d]: rx bank %.1f .. %.1f, two "
                 "banks %.1f .. %.1f Gsample/s" % (big_info["spans"], big_info["fused"],
                                                   c[0], c[-1], d[0], d[-1]))
    lines.append("    (c) / (d): best against best %.2f, range %.2f .. %.2f"
                 % (c[-1] / d[-1], c[0] / d[-1], c[-1] / d[0]))
    us = lambda v: 256 * 1500 / (v * 1e9) * 1e6     # a round's time from its rate
    e, f = small["rx bank"], small["two banks"]
    lines.append("    256 blocks x 1500, 200 rounds back to back [%d spans]: rx bank %.1f "
                 ".. %.1f us a round, two banks %.1f .. %.1f"
                 % (small_info["spans"], us(e[-1]), us(e[0]), us(f[-1]), us(f[0])))
    lines.append("    (e) / (f): best against best %.2f, range %.2f .. %.2f"
                 % (e[-1] / f[-1], e[0] / f[-1], e[-1] / f[0]))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--log2-n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if not 10 <= a.log2_n <= 28:
        ap.error("--log2-n 10 .. 28")
    sys.path.insert(0, TOOLS)
    import bench_common as B
    import torch
    import build_stamp

    n = 1 << a.log2_n
    gen = torch.Generator(device=torch.device("cuda:0"))
    gen.manual_seed(0x5eed)
    st = build_stamp.stamp()
    lines = ["%s, commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
        torch.cuda.get_device_name(0), st["git_head"],
        " + uncommitted changes" if st["git_dirty"] else "",
        st["kernel_sources_sha256"], st["lib_sha256"]),
        "2^%d samples, random tuning words, random full-scale I/Q, a d_acc and a "
        "d_last word; HIP events around %d runs of a leg, legs alternated, min - max "
        "of %d repetitions after one warm-up of every leg; one process; the receiver "
        "checked against the two calls on every sample and both words first"
        % (a.log2_n, a.steps, a.reps)]
    print("\n".join(lines), flush=True)
    pairs = [("cfg2-cfg3", B.WORKLOADS["cfg2"]["cli"], CFG3, False),
             ("nat24-natr2p24", B.WORKLOADS["nat24"]["cli"], NATR2P24, False),
             ("cfg1-io16", CFG1, IO16, True)]
    for name, mcli, ccli, i16 in pairs:
        part = measure(name, mcli, ccli, i16, n, a.reps, a.steps, gen)
        print("\n".join(part), flush=True)
        lines += part
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
