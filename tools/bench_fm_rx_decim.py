#!/usr/bin/env python3
"""bench_fm_rx_decim.py -- the decimating FM receiver (cordic_plan_fm_rx_decim,
_decim16) and the decimating receiver banks against what a caller did before
them: the decimating mixer into two arrays and the discriminator from them.

Per core pair, in ONE process of its own (a fresh child of this tool), on 2^28
INPUT samples (--log2-n) of random tuning words and random full-scale I/Q,
with a d_acc and a d_last word:

  (a) receiver   one cordic_plan_fm_rx_decim call, at k = 2 and at k = 6
  (b) two calls  cordic_plan_fm_mix_decim + cordic_fm_demod on the same inputs,
                 the decimated I/Q in two arrays of their own

  (c) rx bank    1024 blocks x 2^16 samples at k = 3, each with both words, one
                 cordic_rxbank_run of a decimating receiver bank
  (d) two banks  a decimating cordic_mixbank_run and a cordic_demodbank_run over
                 the same blocks
  (e) rx bank    256 blocks x 1536 samples at k = 3, 200 runs back to back,
                 time per round
  (f) two banks  the same round through the two banks

Rates are in INPUT samples.  Before any timing the outputs and all words of
(a), (c), (e) are checked on every sample against those of (b), (d), (f).
Timing: HIP events around `steps` runs of a leg, the legs alternated within
every repetition, one warm-up repetition, then --reps (>= 5) timed ones; min -
max over the repetitions.  (b), (d), (f) are kernels this tool's subject does
not change.  Required: best against best >= 0.97 for (a) / (b) and (c) / (d),
> 1.00 for (e) / (f); a miss is reported as MISSED with its numbers.

  python tools/bench_fm_rx_decim.py --out profiles/r23/fm_rx_decim.txt
"""
import argparse
import os
import subprocess
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
CFG3 = ("r2p", 24, 24, 2, -1, 20)
NATR2P24 = ("r2p", 24, 24, 2, -1, -1)
CFG1 = ("p2r", 16, 16, 2, 16, 16)
IO16 = ("r2p", 16, 16, 2, 16, -1)


def pairs():
    import bench_common as B
    return {"cfg2-cfg3": (B.WORKLOADS["cfg2"]["cli"], CFG3, False),
            "nat24-natr2p24": (B.WORKLOADS["nat24"]["cli"], NATR2P24, False),
            "cfg1-io16": (CFG1, IO16, True)}


def verdict(ratio, need, strict):
    ok = ratio > need if strict else ratio >= need
    return "ok" if ok else "MISSED (required %s %.2f)" % (">" if strict else ">=", need)


def measure(name, mcli, ccli, i16, n, reps, steps):
    import bench_common as B
    import torch
    import cordic_amd as ca

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    mcfg = ca.Config.from_cli(B.MODE[mcli[0]], *mcli[1:])
    ccfg = ca.Config.from_cli(B.MODE[ccli[0]], *ccli[1:])
    plan = ca.Plan(mcfg)
    dt = torch.int16 if i16 else torch.int32
    half = 1 << (mcfg.iw - 1)
    fcw = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device=dev,
                        generator=gen)
    x, y = (torch.randint(-half, half, (n,), dtype=torch.int32, device=dev,
                          generator=gen).to(dt) for _ in range(2))
    # outputs and the two calls' decimated I/Q: n / 2 elements hold every k >= 1
    mag, freq, tx, ty = (torch.empty(n // 2, dtype=dt, device=dev) for _ in range(4))
    words = torch.zeros(8, dtype=torch.int32, device=dev)
    acc, last = words[0:], words[4:]
    z = lambda b: torch.zeros(max(16, b), dtype=torch.uint8, device=dev)
    rxd, mixd = ((plan.fm_rx_decim16, plan.fm_mix_decim16) if i16
                 else (plan.fm_rx_decim, plan.fm_mix_decim))
    wsrx = plan.fm_rx_decim16_workspace if i16 else plan.fm_rx_decim_workspace
    wsmix = plan.fm_mix_decim16_workspace if i16 else plan.fm_mix_decim_workspace
    fused = (plan.fm_rx16_info if i16 else plan.fm_rx_info)(ccfg)[0]

    def timed(legs, count, samples):
        """per leg the sorted rates (input Gsample/s)"""
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

    lines = ["%s  %s -> %s, %s  [%s]" % (name, " ".join(map(str, mcli)),
                                         " ".join(map(str, ccli)),
                                         "int16" if i16 else "int32",
                                         "fused, two launches" if fused else "fallback")]
    # ---- (a) / (b)
    for k in (2, 6):
        m = n >> k
        wrx, wmix, wdem = z(wsrx(ccfg, n, k)), z(wsmix(n, k)), z(ca.fm_demod_workspace(m))

        def receiver():
            rxd(ccfg, k, fcw, x, y, mag, freq, wrx, n=n, acc=acc, last=last)

        def two_calls():
            mixd(k, fcw, x, y, tx, ty, wmix, n=n, acc=acc)
            ca.fm_demod(ccfg, tx, ty, mag, freq, wdem, n=m, last=last)

        words.zero_(); mag.fill_(-1); freq.fill_(-1)
        two_calls()
        torch.cuda.synchronize()
        mref, fref, wref = mag[:m].clone(), freq[:m].clone(), words.clone()
        words.zero_(); mag.fill_(-1); freq.fill_(-1)
        receiver()
        torch.cuda.synchronize()
        if not (torch.equal(mag[:m], mref) and torch.equal(freq[:m], fref)
                and torch.equal(words, wref) and bool((mag[m:] == -1).all())):
            raise SystemExit("%s k = %d: the receiver differs from the two calls" % (name, k))
        del mref, fref, wref
        r = timed([("receiver", receiver), ("two calls", two_calls)], steps, n)
        a, b = r["receiver"], r["two calls"]
        lines.append("    k = %d: receiver %.1f .. %.1f, two calls %.1f .. %.1f input "
                     "Gsample/s" % (k, a[0], a[-1], b[0], b[-1]))
        q = a[-1] / b[-1]
        lines.append("    (a) / (b) at k = %d: best against best %.2f, range %.2f .. %.2f: %s"
                     % (k, q, a[0] / b[-1], a[-1] / b[0], verdict(q, 0.97, False)))

    # ---- the banks at k = 3
    def banks(blocks, length, count, what):
        k = 3
        tot, dl = blocks * length, length >> k
        view = lambda t, j: t[j * length:(j + 1) * length]
        dview = lambda t, j: t[j * dl:(j + 1) * dl]
        wds = torch.zeros(8 * blocks, dtype=torch.int32, device=dev)
        rxj = [(view(fcw, j), None, view(x, j), view(y, j), dview(mag, j), dview(freq, j),
                length, 0, wds[8 * j:], 0, wds[8 * j + 4:]) for j in range(blocks)]
        mxj = [(view(fcw, j), None, view(x, j), view(y, j), dview(tx, j), dview(ty, j),
                length, 0, wds[8 * j:]) for j in range(blocks)]
        dmj = [(dview(tx, j), dview(ty, j), dview(mag, j), dview(freq, j), dl, 0,
                wds[8 * j + 4:]) for j in range(blocks)]
        rxb = (ca.RxBank16 if i16 else ca.RxBank)(plan, ccfg, rxj, log2r=k)
        mxb = (ca.MixBank16 if i16 else ca.MixBank)(plan, mxj, log2r=k)
        dmb = (ca.DemodBank16 if i16 else ca.DemodBank)(ccfg, dmj)

        def two_banks():
            mxb.run()
            dmb.run()

        md = tot >> k
        wds.zero_(); mag[:md].fill_(-1); freq[:md].fill_(-1)
        two_banks()
        torch.cuda.synchronize()
        ref = (mag[:md].clone(), freq[:md].clone(), wds.clone())
        wds.zero_(); mag[:md].fill_(-1); freq[:md].fill_(-1)
        rxb.run()
        torch.cuda.synchronize()
        if not (torch.equal(mag[:md], ref[0]) and torch.equal(freq[:md], ref[1])
                and torch.equal(wds, ref[2])):
            raise SystemExit("%s: the rx bank differs from the two banks (%s)"
                             % (name, what))
        info = rxb.info()
        r = timed([("rx bank", rxb.run), ("two banks", two_banks)], count, tot)
        rxb.close(); mxb.close(); dmb.close()
        return r, info

    big_len = min(1 << 16, n // 1024)
    big, big_info = banks(1024, big_len, 10, "1024 blocks")
    small, small_info = banks(256, 1536, 200, "256 x 1536")
    plan.close()
    c, d = big["rx bank"], big["two banks"]
    lines.append("    1024 blocks x %d at k = 3 [%d spans, fused %d]: rx bank %.1f .. %.1f, "
                 "two banks %.1f .. %.1f input Gsample/s"
                 % (big_len, big_info["spans"], big_info["fused"], c[0], c[-1], d[0], d[-1]))
    q = c[-1] / d[-1]
    lines.append("    (c) / (d): best against best %.2f, range %.2f .. %.2f: %s"
                 % (q, c[0] / d[-1], c[-1] / d[0], verdict(q, 0.97, False)))
    us = lambda v: 256 * 1536 / (v * 1e9) * 1e6     # a round's time from its rate
    e, f = small["rx bank"], small["two banks"]
    lines.append("    256 blocks x 1536 at k = 3, 200 rounds back to back [%d spans]: rx "
                 "bank %.1f .. %.1f us a round, two banks %.1f .. %.1f"
                 % (small_info["spans"], us(e[-1]), us(e[0]), us(f[-1]), us(f[0])))
    q = e[-1] / f[-1]
    lines.append("    (e) / (f): best against best %.2f, range %.2f .. %.2f: %s"
                 % (q, e[0] / f[-1], e[-1] / f[0], verdict(q, 1.0, True)))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--log2-n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--pair", default=None, help="(the tool's own: one pair, this process)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if not 12 <= a.log2_n <= 28:
        ap.error("--log2-n 12 .. 28")
    sys.path.insert(0, TOOLS)
    if a.pair:
        mcli, ccli, i16 = pairs()[a.pair]
        print("\n".join(measure(a.pair, mcli, ccli, i16, 1 << a.log2_n, a.reps, a.steps)),
              flush=True)
        return 0
    import torch
    import build_stamp

    st = build_stamp.stamp()
    lines = ["%s, commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
        torch.cuda.get_device_name(0), st["git_head"],
        " + uncommitted changes" if st["git_dirty"] else "",
        st["kernel_sources_sha256"], st["lib_sha256"]),
        "2^%d input samples, random tuning words, random full-scale I/Q, a d_acc and a "
        "d_last word; HIP events around %d runs of a leg, legs alternated, min - max of "
        "%d repetitions after one warm-up of every leg; one process per pair; the "
        "receiver checked against the two calls on every sample and both words first; "
        "rates in INPUT samples" % (a.log2_n, a.steps, a.reps)]
    print("\n".join(lines), flush=True)
    for name in pairs():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pair", name,
                            "--log2-n", str(a.log2_n), "--reps", str(a.reps),
                            "--steps", str(a.steps)], capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode:
            sys.stderr.write(r.stderr[-3000:])
            return r.returncode
        lines += r.stdout.rstrip("\n").split("\n")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
