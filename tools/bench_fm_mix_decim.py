#!/usr/bin/env python3
"""bench_fm_mix_decim.py -- the decimating FM mixer (cordic_plan_fm_mix_decim,
cordic_mixbank_create_decim) against the mixer it is made of and against what a
caller composed before it.

Single calls, per core in ONE process, on 2^28 samples of random tuning words
and random full-scale I/Q -- cfg2 (the `ddc` workload's core), n20, nat24 on
int32 arrays and cfg1's core on int16 arrays:

  (a) decim k=2, k=6   the call under test, fused: fcw read twice, x and y
                       read, n >> k outputs written: 16 + 8 / R bytes per
                       sample (int16: 12 + 4 / R)
  (b) fm_mix           cordic_plan_fm_mix (_mix16) on the same inputs: 24 bytes
                       per sample (int16: 16)
  (c) mix+sum k=2, 6   the fallback composition, forced with
                       CORDIC_FMXD_FALLBACK=1: the mixer into two full-rate
                       arrays inside the workspace, then the elementwise sum

Banks: (d) a decimating bank of 1024 jobs of 2^16 samples at k = 3 against (e)
cordic_mixbank on the same jobs, on cfg2 (int32) and cfg1's core (int16).

Before any timing every output sample of (a), (c) and (d) is compared with the
sums of (b)'s / (e)'s outputs made by torch in 64 bits.  Timing: HIP events
around 10 calls (4 bank runs), the legs alternated within every repetition, one
warm-up repetition, then --reps (>= 5) timed ones; min and max over the
repetitions, rates in INPUT samples per second.  Required: best (a) / best (b)
>= 0.97 on every core, best (d) / best (e) >= 0.97; exit status 2 where one is
missed.

  python tools/bench_fm_mix_decim.py --out profiles/r22/fm_mix_decim.txt
"""
import argparse
import os
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
STEPS, BANK_STEPS = 10, 4
N20 = ("p2r", 32, 32, 2, 32, 20)
KNOB = "CORDIC_FMXD_FALLBACK"
MARGIN = 0.97


def sums(torch, t, k):
    """floor(the sum of 2^k consecutive values / 2^k), in 64 bits"""
    return (t.view(-1, 1 << k).sum(dim=1, dtype=torch.int64) >> k).to(t.dtype)


def timed(torch, legs, reps, steps, n):
    """{leg: sorted Gsample/s of the repetitions}, the legs alternated"""
    rates = {k: [] for k, _ in legs}
    for rep in range(reps + 1):         # rep 0: warm-up of every leg
        for k, run in legs:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                run()
            e1.record()
            e1.synchronize()
            if rep:
                rates[k].append(n * steps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return {k: sorted(v) for k, v in rates.items()}


def single(name, cli, desc, i16, n, reps, fcw, gen):
    import bench_common as B
    import torch
    import cordic_amd as ca

    cfg = ca.Config.from_cli(B.MODE[cli[0]], *cli[1:])
    plan = ca.Plan(cfg)
    dt = torch.int16 if i16 else torch.int32
    dev = fcw.device
    half = 1 << (cfg.iw - 1)
    x = torch.randint(-half, half, (n,), dtype=torch.int32, device=dev, generator=gen).to(dt)
    y = torch.randint(-half, half, (n,), dtype=torch.int32, device=dev, generator=gen).to(dt)
    ox, oy = torch.empty(n, dtype=dt, device=dev), torch.empty(n, dtype=dt, device=dev)
    mix = plan.fm_mix16 if i16 else plan.fm_mix
    dec = plan.fm_mix_decim16 if i16 else plan.fm_mix_decim
    ws = plan.fm_mix_decim16_workspace if i16 else plan.fm_mix_decim_workspace
    mws = plan.fm_mix16_workspace if i16 else plan.fm_mix_workspace
    os.environ.pop(KNOB, None)
    fused = ws(n, 2) == mws(n)
    os.environ[KNOB] = "1"
    work = torch.zeros(max(16, ws(n, 2), mws(n)), dtype=torch.uint8, device=dev)
    os.environ.pop(KNOB, None)
    phase0 = 0x9e3779b1
    outs = {k: (torch.empty(n >> k, dtype=dt, device=dev),
                torch.empty(n >> k, dtype=dt, device=dev)) for k in (2, 6)}

    def fallback(k):
        os.environ[KNOB] = "1"
        try:
            dec(k, fcw, x, y, outs[k][0], outs[k][1], work, phase0=phase0)
        finally:
            os.environ.pop(KNOB, None)

    # ---- every output sample first
    mix(fcw, x, y, ox, oy, work, phase0=phase0)
    for k in (2, 6):
        wx, wy = sums(torch, ox, k), sums(torch, oy, k)
        for tag, run in (("decim", lambda: dec(k, fcw, x, y, outs[k][0], outs[k][1], work,
                                               phase0=phase0)),
                         ("mix+sum", lambda: fallback(k))):
            outs[k][0].fill_(-1); outs[k][1].fill_(-1)
            run()
            if not torch.equal(outs[k][0], wx) or not torch.equal(outs[k][1], wy):
                raise SystemExit("%s: %s k=%d differs from the sums of fm_mix" % (name, tag, k))
        del wx, wy
    torch.cuda.synchronize()

    legs = [("decim k=2", lambda: dec(2, fcw, x, y, outs[2][0], outs[2][1], work,
                                      phase0=phase0)),
            ("decim k=6", lambda: dec(6, fcw, x, y, outs[6][0], outs[6][1], work,
                                      phase0=phase0)),
            ("fm_mix", lambda: mix(fcw, x, y, ox, oy, work, phase0=phase0)),
            ("mix+sum k=2", lambda: fallback(2)),
            ("mix+sum k=6", lambda: fallback(6))]
    r = timed(torch, legs, reps, STEPS, n)
    es = 2 if i16 else 4
    full = 8 + 4 * es                   # fcw twice, x, y, two outputs
    byts = {"decim k=2": 8 + 2 * es + 2 * es / 4, "decim k=6": 8 + 2 * es + 2 * es / 64,
            "fm_mix": full, "mix+sum k=2": full + 2 * es + 2 * es / 4,
            "mix+sum k=6": full + 2 * es + 2 * es / 64}
    lines = ["%s  %s  [%s, %s]" % (name, desc, "int16" if i16 else "int32",
                                   "fused" if fused else "fallback")]
    for k, _ in legs:
        v = r[k]
        lines.append("    %-12s %5.2f B/sample  min %7.1f  max %7.1f Gsample/s in  "
                     "(%5.2f TB/s at the best)" % (k, byts[k], v[0], v[-1],
                                                   v[-1] * byts[k] / 1e3))
    best_a = max(r["decim k=2"][-1], r["decim k=6"][-1])
    best_b = r["fm_mix"][-1]
    ok = best_a / best_b >= MARGIN
    lines.append("    best decim / best fm_mix = %.3f (k=2: %.3f, k=6: %.3f; the bytes allow "
                 "%.2f and %.2f); best decim / best mix+sum: k=2 %.2fx, k=6 %.2fx"
                 % (best_a / best_b, r["decim k=2"][-1] / best_b, r["decim k=6"][-1] / best_b,
                    full / byts["decim k=2"], full / byts["decim k=6"],
                    r["decim k=2"][-1] / r["mix+sum k=2"][-1],
                    r["decim k=6"][-1] / r["mix+sum k=6"][-1]))
    plan.close()
    return lines, ok and r["decim k=2"][-1] / best_b >= MARGIN \
        and r["decim k=6"][-1] / best_b >= MARGIN


def bank(name, cli, desc, i16, reps, gen, dev):
    import bench_common as B
    import torch
    import cordic_amd as ca

    cfg = ca.Config.from_cli(B.MODE[cli[0]], *cli[1:])
    plan = ca.Plan(cfg)
    J, L, k = 1024, 1 << 16, 3
    n = J * L
    dt = torch.int16 if i16 else torch.int32
    half = 1 << (cfg.iw - 1)
    fcw = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device=dev,
                        generator=gen)
    x = torch.randint(-half, half, (n,), dtype=torch.int32, device=dev, generator=gen).to(dt)
    y = torch.randint(-half, half, (n,), dtype=torch.int32, device=dev, generator=gen).to(dt)
    ox, oy = torch.empty(n, dtype=dt, device=dev), torch.empty(n, dtype=dt, device=dev)
    dx = torch.empty(n >> k, dtype=dt, device=dev)
    dy = torch.empty(n >> k, dtype=dt, device=dev)
    M = L >> k
    v = lambda t, j, l: t[j * l:(j + 1) * l]
    Bank = ca.MixBank16 if i16 else ca.MixBank
    full = Bank(plan, [(v(fcw, j, L), None, v(x, j, L), v(y, j, L), v(ox, j, L), v(oy, j, L),
                        L, 0x9e3779b1, None) for j in range(J)])
    dec = Bank(plan, [(v(fcw, j, L), None, v(x, j, L), v(y, j, L), v(dx, j, M), v(dy, j, M),
                       L, 0x9e3779b1, None) for j in range(J)], log2r=k)
    full.run()
    dx.fill_(-1); dy.fill_(-1)
    dec.run()
    if not torch.equal(dx, sums(torch, ox, k)) or not torch.equal(dy, sums(torch, oy, k)):
        raise SystemExit("%s: the decimating bank differs from the sums of the bank" % name)
    torch.cuda.synchronize()
    r = timed(torch, [("decim bank", dec.run), ("mix bank", full.run)], reps, BANK_STEPS, n)
    info = dec.info()
    lines = ["%s  %s  [%s, %d jobs x 2^16, k = %d, %s, %d spans of %d]"
             % (name, desc, "int16" if i16 else "int32", J, k,
                "fused" if info["fused"] else "one by one", info["spans"], info["tile"])]
    for leg in ("decim bank", "mix bank"):
        lines.append("    %-12s min %7.1f  max %7.1f Gsample/s in" % (leg, r[leg][0], r[leg][-1]))
    ratio = r["decim bank"][-1] / r["mix bank"][-1]
    lines.append("    best decim bank / best mix bank = %.3f" % ratio)
    full.close(); dec.close(); plan.close()
    return lines, ratio >= MARGIN


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--log2-samples", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-banks", action="store_true")
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
    st = build_stamp.stamp()
    lines = ["%s, commit %s%s, kernel_sources_sha256 %s, lib_sha256 %s" % (
        torch.cuda.get_device_name(0), st["git_head"],
        " + uncommitted changes" if st["git_dirty"] else "",
        st["kernel_sources_sha256"], st["lib_sha256"]),
        "single calls: 2^%d samples, random tuning words, random full-scale I/Q; HIP "
        "events around %d calls, legs alternated, %d repetitions after one warm-up of "
        "every leg; one process; every output sample of the decimating call and of the "
        "forced fallback compared with 64-bit sums of fm_mix's outputs first; rates in "
        "input samples" % (a.log2_samples, STEPS, a.reps)]
    print("\n".join(lines), flush=True)
    missed = []
    for name, cli, desc, i16 in (
            ("cfg2", B.WORKLOADS["cfg2"]["cli"], "basiccordic 16-stage, 32-bit: the core of "
             "the `ddc` workload", False),
            ("n20", N20, "basiccordic 20-stage, 32-bit", False),
            ("nat24", B.WORKLOADS["nat24"]["cli"], "gencordic -t p2r -i 24 -o 24: WW27 PW31, "
             "27 stages", False),
            ("cfg1", B.WORKLOADS["cfg1"]["cli"], "basiccordic 16-bit: WW19 PW16, 13 live "
             "stages", True)):
        part, ok = single(name, cli, desc, i16, n, a.reps, fcw, gen)
        print("\n".join(part), flush=True)
        lines += part
        if not ok:
            missed.append(name)
    del fcw
    torch.cuda.empty_cache()
    if not a.no_banks:
        lines.append("banks: HIP events around %d runs, legs alternated, %d repetitions "
                     "after one warm-up" % (BANK_STEPS, a.reps))
        print(lines[-1], flush=True)
        for name, cli, desc, i16 in (
                ("cfg2", B.WORKLOADS["cfg2"]["cli"], "basiccordic 16-stage, 32-bit", False),
                ("cfg1", B.WORKLOADS["cfg1"]["cli"], "basiccordic 16-bit", True)):
            part, ok = bank(name, cli, desc, i16, a.reps, gen, dev)
            print("\n".join(part), flush=True)
            lines += part
            if not ok:
                missed.append(name + " bank")
    lines.append("required (best decimating / best full-rate >= %.2f at k = 2 and k = 6 on "
                 "every core, and for the banks): %s"
                 % (MARGIN, "met" if not missed else "** MISSED on %s **" % ", ".join(missed)))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 2 if missed else 0       # (a script can tell a miss from a pass)


if __name__ == "__main__":
    sys.exit(main())
