#!/usr/bin/env python3
"""bench_table_fm.py -- the table and quadratic sine cores as frequency-
modulated oscillators (cordic_table_fm / cordic_quad_fm) against the two-call
path they replace: cordic_phase_accumulate into a phase array, then the lookup.

For each of bench.py's table workloads (sintbl, qtrtbl16, qtrtbl24, qtrtbl,
quadtbl; parameters from its workload table, tools/bench_common.py) one child
process, under a time limit of its own, measures on 2^28 samples with random
full-range tuning words:

  (a) fm          the fused call, sine only (read 4 + 4 B: the tuning words are
                  read by the reduction and again by the scan; write 4 B)
  (b) fm iq       sine and cosine (read 8, write 8 B)
  (c) fm16 / fm16 iq   the int16 forms where OW <= 16 (read 8, write 2 / 4 B)
  (d) acc+lookup  cordic_phase_accumulate into a phase array, then
                  cordic_*_lookup on it (4 + 4 + 4, then 4 + 4 B)
  (e) nco         the pure-tone oscillator beside them (write 4 B)
  (f) accumulate  cordic_phase_accumulate alone (read 8, write 4 B), and
      copy        a device-to-device copy that moves the same 12 B per sample
                  (1.5 words read, 1.5 written), in the same run

Before any timing the child checks on all samples that (a), (b) and (c) hold
exactly the values of (d) (the cosine: the lookup on the phases moved a
quarter turn).  Timing: HIP events around 10 calls, the legs alternated within
every repetition, one warm-up repetition, then --reps (>= 5) timed ones; min /
median / max over the repetitions.  A child that fails ends the run: nothing
more is started on the GPU.

  python tools/bench_table_fm.py --out profiles/r10/table_fm.txt
"""
import argparse
import json
import os
import subprocess
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
NAMES = ("sintbl", "qtrtbl16", "qtrtbl24", "qtrtbl", "quadtbl")
STEPS = 10


def child(name, log2n, reps):
    import bench_common as B            # the workload table bench.py runs
    import torch
    import cordic_amd as ca
    import build_stamp

    w = B.WORKLOADS[name]
    core = ca.Table(*w["table"]) if "table" in w else ca.Quad(*w["quad"])
    layout = ("lds mode %d" % core.lds_mode) if "table" in w else "quad, lds"
    n = 1 << log2n
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5eed)
    # (full-range words: drawn in 64 bits, the low 32 kept)
    fcw = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device=dev,
                        generator=gen).to(torch.int32)
    phase = torch.empty(n, dtype=torch.int32, device=dev)
    ref = torch.empty(n, dtype=torch.int32, device=dev)
    s = torch.empty(n, dtype=torch.int32, device=dev)
    c = torch.empty(n, dtype=torch.int32, device=dev)
    s16, c16 = s.view(torch.int16)[:n], c.view(torch.int16)[:n]
    has16 = core.ow <= 16
    work = torch.zeros(max(16, ca.fm_workspace(n)), dtype=torch.uint8, device=dev)
    phase0 = 0x12345678

    # ---- the outputs first: fused == accumulate + lookup on every sample
    def same(a, b, what):
        if not torch.equal(a, b):
            raise SystemExit("%s: %s differs from accumulate + lookup"
                             % (name, what))
    ca.phase_accumulate(fcw, phase, phase0=phase0, work=work)
    core.lookup(phase, ref)
    s.fill_(-1)
    core.fm(fcw, s, None, phase0=phase0, work=work)
    same(s, ref, "fm sin")
    s.fill_(-1); c.fill_(-1)
    core.fm(fcw, s, c, phase0=phase0, work=work)
    same(s, ref, "fm iq sin")
    if has16:
        ref16 = ref.to(torch.int16)
        core.fm(fcw, s16, None, phase0=phase0, work=work)
        same(s16, ref16, "fm16 sin")
        s16.fill_(-1)
        core.fm(fcw, s16, c16, phase0=phase0, work=work)
        same(s16, ref16, "fm16 iq sin")
        del ref16
        core.fm(fcw, s, c, phase0=phase0, work=work)
    quarter = 1 << (core.pw - 2)
    if quarter >= 1 << 31:
        quarter -= 1 << 32
    phase.add_(quarter)                 # (wraps: the core takes the low PW bits)
    core.lookup(phase, ref)
    same(c, ref, "fm iq cos")
    if has16:
        core.fm(fcw, s16, c16, phase0=phase0, work=work)
        same(c16, ref.to(torch.int16), "fm16 iq cos")
    torch.cuda.synchronize()

    # the copy of the same bytes as the accumulator moves: 12 B per sample
    half = 3 * n // 4
    dst = ref
    del ref

    def two_calls():
        ca.phase_accumulate(fcw, phase, phase0=phase0, work=work)
        core.lookup(phase, s)

    def copy():
        # 3n/2 words in two pieces (the arrays hold n words each)
        dst[:half].copy_(fcw[:half])
        c[:half].copy_(phase[:half])

    legs = [("fm", 12, lambda: core.fm(fcw, s, None, phase0=phase0, work=work)),
            ("fm iq", 16, lambda: core.fm(fcw, s, c, phase0=phase0, work=work)),
            ("acc+lookup", 20, two_calls),
            ("nco", 4, lambda: core.nco(s, None, phase0=phase0, fcw=0x9e3779b1)),
            ("accumulate", 12, lambda: ca.phase_accumulate(
                fcw, phase, phase0=phase0, work=work)),
            ("copy", 12, copy)]
    if has16:
        legs[2:2] = [("fm16", 10, lambda: core.fm(fcw, s16, None, phase0=phase0,
                                                  work=work)),
                     ("fm16 iq", 12, lambda: core.fm(fcw, s16, c16,
                                                     phase0=phase0, work=work))]
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
    st = build_stamp.stamp()
    out = dict(name=name, desc=w["desc"], layout=layout, log2n=log2n, reps=reps,
               device=torch.cuda.get_device_name(0),
               kernel_sources_sha256=st["kernel_sources_sha256"],
               legs=[dict(leg=k, bytes=b, rates=sorted(rates[k]))
                     for k, b, _ in legs])
    print("RESULT " + json.dumps(out), flush=True)
    core.close()


def fmt(r):
    v = r["rates"]
    med = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    return med, "%-10s %2d B/sample  min %7.1f  median %7.1f  max %7.1f Gsample/s  (%5.2f TB/s)" % (
        r["leg"], r["bytes"], v[0], med, v[-1], med * r["bytes"] / 1e3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--log2-samples", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma-separated workloads")
    ap.add_argument("--limit", type=int, default=150,
                    help="seconds one workload's process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if not 10 <= a.log2_samples <= 28:
        ap.error("--log2-samples: 10 .. 28")
    sys.path.insert(0, TOOLS)
    if a.child:
        child(a.child, a.log2_samples, a.reps)
        return 0
    names = a.only.split(",") if a.only else NAMES
    lines = []
    slow = []
    for name in names:
        if name not in NAMES:
            ap.error("unknown workload %r" % name)
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable,
                            os.path.abspath(__file__), "--child", name,
                            "--log2-samples", str(a.log2_samples),
                            "--reps", str(a.reps)],
                           stdout=subprocess.PIPE, text=True)
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            sys.stderr.write(p.stdout)
            sys.stderr.write("%s: child ended with status %d; stopping\n"
                             % (name, p.returncode))
            return 1
        r = json.loads(res[-1][7:])
        first = len(lines)
        if not lines:
            lines.append("%s, kernel_sources_sha256 %s" % (
                r["device"], r["kernel_sources_sha256"]))
            lines.append("2^%d samples, random tuning words; HIP events around %d "
                         "calls, legs alternated, %d repetitions after one "
                         "warm-up of every leg; outputs checked against "
                         "accumulate + lookup on every sample first"
                         % (r["log2n"], STEPS, r["reps"]))
        lines.append("%s  %s  [%s]" % (name, r["desc"], r["layout"]))
        med, by = {}, {}
        for leg in r["legs"]:
            med[leg["leg"]], text = fmt(leg)
            by[leg["leg"]] = leg["rates"]
            lines.append("    " + text)
        ratio = med["fm"] / med["acc+lookup"]
        lines.append("    fm / (acc+lookup) = %.2fx (medians; the bytes allow "
                     "20/12 = 1.67x); slowest fm repetition %s fastest "
                     "acc+lookup repetition; accumulate / copy = %.2fx"
                     % (ratio, ">" if by["fm"][0] > by["acc+lookup"][-1] else "<=",
                        med["accumulate"] / med["copy"]))
        if ratio <= 1.0:
            slow.append(name)
        if ratio < 1.2:
            lines.append("    ** fm / (acc+lookup) is under 1.2: say below what "
                         "held it **")
        print("\n".join(lines[first:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    if slow:
        sys.stderr.write("fused fm is not faster than accumulate + lookup on: %s\n"
                         % ", ".join(slow))
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
