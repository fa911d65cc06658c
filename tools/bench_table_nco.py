#!/usr/bin/env python3
"""bench_table_nco.py -- the table and quadratic sine cores as oscillators
(cordic_table_nco / cordic_quad_nco) against the lookup on a stored phase ramp.

For each of bench.py's table workloads (sintbl, qtrtbl, qtrtbl16, qtrtbl24,
quadtbl, quadtbl24; parameters from its workload table, tools/bench_common.py)
one child process, under a time limit of its own, measures on 2^30 samples:

  (a) lookup    cordic_*_lookup on a device array holding the ramp (read 4 B,
                write 4 B per sample; filling the ramp is NOT charged)
  (b) nco       the oscillator, sine only (write 4 B)
  (c) nco iq    the oscillator, sine and cosine (write 8 B)
  (d) nco16 / nco16 iq   the int16 forms where OW <= 16 (write 2 / 4 B)

Before any timing the child checks on the whole ramp that (b), (c) and (d)
hold exactly the lookup's values (the cosine: the lookup on the ramp moved a
quarter turn).  Timing: HIP events around 20 calls, the legs alternated within
every repetition, one warm-up repetition, then --reps (>= 5) timed ones;
min / median / max over the repetitions.  A child that fails ends the run:
nothing more is started on the GPU.

  python tools/bench_table_nco.py --out profiles/r08/table_nco.txt
"""
import argparse
import json
import os
import subprocess
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
NAMES = ("sintbl", "qtrtbl16", "qtrtbl24", "qtrtbl", "quadtbl", "quadtbl24")
STEPS = 20


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
    phase = torch.empty(n, dtype=torch.int32, device=dev)
    ref = torch.empty(n, dtype=torch.int32, device=dev)
    s = torch.empty(n, dtype=torch.int32, device=dev)
    c = torch.empty(n, dtype=torch.int32, device=dev)
    s16, c16 = s.view(torch.int16)[:n], c.view(torch.int16)[:n]
    has16 = core.ow <= 16
    ca.fill_phase_ramp(phase, 0, w["shift"])

    # ---- the outputs first: oscillator == lookup on the same ramp
    def same(a, b, what):
        if not torch.equal(a, b):
            raise SystemExit("%s: %s differs from the lookup" % (name, what))
    core.lookup(phase, ref)
    s.fill_(-1)
    core.nco(s, None)
    same(s, ref, "nco sin")
    s.fill_(-1); c.fill_(-1)
    core.nco(s, c)
    same(s, ref, "nco iq sin")
    if has16:
        ref16 = ref.to(torch.int16)
        core.nco(s16, None)
        same(s16, ref16, "nco16 sin")
        s16.fill_(-1)
        core.nco(s16, c16)
        same(s16, ref16, "nco16 iq sin")
        del ref16
        core.nco(s, c)
    quarter = 1 << (core.pw - 2)
    if quarter >= 1 << 31:
        quarter -= 1 << 32
    phase.add_(quarter)                 # (wraps: the core takes the low PW bits)
    core.lookup(phase, ref)
    phase.sub_(quarter)
    same(c, ref, "nco iq cos")
    if has16:
        core.nco(s16, c16)
        same(c16, ref.to(torch.int16), "nco16 iq cos")
    torch.cuda.synchronize()

    legs = [("lookup", 8, lambda: core.lookup(phase, ref)),
            ("nco", 4, lambda: core.nco(s, None)),
            ("nco iq", 8, lambda: core.nco(s, c))]
    if has16:
        legs += [("nco16", 2, lambda: core.nco(s16, None)),
                 ("nco16 iq", 4, lambda: core.nco(s16, c16))]
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
    return med, "%-9s %d B/sample  min %7.1f  median %7.1f  max %7.1f Gsample/s  (%5.2f TB/s)" % (
        r["leg"], r["bytes"], v[0], med, v[-1], med * r["bytes"] / 1e3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--log2-samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma-separated workloads")
    ap.add_argument("--limit", type=int, default=240,
                    help="seconds one workload's process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if not 10 <= a.log2_samples <= 30:
        ap.error("--log2-samples: 10 .. 30")
    sys.path.insert(0, TOOLS)
    if a.child:
        child(a.child, a.log2_samples, a.reps)
        return 0
    names = a.only.split(",") if a.only else NAMES
    lines = []
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
            lines.append("2^%d samples; HIP events around %d calls, legs alternated, "
                         "%d repetitions after one warm-up of every leg; outputs "
                         "checked against the lookup on the whole ramp first"
                         % (r["log2n"], STEPS, r["reps"]))
        lines.append("%s  %s  [%s]" % (name, r["desc"], r["layout"]))
        med = {}
        for leg in r["legs"]:
            med[leg["leg"]], text = fmt(leg)
            lines.append("    " + text)
        lo_b = r["legs"][1]["rates"][0]
        hi_a = r["legs"][0]["rates"][-1]
        lines.append("    nco / lookup = %.2fx (medians); slowest nco repetition "
                     "%s fastest lookup repetition; nco iq / lookup = %.2fx"
                     % (med["nco"] / med["lookup"], ">" if lo_b > hi_a else "<=",
                        med["nco iq"] / med["lookup"]))
        print("\n".join(lines[first:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
