#!/usr/bin/env python3
"""bench_table_bank.py -- oscillator banks (cordic_*_bank_create,
cordic_oscbank_run) against the two ways to do the same work without them.

For each of bench.py's table workloads (sintbl, qtrtbl16, qtrtbl24, qtrtbl,
quadtbl, quadtbl24; parameters from its workload table, tools/bench_common.py)
one child process, under a time limit of its own, measures for the forms

  sin     sine only, int32            (write 4 B per sample)
  iq      sine and cosine, int32      (write 8 B per sample pair)
  sin16   sine only, int16, OW <= 16  (write 2 B)

and the bank shapes 1024 x 2^16, 4096 x 2^12 and 16384 x 2^8 (jobs x samples:
2^26, 2^24 and 2^22 samples per bank; every job with a phase0 / fcw of its own,
the jobs back to back in one array):

  (a) bank     the whole bank in one launch (cordic_oscbank_run)
  (b) per job  one cordic_*_nco call per job on the same arrays
  (c) long     one cordic_*_nco call of the same total length

Rates are samples per second of one stream (an iq pair counts once, as in
tools/bench_table_nco.py).  Before any timing line the child checks that the
bank's arrays hold exactly what the per-job calls write.  Timing: HIP events
around each leg (20 bank runs / one pass over the jobs / 20 long calls), the
legs alternated within every repetition, one warm-up repetition, then --reps
(>= 5) timed ones; min - max over the repetitions and ratios of medians.  At
1024 x 2^16 the bank must reach 10x the per-job rate on every workload (a
launch costs 10-20 us: per-job calls cannot pass 3-7 Gsample/s there), or the
run fails.  A child that fails ends the run: nothing more is started on the GPU.

  python tools/bench_table_bank.py --out FILE [--lib-before BYTES]
"""
import argparse
import json
import os
import subprocess
import sys

TOOLS = os.path.dirname(os.path.abspath(__file__))
NAMES = ("sintbl", "qtrtbl16", "qtrtbl24", "qtrtbl", "quadtbl", "quadtbl24")
SHAPES = ((1024, 16), (4096, 12), (16384, 8))
STEPS = 20
GATE = 10.0


def child(name, reps):
    import bench_common as B            # the workload table bench.py runs
    import torch
    import cordic_amd as ca
    import build_stamp

    w = B.WORKLOADS[name]
    core = ca.Table(*w["table"]) if "table" in w else ca.Quad(*w["quad"])
    layout = ("lds mode %d" % core.lds_mode) if "table" in w else "quad, lds"
    dev = torch.device("cuda:0")
    total = max(j << l for j, l in SHAPES)
    s = torch.empty(total, dtype=torch.int32, device=dev)
    c = torch.empty(total, dtype=torch.int32, device=dev)
    rs = torch.empty(total, dtype=torch.int32, device=dev)
    rc = torch.empty(total, dtype=torch.int32, device=dev)
    forms = [("sin", 4, False, False), ("iq", 8, True, False)]
    if core.ow <= 16:
        forms.append(("sin16", 2, False, True))

    def ev():
        return torch.cuda.Event(enable_timing=True)

    rows = []
    for form, nbytes, iq, i16 in forms:
        view = (lambda t: t.view(torch.int16)[:total]) if i16 else (lambda t: t)
        for jobs, lg in SHAPES:
            n, tot = 1 << lg, jobs << lg
            bs, bc, ps, pc = (view(t)[:tot] for t in (s, c, rs, rc))
            # every job its own tuning (odd fcws, spread over the circle)
            tun = [((0x9e3779b1 * j) & 0xffffffff,
                    ((0x01000193 * (j + 1)) | 1) & 0xffffffff, j * 7)
                   for j in range(jobs)]
            bank = core.bank(
                [(p0, f, i0, n, bs[j * n:(j + 1) * n],
                  bc[j * n:(j + 1) * n] if iq else None)
                 for j, (p0, f, i0) in enumerate(tun)], i16=i16)

            def per_job(os_=ps, oc_=pc):
                for j, (p0, f, i0) in enumerate(tun):
                    core.nco(os_[j * n:(j + 1) * n],
                             oc_[j * n:(j + 1) * n] if iq else None,
                             phase0=p0, fcw=f, index0=i0)

            # ---- the outputs first: bank == per-job calls
            bs.fill_(-1); ps.fill_(-2)
            if iq:
                bc.fill_(-1); pc.fill_(-2)
            bank.run()
            per_job()
            torch.cuda.synchronize()
            if not torch.equal(bs, ps) or (iq and not torch.equal(bc, pc)):
                raise SystemExit("%s %s %dx2^%d: the bank differs from the "
                                 "per-job calls" % (name, form, jobs, lg))
            legs = [("bank", STEPS, lambda: bank.run()),
                    ("per job", 1, lambda: per_job(bs, bc)),
                    ("long", STEPS,
                     lambda: core.nco(bs, bc if iq else None, phase0=1, fcw=3))]
            rates = {k: [] for k, _, _ in legs}
            for rep in range(reps + 1):     # rep 0: warm-up of every leg
                for k, steps, run in legs:
                    e0, e1 = ev(), ev()
                    e0.record()
                    for _ in range(steps):
                        run()
                    e1.record()
                    e1.synchronize()
                    if rep:
                        rates[k].append(
                            tot * steps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
            rows.append(dict(form=form, bytes=nbytes, jobs=jobs, log2n=lg,
                             info=bank.info(),
                             rates={k: sorted(v) for k, v in rates.items()}))
            bank.close()
    st = build_stamp.stamp()
    out = dict(name=name, desc=w["desc"], layout=layout, reps=reps,
               device=torch.cuda.get_device_name(0),
               kernel_sources_sha256=st["kernel_sources_sha256"],
               lib_bytes=os.path.getsize(ca.lib_path()), rows=rows)
    print("RESULT " + json.dumps(out), flush=True)
    core.close()


def median(v):
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma-separated workloads")
    ap.add_argument("--limit", type=int, default=240,
                    help="seconds one workload's process may take")
    ap.add_argument("--lib-before", type=int, default=0,
                    help="bytes of libcordic_amd.so without the bank unit: the "
                         "report then states the growth in per cent")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    sys.path.insert(0, TOOLS)
    if a.child:
        child(a.child, a.reps)
        return 0
    names = a.only.split(",") if a.only else NAMES
    lines, below = [], []
    for name in names:
        if name not in NAMES:
            ap.error("unknown workload %r" % name)
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable,
                            os.path.abspath(__file__), "--child", name,
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
            grow = ""
            if a.lib_before > 0:
                grow = " (%+.2f %% against %d bytes without the bank unit)" % (
                    100.0 * (r["lib_bytes"] - a.lib_before) / a.lib_before,
                    a.lib_before)
            lines.append("libcordic_amd.so: %d bytes%s" % (r["lib_bytes"], grow))
            lines.append("jobs back to back in one array (2^26 / 2^24 / 2^22 samples per "
                         "bank); HIP events "
                         "around %d bank runs / one pass of per-job calls / %d "
                         "long calls, legs alternated, %d repetitions after one "
                         "warm-up of every leg; the bank's outputs checked "
                         "against the per-job calls first; Gsample/s, min - max"
                         % (STEPS, STEPS, r["reps"]))
        lines.append("%s  %s  [%s]" % (name, r["desc"], r["layout"]))
        for row in r["rows"]:
            v = row["rates"]
            m = {k: median(x) for k, x in v.items()}
            x_job, x_long = m["bank"] / m["per job"], m["bank"] / m["long"]
            gated = row["jobs"] == SHAPES[0][0]
            if gated and x_job < GATE:
                below.append("%s %s" % (name, row["form"]))
            lines.append(
                "    %-5s %5d x 2^%-2d  bank %7.1f - %7.1f  per job %6.2f - %6.2f"
                "  long %7.1f - %7.1f  bank/per job %7.1fx%s  bank/long %.2f"
                "  (%d tiles, %d edge samples)" % (
                    row["form"], row["jobs"], row["log2n"], v["bank"][0],
                    v["bank"][-1], v["per job"][0], v["per job"][-1],
                    v["long"][0], v["long"][-1], x_job,
                    (" (>= %gx: %s)" % (GATE, "ok" if x_job >= GATE else "NO"))
                    if gated else "", x_long, row["info"]["tiles"],
                    row["info"]["edge_samples"]))
        print("\n".join(lines[first:]), flush=True)
    if below:
        lines.append("BELOW %gx the per-job rate at %d x 2^%d: %s" % (
            GATE, SHAPES[0][0], SHAPES[0][1], ", ".join(below)))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if below else 0


if __name__ == "__main__":
    sys.exit(main())
