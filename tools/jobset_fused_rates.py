"""Data-fed job sets on an MI355X: 1024 jobs x 2^16 samples as one job set
against ONE call over the same 2^26 samples on the same core, and against one
call per job; HIP events, warm-up, median of 7.  Prints one line per core and
kind (profiles/r07/jobset_fused.txt):  python tools/jobset_fused_rates.py

--io16: the same blocks held in int16 arrays on -i 16 -o 16 -x 2 (mixer at
PW 32, converter and per-sample rotator at PW 16), legs alternated within
every repeat (profiles/r07/jobset16.txt):
  set16     the int16 job set, one launch (cordic_jobset_create16)
  widen32   what an int16 caller could do before there were int16 sets: widen
            every input into int32 arrays, run the int32 job set, narrow the
            outputs (conversions written into fixed arrays -- no allocation --
            because a set holds addresses); timed end to end
  set32     the int32 job set alone, no conversions
  single16  one long 16-bit call over all 2^26 samples
  block16   one 16-bit call per block
A library without the 16-bit sets (an older checkout run with this script)
gets the legs it has: widen32 and set32."""
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import cordic_amd as ca  # noqa: E402
import oracle_lib as O  # noqa: E402

NJ, NS = 1024, 1 << 16
N = NJ * NS
dev = torch.device("cuda:0")


def timed(fn, reps=7, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts))


def main32():
    x = torch.empty(N, dtype=torch.int32, device=dev)
    y, ph, a, b = (torch.empty_like(x) for _ in range(4))
    print("box %s, %s, %d jobs x %d samples vs one call over %d samples, median of 7"
          % (socket.gethostname(), torch.cuda.get_device_name(0), NJ, NS, N))
    for name, args, kind in (("n20", (ca.P2R, 32, 32, 2, 32, 20), ca.JOBS_P2R_XY),
                             ("r2p32", (ca.R2P, 32, 32, 2, 32, 24), ca.JOBS_R2P),
                             ("pw20", (ca.P2R, 13, 13, 2, -1, -1), ca.JOBS_MIX),
                             ("n20", (ca.P2R, 32, 32, 2, 32, 20), ca.JOBS_MIX),
                             ("ww38", (ca.P2R, 32, 32, 5, 32, 24), ca.JOBS_P2R_XY)):
        cfg = ca.Config.from_cli(*args)
        plan = ca.Plan(cfg)
        ca.fill_iq_ramp(x, y, 0, O.IQ_MULX, O.IQ_MULY, cfg.iw)
        ca.fill_phase_ramp(ph, 0, 2)
        fcw = 0x01234567 & ((1 << cfg.pw) - 1)
        jobs = []
        for k in range(NJ):
            s = slice(k * NS, (k + 1) * NS)
            jb = dict(x=x[s], y=y[s], ox=a[s], oy=b[s], n=NS)
            if kind == ca.JOBS_P2R_XY:
                jb["phase"] = ph[s]
            elif kind == ca.JOBS_MIX:
                jb.update(phase0=0, fcw=fcw, index0=k * NS)
            jobs.append(jb)
        js = ca.Jobset(plan, kind, jobs)

        def single():
            if kind == ca.JOBS_R2P:
                ca.r2p(cfg, x, y, a, b)
            elif kind == ca.JOBS_P2R_XY:
                plan.p2r(x, y, ph, a, b)
            else:
                plan.mix(0, fcw, 0, x, y, a, b)

        def one_by_one():
            for jb in jobs:
                if kind == ca.JOBS_R2P:
                    ca.r2p(cfg, jb["x"], jb["y"], jb["ox"], jb["oy"])
                elif kind == ca.JOBS_P2R_XY:
                    plan.p2r(jb["x"], jb["y"], jb["phase"], jb["ox"], jb["oy"])
                else:
                    plan.mix(0, fcw, jb["index0"], jb["x"], jb["y"], jb["ox"], jb["oy"])
        t1 = timed(single)
        k1 = ca.last_kernel()
        tf = timed(js.run)
        kf = ca.last_kernel()
        assert js.path == ca.JOBS_PATH_FUSED, name
        to = timed(one_by_one, reps=5, warm=1)
        kn = {1: "generic", 2: "unrolled", 3: "seeded", 4: "lj", 5: "dirs"}
        print("%-6s %-6s WW %d nlive %2d: single %7.1f Gs/s (%s)  fused %7.1f Gs/s (%s) = %.2fx"
              "  one call per job %6.1f Gs/s -> fused/one-by-one %.1fx"
              % (name, {2: "R2P", 3: "P2R_XY", 4: "MIX"}[kind], cfg.ww, cfg.nlive,
                 N / t1 / 1e9, kn.get(k1), N / tf / 1e9, kn.get(kf), t1 / tf,
                 N / to / 1e9, to / tf))
        sys.stdout.flush()
        js.close()
        plan.close()


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main16(reps=7):
    import build_stamp
    import cordic_amd._native as native
    have16 = "cordic_jobset_create16" in native.ABI
    st = build_stamp.stamp()
    print("box %s, %s, commit %s%s, kernel_sources_sha256 %s"
          % (socket.gethostname(), torch.cuda.get_device_name(0), st["git_head"],
             " (dirty)" if st["git_dirty"] else "", st["kernel_sources_sha256"]))
    print("%d blocks x %d samples (%d in all) on -i 16 -o 16 -x 2; HIP events, legs "
          "alternated, median of %d after one warm-up of every leg; 16-bit job sets: %s"
          % (NJ, NS, N, reps, "yes" if have16 else "NOT IN THIS LIBRARY"))
    x16 = torch.empty(N, dtype=torch.int16, device=dev)
    y16, ph16, a16, b16 = (torch.empty_like(x16) for _ in range(4))
    x32 = torch.empty(N, dtype=torch.int32, device=dev)
    y32, ph32, a32, b32 = (torch.empty_like(x32) for _ in range(4))
    ca.fill_iq_ramp(x32, y32, 0, O.IQ_MULX, O.IQ_MULY, 16)
    ca.fill_phase_ramp(ph32, 0, 2)
    ph32 &= 0xffff
    x16.copy_(x32)
    y16.copy_(y32)
    ph16.copy_(ph32)
    for name, args, kind in (("mix", (ca.P2R, 16, 16, 2, 32, -1), ca.JOBS_MIX),
                             ("r2p", (ca.R2P, 16, 16, 2, 16, -1), ca.JOBS_R2P),
                             ("p2rxy", (ca.P2R, 16, 16, 2, 16, -1), ca.JOBS_P2R_XY)):
        cfg = ca.Config.from_cli(*args)
        plan = ca.Plan(cfg)
        fcw = 0x01234567 & ((1 << cfg.pw) - 1)

        def cut(x, y, ph, a, b):
            jobs = []
            for k in range(NJ):
                s = slice(k * NS, (k + 1) * NS)
                jb = dict(x=x[s], y=y[s], ox=a[s], oy=b[s], n=NS)
                if kind == ca.JOBS_P2R_XY:
                    jb["phase"] = ph[s]
                elif kind == ca.JOBS_MIX:
                    jb.update(phase0=0, fcw=fcw, index0=k * NS)
                jobs.append(jb)
            return jobs
        jobs32 = cut(x32, y32, ph32, a32, b32)
        js32 = ca.Jobset(plan, kind, jobs32)
        legs = {}

        def widen32():
            x32.copy_(x16)
            y32.copy_(y16)
            if kind == ca.JOBS_P2R_XY:
                ph32.copy_(ph16)
            js32.run()
            a16.copy_(a32)
            b16.copy_(b32)
        legs["widen32"] = widen32
        legs["set32"] = js32.run
        if have16:
            jobs16 = cut(x16, y16, ph16, a16, b16)
            js16 = ca.Jobset(plan, kind, jobs16)
            legs["set16"] = js16.run

            def call16(x, y, p, a, b, index0):
                if kind == ca.JOBS_R2P:
                    ca.r2p(cfg, x, y, a, b)
                elif kind == ca.JOBS_P2R_XY:
                    ca.p2r(cfg, x, y, p, a, b)
                else:
                    ca.mix(cfg, 0, fcw, index0, x, y, a, b)
            legs["single16"] = lambda: call16(x16, y16, ph16, a16, b16, 0)

            def block16():
                for k, jb in enumerate(jobs16):
                    call16(jb["x"], jb["y"], jb.get("phase"), jb["ox"], jb["oy"], k * NS)
            legs["block16"] = block16
        ts = {k: [] for k in legs}
        for rep in range(reps + 1):         # (the first round is the warm-up)
            for k, fn in legs.items():
                t = once(fn)
                if rep:
                    ts[k].append(t)
        if have16:
            assert js16.path == ca.JOBS_PATH_FUSED, name
            # the three ways agree on the last outputs (set16 wrote a16 / b16
            # last but for single16 / block16, which write the same values)
            keep_a, keep_b = a16.clone(), b16.clone()
            widen32()
            torch.cuda.synchronize()
            assert torch.equal(keep_a, a16) and torch.equal(keep_b, b16), name
        rate = {k: N / float(np.median(v)) / 1e9 for k, v in ts.items()}
        print("%-6s WW %d nlive %2d PW %2d: %s" % (
            name, cfg.ww, cfg.nlive, cfg.pw,
            "  ".join("%s %7.1f Gs/s" % (k, rate[k]) for k in
                      ("set16", "widen32", "set32", "single16", "block16") if k in rate)))
        if have16:
            print("       set16 / widen32 = %.2fx   set16 / set32 = %.2fx   "
                  "set16 / single16 = %.2fx   set16 / block16 = %.1fx"
                  % (rate["set16"] / rate["widen32"], rate["set16"] / rate["set32"],
                     rate["set16"] / rate["single16"], rate["set16"] / rate["block16"]))
        sys.stdout.flush()
        if have16:
            js16.close()
        js32.close()
        plan.close()


if __name__ == "__main__":
    if "--io16" in sys.argv[1:]:
        main16()
    else:
        main32()
