"""Data-fed job sets on an MI355X: 1024 jobs x 2^16 samples as one job set
against ONE call over the same 2^26 samples on the same core, and against one
call per job; HIP events, warm-up, median of 7.  Prints one line per core and
kind (profiles/r07/jobset_fused.txt):  python tools/jobset_fused_rates.py"""
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
x = torch.empty(N, dtype=torch.int32, device=dev)
y, ph, a, b = (torch.empty_like(x) for _ in range(4))


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
