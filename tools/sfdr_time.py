"""cordic_sfdr_run alone at lgn 24 and 28: HIP events around the call, after
warm-up; the load that precedes every run is outside the timed window."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cordic_amd as ca

for lgn in (24, 28):
    n = 1 << lgn
    g = torch.Generator(device="cuda").manual_seed(lgn)
    re = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    im = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    s = ca.Sfdr(lgn)
    ms, wall = [], []
    for it in range(2 + 5):
        s.load_iq(re, im)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        r = s.run()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= 2:
            ms.append(a.elapsed_time(b)); wall.append((t1 - t0) * 1e3)
    passes = lgn // 2 + (lgn & 1)
    gb = (passes * 32 + 16) * n / 1e9
    print("cordic_sfdr_run lgn %d: events min %.3f ms median %.3f ms max %.3f ms (host clock median %.3f ms); "
          "%d transform passes + spur search = %.2f GB moved, %.2f TB/s at the median; sfdr of noise %.2f dBc"
          % (lgn, min(ms), sorted(ms)[len(ms)//2], max(ms), sorted(wall)[len(wall)//2], passes, gb,
             gb / sorted(ms)[len(ms)//2], r["sfdr_dbc"]), flush=True)
    s.close()
    del re, im
