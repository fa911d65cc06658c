"""Job sets of the data-fed kinds (CORDIC_JOBS_R2P / _P2R_XY / _MIX) in one
launch on every core up to WW 40 whose single call runs a vector kernel, and
the path query cordic_jobset_path (include/cordic_amd.h "job sets").  Per job
the results must be, bit for bit, what the oracle computes for that job alone;
the set must report the path it took."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- no GPU

def test_the_path_query_is_exported_and_declared():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    assert re.search(r"int\s+cordic_jobset_path\s*\(\s*const\s+cordic_jobset\s*\*\s*set\s*,"
                     r"\s*int32_t\s*\*\s*path\s*\)\s*;", text)
    for name, value in (("CORDIC_JOBS_PATH_NONE", 0), ("CORDIC_JOBS_PATH_FUSED", 1),
                        ("CORDIC_JOBS_PATH_ONE_BY_ONE", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text), name
    assert (ca.JOBS_PATH_NONE, ca.JOBS_PATH_FUSED, ca.JOBS_PATH_ONE_BY_ONE) == (0, 1, 2)
    f = ca.lib().cordic_jobset_path          # AttributeError: not exported
    p = C.c_int32(-1)
    assert f(None, C.byref(p)) == ca.ERR_ARGS
    assert p.value == -1


# ---------------------------------------------------------------- GPU

def _gpu():
    torch = pytest.importorskip("torch")
    from gpu_util import DEV, dev_i32, to_np
    from test_jobset import RAGGED, _iq, both, carve
    return torch, DEV, dev_i32, to_np, RAGGED, _iq, both, carve


UG = ca.FLAG_UNIT_GAIN
# name: (cli args, flags, kernel family a fused run reports)
ROT_CORES = {
    "n20": ((ca.P2R, 32, 32, 2, 32, 20), 0, ca.KERNEL_DIRECTIONS),     # WW 35
    "pw20": ((ca.P2R, 13, 13, 2, -1, -1), 0, None),                     # PW 20
    "ww38": ((ca.P2R, 32, 32, 5, 32, 24), 0, ca.KERNEL_UNROLLED),      # LJ 26
    "ww40_mix": ((ca.P2R, 32, 32, 7, 32, 20), 0, ca.KERNEL_UNROLLED),  # LJ 24
    "unit_gain": ((ca.P2R, 32, 32, 2, 32, 16), UG, ca.KERNEL_UNROLLED),
    "unit_gain_lj30": ((ca.P2R, 24, 24, 2, -1, -1), UG, ca.KERNEL_UNROLLED),
    "few_stages": ((ca.P2R, 16, 16, 2, -1, 9), 0, ca.KERNEL_UNROLLED),
    "no_tails": ((ca.P2R, 32, 32, 2, 32, 16), ca.FLAG_NO_TAILS, ca.KERNEL_UNROLLED),
    "wrap32": ((ca.P2R, 24, 2, 7, 32, -1), 0, ca.KERNEL_UNROLLED),
}
POL_CORES = {
    "r2p32": ((ca.R2P, 32, 32, 2, 32, 24), 0, ca.KERNEL_LEFT_JUSTIFIED),   # WW 40
    "r2p35": ((ca.R2P, 27, 27, 2, 32, 20), 0, ca.KERNEL_LEFT_JUSTIFIED),
    "ug_lj": ((ca.R2P, 24, 24, 2, -1, 20), UG, ca.KERNEL_LEFT_JUSTIFIED),  # WW 32
    "ug_ljw": ((ca.R2P, 32, 32, 2, 32, 24), UG, ca.KERNEL_LEFT_JUSTIFIED),
    "wrap32": ((ca.R2P, 24, 1, 2, 32, -1), 0, ca.KERNEL_UNROLLED),
}


def _gain(cfg, flags):
    if not flags & UG:
        return None
    return ca.lib().cordic_config_gain_annihilator(cfg.ref)


def _scaled(a, k):
    """o = (o * K) >> 32 (include/cordic_amd.h: CORDIC_FLAG_UNIT_GAIN)"""
    return a if k is None else ((a.astype(np.int64) * k) >> 32).astype(np.int32)


def _ragged_set(kind, cfg, seed, sizes=None):
    """RAGGED jobs (or jobs of the given sizes) at odd offsets of shared arrays
    with guard words around: (jobs, host inputs, output views, big output
    arrays)"""
    torch, DEV, dev_i32, to_np, RAGGED, _iq, both, carve = _gpu()
    rng = np.random.RandomState(seed)
    sizes = RAGGED if sizes is None else sizes
    offs = [int(v) for v in rng.randint(0, 4, len(sizes))]
    total = sum(sizes) + 32 * len(sizes)
    xv, _ = carve(total, sizes, offs)
    yv, _ = carve(total, sizes, [(o + 3) % 4 for o in offs])
    phv, _ = carve(total, sizes, [(o + 2) % 4 for o in offs])
    av, abig = carve(total, sizes, offs[::-1])
    bv, bbig = carve(total, sizes, [(o + 1) % 4 for o in offs])
    mask = (1 << cfg.pw) - 1
    host, jobs = [], []
    for k, n in enumerate(sizes):
        hx = _iq(rng, n, cfg.iw, full=(k % 5 == 0))
        hy = _iq(rng, n, cfg.iw, full=(k % 5 == 0))
        hp = rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(mask)
        if n:
            xv[k].copy_(dev_i32(hx))
            yv[k].copy_(dev_i32(hy))
            phv[k].copy_(dev_i32(hp))
        jb = dict(x=xv[k], y=yv[k], ox=av[k], oy=bv[k], n=n)
        if kind == ca.JOBS_P2R_XY:
            jb["phase"] = phv[k]
        elif kind == ca.JOBS_MIX:
            jb.update(phase0=int(rng.randint(0, 1 << 32, dtype=np.uint64)),
                      fcw=int(rng.randint(0, 1 << 32, dtype=np.uint64)) | 1,
                      index0=(1 << 32) - n // 2 if k % 3 == 0 else
                      int(rng.randint(0, 1 << 40, dtype=np.uint64)))
        host.append((hx, hy, hp))
        jobs.append(jb)
    return jobs, host, (av, bv), (abig, bbig)


def _want(kind, ocfg, jb, h, k_gain):
    hx, hy, hp = h
    if kind == ca.JOBS_R2P:
        rm, rp = O.topolar(ocfg, hx, hy)
        return _scaled(rm, k_gain), rp
    if kind == ca.JOBS_P2R_XY:
        ra, rb = O.rotate(ocfg, hx, hy, hp)
    else:
        ra, rb = O.mix(ocfg, jb["phase0"], jb["fcw"], jb["index0"], hx, hy)
    return _scaled(ra, k_gain), _scaled(rb, k_gain)


def _check_outputs(kind, ocfg, jobs, host, outs, k_gain, tag, want=None):
    """want: per job what _want gives, where the caller has it already"""
    torch, DEV, dev_i32, to_np = _gpu()[:4]
    for k, jb in enumerate(jobs):
        if not jb["n"]:
            continue
        wa, wb = want[k] if want else _want(kind, ocfg, jb, host[k], k_gain)
        ga = to_np(outs[0][k])
        gb = to_np(outs[1][k], np.uint32 if kind == ca.JOBS_R2P else np.int32)
        assert np.array_equal(ga, wa), (tag, k, jb["n"])
        assert np.array_equal(gb, wb), (tag, k, jb["n"])


def _parity(args, flags, family, kind, seed):
    torch, DEV, dev_i32, to_np, RAGGED, _iq, both, carve = _gpu()
    cfg, ocfg = both(*args, flags=flags)
    plan = ca.Plan(cfg)
    k_gain = _gain(cfg, flags)
    jobs, host, outs, bigs = _ragged_set(kind, cfg, seed)
    js = ca.Jobset(plan, kind, jobs)
    assert js.path == ca.JOBS_PATH_NONE
    total = sum(jb["n"] for jb in jobs)
    for rep in range(2):
        for b in bigs:
            b.fill_(0x5a5a5a5a)
        js.run()
        torch.cuda.synchronize()
        assert js.path == ca.JOBS_PATH_FUSED, (args, flags, kind)
        if family is not None:
            assert ca.last_kernel() == family, (args, flags, kind, ca.last_kernel())
        else:
            assert ca.last_kernel() in (ca.KERNEL_DIRECTIONS, ca.KERNEL_UNROLLED)
        _check_outputs(kind, ocfg, jobs, host, outs, k_gain, rep)
        for b in bigs:              # guard words and gaps untouched
            assert int((b == 0x5a5a5a5a).sum().item()) == b.numel() - total
    for b in bigs:
        b.zero_()
    plan.xy_batch(kind, jobs)        # the one-shot form: the same bits
    torch.cuda.synchronize()
    _check_outputs(kind, ocfg, jobs, host, outs, k_gain, "batch")
    ca.jobset_reap()
    js.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["p2rxy", "mix"])
@pytest.mark.parametrize("name", sorted(ROT_CORES))
def test_rotator_sets_fuse_and_equal_the_oracle_job_by_job(name, kind):
    args, flags, family = ROT_CORES[name]
    _parity(args, flags, family,
            ca.JOBS_P2R_XY if kind == "p2rxy" else ca.JOBS_MIX, 61)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(POL_CORES))
def test_converter_sets_fuse_and_equal_the_oracle_job_by_job(name):
    args, flags, family = POL_CORES[name]
    _parity(args, flags, family, ca.JOBS_R2P, 67)


def test_the_core_table_spans_what_fuses():
    """The table above covers WW 35 .. 40, unit gain, few stages and the wrap
    at WW 32 (the configuration layer alone: no GPU)."""
    def cfg(args, flags):
        c = ca.Config.from_cli(*args)
        return c.with_flags(flags) if flags else c
    rot = {k: cfg(a, f) for k, (a, f, _) in ROT_CORES.items()}
    pol = {k: cfg(a, f) for k, (a, f, _) in POL_CORES.items()}
    assert rot["n20"].ww == 35 and rot["ww38"].ww == 38 and rot["ww40_mix"].ww == 40
    assert rot["pw20"].pw == 20
    assert rot["few_stages"].nlive < 13
    assert rot["wrap32"].needs_wrap and rot["wrap32"].ww == 32
    assert pol["wrap32"].needs_wrap and pol["wrap32"].ww == 32
    assert pol["r2p32"].ww == 40 and pol["r2p35"].ww == 35
    assert pol["ug_lj"].ww <= 34 and 35 <= pol["ug_ljw"].ww <= 40
    for c in list(rot.values()) + list(pol.values()):
        assert c.ww <= 40


@pytest.mark.gpu
def test_the_path_says_how_the_last_run_went():
    torch, DEV, dev_i32, to_np, RAGGED, _iq, both, carve = _gpu()
    t = torch.zeros(1 << 12, dtype=torch.int32, device=DEV)
    jobs_xy = [dict(x=t[0:100], y=t[128:228], phase=t[256:356], ox=t[512:612],
                    oy=t[768:868], n=100),
               dict(x=t[1024:1027], y=t[1100:1103], phase=t[1200:1203],
                    ox=t[1300:1303], oy=t[1400:1403], n=3)]
    jobs_ph = [dict(phase=j["phase"], ox=j["ox"], oy=j["oy"], n=j["n"]) for j in jobs_xy]

    def path_after_run(args, flags, kind, jobs):
        cfg, _ = both(*args, flags=flags)
        plan = ca.Plan(cfg)
        js = ca.Jobset(plan, kind, jobs)
        assert js.path == ca.JOBS_PATH_NONE
        js.run(1000, -77)
        torch.cuda.synchronize()
        p = js.path
        js.close()
        plan.close()
        return p
    cfg2 = (ca.P2R, 32, 32, 2, 32, 16)
    # one by one: WW 41, the generic kernel forced, constant vectors without
    # a seeded kernel
    assert path_after_run((ca.P2R, 32, 32, 8, 32, 24), 0, ca.JOBS_P2R_XY,
                          jobs_xy) == ca.JOBS_PATH_ONE_BY_ONE
    assert path_after_run((ca.P2R, 32, 32, 8, 32, 24), 0, ca.JOBS_MIX,
                          jobs_xy) == ca.JOBS_PATH_ONE_BY_ONE
    assert path_after_run(cfg2, ca.FLAG_FORCE_GENERIC, ca.JOBS_P2R_XY,
                          jobs_xy) == ca.JOBS_PATH_ONE_BY_ONE
    assert path_after_run(cfg2, ca.FLAG_NO_SEED, ca.JOBS_PHASE_ARRAYS,
                          jobs_ph) == ca.JOBS_PATH_ONE_BY_ONE
    # fused
    assert path_after_run(cfg2, 0, ca.JOBS_PHASE_ARRAYS, jobs_ph) == ca.JOBS_PATH_FUSED
    assert path_after_run(cfg2, 0, ca.JOBS_P2R_XY, jobs_xy) == ca.JOBS_PATH_FUSED
    assert path_after_run((ca.P2R, 32, 32, 2, 32, 20), 0, ca.JOBS_P2R_XY,
                          jobs_xy) == ca.JOBS_PATH_FUSED


# ---- one launch, seen from outside the library: the set's run captured into
# a HIP graph whose kernel nodes are counted; the graph is destroyed without
# being instantiated or launched

def _hip():
    for name in ("libamdhip64.so", "libamdhip64.so.6", "libamdhip64.so.7"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    return C.CDLL("/opt/rocm/lib/libamdhip64.so")


def _kernel_nodes_of_run(js, stream):
    hip = _hip()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    h = C.c_void_p(stream.cuda_stream)
    assert hip.hipStreamBeginCapture(h, 2) == 0      # hipStreamCaptureModeRelaxed
    graph = C.c_void_p()
    try:
        js.run(stream=stream.cuda_stream)
    finally:
        rc = hip.hipStreamEndCapture(h, C.byref(graph))
    assert rc == 0 and graph.value
    try:
        n = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
        nodes = (C.c_void_p * max(1, n.value))()
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
        kernels = 0
        for i in range(n.value):
            t = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
            kernels += t.value == 0                    # hipGraphNodeTypeKernel
        return kernels, n.value
    finally:
        hip.hipGraphDestroy(graph)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROT_CORES) + ["r2p:" + k for k in sorted(POL_CORES)])
def test_a_set_of_64_jobs_is_at_most_two_kernel_launches(name):
    torch, DEV, dev_i32, to_np, RAGGED, _iq, both, carve = _gpu()
    pol = name.startswith("r2p:")
    args, flags, _ = POL_CORES[name[4:]] if pol else ROT_CORES[name]
    cfg, _ = both(*args, flags=flags)
    plan = ca.Plan(cfg)
    nj, n = 64, 4099                     # 3 trailing samples per job
    x = torch.zeros(nj * 4104, dtype=torch.int32, device=DEV)
    y, ph, a, b = (torch.zeros_like(x) for _ in range(4))
    jobs = []
    for k in range(nj):
        s = slice(k * 4104, k * 4104 + n)
        jb = dict(x=x[s], y=y[s], ox=a[s], oy=b[s], n=n)
        if not pol:
            jb["phase"] = ph[s]
        jobs.append(jb)
    js = ca.Jobset(plan, ca.JOBS_R2P if pol else ca.JOBS_P2R_XY, jobs)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    kernels, nodes = _kernel_nodes_of_run(js, s)
    assert 1 <= kernels <= 2, (name, kernels, nodes)
    assert js.path == ca.JOBS_PATH_FUSED
    js.close()
    plan.close()
