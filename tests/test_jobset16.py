"""Job sets of the data-fed kinds on int16 / uint16 arrays
(cordic_jobset_create16; include/cordic_amd.h "16-bit sample containers").
Per job the outputs must be, bit for bit, the oracle's values for that job
alone narrowed to 16 bits, and what the per-job single 16-bit call delivers;
on the cores whose single 16-bit call runs the vector kernel the set must run
fused (one tile-reading launch + one for trailing samples), elsewhere one by
one -- and say which."""
import ctypes as C

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
UG = ca.FLAG_UNIT_GAIN
GUARD = 0x5a5a
KINDS = {"r2p": ca.JOBS_R2P, "p2rxy": ca.JOBS_P2R_XY, "mix": ca.JOBS_MIX}


def both(args, flags=0):
    cfg = ca.Config.from_cli(*args)
    if flags:
        cfg = cfg.with_flags(flags)
    return cfg, O.config_cli(*args)


def sizes_of_the_set(rng):
    """about 100 ragged jobs: empty ones, fewer samples than a vector, one
    vector, trailing samples behind whole vectors, one job of several tiles (a
    set of this size has tiles of one pass, 1024 samples; a tile of the full
    8192 runs in test_jobset_instances.py, under CORDIC_JOBS_TILE_PASSES)"""
    fixed = [0, 1, 3, 4, 5, 255 * 4 + 2, 8192 * 2 + 4097, 0, 2, 1024, 1027]
    more = [int(v) for v in rng.randint(0, 3000, 100 - len(fixed))]
    sizes = fixed + more
    rng.shuffle(sizes)
    return sizes


def carve16(sizes, offsets):
    """sizes[k] int16 elements at element offset offsets[k] (odd: 2-byte
    aligned only) past job k's own 64-byte aligned start, guard elements in
    between: (views, flat array)"""
    total = sum(sizes) + 64 * len(sizes)
    big = torch.zeros(total, dtype=torch.int16, device=DEV)
    views, at = [], 0
    for n, off in zip(sizes, offsets):
        at = (at + 31) // 32 * 32 + off
        views.append(big[at:at + n])
        at += n
    assert at <= total
    return views, big


def iq16(rng, n, iw, full):
    lo, hi = -(1 << (iw - 1)), (1 << (iw - 1))
    a = rng.randint(lo, hi, n).astype(np.int16)
    if full and n:
        a[rng.randint(0, n, max(1, n // 16))] = rng.choice([lo, hi - 1, 0, -1, 1])
    return a


def put(view, host):
    if host.size:
        view.copy_(torch.from_numpy(np.ascontiguousarray(host).view(np.int16)).to(DEV))


class Set16:
    """the arrays of one set (jobs of `sizes`, else of sizes_of_the_set);
    fill() writes new inputs into the same arrays"""

    def __init__(self, kind, cfg, seed, sizes=None):
        self.kind, self.cfg = kind, cfg
        rng = np.random.RandomState(seed)
        self.sizes = sizes_of_the_set(rng) if sizes is None else list(sizes)
        nj = len(self.sizes)
        odd = [int(v) | 1 for v in rng.randint(0, 8, nj)]
        self.xv, _ = carve16(self.sizes, odd)
        self.yv, _ = carve16(self.sizes, [(o + 2) % 8 for o in odd])
        self.phv, _ = carve16(self.sizes, [(o + 4) % 8 for o in odd])
        self.av, self.abig = carve16(self.sizes, odd[::-1])
        self.bv, self.bbig = carve16(self.sizes, [(o + 6) % 8 for o in odd])
        self.jobs = []
        for k, n in enumerate(self.sizes):
            jb = dict(x=self.xv[k], y=self.yv[k], ox=self.av[k], oy=self.bv[k], n=n)
            assert n == 0 or jb["x"].data_ptr() % 4 == 2
            if kind == ca.JOBS_P2R_XY:
                jb["phase"] = self.phv[k]
            elif kind == ca.JOBS_MIX:
                jb.update(phase0=int(rng.randint(0, 1 << 32, dtype=np.uint64)),
                          fcw=int(rng.randint(0, 1 << 32, dtype=np.uint64)) | 1,
                          index0=(1 << 32) - n // 2 if k % 3 == 0 else
                          int(rng.randint(0, 1 << 40, dtype=np.uint64)))
            self.jobs.append(jb)
        self.total = sum(self.sizes)
        self.tails = sum(n % 4 for n in self.sizes)

    def fill(self, seed):
        rng = np.random.RandomState(seed)
        self.host = []
        for k, n in enumerate(self.sizes):
            hx = iq16(rng, n, self.cfg.iw, k % 5 == 0)
            hy = iq16(rng, n, self.cfg.iw, k % 5 == 0)
            hp = rng.randint(0, 1 << min(self.cfg.pw, 16), n).astype(np.uint16)
            put(self.xv[k], hx)
            put(self.yv[k], hy)
            put(self.phv[k], hp)
            self.host.append((hx, hy, hp))
        self.abig.fill_(GUARD)
        self.bbig.fill_(GUARD)

    def want(self, ocfg, k, gain):
        hx, hy, hp = self.host[k]
        hx, hy = hx.astype(np.int32), hy.astype(np.int32)
        jb = self.jobs[k]

        def scaled(a):
            return a if gain is None else (a.astype(np.int64) * gain) >> 32
        if self.kind == ca.JOBS_R2P:
            rm, rp = O.topolar(ocfg, hx, hy)
            return scaled(rm).astype(np.int16), rp.astype(np.uint16).view(np.int16)
        if self.kind == ca.JOBS_P2R_XY:
            ra, rb = O.rotate(ocfg, hx, hy, hp.astype(np.uint32))
        else:
            ra, rb = O.mix(ocfg, jb["phase0"], jb["fcw"], jb["index0"], hx, hy)
        return scaled(ra).astype(np.int16), scaled(rb).astype(np.int16)

    def single(self, k):
        """job k through the single 16-bit call, into arrays of its own"""
        jb = self.jobs[k]
        n = jb["n"]
        a = torch.zeros(n + 9, dtype=torch.int16, device=DEV)[1:1 + n]
        b = torch.zeros(n + 9, dtype=torch.int16, device=DEV)[3:3 + n]
        if self.kind == ca.JOBS_R2P:
            ca.r2p(self.cfg, jb["x"], jb["y"], a, b, n=n)
        elif self.kind == ca.JOBS_P2R_XY:
            ca.p2r(self.cfg, jb["x"], jb["y"], jb["phase"], a, b, n=n)
        else:
            ca.mix(self.cfg, jb["phase0"], jb["fcw"], jb["index0"], jb["x"], jb["y"],
                   a, b, n=n)
        return a, b

    def check(self, ocfg, gain, tag, want=None):
        """want: per job what self.want gives, where the caller has it already"""
        for k, jb in enumerate(self.jobs):
            if not jb["n"]:
                continue
            wa, wb = want[k] if want else self.want(ocfg, k, gain)
            ga, gb = self.av[k].cpu().numpy(), self.bv[k].cpu().numpy()
            assert np.array_equal(ga, wa), (tag, k, jb["n"])
            assert np.array_equal(gb, wb), (tag, k, jb["n"])
            sa, sb = self.single(k)
            assert torch.equal(sa, self.av[k]) and torch.equal(sb, self.bv[k]), (tag, k)
        for big in (self.abig, self.bbig):     # guard elements and gaps untouched
            keep = torch.ones_like(big, dtype=torch.bool)
            base = big.data_ptr()
            for v in (self.av if big is self.abig else self.bv):
                at = (v.data_ptr() - base) // 2
                keep[at:at + v.numel()] = False
            assert bool((big[keep] == GUARD).all()), tag


P2R16 = (ca.P2R, 16, 16, 2, 16, -1)
P2R16_PW32 = (ca.P2R, 16, 16, 2, 32, -1)
R2P16 = (ca.R2P, 16, 16, 2, 16, -1)
SR2P16 = (ca.SR2P, 16, 12, 2, 14, -1)
WW35 = (ca.P2R, 16, 16, 18, 16, -1)
# (cli args, flags, kind): every one of these must run fused
FUSED = {
    "p2rxy": (P2R16, 0, "p2rxy"),
    "mix": (P2R16, 0, "mix"),
    "mix_pw32": (P2R16_PW32, 0, "mix"),
    "r2p": (R2P16, 0, "r2p"),
    "sr2p": (SR2P16, 0, "r2p"),
    "p2rxy_unit_gain": (P2R16, UG, "p2rxy"),
    "mix_unit_gain": (P2R16_PW32, UG, "mix"),
    "r2p_unit_gain": (R2P16, UG, "r2p"),
}
ONE_BY_ONE = {
    "p2rxy_generic": (P2R16, ca.FLAG_FORCE_GENERIC, "p2rxy"),
    "mix_generic": (P2R16_PW32, ca.FLAG_FORCE_GENERIC, "mix"),
    "r2p_generic": (R2P16, ca.FLAG_FORCE_GENERIC, "r2p"),
    "p2rxy_ww35": (WW35, 0, "p2rxy"),
    "mix_ww35": (WW35, 0, "mix"),
}


def _run_set(args, flags, kind, path, seed):
    cfg, ocfg = both(args, flags)
    gain = ca.lib().cordic_config_gain_annihilator(cfg.ref) if flags & UG else None
    plan = ca.Plan(cfg)
    s = Set16(KINDS[kind], cfg, seed)
    js = ca.Jobset(plan, s.kind, s.jobs)
    assert js.io16
    assert js.path == ca.JOBS_PATH_NONE
    info = js.info
    assert info["samples"] == s.total
    assert info["tail_samples"] == s.tails
    for rep in range(2):                    # new data in the same arrays
        s.fill(seed + 100 * rep)
        js.run()
        torch.cuda.synchronize()
        assert js.path == path, (args, flags, kind)
        if path == ca.JOBS_PATH_FUSED:
            assert ca.last_kernel() == ca.KERNEL_UNROLLED
        s.check(ocfg, gain, rep)
    js.close()
    plan.close()


@pytest.mark.parametrize("name", sorted(FUSED))
def test_sets_on_int16_arrays_fuse_and_equal_the_oracle_job_by_job(name):
    args, flags, kind = FUSED[name]
    cfg = ca.Config.from_cli(*args)
    assert cfg.ww <= 32 and not cfg.needs_wrap
    _run_set(args, flags, kind, ca.JOBS_PATH_FUSED, 81)


@pytest.mark.parametrize("name", sorted(ONE_BY_ONE))
def test_other_cores_run_the_jobs_one_by_one_and_say_so(name):
    args, flags, kind = ONE_BY_ONE[name]
    assert ca.Config.from_cli(*WW35).ww == 35
    _run_set(args, flags, kind, ca.JOBS_PATH_ONE_BY_ONE, 83)


def test_create16_refusals():
    t = torch.zeros(256, dtype=torch.int16, device=DEV)
    jb = dict(x=t[0:16], y=t[32:48], phase=t[64:80], ox=t[96:112], oy=t[128:144], n=16)
    plan = ca.Plan(ca.Config.from_cli(*P2R16))

    def status(plan, kind, jobs):
        with pytest.raises(ca.CordicError) as e:
            ca.Jobset(plan, kind, jobs)
        return e.value.status
    # the constant-vector kinds have no 16-bit form
    assert status(plan, ca.JOBS_PHASE_ARRAYS, [jb]) == ca.ERR_UNSUPPORTED
    assert status(plan, ca.JOBS_NCO, [jb]) == ca.ERR_UNSUPPORTED
    # a converter kind on a rotator plan and the other way round
    assert status(plan, ca.JOBS_R2P, [jb]) == ca.ERR_MODE
    pol = ca.Plan(ca.Config.from_cli(*R2P16))
    assert status(pol, ca.JOBS_MIX, [jb]) == ca.ERR_MODE
    # phase arrays need PW <= 16; the mixer's scalars do not
    p17 = ca.Plan(ca.Config.from_cli(ca.P2R, 16, 16, 2, 17, 16))
    assert status(p17, ca.JOBS_P2R_XY, [jb]) == ca.ERR_CONTAINER
    ca.Jobset(p17, ca.JOBS_MIX, [jb]).close()
    iw17 = ca.Plan(ca.Config.from_cli(ca.P2R, 17, 16, 2, 16, 16))
    assert status(iw17, ca.JOBS_MIX, [jb]) == ca.ERR_CONTAINER
    # an odd byte address; a missing array
    assert status(plan, ca.JOBS_MIX, [dict(jb, x=t.data_ptr() + 1)]) == ca.ERR_ARGS
    assert status(plan, ca.JOBS_MIX, [dict(jb, oy=t.data_ptr() + 33)]) == ca.ERR_ARGS
    assert status(plan, ca.JOBS_P2R_XY, [dict(jb, phase=None)]) == ca.ERR_ARGS
    # ... but 2-byte alignment is enough, and empty jobs need no arrays
    ca.Jobset(plan, ca.JOBS_MIX, [dict(jb, x=t[1:17]), dict(jb, n=0, x=None)]).close()
    # a set cut for one core does not run on another
    js = ca.Jobset(plan, ca.JOBS_MIX, [jb])
    other = ca.Plan(ca.Config.from_cli(*P2R16_PW32))
    with pytest.raises(ca.CordicError) as e:
        js.run(plan=other)
    assert e.value.status == ca.ERR_ARGS
    js.close()
    # (closed here, not by the collector: the frames that pytest.raises keeps
    # hold them in cycles, and a plan destroyed by a collection inside a later
    # test's global-mode capture invalidates that capture)
    for p in (plan, pol, p17, iw17, other):
        p.close()


def test_python_picks_the_entry_point_by_the_tensors(monkeypatch):
    t16 = torch.zeros(256, dtype=torch.int16, device=DEV)
    t32 = torch.zeros(256, dtype=torch.int32, device=DEV)
    plan = ca.Plan(ca.Config.from_cli(*P2R16))
    real = ca.lib()
    calls = []

    class Spy:
        def __getattr__(self, name):
            f = getattr(real, name)
            if name.startswith("cordic_jobset_create"):
                calls.append(name)
            return f
    import cordic_amd._native as N
    monkeypatch.setattr(N, "lib", lambda: Spy())

    def job(t):
        return dict(x=t[0:16], y=t[32:48], ox=t[96:112], oy=t[128:144], n=16)
    a = ca.Jobset(plan, ca.JOBS_MIX, [job(t16)])
    b = ca.Jobset(plan, ca.JOBS_MIX, [job(t32)])
    assert calls == ["cordic_jobset_create16", "cordic_jobset_create"]
    assert a.io16 and not b.io16
    with pytest.raises(TypeError):
        ca.Jobset(plan, ca.JOBS_MIX, [job(t16), job(t32)])
    with pytest.raises(TypeError):
        ca.Jobset(plan, ca.JOBS_MIX, [dict(job(t16), ox=t32[0:16])])
    a.close()
    b.close()
    plan.close()


# ---- one launch, seen from outside the library: the run captured into a HIP
# graph (a linear one: the set's launches follow each other on one stream)

def _hip():
    for name in ("libamdhip64.so", "libamdhip64.so.6", "libamdhip64.so.7"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    return C.CDLL("/opt/rocm/lib/libamdhip64.so")


def _kernel_nodes_of_run(js, stream):
    """kernel nodes of the set's run; the graph is destroyed unlaunched"""
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


def test_a_mixer_set_of_64_jobs_is_two_kernel_nodes_and_replays():
    cfg, ocfg = both(P2R16_PW32)
    plan = ca.Plan(cfg)
    nj, n, pitch = 64, 4099, 4104            # 3 trailing samples per job
    x = torch.zeros(nj * pitch + 1, dtype=torch.int16, device=DEV)[1:]
    y, a, b = (torch.zeros(nj * pitch + 1, dtype=torch.int16, device=DEV)[1:]
               for _ in range(3))
    jobs = []
    for k in range(nj):
        s = slice(k * pitch, k * pitch + n)
        jobs.append(dict(x=x[s], y=y[s], ox=a[s], oy=b[s], n=n, phase0=977 * k,
                         fcw=0x01234567 + 2 * k, index0=(1 << 32) - 5 + k))
    js = ca.Jobset(plan, ca.JOBS_MIX, jobs)
    js.run()
    torch.cuda.synchronize()
    kernels, nodes = _kernel_nodes_of_run(js, torch.cuda.Stream())
    assert 1 <= kernels <= 2, (kernels, nodes)
    assert js.path == ca.JOBS_PATH_FUSED

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        js.run()
    rng = np.random.RandomState(91)
    for rep in range(2):                    # new samples, the same graph
        hx = rng.randint(-32768, 32768, nj * pitch).astype(np.int16)
        hy = rng.randint(-32768, 32768, nj * pitch).astype(np.int16)
        x.copy_(torch.from_numpy(hx).to(DEV))
        y.copy_(torch.from_numpy(hy).to(DEV))
        a.fill_(GUARD)
        b.fill_(GUARD)
        g.replay()
        torch.cuda.synchronize()
        ga, gb = a.cpu().numpy(), b.cpu().numpy()
        for k, jb in enumerate(jobs):
            s = slice(k * pitch, k * pitch + n)
            rx, ry = O.mix(ocfg, jb["phase0"], jb["fcw"], jb["index0"],
                           hx[s].astype(np.int32), hy[s].astype(np.int32))
            assert np.array_equal(ga[s], rx.astype(np.int16)), (rep, k)
            assert np.array_equal(gb[s], ry.astype(np.int16)), (rep, k)
            assert (ga[k * pitch + n:(k + 1) * pitch] == GUARD).all()
            assert (gb[k * pitch + n:(k + 1) * pitch] == GUARD).all()
    del g
    js.close()
    plan.close()
