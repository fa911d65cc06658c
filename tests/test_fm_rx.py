"""The tuned FM receiver (cordic_plan_fm_rx; include/cordic_amd.h): the FM mixer
and FM demodulation in one kernel.  Every output sample and both words are
compared with the oracle (O.rotate on the wrapping running sum, O.topolar, the
difference) AND with the two existing calls run on the same arrays; nothing has
a tolerance."""
import ctypes as C

import numpy as np
import pytest

import cordic_amd as ca
import test_fm_demod as DEM
import test_fm_mix as MIX
from test_fm_demod import Padded, last_value, last_word
from test_table_fm import expected as phases, words

# (plan, converter, fused)
PAIRS = {
    "nat24-cfg3": ("nat24", "cfg3", 1),         # LJ 30, 27 stages into 20
    "cfg2-cfg3": ("cfg2", "cfg3", 1),           # LJ 29; OW 32 into IW 24
    "nat16-natr2p24": ("nat16", "natr2p24", 1),
    "ww38-cfg3": ("ww38", "cfg3", 0),           # no fused mixer
    "cfg2-r2p35": ("cfg2", "r2p35", 0),         # no fused discriminator
    "cfg2-ug_lj": ("cfg2", "ug_lj", 0),         # unit gain
}
LENGTHS = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1028, 2049, 5 * 1024 + 3)
PHASE0, ACC0 = 0x9e3779b1, 0x7f4a7c15           # their sum wraps
DPHASE0, LAST0 = 0x85ebca77, 0xc2b2ae3d
# every array 4 bytes off a 16-byte boundary, or further
OFFS = dict(fcw=1, pm=3, x=1, y=5, mag=1, freq=3)


def cores(pair):
    m, c, fused = PAIRS[pair]
    return m, c, fused, MIX.both(m)[0], DEM.both(c)[0]


def data(pair, n, seed, with_pm=True):
    m, _, _, mcfg, _ = cores(pair)
    rng = np.random.default_rng(seed)
    fcw = words("random", n, seed + 1)
    pm = words("random", n, seed + 2) if with_pm else None
    x, y = MIX.iq(rng, n, mcfg.iw)              # full scale
    return fcw, pm, x, y


def oracle(pair, fcw, pm, x, y, phase0, acc0, dphase0, last0):
    """(mag, freq, *d_acc afterwards, *d_last afterwards)"""
    m, c, _, _, ccfg = cores(pair)
    p, final = phases(fcw, pm, phase0, acc0)
    tx, ty = MIX.want(m, x, y, p)
    _, ocfg, gain = DEM.both(c)
    mag, freq, last = DEM.expected(ocfg, gain, ccfg.pw, MIX.sext(tx, ccfg.iw),
                                   MIX.sext(ty, ccfg.iw), dphase0 + last0)
    return mag, freq, final, last


def buffers(torch, plan, ccfg, n):
    from gpu_util import DEV
    z = lambda b: torch.zeros(max(16, b), dtype=torch.uint8, device=DEV)
    return dict(rx=z(plan.fm_rx_workspace(ccfg, n)), mix=z(plan.fm_mix_workspace(n)),
                dem=z(ca.fm_demod_workspace(n)))


def run(torch, plan, ccfg, work, fcw, pm, x, y, phase0=0, acc=None, dphase0=0,
        last=None, offs=OFFS, two_calls=False):
    """one receiver call (or the mixer call into arrays of its own and the
    discriminator call from them) with every array at its offset; (mag, freq)
    after checking the guards and the inputs"""
    n = x.size
    i32 = lambda a: None if a is None else a.view(np.int32)
    df = Padded(torch, n, offs["fcw"], src=i32(fcw))
    dm = None if pm is None else Padded(torch, n, offs["pm"], src=i32(pm))
    dx = Padded(torch, n, offs["x"], src=x)
    dy = Padded(torch, n, offs["y"], src=y)
    mag, freq = Padded(torch, n, offs["mag"]), Padded(torch, n, offs["freq"])
    pmv = None if dm is None else dm.view
    if two_calls:
        tx, ty = Padded(torch, n, 4), Padded(torch, n, 4)
        plan.fm_mix(df.view, dx.view, dy.view, tx.view, ty.view, work["mix"], pm=pmv,
                    n=n, phase0=phase0, acc=acc)
        ca.fm_demod(ccfg, tx.view, ty.view, mag.view, freq.view, work["dem"], n=n,
                    phase0=dphase0, last=last)
    else:
        plan.fm_rx(ccfg, df.view, dx.view, dy.view, mag.view, freq.view, work["rx"],
                   pm=pmv, n=n, phase0=phase0, acc=acc, dphase0=dphase0, last=last)
    torch.cuda.synchronize()
    assert np.array_equal(df.get(), i32(fcw))
    assert dm is None or np.array_equal(dm.get(), i32(pm))
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    return mag.get(), freq.get()


def check(torch, pair, plan, work, fcw, pm, x, y, tag=None):
    """with both words preset and without either, against the oracle and the
    two calls"""
    _, _, _, _, ccfg = cores(pair)
    n = x.size
    for with_words in (True, False):
        a0, l0 = (ACC0, LAST0) if with_words else (0, 0)
        wm, wf, wacc, wlast = oracle(pair, fcw, pm, x, y, PHASE0, a0, DPHASE0, l0)
        for two in (False, True):
            acc = last_word(torch, a0) if with_words else None
            last = last_word(torch, l0) if with_words else None
            gm, gf = run(torch, plan, ccfg, work, fcw, pm, x, y, PHASE0, acc, DPHASE0,
                         last, two_calls=two)
            what = (pair, n, tag, with_words, "two calls" if two else "rx")
            assert np.array_equal(gm, wm), what
            assert np.array_equal(gf, wf), what
            if with_words:
                assert last_value(acc) == wacc, what
                assert last_value(last) == wlast, what


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_gpu_the_path_query_names_the_fused_pairs(pair):
    _, _, fused, mcfg, ccfg = cores(pair)
    plan = ca.Plan(mcfg)
    assert plan.fm_rx_info(ccfg) == (fused, 1024 if fused else 0)
    last = 0
    for n in (0, 1, 255, 1024, 1 << 20, 1 << 33):
        w = plan.fm_rx_workspace(ccfg, n)
        assert w % 16 == 0 and w >= last and (w == 0) == (n == 0), n
        assert w <= (n // 256 + 65536 if fused else 13 * n + 65536 + 128), n
        last = w
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_pm", [True, False])
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_gpu_every_length_equals_the_oracle_and_the_two_calls(pair, with_pm, monkeypatch):
    import torch
    monkeypatch.delenv("CORDIC_FMRX_MAX_BLOCKS", raising=False)
    _, _, _, mcfg, ccfg = cores(pair)
    plan = ca.Plan(mcfg)
    work = buffers(torch, plan, ccfg, max(LENGTHS))
    for n in LENGTHS:
        check(torch, pair, plan, work, *data(pair, n, 1000 + n, with_pm))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["nat24-cfg3", "cfg2-cfg3", "nat16-natr2p24"])
def test_gpu_a_halo_inside_a_span_of_three_passes_gives_the_same_bits(pair, monkeypatch):
    """two blocks over 5 * 1024 + 3 samples: spans of three passes, the second
    one's halo behind a multi-pass span, a partial last vector behind it"""
    import torch
    monkeypatch.setenv("CORDIC_FMRX_MAX_BLOCKS", "2")
    _, _, _, mcfg, ccfg = cores(pair)
    n = 5 * 1024 + 3
    plan = ca.Plan(mcfg)
    work = buffers(torch, plan, ccfg, n)
    for with_pm in (True, False):
        check(torch, pair, plan, work, *data(pair, n, 77, with_pm), tag="2 blocks")
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lj", [29, 30])
@pytest.mark.parametrize("stages", MIX.INSTANCES)
def test_gpu_every_rotator_instance_equals_the_oracle(stages, lj):
    """7 stage counts x LJ 29 / 30 into cfg3, n = 2049"""
    import torch
    args = (ca.P2R, 32, 32, 2, 32, stages) if lj == 29 else (ca.P2R, 31, 31, 2, 32, stages)
    name = "inst%d_%d" % (lj, stages)
    MIX.CORES[name] = (args, 0)
    PAIRS[name] = (name, "cfg3", 1)
    try:
        _, _, _, mcfg, ccfg = cores(name)
        assert mcfg.ww == 64 - lj and mcfg.nlive == stages and mcfg.pw == 32
        plan = ca.Plan(mcfg)
        assert plan.fm_rx_info(ccfg) == (1, 1024)
        n = 2049
        work = buffers(torch, plan, ccfg, n)
        check(torch, name, plan, work, *data(name, n, stages * lj))
        plan.close()
    finally:
        del MIX.CORES[name], PAIRS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["cfg2-cfg3", "ww38-cfg3"])
def test_gpu_three_calls_that_share_both_words_equal_one_call(pair):
    import torch
    _, _, _, mcfg, ccfg = cores(pair)
    n, cuts = 3 * 1024 + 7, (0, 1021, 2050, 3 * 1024 + 7)
    fcw, pm, x, y = data(pair, n, 5)
    wm, wf, wacc, wlast = oracle(pair, fcw, pm, x, y, PHASE0, 0, DPHASE0, 0)
    plan = ca.Plan(mcfg)
    work = buffers(torch, plan, ccfg, n)
    acc, last = last_word(torch, 0), last_word(torch, 0)
    gm, gf = [], []
    for k in range(3):
        s = slice(cuts[k], cuts[k + 1])
        m, f = run(torch, plan, ccfg, work, fcw[s], pm[s], x[s], y[s],
                   PHASE0 if k == 0 else 0, acc, DPHASE0 if k == 0 else 0, last)
        gm.append(m)
        gf.append(f)
    assert np.array_equal(np.concatenate(gm), wm)
    assert np.array_equal(np.concatenate(gf), wf)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["cfg2-cfg3", "cfg2-r2p35"])
def test_gpu_a_captured_call_replayed_three_times_continues_three_times(pair):
    """phase0 = dphase0 = 0 and both words: replay k is call k of a job three
    times as long on the same inputs.  The fused call is two kernel nodes with
    one edge between them, counted as tests/test_fm_mix_bank.py counts"""
    import torch
    from gpu_util import DEV
    _, _, fused, mcfg, ccfg = cores(pair)
    n = 2049
    fcw, pm, x, y = data(pair, n, 9)
    rep = lambda a: np.concatenate([a, a, a])
    wm, wf, wacc, wlast = oracle(pair, rep(fcw), rep(pm), rep(x), rep(y), 0, ACC0, 0, LAST0)
    plan = ca.Plan(mcfg)
    work = buffers(torch, plan, ccfg, n)
    i32 = lambda a: a.view(np.int32)
    df, dm = Padded(torch, n, 1, src=i32(fcw)), Padded(torch, n, 3, src=i32(pm))
    dx, dy = Padded(torch, n, 1, src=x), Padded(torch, n, 5, src=y)
    mag, freq = Padded(torch, n, 1), Padded(torch, n, 3)
    acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
    call = lambda s: plan.fm_rx(ccfg, df.view, dx.view, dy.view, mag.view, freq.view,
                                work["rx"], pm=dm.view, n=n, acc=acc, last=last, stream=s)
    # once outside the capture first, on words of its own
    warm_a, warm_l = last_word(torch, 0), last_word(torch, 0)
    plan.fm_rx(ccfg, df.view, dx.view, dy.view, mag.view, freq.view, work["rx"],
               pm=dm.view, n=n, acc=warm_a, last=warm_l)
    torch.cuda.synchronize()
    mag.t.fill_(mag.sent)
    freq.t.fill_(freq.sent)

    hip = MIX._hip()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipGraphExecDestroy.argtypes = [C.c_void_p]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    h = C.c_void_p(stream.cuda_stream)
    assert hip.hipStreamBeginCapture(h, 2) == 0      # hipStreamCaptureModeRelaxed
    graph = C.c_void_p()
    try:
        call(stream.cuda_stream)
    finally:
        rc = hip.hipStreamEndCapture(h, C.byref(graph))
    assert rc == 0 and graph.value
    try:
        assert mag.untouched() and freq.untouched()  # captured, not run
        cnt = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(cnt)) == 0
        if fused:
            assert cnt.value == 2
            nodes = (C.c_void_p * 2)()
            assert hip.hipGraphGetNodes(graph, nodes, C.byref(cnt)) == 0
            for i in range(2):
                t = C.c_int(-1)
                assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
                assert t.value == 0                  # hipGraphNodeTypeKernel
            edges = C.c_size_t(0)
            assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0
            assert edges.value == 1                  # two nodes, one chain
        ex = C.c_void_p()
        assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
        try:
            for r in range(3):
                assert hip.hipGraphLaunch(ex, h) == 0
                stream.synchronize()
                s = slice(r * n, (r + 1) * n)
                assert np.array_equal(mag.get(), wm[s]), (pair, r)
                assert np.array_equal(freq.get(), wf[s]), (pair, r)
        finally:
            hip.hipGraphExecDestroy(ex)
    finally:
        hip.hipGraphDestroy(graph)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["cfg2-cfg3", "ww38-cfg3"])
def test_gpu_x_aliased_to_y_is_served(pair):
    import torch
    _, _, _, mcfg, ccfg = cores(pair)
    n = 1025
    fcw, pm, x, _ = data(pair, n, 11)
    wm, wf, _, _ = oracle(pair, fcw, pm, x, x, 0, 0, 0, 0)
    plan = ca.Plan(mcfg)
    work = buffers(torch, plan, ccfg, n)
    i32 = lambda a: a.view(np.int32)
    df, dm = Padded(torch, n, 1, src=i32(fcw)), Padded(torch, n, 3, src=i32(pm))
    dx = Padded(torch, n, 1, src=x)
    mag, freq = Padded(torch, n, 1), Padded(torch, n, 3)
    plan.fm_rx(ccfg, df.view, dx.view, dx.view, mag.view, freq.view, work["rx"],
               pm=dm.view, n=n)
    torch.cuda.synchronize()
    assert np.array_equal(mag.get(), wm) and np.array_equal(freq.get(), wf)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["cfg2-cfg3", "ww38-cfg3"])
def test_gpu_overlaps_and_bad_pointers_are_refused_and_nothing_is_written(pair):
    import torch
    _, _, _, mcfg, ccfg = cores(pair)
    n = 1024
    fcw, pm, x, y = data(pair, n, 13)
    plan = ca.Plan(mcfg)
    work = buffers(torch, plan, ccfg, n)["rx"]
    i32 = lambda a: a.view(np.int32)
    df, dm = Padded(torch, n, 4, src=i32(fcw)), Padded(torch, n, 4, src=i32(pm))
    dx, dy = Padded(torch, n, 4, src=x), Padded(torch, n, 4, src=y)
    mag, freq = Padded(torch, n, 4), Padded(torch, n, 4)
    acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
    L = ca.lib()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(**kw):
        a = dict(fcw=df.view, pm=dm.view, acc=acc, x=dx.view, y=dy.view, last=last,
                 mag=mag.view, freq=freq.view, work=work)
        a.update(kw)
        ptr = lambda v: v if isinstance(v, (int, type(None))) else p(v)
        return L.cordic_plan_fm_rx(plan._h, ccfg.ref, n, ptr(a["fcw"]), ptr(a["pm"]),
                                   0, ptr(a["acc"]), ptr(a["x"]), ptr(a["y"]), 0,
                                   ptr(a["last"]), ptr(a["mag"]), ptr(a["freq"]),
                                   ptr(a["work"]), None)

    bad = [dict(mag=dx.view), dict(freq=dy.view), dict(mag=df.view), dict(freq=dm.view),
           dict(mag=freq.view), dict(freq=mag.view[n - 1:]),
           dict(last=mag.view[5:]), dict(last=freq.view[n - 1:]), dict(acc=mag.view[7:]),
           dict(acc=last), dict(last=dx.view[3:]), dict(acc=df.view[n - 1:]),
           dict(work=mag.view), dict(fcw=None), dict(x=None), dict(y=None),
           dict(mag=None), dict(freq=None), dict(work=None),
           dict(x=dx.view.data_ptr() + 2), dict(mag=mag.view.data_ptr() + 1),
           dict(last=last.data_ptr() + 2), dict(acc=acc.data_ptr() + 1),
           dict(pm=dm.view.data_ptr() + 2), dict(work=work.data_ptr() + 8)]
    for kw in bad:
        assert call(**kw) == ca.ERR_ARGS, sorted(kw)
    torch.cuda.synchronize()
    assert mag.untouched() and freq.untouched()
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    assert np.array_equal(df.get(), i32(fcw)) and np.array_equal(dm.get(), i32(pm))
    assert last_value(acc) == ACC0 and last_value(last) == LAST0
    assert not work.any().item()
    assert call() == 0                              # and the same call, clean
    torch.cuda.synchronize()
    wm, wf, wacc, wlast = oracle(pair, fcw, pm, x, y, 0, ACC0, 0, LAST0)
    assert np.array_equal(mag.get(), wm) and np.array_equal(freq.get(), wf)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()
