"""The tuned FM receiver on int16 arrays (cordic_plan_fm_rx16;
include/cordic_amd.h): every output sample and both words against the oracle,
against the 32-bit call on widened copies and against cordic_plan_fm_mix16 +
cordic_fm_demod16 on the same arrays; nothing has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O
import test_fm_demod16 as DEM16
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
from test_fm_demod import Padded, expected, last_value, last_word
from test_fm_rx import ACC0, DPHASE0, LAST0, LENGTHS, PHASE0
from test_table_fm import expected as phases, words

# (plan, converter, fused): cfg1 is p2r 16 16 2 16 16 (13 live stages), io16 is
# r2p 16 16 2 16 -1, ww36 has no fused discriminator
PAIRS = {"cfg1-io16": ("cfg1", "io16", 1), "cfg1-ww36": ("cfg1", "ww36", 0)}
OFFS = dict(fcw=1, pm=3, x=1, y=3, mag=1, freq=5)   # shorts: 2, 6, 10 bytes off


def configs(pair):
    m, c, fused = PAIRS[pair]
    margs, cargs = MIX16.CORES16[m][0], DEM16.CORES[c][0]
    return (ca.Config.from_cli(*margs), O.config_cli(*margs),
            ca.Config.from_cli(*cargs), O.config_cli(*cargs), fused)


def data(n, seed, with_pm=True):
    rng = np.random.default_rng(seed)
    x, y = MIX.iq(rng, n, 16)                       # full scale
    return (words("random", n, seed + 1),
            words("random", n, seed + 2) if with_pm else None, x, y)


def oracle(pair, fcw, pm, x, y, phase0, acc0, dphase0, last0):
    mcfg, mo, ccfg, co, _ = configs(pair)
    p, final = phases(fcw, pm, phase0, acc0)
    mask = np.uint32((1 << mcfg.pw) - 1 & 0xffffffff)
    tx, ty = O.rotate(mo, MIX.sext(x, mcfg.iw), MIX.sext(y, mcfg.iw), p & mask)
    mag, freq, last = expected(co, None, ccfg.pw, MIX.sext(tx, ccfg.iw),
                               MIX.sext(ty, ccfg.iw), dphase0 + last0)
    return mag, freq, final, last


def zeros(torch, nbytes):
    from gpu_util import DEV
    return torch.zeros(max(16, nbytes), dtype=torch.uint8, device=DEV)


def run(torch, plan, ccfg, fcw, pm, x, y, phase0, acc, dphase0, last, form):
    """form: "rx16", "rx32" (the 32-bit call on widened copies) or "two" (the
    two 16-bit calls); (mag, freq) as int32"""
    n = x.size
    i16 = form != "rx32"
    i32 = lambda a: None if a is None else a.view(np.int32)
    df = Padded(torch, n, OFFS["fcw"], src=i32(fcw))
    dm = None if pm is None else Padded(torch, n, OFFS["pm"], src=i32(pm))
    dx, dy = Padded(torch, n, OFFS["x"], i16, src=x), Padded(torch, n, OFFS["y"], i16, src=y)
    mag, freq = Padded(torch, n, OFFS["mag"], i16), Padded(torch, n, OFFS["freq"], i16)
    pmv = None if dm is None else dm.view
    kw = dict(pm=pmv, n=n, phase0=phase0, acc=acc)
    if form == "rx16":
        plan.fm_rx16(ccfg, df.view, dx.view, dy.view, mag.view, freq.view,
                     zeros(torch, plan.fm_rx16_workspace(ccfg, n)), dphase0=dphase0,
                     last=last, **kw)
    elif form == "rx32":
        plan.fm_rx(ccfg, df.view, dx.view, dy.view, mag.view, freq.view,
                   zeros(torch, plan.fm_rx_workspace(ccfg, n)), dphase0=dphase0,
                   last=last, **kw)
    else:
        tx, ty = Padded(torch, n, 3, True), Padded(torch, n, 1, True)
        plan.fm_mix16(df.view, dx.view, dy.view, tx.view, ty.view,
                      zeros(torch, plan.fm_mix16_workspace(n)), **kw)
        ca.fm_demod(ccfg, tx.view, ty.view, mag.view, freq.view,
                    zeros(torch, ca.fm_demod_workspace(n)), n=n, phase0=dphase0,
                    last=last)
    torch.cuda.synchronize()
    assert np.array_equal(df.get(), i32(fcw))
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    return mag.get().astype(np.int32), freq.get().astype(np.int32)


def test_the_16_bit_binding_asks_for_shorts():
    import torch
    plan = ca.Plan(MIX.both("ww38")[0])
    a = torch.zeros(8, dtype=torch.int32)
    with pytest.raises((TypeError, ValueError)):
        plan.fm_rx16(ca.Config.from_cli(*DEM16.CORES["io16"][0]), a, a, a, a, a, a, n=8)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_gpu_the_path_query_and_the_workspace(pair):
    mcfg, _, ccfg, _, fused = configs(pair)
    plan = ca.Plan(mcfg)
    assert plan.fm_rx16_info(ccfg) == (fused, 1024 if fused else 0)
    last = 0
    for n in (0, 1, 255, 1024, 1 << 20, 1 << 33):
        w = plan.fm_rx16_workspace(ccfg, n)
        assert w % 16 == 0 and w >= last and (w == 0) == (n == 0), n
        assert w <= (n // 256 + 65536 if fused else 25 * n + 65536 + 256), n
        last = w
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_pm", [True, False])
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_gpu_every_length_equals_the_oracle_the_32_bit_call_and_the_two_calls(
        pair, with_pm, monkeypatch):
    import torch
    monkeypatch.delenv("CORDIC_FMRX_MAX_BLOCKS", raising=False)
    mcfg, _, ccfg, _, _ = configs(pair)
    plan = ca.Plan(mcfg)
    for n in LENGTHS:
        fcw, pm, x, y = data(n, 3000 + n, with_pm)
        for with_words in (True, False):
            a0, l0 = (ACC0, LAST0) if with_words else (0, 0)
            wm, wf, wacc, wlast = oracle(pair, fcw, pm, x, y, PHASE0, a0, DPHASE0, l0)
            for form in ("rx16", "rx32", "two"):
                acc = last_word(torch, a0) if with_words else None
                last = last_word(torch, l0) if with_words else None
                gm, gf = run(torch, plan, ccfg, fcw, pm, x, y, PHASE0, acc, DPHASE0,
                             last, form)
                what = (pair, n, with_words, form)
                assert np.array_equal(gm, wm), what
                assert np.array_equal(gf, wf), what
                if with_words:
                    assert last_value(acc) == wacc and last_value(last) == wlast, what
    plan.close()


@pytest.mark.gpu
def test_gpu_a_halo_inside_a_span_of_three_passes_gives_the_same_bits(monkeypatch):
    import torch
    monkeypatch.setenv("CORDIC_FMRX_MAX_BLOCKS", "2")
    pair = "cfg1-io16"
    mcfg, _, ccfg, _, _ = configs(pair)
    plan = ca.Plan(mcfg)
    n = 5 * 1024 + 3
    for with_pm in (True, False):
        fcw, pm, x, y = data(n, 41, with_pm)
        wm, wf, wacc, wlast = oracle(pair, fcw, pm, x, y, PHASE0, ACC0, DPHASE0, LAST0)
        acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
        gm, gf = run(torch, plan, ccfg, fcw, pm, x, y, PHASE0, acc, DPHASE0, last, "rx16")
        assert np.array_equal(gm, wm) and np.array_equal(gf, wf), with_pm
        assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()


@pytest.mark.gpu
def test_gpu_wide_cores_are_refused_in_the_documented_order():
    """the plan's container rule, then the converter's; behind the modes"""
    L = ca.lib()
    io16 = ca.Config.from_cli(*DEM16.CORES["io16"][0])
    cfg1 = ca.Config.from_cli(*MIX16.CORES16["cfg1"][0])
    wide_plan = ca.Plan(MIX.both("nat24")[0])       # OW 24
    f, t = C.c_int32(-5), C.c_int32(-5)
    assert L.cordic_plan_fm_rx16_info(wide_plan._h, io16.ref, C.byref(f),
                                      C.byref(t)) == ca.ERR_CONTAINER
    assert (f.value, t.value) == (-5, -5)
    assert wide_plan.fm_rx16_workspace(io16, 64) == 0
    for n in (0, 8):
        assert L.cordic_plan_fm_rx16(wide_plan._h, io16.ref, n, None, None, 0, None, None,
                                     None, 0, None, None, None, None,
                                     None) == ca.ERR_CONTAINER
    # a rotator as the converter is a mode error even on a wide plan
    assert L.cordic_plan_fm_rx16_info(wide_plan._h, cfg1.ref, None, None) == ca.ERR_MODE
    wide_plan.close()
    plan = ca.Plan(cfg1)
    cfg3 = ca.Config.from_cli(ca.R2P, 24, 24, 2, -1, 20)    # IW 24
    assert L.cordic_plan_fm_rx16_info(plan._h, cfg3.ref, None, None) == ca.ERR_CONTAINER
    assert L.cordic_plan_fm_rx_info(plan._h, cfg3.ref, None, None) == 0
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stages", MIX.INSTANCES)
def test_gpu_every_16_bit_rotator_instance_equals_the_oracle(stages, monkeypatch):
    """fm_rx_xydir<30, N, Io16> for all 7 N: 16-bit ports with 15 extra bits (WW
    32) into io16, n = 2049"""
    import torch
    monkeypatch.delenv("CORDIC_FMRX_MAX_BLOCKS", raising=False)
    name = "inst16_%d" % stages
    MIX16.CORES16[name] = ((ca.P2R, 16, 16, 15, 32, stages), 0)
    PAIRS[name] = (name, "io16", 1)
    try:
        mcfg, _, ccfg, _, _ = configs(name)
        assert mcfg.ww == 32 and mcfg.nlive == stages and mcfg.pw == 32
        plan = ca.Plan(mcfg)
        assert plan.fm_rx16_info(ccfg) == (1, 1024)
        n = 2049
        fcw, pm, x, y = data(n, 500 + stages)
        wm, wf, wacc, wlast = oracle(name, fcw, pm, x, y, PHASE0, ACC0, DPHASE0, LAST0)
        for form in ("rx16", "two"):
            acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
            gm, gf = run(torch, plan, ccfg, fcw, pm, x, y, PHASE0, acc, DPHASE0, last, form)
            assert np.array_equal(gm, wm) and np.array_equal(gf, wf), (stages, form)
            assert last_value(acc) == wacc and last_value(last) == wlast, (stages, form)
        plan.close()
    finally:
        del MIX16.CORES16[name], PAIRS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_gpu_three_calls_that_share_both_words_equal_one_call(pair):
    import torch
    mcfg, _, ccfg, _, _ = configs(pair)
    n, cuts = 3 * 1024 + 7, (0, 1021, 2050, 3 * 1024 + 7)
    fcw, pm, x, y = data(n, 5)
    wm, wf, wacc, wlast = oracle(pair, fcw, pm, x, y, PHASE0, 0, DPHASE0, 0)
    plan = ca.Plan(mcfg)
    acc, last = last_word(torch, 0), last_word(torch, 0)
    gm, gf = [], []
    for k in range(3):
        s = slice(cuts[k], cuts[k + 1])
        m, f = run(torch, plan, ccfg, fcw[s], pm[s], x[s], y[s], PHASE0 if k == 0 else 0,
                   acc, DPHASE0 if k == 0 else 0, last, "rx16")
        gm.append(m)
        gf.append(f)
    assert np.array_equal(np.concatenate(gm), wm)
    assert np.array_equal(np.concatenate(gf), wf)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()


def device_arrays(torch, n, fcw, pm, x, y):
    i32 = lambda a: a.view(np.int32)
    return (Padded(torch, n, OFFS["fcw"], src=i32(fcw)), Padded(torch, n, OFFS["pm"], src=i32(pm)),
            Padded(torch, n, OFFS["x"], True, src=x), Padded(torch, n, OFFS["y"], True, src=y),
            Padded(torch, n, OFFS["mag"], True), Padded(torch, n, OFFS["freq"], True))


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_gpu_a_captured_call_replayed_three_times_continues_three_times(pair):
    """as tests/test_fm_rx.py has it for the 32-bit call: the fused call is two
    kernel nodes with one edge between them"""
    import torch
    mcfg, _, ccfg, _, fused = configs(pair)
    n = 2049
    fcw, pm, x, y = data(n, 9)
    rep = lambda a: np.concatenate([a, a, a])
    wm, wf, wacc, wlast = oracle(pair, rep(fcw), rep(pm), rep(x), rep(y), 0, ACC0, 0, LAST0)
    plan = ca.Plan(mcfg)
    work = zeros(torch, plan.fm_rx16_workspace(ccfg, n))
    df, dm, dx, dy, mag, freq = device_arrays(torch, n, fcw, pm, x, y)
    acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
    call = lambda a, l, s: plan.fm_rx16(ccfg, df.view, dx.view, dy.view, mag.view, freq.view,
                                        work, pm=dm.view, n=n, acc=a, last=l, stream=s)
    call(last_word(torch, 0), last_word(torch, 0), None)    # once outside the capture
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
        call(acc, last, stream.cuda_stream)
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
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_gpu_x_aliased_to_y_is_served(pair):
    import torch
    mcfg, _, ccfg, _, _ = configs(pair)
    n = 1025
    fcw, pm, x, _ = data(n, 11)
    wm, wf, _, _ = oracle(pair, fcw, pm, x, x, 0, 0, 0, 0)
    plan = ca.Plan(mcfg)
    df, dm, dx, _, mag, freq = device_arrays(torch, n, fcw, pm, x, x)
    plan.fm_rx16(ccfg, df.view, dx.view, dx.view, mag.view, freq.view,
                 zeros(torch, plan.fm_rx16_workspace(ccfg, n)), pm=dm.view, n=n)
    torch.cuda.synchronize()
    assert np.array_equal(mag.get(), wm) and np.array_equal(freq.get(), wf)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_gpu_overlaps_and_bad_pointers_are_refused_and_nothing_is_written(pair):
    """the byte ranges of the shorts are n * 2: what lies one short behind an
    array is clear, what lies on its last short is not"""
    import torch
    mcfg, _, ccfg, _, _ = configs(pair)
    n = 1024
    fcw, pm, x, y = data(n, 13)
    plan = ca.Plan(mcfg)
    work = zeros(torch, plan.fm_rx16_workspace(ccfg, n))
    df, dm, dx, dy, mag, freq = device_arrays(torch, n, fcw, pm, x, y)
    acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
    L = ca.lib()

    def call(**kw):
        a = dict(fcw=df.view, pm=dm.view, acc=acc, x=dx.view, y=dy.view, last=last,
                 mag=mag.view, freq=freq.view, work=work)
        a.update(kw)
        ptr = lambda v: v if isinstance(v, (int, type(None))) else C.c_void_p(v.data_ptr())
        return L.cordic_plan_fm_rx16(plan._h, ccfg.ref, n, ptr(a["fcw"]), ptr(a["pm"]), 0,
                                     ptr(a["acc"]), ptr(a["x"]), ptr(a["y"]), 0,
                                     ptr(a["last"]), ptr(a["mag"]), ptr(a["freq"]),
                                     ptr(a["work"]), None)

    at = lambda p, k: p.view.data_ptr() + 2 * k      # element k of a short array
    word_in = lambda p, k: (at(p, k) + 3) & ~3       # a 4-byte-aligned word at or behind it
    bad = [dict(mag=dx.view), dict(freq=dy.view), dict(mag=at(dx, n - 1)),
           dict(freq=at(mag, n - 1)), dict(mag=freq.view), dict(mag=df.view),
           dict(freq=at(dm, 2 * n - 1)),                # the last short of d_pm's n words
           dict(last=word_in(mag, 5)), dict(last=word_in(freq, n - 4)),
           dict(acc=word_in(mag, 9)), dict(acc=last), dict(last=word_in(dx, 3)),
           dict(acc=df.view[n - 1:]), dict(work=mag.view), dict(fcw=None), dict(x=None),
           dict(y=None), dict(mag=None), dict(freq=None), dict(work=None),
           dict(x=at(dx, 0) + 1), dict(mag=at(mag, 0) + 1), dict(last=last.data_ptr() + 2),
           dict(acc=acc.data_ptr() + 2), dict(pm=dm.view.data_ptr() + 2),
           dict(fcw=df.view.data_ptr() + 2), dict(work=work.data_ptr() + 8)]
    for kw in bad:
        assert call(**kw) == ca.ERR_ARGS, sorted(kw)
    torch.cuda.synchronize()
    assert mag.untouched() and freq.untouched()
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    assert np.array_equal(df.get(), fcw.view(np.int32)) and np.array_equal(dm.get(), pm.view(np.int32))
    assert last_value(acc) == ACC0 and last_value(last) == LAST0
    assert not work.any().item()
    assert call() == 0                              # and the same call, clean
    torch.cuda.synchronize()
    wm, wf, wacc, wlast = oracle(pair, fcw, pm, x, y, 0, ACC0, 0, LAST0)
    assert np.array_equal(mag.get(), wm) and np.array_equal(freq.get(), wf)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()
