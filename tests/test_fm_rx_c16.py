"""The tuned FM receiver on interleaved int16 I/Q (cordic_plan_fm_rx_c16 and
cordic_plan_fm_rx_decim_c16; include/cordic_amd.h): every output sample and
both words against the oracle on (iq[0::2], iq[1::2]) and against the *16 twin
on split copies.  Nothing has a tolerance.  Every iq buffer lies 1, 2 or 3
complex samples off the 16-byte grid between sentinels and is read back
unchanged after every call."""
import ctypes as C

import numpy as np
import pytest

import cordic_amd as ca
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
import test_fm_rx16 as RX16
import test_fm_rx_decim as RXD
from test_fm_demod import Padded, last_value, last_word
from test_fm_rx import ACC0, DPHASE0, LAST0, LENGTHS, PHASE0

PAIRS = ("cfg1-io16", "cfg1-ww36")                  # fused, fallback
OFFS = dict(fcw=1, pm=3, mag=1, freq=5)             # as RX16.OFFS
zeros = RX16.zeros


def interleave(x, y):
    iq = np.empty(2 * x.size, dtype=np.int16)
    iq[0::2], iq[1::2] = x, y
    return iq


def iq_buffer(torch, x, y, c):
    """the 2 n shorts of (x, y) interleaved, c complex samples off the grid"""
    assert c in (1, 2, 3)
    return Padded(torch, 2 * x.size, 2 * c, True, src=interleave(x, y))


def run(torch, plan, ccfg, k, fcw, pm, x, y, phase0=0, acc=None, dphase0=0, last=None, c=1,
        stream=None):
    """one call of the interleaved form (k None: the plain call); (mag, freq) as
    int32 after checking the guards and that no input was written"""
    n = x.size
    m = n if k is None else n >> k
    i32 = lambda a: None if a is None else a.view(np.int32)
    df = Padded(torch, n, OFFS["fcw"], src=i32(fcw))
    dm = None if pm is None else Padded(torch, n, OFFS["pm"], src=i32(pm))
    diq = iq_buffer(torch, x, y, c)
    mag, freq = Padded(torch, m, OFFS["mag"], True), Padded(torch, m, OFFS["freq"], True)
    kw = dict(pm=None if dm is None else dm.view, n=n, phase0=phase0, acc=acc,
              dphase0=dphase0, last=last, stream=stream)
    if k is None:
        plan.fm_rx_c16(ccfg, df.view, diq.view, mag.view, freq.view,
                       zeros(torch, plan.fm_rx_c16_workspace(ccfg, n)), **kw)
    else:
        plan.fm_rx_decim_c16(ccfg, k, df.view, diq.view, mag.view, freq.view,
                             zeros(torch, plan.fm_rx_decim_c16_workspace(ccfg, n, k)), **kw)
    torch.cuda.synchronize()
    assert np.array_equal(df.get(), i32(fcw))
    assert dm is None or np.array_equal(dm.get(), i32(pm))
    assert np.array_equal(diq.get(), interleave(x, y))
    return mag.get().astype(np.int32), freq.get().astype(np.int32)


# ---------------------------------------------------------------- the plain call

@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_gpu_the_path_query_is_the_twins_and_the_workspace_holds_the_split(pair):
    mcfg, _, ccfg, _, fused = RX16.configs(pair)
    plan = ca.Plan(mcfg)
    assert plan.fm_rx_c16_info(ccfg) == plan.fm_rx16_info(ccfg) == (fused, 1024 if fused else 0)
    a16 = lambda b: (b + 15) // 16 * 16
    for n in (0, 1, 255, 1024, 1 << 20, 1 << 33):
        w, twin = plan.fm_rx_c16_workspace(ccfg, n), plan.fm_rx16_workspace(ccfg, n)
        assert w == (twin if fused or not n else a16(twin) + 2 * a16(2 * n)), n
        for k in (0, 3):
            wd = plan.fm_rx_decim_c16_workspace(ccfg, n, k)
            twin = plan.fm_rx_decim16_workspace(ccfg, n, k)
            # (0 where the twin answers 0: no samples, or no whole groups)
            assert wd == (twin if fused or not twin else a16(twin) + 2 * a16(2 * n)), (n, k)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_pm", [True, False])
@pytest.mark.parametrize("pair", PAIRS)
def test_gpu_every_length_equals_the_oracle_and_the_16_bit_call_on_split_copies(
        pair, with_pm, monkeypatch):
    import torch
    monkeypatch.delenv("CORDIC_FMRX_MAX_BLOCKS", raising=False)
    mcfg, _, ccfg, _, _ = RX16.configs(pair)
    plan = ca.Plan(mcfg)
    for n in LENGTHS:
        fcw, pm, x, y = RX16.data(n, 3000 + n, with_pm)
        for with_words in (True, False):
            a0, l0 = (ACC0, LAST0) if with_words else (0, 0)
            wm, wf, wacc, wlast = RX16.oracle(pair, fcw, pm, x, y, PHASE0, a0, DPHASE0, l0)
            words = lambda: ((last_word(torch, a0), last_word(torch, l0)) if with_words
                             else (None, None))
            acc, last = words()
            gm, gf = run(torch, plan, ccfg, None, fcw, pm, x, y, PHASE0, acc, DPHASE0, last,
                         c=1 + n % 3)
            acc2, last2 = words()
            tm, tf = RX16.run(torch, plan, ccfg, fcw, pm, x, y, PHASE0, acc2, DPHASE0, last2,
                              "rx16")
            what = (pair, n, with_words)
            assert np.array_equal(gm, wm) and np.array_equal(gf, wf), what
            assert np.array_equal(gm, tm) and np.array_equal(gf, tf), what
            if with_words:
                assert last_value(acc) == wacc == last_value(acc2), what
                assert last_value(last) == wlast == last_value(last2), what
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stages", MIX.INSTANCES)
def test_gpu_every_rotator_instance_of_the_new_units_equals_the_oracle(stages, monkeypatch):
    """fm_rx_xydir<30, N, IoC16> and fm_rx_decim_xydir<30, N, IoC16> for all 7 N:
    16-bit ports with 15 extra bits (WW 32) into io16, n = 2049 (k = 3: 2048)"""
    import torch
    monkeypatch.delenv("CORDIC_FMRX_MAX_BLOCKS", raising=False)
    monkeypatch.delenv("CORDIC_FMRXD_MAX_BLOCKS", raising=False)
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    name = "instc16_%d" % stages
    MIX16.CORES16[name] = ((ca.P2R, 16, 16, 15, 32, stages), 0)
    RX16.PAIRS[name] = (name, "io16", 1)
    try:
        mcfg, _, ccfg, _, _ = RX16.configs(name)
        assert mcfg.ww == 32 and mcfg.nlive == stages and mcfg.pw == 32
        plan = ca.Plan(mcfg)
        assert plan.fm_rx_c16_info(ccfg) == (1, 1024)
        n = 2049
        fcw, pm, x, y = RX16.data(n, 500 + stages)
        wm, wf, wacc, wlast = RX16.oracle(name, fcw, pm, x, y, PHASE0, ACC0, DPHASE0, LAST0)
        acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
        gm, gf = run(torch, plan, ccfg, None, fcw, pm, x, y, PHASE0, acc, DPHASE0, last, c=3)
        assert np.array_equal(gm, wm) and np.array_equal(gf, wf), stages
        assert last_value(acc) == wacc and last_value(last) == wlast, stages
        P, k, s = RXD.Pair(name), 3, slice(0, 2048)
        W = RXD.Want(P, k, fcw[s], pm[s], x[s], y[s], PHASE0, ACC0, DPHASE0, LAST0)
        wm, wf, wacc, wlast = W.prefix(2048 >> k)
        acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
        gm, gf = run(torch, plan, ccfg, k, fcw[s], pm[s], x[s], y[s], PHASE0, acc, DPHASE0,
                     last, c=2)
        assert np.array_equal(gm, wm) and np.array_equal(gf, wf), (stages, k)
        assert last_value(acc) == wacc and last_value(last) == wlast, (stages, k)
        plan.close()
    finally:
        del MIX16.CORES16[name], RX16.PAIRS[name]


@pytest.mark.gpu
def test_gpu_a_halo_inside_a_span_of_three_passes_gives_the_same_bits(monkeypatch):
    import torch
    monkeypatch.setenv("CORDIC_FMRX_MAX_BLOCKS", "2")
    pair = "cfg1-io16"
    mcfg, _, ccfg, _, _ = RX16.configs(pair)
    plan = ca.Plan(mcfg)
    n = 5 * 1024 + 3
    for with_pm in (True, False):
        fcw, pm, x, y = RX16.data(n, 41, with_pm)
        wm, wf, wacc, wlast = RX16.oracle(pair, fcw, pm, x, y, PHASE0, ACC0, DPHASE0, LAST0)
        acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
        gm, gf = run(torch, plan, ccfg, None, fcw, pm, x, y, PHASE0, acc, DPHASE0, last, c=3)
        assert np.array_equal(gm, wm) and np.array_equal(gf, wf), with_pm
        assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_gpu_three_calls_that_share_both_words_equal_one_call(pair):
    import torch
    mcfg, _, ccfg, _, _ = RX16.configs(pair)
    n, cuts = 3 * 1024 + 7, (0, 1021, 2050, 3 * 1024 + 7)
    fcw, pm, x, y = RX16.data(n, 5)
    wm, wf, wacc, wlast = RX16.oracle(pair, fcw, pm, x, y, PHASE0, 0, DPHASE0, 0)
    plan = ca.Plan(mcfg)
    acc, last = last_word(torch, 0), last_word(torch, 0)
    gm, gf = [], []
    for j in range(3):
        s = slice(cuts[j], cuts[j + 1])
        m, f = run(torch, plan, ccfg, None, fcw[s], pm[s], x[s], y[s], PHASE0 if j == 0 else 0,
                   acc, DPHASE0 if j == 0 else 0, last, c=1 + j)
        gm.append(m)
        gf.append(f)
    assert np.array_equal(np.concatenate(gm), wm)
    assert np.array_equal(np.concatenate(gf), wf)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()


def replay_three_times(torch, call, mag, freq, fused, wm, wf, m, tag):
    """captures call(stream) once; fused: two kernel nodes with one edge.  Replay
    r gives samples [r m, (r + 1) m) of the job three times as long"""
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
                s = slice(r * m, (r + 1) * m)
                assert np.array_equal(mag.get(), wm[s]), (tag, r)
                assert np.array_equal(freq.get(), wf[s]), (tag, r)
        finally:
            hip.hipGraphExecDestroy(ex)
    finally:
        hip.hipGraphDestroy(graph)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [None, 3])
def test_gpu_a_captured_fused_call_is_two_kernel_nodes_and_continues_on_replay(k, monkeypatch):
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    pair = "cfg1-io16"
    P = RXD.Pair(pair)
    n = 2049 if k is None else 1025 << k
    m = n if k is None else n >> k
    fcw, pm, x, y = RX16.data(n, 9)
    rep = lambda a: np.concatenate([a, a, a])
    if k is None:
        wm, wf, wacc, wlast = RX16.oracle(pair, rep(fcw), rep(pm), rep(x), rep(y), 0, ACC0, 0,
                                          LAST0)
    else:
        wm, wf, wacc, wlast = RXD.Want(P, k, rep(fcw), rep(pm), rep(x), rep(y), 0, ACC0, 0,
                                       LAST0).prefix(3 * m)
    plan = P.plan()
    i32 = lambda a: a.view(np.int32)
    df, dm = Padded(torch, n, 1, src=i32(fcw)), Padded(torch, n, 3, src=i32(pm))
    diq = iq_buffer(torch, x, y, 3)
    mag, freq = Padded(torch, m, 1, True), Padded(torch, m, 5, True)
    acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
    if k is None:
        work = zeros(torch, plan.fm_rx_c16_workspace(P.ccfg, n))
        call = lambda a, l, s: plan.fm_rx_c16(P.ccfg, df.view, diq.view, mag.view, freq.view,
                                              work, pm=dm.view, n=n, acc=a, last=l, stream=s)
    else:
        work = zeros(torch, plan.fm_rx_decim_c16_workspace(P.ccfg, n, k))
        call = lambda a, l, s: plan.fm_rx_decim_c16(P.ccfg, k, df.view, diq.view, mag.view,
                                                    freq.view, work, pm=dm.view, n=n, acc=a,
                                                    last=l, stream=s)
    call(last_word(torch, 0), last_word(torch, 0), None)    # once outside the capture
    torch.cuda.synchronize()
    mag.t.fill_(mag.sent)
    freq.t.fill_(freq.sent)
    replay_three_times(torch, lambda s: call(acc, last, s), mag, freq, True, wm, wf, m, k)
    assert last_value(acc) == wacc and last_value(last) == wlast
    assert np.array_equal(diq.get(), interleave(x, y))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_gpu_overlaps_and_bad_pointers_are_refused_and_nothing_is_written(pair):
    """d_iq's byte range is 4 n: what lies on its last short is an overlap, in
    its second half as in its first; one short behind it is clear"""
    import torch
    mcfg, _, ccfg, _, _ = RX16.configs(pair)
    n = 1024
    fcw, pm, x, y = RX16.data(n, 13)
    plan = ca.Plan(mcfg)
    work = zeros(torch, plan.fm_rx_c16_workspace(ccfg, n))
    i32 = lambda a: a.view(np.int32)
    df, dm = Padded(torch, n, 1, src=i32(fcw)), Padded(torch, n, 3, src=i32(pm))
    diq = iq_buffer(torch, x, y, 1)
    mag, freq = Padded(torch, n, 1, True), Padded(torch, n, 5, True)
    acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
    L = ca.lib()

    def call(k=None, **kw):
        a = dict(fcw=df.view, pm=dm.view, acc=acc, iq=diq.view, last=last, mag=mag.view,
                 freq=freq.view, work=work)
        a.update(kw)
        ptr = lambda v: v if isinstance(v, (int, type(None))) else C.c_void_p(v.data_ptr())
        head = (plan._h, ccfg.ref, n) + (() if k is None else (k,))
        fn = L.cordic_plan_fm_rx_c16 if k is None else L.cordic_plan_fm_rx_decim_c16
        return fn(*head, ptr(a["fcw"]), ptr(a["pm"]), 0, ptr(a["acc"]), ptr(a["iq"]), 0,
                  ptr(a["last"]), ptr(a["mag"]), ptr(a["freq"]), ptr(a["work"]), None)

    at = lambda p, j: p.view.data_ptr() + 2 * j      # short j of an array
    word_in = lambda p, j: (at(p, j) + 3) & ~3       # a 4-byte-aligned word at or behind it
    bad = [dict(mag=diq.view), dict(freq=diq.view), dict(mag=at(diq, n - 1)),
           dict(mag=at(diq, n)), dict(freq=at(diq, 2 * n - 1)),     # the second half
           dict(mag=at(diq, 2)), dict(last=word_in(diq, 3)), dict(last=word_in(diq, 2 * n - 2)),
           dict(acc=word_in(diq, n + 4)), dict(acc=word_in(diq, 8)),
           dict(iq=at(diq, 1)), dict(iq=at(diq, 0) + 1), dict(iq=None),
           dict(work=diq.view.data_ptr() & ~15), dict(work=(at(diq, 2 * n - 1) & ~15)),
           dict(mag=freq.view), dict(freq=at(mag, 3)), dict(mag=df.view),
           dict(last=word_in(mag, 5)), dict(acc=last), dict(work=mag.view), dict(fcw=None),
           dict(mag=None), dict(freq=None), dict(work=None), dict(mag=at(mag, 0) + 1),
           dict(last=last.data_ptr() + 2), dict(work=work.data_ptr() + 8)]
    for kw in bad:
        assert call(**kw) == ca.ERR_ARGS, sorted(kw)
        assert call(k=3, **kw) == ca.ERR_ARGS, sorted(kw)
    torch.cuda.synchronize()
    assert mag.untouched() and freq.untouched()
    assert np.array_equal(diq.get(), interleave(x, y))
    assert np.array_equal(df.get(), i32(fcw)) and np.array_equal(dm.get(), i32(pm))
    assert last_value(acc) == ACC0 and last_value(last) == LAST0
    assert not work.any().item()
    # one short behind the 4 n bytes is clear: the outputs packed against d_iq
    tight = torch.full((2 + 2 * n + n + n + 8,), 0x5a5a, dtype=torch.int16,
                       device=work.device)
    tight[2:2 + 2 * n].copy_(torch.from_numpy(interleave(x, y)).to(work.device))
    iq, m2, f2 = tight[2:], tight[2 + 2 * n:], tight[2 + 3 * n:]
    assert call(iq=iq, mag=m2, freq=f2) == 0        # and the same call, clean
    torch.cuda.synchronize()
    wm, wf, wacc, wlast = RX16.oracle(pair, fcw, pm, x, y, 0, ACC0, 0, LAST0)
    h = tight.cpu().numpy()
    assert np.array_equal(h[2:2 + 2 * n], interleave(x, y))
    assert np.array_equal(h[2 + 2 * n:2 + 3 * n], wm) and np.array_equal(h[2 + 3 * n:2 + 4 * n], wf)
    assert (h[:2] == 0x5a5a).all() and (h[2 + 4 * n:] == 0x5a5a).all()
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()


# ---------------------------------------------------------------- the decimating call

@pytest.mark.gpu
@pytest.mark.parametrize("with_pm", [True, False])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("pair", PAIRS)
def test_gpu_every_decimated_length_equals_the_oracle_and_the_16_bit_call(pair, k, with_pm,
                                                                         monkeypatch):
    """every m of RXD.MS as a prefix of one job's data, as RXD.check_lengths"""
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_MAX_BLOCKS", raising=False)
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = RXD.Pair(pair)
    plan = P.plan()
    fcw, pm, x, y = P.data(max(RXD.MS) << k, 2000 + 10 * k + with_pm, with_pm)
    W = RXD.Want(P, k, fcw, pm, x, y, PHASE0, ACC0, DPHASE0, LAST0)
    for m in RXD.MS:
        n = m << k
        wm, wf, wacc, wlast = W.prefix(m)
        a = (fcw[:n], None if pm is None else pm[:n], x[:n], y[:n])
        for with_words in (True, False):
            words = lambda: ((last_word(torch, ACC0), last_word(torch, LAST0)) if with_words
                             else (None, None))
            p0, d0 = (PHASE0, DPHASE0) if with_words else (PHASE0 + ACC0, DPHASE0 + LAST0)
            acc, last = words()
            gm, gf = run(torch, plan, P.ccfg, k, *a, p0, acc, d0, last, c=1 + m % 3)
            what = (pair, k, m, with_words)
            assert np.array_equal(gm, wm) and np.array_equal(gf, wf), what
            if with_words:
                assert last_value(acc) == wacc and last_value(last) == wlast, what
            if with_words or m % 64 == 1:           # the twin, on split copies
                acc2, last2 = words()
                tm, tf = RXD.run(torch, P, plan, k, *a, p0, acc2, d0, last2)
                assert np.array_equal(gm, tm) and np.array_equal(gf, tf), what
                if with_words:
                    assert last_value(acc2) == wacc and last_value(last2) == wlast, what
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_gpu_k_0_is_the_plain_call(pair):
    import torch
    P = RXD.Pair(pair)
    plan = P.plan()
    for n in LENGTHS:
        fcw, pm, x, y = P.data(n, 2200 + n)
        acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
        gm, gf = run(torch, plan, P.ccfg, 0, fcw, pm, x, y, PHASE0, acc, DPHASE0, last, c=2)
        acc2, last2 = last_word(torch, ACC0), last_word(torch, LAST0)
        pm_, pf = run(torch, plan, P.ccfg, None, fcw, pm, x, y, PHASE0, acc2, DPHASE0, last2, c=2)
        assert np.array_equal(gm, pm_) and np.array_equal(gf, pf), n
        assert last_value(acc) == last_value(acc2) and last_value(last) == last_value(last2)
        assert plan.fm_rx_decim_c16_workspace(P.ccfg, n, 0) == plan.fm_rx_c16_workspace(P.ccfg, n)
    plan.close()


@pytest.mark.gpu
def test_gpu_the_forced_fallback_gives_the_fused_bits(monkeypatch):
    import torch
    P = RXD.Pair("cfg1-io16")
    plan = P.plan()
    k, m = 3, 1283
    n = m << k
    fcw, pm, x, y = P.data(n, 2400)
    wm, wf, wacc, wlast = RXD.Want(P, k, fcw, pm, x, y, PHASE0, ACC0, DPHASE0, LAST0).prefix(m)
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    fused_bytes = plan.fm_rx_decim_c16_workspace(P.ccfg, n, k)
    assert fused_bytes == plan.fm_rx16_workspace(P.ccfg, n)
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("CORDIC_FMRXD_FALLBACK", "1")
            assert plan.fm_rx_decim_c16_workspace(P.ccfg, n, k) \
                >= plan.fm_rx_decim16_workspace(P.ccfg, n, k) + 4 * n > fused_bytes
        acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
        gm, gf = run(torch, plan, P.ccfg, k, fcw, pm, x, y, PHASE0, acc, DPHASE0, last, c=1)
        assert np.array_equal(gm, wm) and np.array_equal(gf, wf), forced
        assert last_value(acc) == wacc and last_value(last) == wlast, forced
    plan.close()


@pytest.mark.gpu
def test_gpu_a_decimating_halo_inside_a_span_of_several_passes_gives_the_same_bits(monkeypatch):
    """k = 3 on two blocks: 11 passes, spans of 6, a halo of two lanes"""
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = RXD.Pair("cfg1-io16")
    plan = P.plan()
    k, m = 3, 1283
    n = m << k
    fcw, pm, x, y = P.data(n, 2303)
    wm, wf, wacc, wlast = RXD.Want(P, k, fcw, pm, x, y, PHASE0, ACC0, DPHASE0, LAST0).prefix(m)
    for cap in ("2", None):
        if cap:
            monkeypatch.setenv("CORDIC_FMRXD_MAX_BLOCKS", cap)
        else:
            monkeypatch.delenv("CORDIC_FMRXD_MAX_BLOCKS")
        acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
        gm, gf = run(torch, plan, P.ccfg, k, fcw, pm, x, y, PHASE0, acc, DPHASE0, last, c=3)
        assert np.array_equal(gm, wm) and np.array_equal(gf, wf), cap
        assert last_value(acc) == wacc and last_value(last) == wlast, cap
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair, k", [("cfg1-io16", 1), ("cfg1-io16", 3), ("cfg1-ww36", 2)])
def test_gpu_three_decimating_calls_cut_at_multiples_of_r_equal_one_call(pair, k, monkeypatch):
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = RXD.Pair(pair)
    m, cuts = 2049 + 7, (0, 1021, 2050, 2049 + 7)
    fcw, pm, x, y = P.data(m << k, 5)
    wm, wf, wacc, wlast = RXD.Want(P, k, fcw, pm, x, y, PHASE0, 0, DPHASE0, 0).prefix(m)
    plan = P.plan()
    acc, last = last_word(torch, 0), last_word(torch, 0)
    gm, gf = [], []
    for j in range(3):
        s = slice(cuts[j] << k, cuts[j + 1] << k)
        a, b = run(torch, plan, P.ccfg, k, fcw[s], pm[s], x[s], y[s], PHASE0 if j == 0 else 0,
                   acc, DPHASE0 if j == 0 else 0, last, c=1 + j)
        gm.append(a)
        gf.append(b)
    assert np.array_equal(np.concatenate(gm), wm)
    assert np.array_equal(np.concatenate(gf), wf)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()
