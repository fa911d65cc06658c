"""The FM mixer on interleaved int16 I/Q, in and out (cordic_plan_fm_mix_c16 and
cordic_plan_fm_mix_decim_c16; include/cordic_amd.h): every output short and the
word at d_acc against the oracle on (iq[0::2], iq[1::2]) -- want16 of
tests/test_fm_mix16.py, summed in 64 bits by decimate of
tests/test_fm_mix_decim.py -- and against the *16 twin on split copies.
Nothing has a tolerance.  Every iq and oiq buffer lies 1, 2 or 3 complex samples
off the 16-byte grid, the two at different offsets, between sentinels, and the
inputs are read back unchanged after every call."""
import ctypes as C

import numpy as np
import pytest

import cordic_amd as ca
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
import test_fm_mix_decim as MIXD
from test_fm_demod import Padded, last_value, last_word
from test_fm_mix import PHASE0, PRESET
from test_fm_rx_c16 import replay_three_times
from test_table_fm import expected as phases, words

FUSED = ("cfg1", "nat16", "pw32")
FALLBACK = ("n9", "cfg1_ug", "sp2r16", "ww35_16")
KNOBS = ("CORDIC_FMX_MAX_BLOCKS", "CORDIC_FMXD_FALLBACK")


def interleave(x, y):
    iq = np.empty(2 * x.size, dtype=np.int16)
    iq[0::2], iq[1::2] = x, y
    return iq


def zeros(torch, nbytes):
    from gpu_util import DEV
    return torch.zeros(max(16, nbytes), dtype=torch.uint8, device=DEV)


def workspace(plan, n, k):
    return plan.fm_mix_c16_workspace(n) if k is None else plan.fm_mix_decim_c16_workspace(n, k)


def buffers(torch, fcw, pm, x, y, m, c):
    """fcw, pm, iq (c complex samples off the grid) and oiq (m complex samples,
    at another offset) between sentinels"""
    assert c in (1, 2, 3)
    i32 = lambda a: None if a is None else a.view(np.int32)
    n = x.size
    df = Padded(torch, n, 1 + c % 3, src=i32(fcw))
    dm = None if pm is None else Padded(torch, n, 3, src=i32(pm))
    diq = Padded(torch, 2 * n, 2 * c, True, src=interleave(x, y))
    oiq = Padded(torch, 2 * m, 2 * (1 + c % 3), True)
    return df, dm, diq, oiq


def run(torch, plan, k, fcw, pm, x, y, phase0=0, acc=None, c=1, work=None):
    """one call of the interleaved form (k None: the plain call); (ox, oy) after
    checking the sentinels -- the short directly behind d_oiq[2 m - 1] among
    them -- and that no input was written"""
    n = x.size
    m = n if k is None else n >> k
    i32 = lambda a: None if a is None else a.view(np.int32)
    df, dm, diq, oiq = buffers(torch, fcw, pm, x, y, m, c)
    if work is None:
        work = zeros(torch, workspace(plan, n, k))
    kw = dict(pm=None if dm is None else dm.view, n=n, phase0=phase0, acc=acc)
    if k is None:
        plan.fm_mix_c16(df.view, diq.view, oiq.view, work, **kw)
    else:
        plan.fm_mix_decim_c16(k, df.view, diq.view, oiq.view, work, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(df.get(), i32(fcw))
    assert dm is None or np.array_equal(dm.get(), i32(pm))
    assert np.array_equal(diq.get(), interleave(x, y))
    assert int(oiq.t[oiq.off + 2 * m].item()) == oiq.sent       # directly behind the last Q
    got = oiq.get()
    return got[0::2].copy(), got[1::2].copy()


def twin(torch, plan, k, fcw, pm, x, y, phase0=0, acc=None):
    """the *16 call on split copies (k None: cordic_plan_fm_mix16)"""
    if k is None:
        return MIX16.run16(torch, plan, MIX16.work_buffer(torch, plan, x.size), fcw, pm, x, y,
                           phase0, acc, MIX16.offsets(1))
    return MIXD.run(torch, plan, k, MIXD.work_buffer(torch, plan, x.size, k, True), fcw, pm, x,
                    y, phase0, acc, True)


def data(name, n, seed, with_pm=True):
    cfg = MIXD.core(name, True)
    rng = np.random.default_rng(seed)
    x, y = MIX16.iq16(rng, n, cfg.iw)
    return words("random", n, seed + 1), (words("random", n, seed + 2) if with_pm else None), x, y


def want(name, k, fcw, pm, x, y, phase0, start):
    """the oracle's (ox, oy) and the word behind the call"""
    p, final = phases(fcw, pm, phase0, start)
    wx, wy = MIXD.tuned(name, True, x, y, p)
    if k:
        wx, wy = MIXD.decimate(wx, k), MIXD.decimate(wy, k)
    return wx, wy, final


def clear(monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)


# ---------------------------------------------------------------- the plain call

@pytest.mark.gpu
@pytest.mark.parametrize("name,fused", [("cfg1", 1), ("n9", 0)])
def test_gpu_the_path_query_is_the_twins_and_a_fused_workspace_is_the_twins(name, fused,
                                                                           monkeypatch):
    clear(monkeypatch)
    a16 = lambda b: (b + 15) // 16 * 16
    plan = ca.Plan(MIXD.core(name, True))
    assert MIX16.fused16(plan) == bool(fused)
    assert plan.fm_mix_c16_info() == (fused, 1024 if fused else 0)
    assert plan.fm_mix_c16_info() == (plan.fm_mix_info() if plan.cfg.ww < 35 else (0, 0))
    for n in (0, 1, 255, 1024, 1 << 20, 1 << 33):
        w, tw = plan.fm_mix_c16_workspace(n), plan.fm_mix16_workspace(n)
        assert w == (tw if fused or not n else a16(tw) + 4 * a16(2 * n)), n
        for k in (0, 3):
            wd, tw = plan.fm_mix_decim_c16_workspace(n, k), plan.fm_mix_decim16_workspace(n, k)
            assert wd == (tw if fused or not tw
                          else a16(tw) + 2 * a16(2 * n) + 2 * a16(2 * (n >> k))), (n, k)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_pm", [True, False])
@pytest.mark.parametrize("name", FUSED + FALLBACK)
def test_gpu_every_length_equals_the_oracle_and_the_16_bit_call_on_split_copies(
        name, with_pm, monkeypatch):
    import torch
    clear(monkeypatch)
    plan = ca.Plan(MIXD.core(name, True))
    assert plan.fm_mix_c16_info()[0] == (name in FUSED)
    for n in MIX16.LENGTHS:
        fcw, pm, x, y = data(name, n, 7000 + n, with_pm)
        for with_acc in (True, False):
            start = PRESET if with_acc else 0
            wx, wy, final = want(name, 0, fcw, pm, x, y, PHASE0, start)
            acc = last_word(torch, PRESET) if with_acc else None
            gx, gy = run(torch, plan, None, fcw, pm, x, y, PHASE0, acc, c=1 + n % 3)
            what = (name, n, with_pm, with_acc)
            assert np.array_equal(gx, wx) and np.array_equal(gy, wy), what
            acc2 = last_word(torch, PRESET) if with_acc else None
            tx, ty = twin(torch, plan, None, fcw, pm, x, y, PHASE0, acc2)
            assert np.array_equal(gx, tx) and np.array_equal(gy, ty), what
            if with_acc:
                assert last_value(acc) == final == last_value(acc2), what
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [None, 2])
def test_gpu_the_two_shorts_of_every_output_dword_are_the_oracles_independently(k, monkeypatch):
    """zero tuning words and a zero phase on cfg1 (no unit gain), full-scale
    random I/Q at n = 1024: the outputs have all four sign combinations, so a
    negative I that bled into Q, or a Q that lost its sign, would show"""
    import torch
    clear(monkeypatch)
    name, n = "cfg1", 1024
    plan = ca.Plan(MIXD.core(name, True))
    _, _, x, y = data(name, n, 99)
    assert x.min() == y.min() == -32768 and x.max() == y.max() == 32767     # +- full scale
    fcw = np.zeros(n, dtype=np.uint32)
    wx, wy, _ = want(name, k or 0, fcw, None, x, y, 0, 0)
    signs = {(bool(a < 0), bool(b < 0)) for a, b in zip(wx, wy)}
    assert signs == {(False, False), (False, True), (True, False), (True, True)}
    m = n >> (k or 0)
    df, _, diq, oiq = buffers(torch, fcw, None, x, y, m, 3)
    work = zeros(torch, workspace(plan, n, k))
    if k is None:
        plan.fm_mix_c16(df.view, diq.view, oiq.view, work, n=n)
    else:
        plan.fm_mix_decim_c16(k, df.view, diq.view, oiq.view, work, n=n)
    torch.cuda.synchronize()
    dwords = oiq.get().view(np.uint32)
    assert dwords.size == m
    assert np.array_equal((dwords & 0xffff).astype(np.uint16), wx.view(np.uint16))
    assert np.array_equal((dwords >> 16).astype(np.uint16), wy.view(np.uint16))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg1", "n9"])
def test_gpu_the_short_behind_a_partial_last_vector_is_intact(name, monkeypatch):
    """n % 4 in (1, 2, 3), and decimated lengths n >> k that are no multiple of
    4: run() looks at the sentinel directly behind d_oiq[2 m - 1]"""
    import torch
    clear(monkeypatch)
    plan = ca.Plan(MIXD.core(name, True))
    for k, ms in ((None, (1, 2, 3, 1025, 1026, 1027)), (1, (1, 2, 3, 513, 1026, 2051)),
                  (2, (1, 3, 257, 258)), (3, (5, 6, 7, 129))):
        for m in ms:
            n = m << (k or 0)
            fcw, pm, x, y = data(name, n, 300 + m)
            wx, wy, final = want(name, k or 0, fcw, pm, x, y, PHASE0, PRESET)
            acc = last_word(torch, PRESET)
            gx, gy = run(torch, plan, k, fcw, pm, x, y, PHASE0, acc, c=1 + m % 3)
            assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (k, m)
            assert last_value(acc) == final, (k, m)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stages", MIX.INSTANCES)
def test_gpu_every_rotator_instance_of_the_new_units_equals_the_oracle(stages, monkeypatch):
    """fm_mix_xydir<30, N, IoC16io> and fm_mix_decim_xydir<30, N, IoC16io> for all
    7 N: 16-bit ports with 15 extra bits (WW 32), n = 2049 (k = 3: 2048)"""
    import torch
    clear(monkeypatch)
    name = "mixc16_%d" % stages
    MIX16.CORES16[name] = ((ca.P2R, 16, 16, 15, 32, stages), 0)
    try:
        cfg = MIXD.core(name, True)
        assert cfg.ww == 32 and cfg.nlive == stages and cfg.pw == 32
        plan = ca.Plan(cfg)
        assert plan.fm_mix_c16_info() == (1, 1024)
        n = 2049
        fcw, pm, x, y = data(name, n, 500 + stages)
        wx, wy, final = want(name, 0, fcw, pm, x, y, PHASE0, PRESET)
        acc = last_word(torch, PRESET)
        gx, gy = run(torch, plan, None, fcw, pm, x, y, PHASE0, acc, c=3)
        assert np.array_equal(gx, wx) and np.array_equal(gy, wy), stages
        assert last_value(acc) == final, stages
        k, s = 3, slice(0, 2048)
        acc = last_word(torch, PRESET)
        gx, gy = run(torch, plan, k, fcw[s], pm[s], x[s], y[s], PHASE0, acc, c=2)
        assert np.array_equal(gx, MIXD.decimate(wx[s], k)), (stages, k)
        assert np.array_equal(gy, MIXD.decimate(wy[s], k)), (stages, k)
        assert last_value(acc) == MIXD.acc_after(fcw, 2048, PHASE0 + PRESET), (stages, k)
        plan.close()
    finally:
        del MIX16.CORES16[name]


@pytest.mark.gpu
@pytest.mark.parametrize("k,n", [(None, 5 * 1024 + 3), (3, 1283 << 3)])
def test_gpu_several_passes_per_block_give_the_same_bits(k, n, monkeypatch):
    import torch
    clear(monkeypatch)
    name = "cfg1"
    plan = ca.Plan(MIXD.core(name, True))
    for with_pm in (True, False):
        fcw, pm, x, y = data(name, n, 41, with_pm)
        wx, wy, final = want(name, k or 0, fcw, pm, x, y, PHASE0, PRESET)
        for cap in ("2", None):
            if cap:
                monkeypatch.setenv("CORDIC_FMX_MAX_BLOCKS", cap)
            else:
                monkeypatch.delenv("CORDIC_FMX_MAX_BLOCKS")
            acc = last_word(torch, PRESET)
            gx, gy = run(torch, plan, k, fcw, pm, x, y, PHASE0, acc, c=3)
            assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (with_pm, cap)
            assert last_value(acc) == final, (with_pm, cap)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("cfg1", None), ("n9", None), ("cfg1", 1), ("cfg1", 3),
                                    ("n9", 2)])
def test_gpu_three_calls_that_share_the_accumulator_equal_one_call(name, k, monkeypatch):
    """cut at 1021 and 2050 (<< k for the decimating form: multiples of R)"""
    import torch
    clear(monkeypatch)
    sh = k or 0
    m, cuts = 3 * 1024 + 7, (0, 1021, 2050, 3 * 1024 + 7)
    fcw, pm, x, y = data(name, m << sh, 5)
    wx, wy, final = want(name, sh, fcw, pm, x, y, PHASE0, 0)
    plan = ca.Plan(MIXD.core(name, True))
    acc = last_word(torch, 0)
    gx, gy = [], []
    for j in range(3):
        s = slice(cuts[j] << sh, cuts[j + 1] << sh)
        a, b = run(torch, plan, k, fcw[s], pm[s], x[s], y[s], PHASE0 if j == 0 else 0, acc,
                   c=1 + j)
        gx.append(a)
        gy.append(b)
    assert np.array_equal(np.concatenate(gx), wx) and np.array_equal(np.concatenate(gy), wy)
    assert last_value(acc) == final
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [None, 3])
def test_gpu_a_captured_fused_call_is_two_kernel_nodes_and_continues_on_replay(k, monkeypatch):
    import torch
    clear(monkeypatch)
    name, sh = "cfg1", k or 0
    n = 2049 if k is None else 1025 << k
    m = n >> sh
    fcw, pm, x, y = data(name, n, 9)
    rep = lambda a: np.concatenate([a, a, a])
    wx, wy, final = want(name, sh, rep(fcw), rep(pm), rep(x), rep(y), 0, PRESET)
    w = interleave(wx, wy)
    plan = ca.Plan(MIXD.core(name, True))
    df, dm, diq, oiq = buffers(torch, fcw, pm, x, y, m, 3)
    work = zeros(torch, workspace(plan, n, k))
    if k is None:
        call = lambda a, s: plan.fm_mix_c16(df.view, diq.view, oiq.view, work, pm=dm.view, n=n,
                                            acc=a, stream=s)
    else:
        call = lambda a, s: plan.fm_mix_decim_c16(k, df.view, diq.view, oiq.view, work,
                                                  pm=dm.view, n=n, acc=a, stream=s)
    call(last_word(torch, 0), None)             # once outside the capture
    torch.cuda.synchronize()
    oiq.t.fill_(oiq.sent)
    acc = last_word(torch, PRESET)
    replay_three_times(torch, lambda s: call(acc, s), oiq, oiq, True, w, w, 2 * m, k)
    assert last_value(acc) == final
    assert np.array_equal(diq.get(), interleave(x, y))
    plan.close()


@pytest.mark.gpu
def test_gpu_overlaps_and_bad_pointers_are_refused_and_nothing_is_written(monkeypatch):
    """d_iq's byte range is 4 n and d_oiq's 4 (n >> k): what lies on the last
    short of d_iq is an overlap, in its second half as in its first; d_oiq packed
    directly behind d_iq's 4 n bytes is accepted and correct"""
    import torch
    clear(monkeypatch)
    L = ca.lib()
    for name in ("cfg1", "n9"):
        n = 1024
        fcw, pm, x, y = data(name, n, 13)
        plan = ca.Plan(MIXD.core(name, True))
        work = zeros(torch, max(workspace(plan, n, None), workspace(plan, n, 3)))
        df, dm, diq, oiq = buffers(torch, fcw, pm, x, y, n, 1)
        acc = last_word(torch, PRESET)
        other = last_word(torch, 7)

        def call(k=None, **kw):
            a = dict(fcw=df.view, pm=dm.view, acc=acc, iq=diq.view, oiq=oiq.view, work=work)
            a.update(kw)
            ptr = lambda v: v if isinstance(v, (int, type(None))) else C.c_void_p(v.data_ptr())
            head = (plan._h, n) + (() if k is None else (k,))
            fn = L.cordic_plan_fm_mix_c16 if k is None else L.cordic_plan_fm_mix_decim_c16
            return fn(*head, ptr(a["fcw"]), ptr(a["pm"]), 0, ptr(a["acc"]), ptr(a["iq"]),
                      ptr(a["oiq"]), ptr(a["work"]), None)

        at = lambda p, j: p.view.data_ptr() + 2 * j      # short j of an array
        bad = [dict(oiq=diq.view),                       # in place: the first short
               dict(oiq=at(diq, 2 * n - 2)),             # the last short (its dword)
               dict(oiq=at(diq, n)), dict(oiq=at(diq, n + 2)),      # the second half
               dict(oiq=at(diq, 2)),
               dict(acc=at(diq, 4)), dict(acc=at(diq, 2 * n - 2)), dict(acc=at(diq, n + 4)),
               dict(acc=at(oiq, 0)), dict(acc=at(oiq, 2 * (n >> 3) - 2)),
               dict(work=diq.view.data_ptr() & ~15), dict(work=at(diq, 2 * n - 1) & ~15),
               dict(work=oiq.view.data_ptr() & ~15),
               dict(iq=at(diq, 1)), dict(oiq=at(oiq, 1)), dict(iq=at(diq, 0) + 1),
               dict(iq=None), dict(oiq=None), dict(fcw=None), dict(work=None),
               dict(oiq=df.view), dict(oiq=dm.view), dict(work=work.data_ptr() + 8),
               dict(acc=other.data_ptr() + 2)]
        for kw in bad:
            assert call(**kw) == ca.ERR_ARGS, (name, sorted(kw))
            assert call(k=3, **kw) == ca.ERR_ARGS, (name, sorted(kw))
        # (behind a decimating call's 4 (n >> k) bytes, inside the plain call's 4 n)
        assert call(acc=at(oiq, 2 * (n >> 3) + 2)) == ca.ERR_ARGS
        torch.cuda.synchronize()
        assert oiq.untouched()
        assert np.array_equal(diq.get(), interleave(x, y))
        i32 = lambda a: a.view(np.int32)
        assert np.array_equal(df.get(), i32(fcw)) and np.array_equal(dm.get(), i32(pm))
        assert last_value(acc) == PRESET and last_value(other) == 7
        assert not work.any().item()
        # the tight case, and the same call clean
        for k in (None, 3):
            m = n >> (k or 0)
            tight = torch.full((2 + 2 * n + 2 * m + 8,), 0x5a5a, dtype=torch.int16,
                               device=work.device)
            tight[2:2 + 2 * n].copy_(torch.from_numpy(interleave(x, y)).to(work.device))
            acc = last_word(torch, PRESET)
            assert call(k, iq=tight[2:], oiq=tight[2 + 2 * n:], acc=acc) == 0
            torch.cuda.synchronize()
            wx, wy, final = want(name, k or 0, fcw, pm, x, y, 0, PRESET)
            h = tight.cpu().numpy()
            assert np.array_equal(h[2:2 + 2 * n], interleave(x, y))
            assert np.array_equal(h[2 + 2 * n:2 + 2 * n + 2 * m], interleave(wx, wy)), (name, k)
            assert (h[:2] == 0x5a5a).all() and (h[2 + 2 * n + 2 * m:] == 0x5a5a).all()
            assert last_value(acc) == final
        plan.close()


# ---------------------------------------------------------------- the decimating call

@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["nat16", "n9"])
def test_gpu_every_decimated_length_equals_the_oracle_and_the_16_bit_call(name, k, monkeypatch):
    """the lengths of MIXD.lengths(k) as prefixes of MIXD.reference's one job"""
    import torch
    clear(monkeypatch)
    plan = ca.Plan(MIXD.core(name, True))
    assert plan.fm_mix_c16_info()[0] == (name == "nat16")
    x, y, fcw, pm, full, bare = MIXD.reference(name, True)
    for n in MIXD.lengths(k):
        acc = last_word(torch, PRESET)
        gx, gy = run(torch, plan, k, fcw[:n], pm[:n], x[:n], y[:n], PHASE0, acc,
                     c=1 + (n >> k) % 3)
        assert np.array_equal(gx, MIXD.decimate(full[0][:n], k)), (n, "pm, acc")
        assert np.array_equal(gy, MIXD.decimate(full[1][:n], k)), (n, "pm, acc")
        assert last_value(acc) == MIXD.acc_after(fcw, n, PHASE0 + PRESET), n
        acc2 = last_word(torch, PRESET)
        tx, ty = twin(torch, plan, k, fcw[:n], pm[:n], x[:n], y[:n], PHASE0, acc2)
        assert np.array_equal(gx, tx) and np.array_equal(gy, ty), n
        assert last_value(acc2) == last_value(acc), n
        gx, gy = run(torch, plan, k, fcw[:n], None, x[:n], y[:n], PHASE0, None, c=2)
        assert np.array_equal(gx, MIXD.decimate(bare[0][:n], k)), n
        assert np.array_equal(gy, MIXD.decimate(bare[1][:n], k)), n
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nat16", "n9"])
def test_gpu_k_0_is_the_plain_call(name, monkeypatch):
    import torch
    clear(monkeypatch)
    plan = ca.Plan(MIXD.core(name, True))
    x, y, fcw, pm, full, _ = MIXD.reference(name, True)
    for n in (1, 5, 1023, 1025, 2051):
        a = (fcw[:n], pm[:n], x[:n], y[:n])
        acc, acc2 = last_word(torch, PRESET), last_word(torch, PRESET)
        gx, gy = run(torch, plan, 0, *a, PHASE0, acc, c=2)
        px, py = run(torch, plan, None, *a, PHASE0, acc2, c=2)
        assert np.array_equal(gx, px) and np.array_equal(gy, py), n
        assert np.array_equal(gx, full[0][:n]) and np.array_equal(gy, full[1][:n]), n
        assert last_value(acc) == last_value(acc2) == MIXD.acc_after(fcw, n, PHASE0 + PRESET)
        assert plan.fm_mix_decim_c16_workspace(n, 0) == plan.fm_mix_c16_workspace(n)
    plan.close()


@pytest.mark.gpu
def test_gpu_the_forced_fallback_gives_the_fused_bits(monkeypatch):
    import torch
    clear(monkeypatch)
    name, k, m = "cfg1", 3, 1283
    n = m << k
    plan = ca.Plan(MIXD.core(name, True))
    fcw, pm, x, y = data(name, n, 2400)
    wx, wy, final = want(name, k, fcw, pm, x, y, PHASE0, PRESET)
    fused_bytes = plan.fm_mix_decim_c16_workspace(n, k)
    assert fused_bytes == plan.fm_mix16_workspace(n) == plan.fm_mix_decim16_workspace(n, k)
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("CORDIC_FMXD_FALLBACK", "1")
            assert plan.fm_mix_decim_c16_workspace(n, k) \
                >= plan.fm_mix_decim16_workspace(n, k) + 4 * n + 4 * m > fused_bytes
            # (k = 0 is the plain call: the knob does not reach it)
            assert plan.fm_mix_decim_c16_workspace(n, 0) == fused_bytes
        acc = last_word(torch, PRESET)
        gx, gy = run(torch, plan, k, fcw, pm, x, y, PHASE0, acc, c=1)
        assert np.array_equal(gx, wx) and np.array_equal(gy, wy), forced
        assert last_value(acc) == final, forced
    plan.close()
