"""The decimating FM receiver (cordic_plan_fm_rx_decim, _decim16 and their
_workspace; include/cordic_amd.h): tune, sum by R = 2^k and discriminate in one
kernel.  Every output sample and both words are compared, bit for bit, with the
existing oracle helpers composed -- MIX.want on numpy's wrapping running sum, a
64-bit sum and floor, DEM.expected -- AND with cordic_plan_fm_mix_decim into
cordic_fm_demod on the same arrays.  Lengths are in DECIMATED samples m = n / R."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O
import test_fm_demod as DEM
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
import test_fm_rx as RX
import test_fm_rx16 as RX16
from test_fm_demod import Padded, last_value, last_word
from test_fm_mix_decim import decimate
from test_fm_rx import ACC0, DPHASE0, LAST0, PAIRS, PHASE0
from test_table_fm import expected as phases, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_plan_fm_rx_decim_workspace", "cordic_plan_fm_rx_decim",
         "cordic_plan_fm_rx_decim16_workspace", "cordic_plan_fm_rx_decim16",
         "cordic_rxbank_create_decim", "cordic_rxbank_create_decim16")
M32 = 0xffffffff
# one fused pair per unit of the instance chooser; "cfg1-io16" runs on shorts
UNITS = ("nat24-cfg3", "cfg2-cfg3", "cfg1-io16")
MS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1019, 1020, 1021, 1023, 1024, 1025, 2049)
# every array 4 bytes (2 on shorts) off a 16-byte boundary, or further
OFFS = dict(fcw=1, pm=3, x=1, y=5, mag=1, freq=3)
OFFS16 = dict(fcw=1, pm=3, x=1, y=3, mag=1, freq=5)


class Pair:
    """the two cores of a pair, their container and the oracle pieces"""

    def __init__(self, pair):
        self.name, self.i16 = pair, pair in RX16.PAIRS
        if self.i16:
            self.mcfg, self.mo, self.ccfg, self.co, self.fused = RX16.configs(pair)
            self.gain = None
        else:
            m, c, self.fused, self.mcfg, self.ccfg = RX.cores(pair)
            self.m = m
            _, self.co, self.gain = DEM.both(c)
        self.offs = OFFS16 if self.i16 else OFFS

    def tuned(self, x, y, p):
        """what cordic_plan_fm_mix (_mix16) writes for the phases p, as int32"""
        if not self.i16:
            return MIX.want(self.m, x, y, p)
        mask = np.uint32((1 << self.mcfg.pw) - 1 & M32)
        return O.rotate(self.mo, MIX.sext(x, self.mcfg.iw), MIX.sext(y, self.mcfg.iw),
                        p & mask)

    def data(self, n, seed, with_pm=True):
        rng = np.random.default_rng(seed)
        x, y = MIX.iq(rng, n, self.mcfg.iw)             # full scale
        return (words("random", n, seed + 1),
                words("random", n, seed + 2) if with_pm else None, x, y)

    def plan(self):
        return ca.Plan(self.mcfg)


class Want:
    """The composed oracle of ONE job of n = m << k samples, and of every
    prefix of it that ends on a multiple of R: the phases are prefix sums and a
    frequency depends on nothing behind it."""

    def __init__(self, P, k, fcw, pm, x, y, phase0, acc0, dphase0, last0):
        p, _ = phases(fcw, pm, phase0, acc0)
        tx, ty = P.tuned(x, y, p)
        self.dx, self.dy = decimate(tx, k), decimate(ty, k)
        iw, self.pw = P.ccfg.iw, P.ccfg.pw
        self.mag, self.freq, _ = DEM.expected(P.co, P.gain, self.pw, MIX.sext(self.dx, iw),
                                              MIX.sext(self.dy, iw), dphase0 + last0)
        self.k = k
        self.acc = (np.uint64(phase0 + acc0 & M32)
                    + np.cumsum(fcw.astype(np.uint64))) & np.uint64(M32)
        # ph_j = prev + the steps up to j (mod 2^PW)
        mask = (1 << self.pw) - 1
        self.ph = ((dphase0 + last0 & mask) + np.cumsum(self.freq.astype(np.int64))) & mask

    def prefix(self, m):
        """(mag, freq, *d_acc afterwards, *d_last afterwards) of the first m"""
        return (self.mag[:m], self.freq[:m], int(self.acc[(m << self.k) - 1]),
                int(self.ph[m - 1]))


def zeros(torch, nbytes):
    from gpu_util import DEV
    return torch.zeros(max(16, nbytes), dtype=torch.uint8, device=DEV)


def run(torch, P, plan, k, fcw, pm, x, y, phase0=0, acc=None, dphase0=0, last=None,
        form="rxd", stream=None):
    """one decimating receiver call ("rxd"), or cordic_plan_fm_mix_decim into
    arrays of its own and cordic_fm_demod from them ("two"), with every array at
    its offset; (mag, freq) as int32 after checking the guards and the inputs"""
    n, m, i16, offs = x.size, x.size >> k, P.i16, P.offs
    i32 = lambda a: None if a is None else a.view(np.int32)
    df = Padded(torch, n, offs["fcw"], src=i32(fcw))
    dm = None if pm is None else Padded(torch, n, offs["pm"], src=i32(pm))
    dx, dy = Padded(torch, n, offs["x"], i16, src=x), Padded(torch, n, offs["y"], i16, src=y)
    mag, freq = Padded(torch, m, offs["mag"], i16), Padded(torch, m, offs["freq"], i16)
    pmv = None if dm is None else dm.view
    kw = dict(pm=pmv, n=n, phase0=phase0, acc=acc)
    if form == "rxd":
        ws = plan.fm_rx_decim16_workspace if i16 else plan.fm_rx_decim_workspace
        fn = plan.fm_rx_decim16 if i16 else plan.fm_rx_decim
        fn(P.ccfg, k, df.view, dx.view, dy.view, mag.view, freq.view,
           zeros(torch, ws(P.ccfg, n, k)), dphase0=dphase0, last=last, stream=stream, **kw)
    else:
        tx, ty = Padded(torch, m, 3, i16), Padded(torch, m, 1, i16)
        ws = plan.fm_mix_decim16_workspace if i16 else plan.fm_mix_decim_workspace
        fn = plan.fm_mix_decim16 if i16 else plan.fm_mix_decim
        fn(k, df.view, dx.view, dy.view, tx.view, ty.view, zeros(torch, ws(n, k)), **kw)
        ca.fm_demod(P.ccfg, tx.view, ty.view, mag.view, freq.view,
                    zeros(torch, ca.fm_demod_workspace(m)), n=m, phase0=dphase0, last=last)
    torch.cuda.synchronize()
    assert np.array_equal(df.get(), i32(fcw))
    assert dm is None or np.array_equal(dm.get(), i32(pm))
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    return mag.get().astype(np.int32), freq.get().astype(np.int32)


def check_lengths(torch, P, plan, k, ms, seed, with_pm=True, forms=("rxd", "two"), tag=None):
    """every m of `ms` as a prefix of one job's data: with both words preset,
    and without either and their values in phase0 and dphase0 -- the same start
    and the same prev, so one oracle serves both"""
    fcw, pm, x, y = P.data(max(ms) << k, seed, with_pm)
    W = Want(P, k, fcw, pm, x, y, PHASE0, ACC0, DPHASE0, LAST0)
    for m in ms:
        n = m << k
        wm, wf, wacc, wlast = W.prefix(m)
        for with_words in (True, False):
            for form in forms:
                acc = last_word(torch, ACC0) if with_words else None
                last = last_word(torch, LAST0) if with_words else None
                p0, d0 = (PHASE0, DPHASE0) if with_words else (PHASE0 + ACC0, DPHASE0 + LAST0)
                gm, gf = run(torch, P, plan, k, fcw[:n], None if pm is None else pm[:n],
                             x[:n], y[:n], p0, acc, d0, last, form)
                what = (P.name, k, m, tag, with_words, form)
                assert np.array_equal(gm, wm), what
                assert np.array_equal(gf, wf), what
                if with_words:
                    assert last_value(acc) == wacc, what
                    assert last_value(last) == wlast, what


# ---------------------------------------------------------------- no GPU

def test_the_new_functions_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    for t, tag in (("int32_t", ""), ("int16_t", "16")):
        assert re.search(
            r"size_t\s+cordic_plan_fm_rx_decim%s_workspace\s*\(\s*const\s+cordic_plan\s*\*"
            r"\s*plan\s*,\s*const\s+cordic_config\s*\*\s*conv\s*,\s*size_t\s+n\s*,"
            r"\s*uint32_t\s+log2r\s*\)\s*;" % tag, text)
        assert re.search(
            r"int\s+cordic_plan_fm_rx_decim%s\s*\(\s*const\s+cordic_plan\s*\*\s*plan\s*,"
            r"\s*const\s+cordic_config\s*\*\s*conv\s*,\s*size_t\s+n\s*,\s*uint32_t\s+log2r\s*,"
            r"\s*const\s+uint32_t\s*\*\s*d_fcw\s*,\s*const\s+uint32_t\s*\*\s*d_pm\s*,"
            r"\s*uint32_t\s+phase0\s*,\s*uint32_t\s*\*\s*d_acc\s*,\s*const\s+%s\s*\*\s*d_xval\s*,"
            r"\s*const\s+%s\s*\*\s*d_yval\s*,\s*uint32_t\s+dphase0\s*,\s*uint32_t\s*\*"
            r"\s*d_last\s*,\s*%s\s*\*\s*d_omag\s*,\s*%s\s*\*\s*d_ofreq\s*,\s*void\s*\*"
            r"\s*d_work\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (tag, t, t, t, t), text)
        assert re.search(
            r"int\s+cordic_rxbank_create_decim%s\s*\(\s*const\s+cordic_plan\s*\*\s*plan\s*,"
            r"\s*const\s+cordic_config\s*\*\s*conv\s*,\s*uint32_t\s+log2r\s*,\s*size_t\s+njobs"
            r"\s*,\s*const\s+cordic_fmrx_job%s\s*\*\s*jobs\s*,\s*cordic_rxbank\s*\*\*\s*bank"
            r"\s*\)\s*;" % (tag, tag), text)
    from cordic_amd import _native
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
        assert name in _native.ABI
    for name in ("fm_rx_decim", "fm_rx_decim16", "fm_rx_decim_workspace",
                 "fm_rx_decim16_workspace"):
        assert callable(getattr(ca.Plan, name))
    assert "log2r" in ca.RxBank.__init__.__code__.co_varnames
    assert "log2r" in ca.RxBank16.__init__.__code__.co_varnames


def test_the_header_is_still_plain_c99_and_the_jobs_keep_their_88_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { const cordic_plan *p = 0; const cordic_config *c = 0;\n'
        'int32_t *a = 0; int16_t *s = 0; uint32_t *w = 0; cordic_rxbank *b = 0;\n'
        'cordic_fmrx_job *j = 0; cordic_fmrx_job16 *h = 0;\n'
        'char a88[sizeof(cordic_fmrx_job) == 88 ? 1 : -1];\n'
        'char b88[sizeof(cordic_fmrx_job16) == 88 ? 1 : -1];\n'
        'size_t t = cordic_plan_fm_rx_decim_workspace(p, c, 8, 3)\n'
        ' + cordic_plan_fm_rx_decim16_workspace(p, c, 8, 3); (void)a88; (void)b88;\n'
        'return cordic_plan_fm_rx_decim(p, c, 0, 3, w, w, 0, w, a, a, 0, w, a, a, 0, 0)\n'
        ' + cordic_plan_fm_rx_decim16(p, c, 0, 3, w, w, 0, w, s, s, 0, w, s, s, 0, 0)\n'
        ' + cordic_rxbank_create_decim(p, c, 3, 0, j, &b)\n'
        ' + cordic_rxbank_create_decim16(p, c, 3, 0, h, &b) + (int)t; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_a_null_plan_or_conv_k_9_and_a_partial_group_are_refused_without_a_device():
    """(WW 38 and 9 live stages: no seed table, so the plans need no device)"""
    L = ca.lib()
    cfg3 = DEM.both("cfg3")[0]
    io16 = ca.Config.from_cli(*RX16.DEM16.CORES["io16"][0])
    nul = (None,) * 2
    plan32, plan16 = ca.Plan(MIX.both("ww38")[0]), ca.Plan(MIX16.both("n9")[0])
    for fn, ws, plan, conv in (
            (L.cordic_plan_fm_rx_decim, L.cordic_plan_fm_rx_decim_workspace, plan32, cfg3),
            (L.cordic_plan_fm_rx_decim16, L.cordic_plan_fm_rx_decim16_workspace, plan16, io16)):
        for n in (0, 8):
            for p, c in ((None, conv.ref), (plan._h, None), (None, None)):
                assert fn(p, c, n, 1, None, None, 0, None, *nul, 0, None, *nul, None,
                          None) == ca.ERR_ARGS
                assert ws(p, c, n, 1) == 0
        a = 0x10000
        args = (a, None, 0, None, 2 * a, 3 * a, 0, None, 4 * a, 5 * a, 6 * a, None)
        for n, k in ((1024, 9), (0, 9), (1020, 3), (255, 8), (1, 1)):
            assert fn(plan._h, conv.ref, n, k, *args) == ca.ERR_ARGS, (n, k)
            assert ws(plan._h, conv.ref, n, k) == 0, (n, k)
        # a no-op, and what the workspace of whole groups is not
        assert fn(plan._h, conv.ref, 0, 8, None, None, 0, None, *nul, 0, None, *nul, None,
                  None) == 0
        assert ws(plan._h, conv.ref, 0, 8) == 0 and ws(plan._h, conv.ref, 1024, 8) > 0
    # the container in front of the shape: cordic_plan_fm_rx16's order
    assert L.cordic_plan_fm_rx_decim16(plan32._h, io16.ref, 1020, 9, None, None, 0, None,
                                       *nul, 0, None, *nul, None, None) == ca.ERR_CONTAINER
    assert L.cordic_plan_fm_rx_decim16_workspace(plan32._h, io16.ref, 1024, 3) == 0
    # a rotator as the converter: the receiver's mode error, in front of k
    assert L.cordic_plan_fm_rx_decim(plan32._h, plan32.cfg.ref, 1024, 9, None, None, 0, None,
                                     *nul, 0, None, *nul, None, None) == ca.ERR_MODE
    plan32.close()
    plan16.close()


def test_the_workspace_of_a_pair_that_is_not_fused_is_the_two_calls_and_two_arrays():
    cfg3 = DEM.both("cfg3")[0]
    io16 = ca.Config.from_cli(*RX16.DEM16.CORES["io16"][0])
    a16 = lambda b: (b + 15) // 16 * 16
    for plan, conv, es in ((ca.Plan(MIX.both("ww38")[0]), cfg3, 4),
                           (ca.Plan(MIX16.both("n9")[0]), io16, 2),
                           (ca.Plan(MIX16.both("n9")[0]), io16, 4)):
        ws = plan.fm_rx_decim16_workspace if es == 2 else plan.fm_rx_decim_workspace
        mixd = plan.fm_mix_decim16_workspace if es == 2 else plan.fm_mix_decim_workspace
        rx = plan.fm_rx16_workspace if es == 2 else plan.fm_rx_workspace
        for k in (0, 1, 2, 5, 8):
            R, last = 1 << k, 0
            for n in sorted({0, R, 3 * R, 256, 1024, 1024 + R, 1 << 20, 1 << 33}):
                w = ws(conv, n, k)
                assert w % 16 == 0 and w >= last and (w == 0) == (n == 0), (k, n)
                if k == 0:
                    assert w == rx(conv, n), n
                elif n:
                    m = n >> k
                    assert w == mixd(n, k) + 2 * a16(m * es) + ca.fm_demod_workspace(m), (k, n)
                    assert w <= mixd(n, k) + (9 if es == 4 else 5) * m + 96, (k, n)
                last = w
        plan.close()


def test_the_binding_asks_the_caller_for_the_scratch():
    import torch
    plan = ca.Plan(MIX.both("ww38")[0])
    cfg3 = DEM.both("cfg3")[0]
    with pytest.raises(TypeError):
        plan.fm_rx_decim(cfg3, 3, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, n=8)
    short = torch.zeros(plan.fm_rx_decim_workspace(cfg3, 8, 3) - 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        plan.fm_rx_decim(cfg3, 3, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, short, n=8)
    a = torch.zeros(8, dtype=torch.int32)
    with pytest.raises((TypeError, ValueError)):
        plan.fm_rx_decim16(cfg3, 3, a, a, a, a, a, a, n=8)
    plan.close()


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("pair", UNITS + ("ww38-cfg3", "cfg1-ww36"))
def test_gpu_the_workspace_of_a_fused_pair_is_the_receivers(pair, monkeypatch):
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = Pair(pair)
    plan = P.plan()
    ws = plan.fm_rx_decim16_workspace if P.i16 else plan.fm_rx_decim_workspace
    rx = plan.fm_rx16_workspace if P.i16 else plan.fm_rx_workspace
    info = plan.fm_rx16_info if P.i16 else plan.fm_rx_info
    assert info(P.ccfg)[0] == P.fused
    for k in (0, 1, 3, 8):
        for n in (0, 1 << k, 1024, 1 << 20, 1 << 33):
            if P.fused or k == 0:
                assert ws(P.ccfg, n, k) == rx(P.ccfg, n), (k, n)
            else:
                assert (ws(P.ccfg, n, k) > 0) == (n > 0), (k, n)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_pm", [True, False])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("pair", UNITS)
def test_gpu_every_length_equals_the_oracle_and_the_two_calls(pair, k, with_pm, monkeypatch):
    """m = 1 .. 5: the partial vector; 63 .. 65: the wave edge; 1019 .. 1021:
    the first flush's 1020 own samples; 1023 .. 1025: a second flush; 2049: the
    ring's wrap and a third"""
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_MAX_BLOCKS", raising=False)
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = Pair(pair)
    plan = P.plan()
    check_lengths(torch, P, plan, k, MS, 2000 + 10 * k + with_pm, with_pm)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 5, 6, 7])
def test_gpu_every_other_k(k, monkeypatch):
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_MAX_BLOCKS", raising=False)
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = Pair("cfg2-cfg3")
    plan = P.plan()
    check_lengths(torch, P, plan, k, (1, 257, 1021, 2049), 2100 + k)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["cfg2-cfg3", "cfg1-io16"])
def test_gpu_k_0_is_the_receiver(pair):
    import torch
    P = Pair(pair)
    plan = P.plan()
    ws = plan.fm_rx16_workspace if P.i16 else plan.fm_rx_workspace
    fn = plan.fm_rx16 if P.i16 else plan.fm_rx
    for n in RX.LENGTHS:
        fcw, pm, x, y = P.data(n, 2200 + n)
        acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
        gm, gf = run(torch, P, plan, 0, fcw, pm, x, y, PHASE0, acc, DPHASE0, last)
        offs, i32 = P.offs, lambda a: a.view(np.int32)
        df, dm = Padded(torch, n, offs["fcw"], src=i32(fcw)), Padded(torch, n, offs["pm"], src=i32(pm))
        dx, dy = Padded(torch, n, offs["x"], P.i16, src=x), Padded(torch, n, offs["y"], P.i16, src=y)
        mag, freq = Padded(torch, n, offs["mag"], P.i16), Padded(torch, n, offs["freq"], P.i16)
        acc2, last2 = last_word(torch, ACC0), last_word(torch, LAST0)
        fn(P.ccfg, df.view, dx.view, dy.view, mag.view, freq.view, zeros(torch, ws(P.ccfg, n)),
           pm=dm.view, n=n, phase0=PHASE0, acc=acc2, dphase0=DPHASE0, last=last2)
        torch.cuda.synchronize()
        assert np.array_equal(gm, mag.get()) and np.array_equal(gf, freq.get()), n
        assert last_value(acc) == last_value(acc2) and last_value(last) == last_value(last2)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k, m", [(1, 5 * 1024 + 3), (3, 1283), (8, 41)])
@pytest.mark.parametrize("pair", UNITS)
def test_gpu_two_blocks_give_the_bits_of_the_grid_the_library_chooses(pair, k, m, monkeypatch):
    """k = 1: 11 passes, spans of 6, three flushes each, a halo of one lane; k =
    3: a halo of two lanes; k = 8: 11 passes and a halo that is all of wave 0"""
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = Pair(pair)
    plan = P.plan()
    n = m << k
    fcw, pm, x, y = P.data(n, 2300 + k)
    wm, wf, wacc, wlast = Want(P, k, fcw, pm, x, y, PHASE0, ACC0, DPHASE0, LAST0).prefix(m)
    for cap in ("2", None):
        if cap:
            monkeypatch.setenv("CORDIC_FMRXD_MAX_BLOCKS", cap)
        else:
            monkeypatch.delenv("CORDIC_FMRXD_MAX_BLOCKS")
        for with_pm in (True, False) if cap else (True,):
            if not with_pm:
                wm2, wf2, wacc2, wlast2 = Want(P, k, fcw, None, x, y, PHASE0, ACC0, DPHASE0,
                                               LAST0).prefix(m)
            acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
            gm, gf = run(torch, P, plan, k, fcw, pm if with_pm else None, x, y, PHASE0, acc,
                         DPHASE0, last)
            e = (wm, wf, wacc, wlast) if with_pm else (wm2, wf2, wacc2, wlast2)
            assert np.array_equal(gm, e[0]) and np.array_equal(gf, e[1]), (cap, with_pm)
            assert last_value(acc) == e[2] and last_value(last) == e[3], (cap, with_pm)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lj", [29, 30])
@pytest.mark.parametrize("stages", MIX.INSTANCES)
def test_gpu_every_rotator_instance_equals_the_oracle(stages, lj, monkeypatch):
    """7 stage counts x LJ 29 / 30 into cfg3 at k = 3, m = 1025"""
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    args = (ca.P2R, 32, 32, 2, 32, stages) if lj == 29 else (ca.P2R, 31, 31, 2, 32, stages)
    name = "dinst%d_%d" % (lj, stages)
    MIX.CORES[name] = (args, 0)
    PAIRS[name] = (name, "cfg3", 1)
    try:
        P = Pair(name)
        assert P.mcfg.ww == 64 - lj and P.mcfg.nlive == stages
        plan = P.plan()
        assert plan.fm_rx_info(P.ccfg) == (1, 1024)
        check_lengths(torch, P, plan, 3, (1025,), stages * lj, forms=("rxd",))
        plan.close()
    finally:
        del MIX.CORES[name], PAIRS[name]


@pytest.mark.gpu
def test_gpu_sums_beyond_32_bits_and_negative_floors_reach_the_converter_exact(monkeypatch):
    """cfg2 has OW 32: 256 full-scale tuned samples sum to 40 bits; and a group
    whose sum is negative and no multiple of R floors below what truncation
    gives.  Both are in the data the oracle sums as int64; the test asserts
    that they are, then compares"""
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = Pair("cfg2-cfg3")
    k, m = 8, 9
    n = m << k
    rng = np.random.default_rng(77)
    fcw = np.zeros(n, dtype=np.uint32)              # no rotation: the sums stay large
    hi = (1 << 31) - 1
    x = np.full(n, hi // 2, dtype=np.int32)         # (the core's gain keeps OW 32 from wrapping)
    y = np.full(n, -(hi // 2), dtype=np.int32)
    x[n // 2:] = rng.integers(-1000, 1000, n - n // 2)
    y[n // 2:] = rng.integers(-1000, 0, n - n // 2)
    p, _ = phases(fcw, None, 0, 0)
    tx, ty = P.tuned(x, y, p)
    sx = tx.astype(np.int64).reshape(-1, 1 << k).sum(axis=1)
    sy = ty.astype(np.int64).reshape(-1, 1 << k).sum(axis=1)
    assert (np.abs(sx) >= 1 << 32).any() and (np.abs(sy) >= 1 << 32).any()
    neg = sy[(sy < 0) & (sy % (1 << k) != 0)]
    assert neg.size and ((neg >> k) != -((-neg) >> k)).all()    # floor is not truncation
    plan = P.plan()
    wm, wf, wacc, wlast = Want(P, k, fcw, None, x, y, 0, 0, 0, 0).prefix(m)
    for form in ("rxd", "two"):
        acc, last = last_word(torch, 0), last_word(torch, 0)
        gm, gf = run(torch, P, plan, k, fcw, None, x, y, 0, acc, 0, last, form)
        assert np.array_equal(gm, wm) and np.array_equal(gf, wf), form
        assert last_value(acc) == wacc and last_value(last) == wlast, form
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair, k", [("cfg2-cfg3", 3), ("cfg1-io16", 1), ("ww38-cfg3", 2)])
def test_gpu_three_calls_cut_at_multiples_of_r_equal_one_call(pair, k, monkeypatch):
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = Pair(pair)
    m, cuts = 2049 + 7, (0, 1021, 2050, 2049 + 7)
    fcw, pm, x, y = P.data(m << k, 5)
    wm, wf, wacc, wlast = Want(P, k, fcw, pm, x, y, PHASE0, 0, DPHASE0, 0).prefix(m)
    plan = P.plan()
    acc, last = last_word(torch, 0), last_word(torch, 0)
    gm, gf = [], []
    for c in range(3):
        s = slice(cuts[c] << k, cuts[c + 1] << k)
        a, b = run(torch, P, plan, k, fcw[s], pm[s], x[s], y[s], PHASE0 if c == 0 else 0, acc,
                   DPHASE0 if c == 0 else 0, last)
        gm.append(a)
        gf.append(b)
    assert np.array_equal(np.concatenate(gm), wm)
    assert np.array_equal(np.concatenate(gf), wf)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["cfg2-cfg3", "cfg1-io16"])
def test_gpu_a_captured_call_is_two_kernel_nodes_and_continues_on_replay(pair, monkeypatch):
    """phase0 = dphase0 = 0 and both words: replay r is call r of a job three
    times as long on the same inputs (tests/test_fm_rx.py)"""
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = Pair(pair)
    k, m = 3, 1025
    n = m << k
    fcw, pm, x, y = P.data(n, 9)
    rep = lambda a: np.concatenate([a, a, a])
    W = Want(P, k, rep(fcw), rep(pm), rep(x), rep(y), 0, ACC0, 0, LAST0)
    wm, wf, wacc, wlast = W.prefix(3 * m)
    plan = P.plan()
    ws = plan.fm_rx_decim16_workspace if P.i16 else plan.fm_rx_decim_workspace
    fn = plan.fm_rx_decim16 if P.i16 else plan.fm_rx_decim
    work = zeros(torch, ws(P.ccfg, n, k))
    offs, i32 = P.offs, lambda a: a.view(np.int32)
    df, dm = Padded(torch, n, offs["fcw"], src=i32(fcw)), Padded(torch, n, offs["pm"], src=i32(pm))
    dx, dy = Padded(torch, n, offs["x"], P.i16, src=x), Padded(torch, n, offs["y"], P.i16, src=y)
    mag, freq = Padded(torch, m, offs["mag"], P.i16), Padded(torch, m, offs["freq"], P.i16)
    acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
    call = lambda a, l, s: fn(P.ccfg, k, df.view, dx.view, dy.view, mag.view, freq.view, work,
                              pm=dm.view, n=n, acc=a, last=l, stream=s)
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
        assert cnt.value == 2
        nodes = (C.c_void_p * 2)()
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(cnt)) == 0
        for i in range(2):
            t = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
            assert t.value == 0                      # hipGraphNodeTypeKernel
        edges = C.c_size_t(0)
        assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0
        assert edges.value == 1                      # two nodes, one chain
        ex = C.c_void_p()
        assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
        try:
            for r in range(3):
                assert hip.hipGraphLaunch(ex, h) == 0
                stream.synchronize()
                s = slice(r * m, (r + 1) * m)
                assert np.array_equal(mag.get().astype(np.int32), wm[s]), (pair, r)
                assert np.array_equal(freq.get().astype(np.int32), wf[s]), (pair, r)
        finally:
            hip.hipGraphExecDestroy(ex)
    finally:
        hip.hipGraphDestroy(graph)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("pair", ["ww38-cfg3", "cfg2-r2p35", "cfg2-ug_lj"])
def test_gpu_fallback_pairs_equal_the_oracle_and_the_two_calls(pair, k, monkeypatch):
    import torch
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = Pair(pair)
    assert not P.fused
    plan = P.plan()
    check_lengths(torch, P, plan, k, (1, 257, 1025), 2400 + k)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["cfg2-cfg3", "cfg1-io16"])
def test_gpu_the_forced_fallback_gives_the_fused_bits(pair, monkeypatch):
    import torch
    P = Pair(pair)
    plan = P.plan()
    ws = plan.fm_rx_decim16_workspace if P.i16 else plan.fm_rx_decim_workspace
    k, m = 3, 1025
    fcw, pm, x, y = P.data(m << k, 31)
    got = {}
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("CORDIC_FMRXD_FALLBACK", "1")
        else:
            monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
        size = ws(P.ccfg, m << k, k)
        acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
        gm, gf = run(torch, P, plan, k, fcw, pm, x, y, PHASE0, acc, DPHASE0, last)
        got[forced] = (gm, gf, last_value(acc), last_value(last), size)
    assert got[True][4] > got[False][4]             # the fallback's larger workspace
    assert np.array_equal(got[True][0], got[False][0])
    assert np.array_equal(got[True][1], got[False][1])
    assert got[True][2:4] == got[False][2:4]
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["cfg2-cfg3", "ww38-cfg3"])
def test_gpu_overlaps_by_the_decimated_ranges_and_bad_pointers_are_refused(pair, monkeypatch):
    """an output's byte range is (n >> k) elements: what lies behind them is
    clear, even inside what n elements would cover"""
    import torch
    from gpu_util import DEV
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    P = Pair(pair)
    k, m = 3, 128
    n = m << k
    fcw, pm, x, y = P.data(n, 13)
    plan = P.plan()
    work = zeros(torch, plan.fm_rx_decim_workspace(P.ccfg, n, k))
    i32 = lambda a: a.view(np.int32)
    df, dm = Padded(torch, n, 4, src=i32(fcw)), Padded(torch, n, 4, src=i32(pm))
    dx, dy = Padded(torch, n, 4, src=x), Padded(torch, n, 4, src=y)
    mag, freq = Padded(torch, m, 4), Padded(torch, m, 4)
    # two outputs in one buffer, m elements each, back to back: clear by (n >> k)
    both = torch.full((4 + 2 * m + 16,), DEM.S32, dtype=torch.int32, device=DEV)
    acc, last = last_word(torch, ACC0), last_word(torch, LAST0)
    L = ca.lib()

    def call(**kw):
        a = dict(fcw=df.view, pm=dm.view, acc=acc, x=dx.view, y=dy.view, last=last,
                 mag=mag.view, freq=freq.view, work=work, n=n, k=k)
        a.update(kw)
        ptr = lambda v: v if isinstance(v, (int, type(None))) else C.c_void_p(v.data_ptr())
        return L.cordic_plan_fm_rx_decim(plan._h, P.ccfg.ref, a["n"], a["k"], ptr(a["fcw"]),
                                         ptr(a["pm"]), 0, ptr(a["acc"]), ptr(a["x"]),
                                         ptr(a["y"]), 0, ptr(a["last"]), ptr(a["mag"]),
                                         ptr(a["freq"]), ptr(a["work"]), None)

    bad = [dict(mag=dx.view), dict(freq=dy.view), dict(mag=df.view), dict(freq=dm.view),
           dict(mag=freq.view), dict(freq=mag.view[m - 1:]), dict(mag=dx.view[n - 1:]),
           dict(last=mag.view[5:]), dict(last=freq.view[m - 1:]), dict(acc=mag.view[7:]),
           dict(acc=last), dict(last=dx.view[3:]), dict(acc=df.view[n - 1:]),
           dict(work=mag.view), dict(fcw=None), dict(x=None), dict(y=None),
           dict(mag=None), dict(freq=None), dict(work=None),
           dict(x=dx.view.data_ptr() + 2), dict(mag=mag.view.data_ptr() + 1),
           dict(last=last.data_ptr() + 2), dict(acc=acc.data_ptr() + 1),
           dict(pm=dm.view.data_ptr() + 2), dict(work=work.data_ptr() + 8),
           dict(k=9), dict(n=n - 4), dict(n=n + 1)]
    for kw in bad:
        assert call(**kw) == ca.ERR_ARGS, sorted(kw)
    torch.cuda.synchronize()
    assert mag.untouched() and freq.untouched()
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    assert np.array_equal(df.get(), i32(fcw)) and np.array_equal(dm.get(), i32(pm))
    assert last_value(acc) == ACC0 and last_value(last) == LAST0
    assert not work.any().item()
    # freq begins m elements behind mag's start: inside mag's n elements, behind
    # its n >> k
    wm, wf, wacc, wlast = Want(P, k, fcw, pm, x, y, 0, ACC0, 0, LAST0).prefix(m)
    assert call(mag=both[4:], freq=both[4 + m:]) == 0
    torch.cuda.synchronize()
    h = both.cpu().numpy()
    assert (h[:4] == DEM.S32).all() and (h[4 + 2 * m:] == DEM.S32).all()
    assert np.array_equal(h[4:4 + m], wm) and np.array_equal(h[4 + m:4 + 2 * m], wf)
    assert last_value(acc) == wacc and last_value(last) == wlast
    plan.close()
