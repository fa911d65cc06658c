"""FM demodulation (cordic_fm_demod, cordic_fm_demod16, cordic_fm_demod_info,
cordic_fm_demod_workspace; include/cordic_amd.h): the r2p converter with its
phase differenced from sample to sample on the device.  Expected values need no
tolerance: the oracle's topolar, a numpy difference mod 2^PW and a sign
extension."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_fm_demod_workspace", "cordic_fm_demod_info", "cordic_fm_demod",
         "cordic_fm_demod16")
UG = ca.FLAG_UNIT_GAIN
# name: (cli args, flags).  cfg3 / natr2p24: tools/bench_common.py:73,86; ug_lj,
# r2p35, r2p32, wrap32: tests/test_jobset_fused.py:58-62
CORES = {
    "cfg3": ((ca.R2P, 24, 24, 2, -1, 20), 0),
    "natr2p24": ((ca.R2P, 24, 24, 2, -1, -1), 0),
    "ug_lj": ((ca.R2P, 24, 24, 2, -1, 20), UG),
    # the sequential core with cfg3's ports: cordic_fm_demod_info answers
    # fused = 1 for it (WW 32, no wrap: cordic_r2p runs it on topolar_lj too)
    "sr2p": ((ca.SR2P, 24, 24, 2, -1, 20), 0),
    "r2p35": ((ca.R2P, 27, 27, 2, 32, 20), 0),
    "r2p32": ((ca.R2P, 32, 32, 2, 32, 24), 0),             # WW 40
    "wrap32": ((ca.R2P, 24, 1, 2, 32, -1), 0),
    "cfg3_no_lj": ((ca.R2P, 24, 24, 2, -1, 20), ca.FLAG_NO_LJ),
    "cfg3_generic": ((ca.R2P, 24, 24, 2, -1, 20), ca.FLAG_FORCE_GENERIC),
    "pw20": ((ca.R2P, 16, 16, 2, 20, -1), 0),              # 17 live stages
    # fused cores on the dynamic-exit instance without unit gain
    "ww33": ((ca.R2P, 25, 25, 2, 32, -1), 0),              # 29 live stages
    "ww34_ow2": ((ca.R2P, 26, 2, 2, 32, 20), 0),
    "io16": ((ca.R2P, 16, 16, 2, 16, -1), 0),
}
FUSED = ("cfg3", "natr2p24", "ug_lj", "sr2p")


def both(name):
    args, flags = CORES[name]
    cfg = ca.Config.from_cli(*args)
    if flags:
        cfg = cfg.with_flags(flags)
    gain = ca.lib().cordic_config_gain_annihilator(cfg.ref) if flags & UG else None
    return cfg, O.config_cli(*args), gain


# ---------------------------------------------------------------- no GPU

def test_the_four_functions_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    assert re.search(r"size_t\s+cordic_fm_demod_workspace\s*\(\s*size_t\s+n\s*\)\s*;",
                     text)
    assert re.search(r"int\s+cordic_fm_demod_info\s*\(\s*const\s+cordic_config\s*\*\s*"
                     r"cfg\s*,\s*int32_t\s*\*\s*fused\s*,\s*int32_t\s*\*\s*tile\s*\)\s*;",
                     text)
    for name, elem in (("cordic_fm_demod", "int32_t"), ("cordic_fm_demod16", "int16_t")):
        assert re.search(
            r"int\s+%s\s*\(\s*const\s+cordic_config\s*\*\s*cfg\s*,\s*size_t\s+n\s*,\s*"
            r"const\s+%s\s*\*\s*d_xval\s*,\s*const\s+%s\s*\*\s*d_yval\s*,\s*"
            r"uint32_t\s+phase0\s*,\s*uint32_t\s*\*\s*d_last\s*,\s*%s\s*\*\s*d_omag\s*,"
            r"\s*%s\s*\*\s*d_ofreq\s*,\s*void\s*\*\s*d_work\s*,\s*void\s*\*\s*stream"
            r"\s*\)\s*;" % (name, elem, elem, elem, elem), text), name
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
    for name in ("fm_demod_workspace", "fm_demod_info", "fm_demod"):
        assert name in ca.__all__ and callable(getattr(ca, name))
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_header_with_the_new_block_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { cordic_config c; int32_t f, t; int32_t *a = 0; int16_t *b = 0;\n'
        'uint32_t *l = 0; size_t w = cordic_fm_demod_workspace(8);\n'
        'cordic_config_init(&c, CORDIC_R2P, 24, 24, 2, -1, 20);\n'
        'return cordic_fm_demod_info(&c, &f, &t) + cordic_fm_demod(&c, 0, a, a, 0, l,'
        ' a, a, 0, 0) + cordic_fm_demod16(&c, 0, b, b, 0, l, b, b, 0, 0) + (int)w; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_workspace_size_is_small_aligned_and_monotonic():
    assert ca.fm_demod_workspace(0) == 0
    last = 0
    for n in (0, 1, 255, 256, 257, 1 << 20, 1 << 33):
        w = ca.fm_demod_workspace(n)
        assert w % 16 == 0, n
        assert w >= last, n
        assert w <= n // 256 + 65536, n
        assert (w == 0) == (n == 0), n
        last = w


@pytest.mark.parametrize("name,fused", [
    ("cfg3", 1), ("natr2p24", 1), ("ug_lj", 1), ("sr2p", 1), ("r2p35", 0),
    ("r2p32", 0), ("wrap32", 0), ("cfg3_no_lj", 0), ("cfg3_generic", 0),
    ("ww33", 1), ("ww34_ow2", 1), ("pw20", 1)])
def test_the_path_query_names_the_fused_cores(name, fused):
    cfg = both(name)[0]
    got, tile = ca.fm_demod_info(cfg)
    assert got == fused
    if fused:
        assert tile > 0 and tile % 4 == 0
    else:
        assert tile == 0


def test_the_path_query_refuses_a_rotator_and_a_null():
    f, t = C.c_int32(-5), C.c_int32(-5)
    p2r = ca.Config.from_cli(ca.P2R, 24, 24, 2, -1, -1)
    L = ca.lib()
    assert L.cordic_fm_demod_info(p2r.ref, C.byref(f), C.byref(t)) == ca.ERR_MODE
    assert L.cordic_fm_demod_info(None, C.byref(f), C.byref(t)) == ca.ERR_ARGS
    assert (f.value, t.value) == (-5, -5)
    # either pointer may be NULL
    assert L.cordic_fm_demod_info(both("cfg3")[0].ref, None, None) == 0
    # the calls themselves: the mode, a NULL configuration, n = 0
    assert L.cordic_fm_demod(p2r.ref, 0, None, None, 0, None, None, None, None,
                             None) == ca.ERR_MODE
    for fn in (L.cordic_fm_demod, L.cordic_fm_demod16):
        assert fn(None, 0, None, None, 0, None, None, None, None, None) == ca.ERR_ARGS
    assert L.cordic_fm_demod(both("cfg3")[0].ref, 0, None, None, 0, None, None,
                             None, None, None) == 0
    assert L.cordic_fm_demod16(both("cfg3")[0].ref, 0, None, None, 0, None, None,
                               None, None, None) == ca.ERR_CONTAINER


def test_the_binding_asks_the_caller_for_the_scratch():
    import torch
    cfg = both("cfg3")[0]
    with pytest.raises(TypeError):
        ca.fm_demod(cfg, 0x1000, 0x2000, 0x3000, 0x4000, None, n=8)
    short = torch.zeros(ca.fm_demod_workspace(8) - 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ca.fm_demod(cfg, 0x1000, 0x2000, 0x3000, 0x4000, short, n=8)


# ---------------------------------------------------------------- GPU

S32, S16 = -0x5a5a5a5b, 0x5a5b        # sentinels
PAD = 16
BIG = (1 << 23) + 4099


class Padded:
    """A sentinel-filled device array with `off` guard elements in front of and
    PAD behind the n that a call may write.  torch allocations sit on 256-byte
    boundaries: off = 4 (32-bit) keeps the 16-byte alignment, off = 5 breaks it."""

    def __init__(self, torch, n, off, i16=False, src=None):
        from gpu_util import DEV
        self.dt, self.sent = (torch.int16, S16) if i16 else (torch.int32, S32)
        self.np = np.int16 if i16 else np.int32
        self.n, self.off = n, off
        self.t = torch.full((off + n + PAD,), self.sent, dtype=self.dt, device=DEV)
        if src is not None and n:
            self.t[off:off + n].copy_(torch.from_numpy(
                np.ascontiguousarray(src).astype(self.np)).to(DEV))

    @property
    def view(self):
        return self.t[self.off:]

    def get(self):
        """the n values, after checking that nothing around them was written"""
        h = self.t.cpu().numpy()
        assert (h[:self.off] == self.sent).all()
        assert (h[self.off + self.n:] == self.sent).all()
        return h[self.off:self.off + self.n]

    def untouched(self):
        return bool((self.t == self.sent).all().item())


def work_buffer(torch, n=BIG):
    from gpu_util import DEV
    return torch.zeros(max(16, ca.fm_demod_workspace(n)), dtype=torch.uint8,
                       device=DEV)


def last_word(torch, value):
    from gpu_util import DEV
    v = value - (1 << 32) if value >= 1 << 31 else value
    return torch.full((4,), v, dtype=torch.int32, device=DEV)


def last_value(last):
    h = last.cpu().numpy().view(np.uint32)
    assert (h[1:] == h[1]).all()            # only the first word is the call's
    return int(h[0])


def iq(rng, n, iw):
    lo, hi = -(1 << (iw - 1)), (1 << (iw - 1)) - 1
    return (rng.integers(lo, hi + 1, n).astype(np.int32),
            rng.integers(lo, hi + 1, n).astype(np.int32))


def hard_points(rng, n, iw):
    """x = y = 0, the axes, the diagonals, +/-1 LSB around each and the most
    negative port value, in random order in front of random samples: topolar's
    phase wraps between such neighbours and the sign extension flips"""
    lo, hi = -(1 << (iw - 1)), (1 << (iw - 1)) - 1
    pts = []
    for a in (1, 2, 1000, hi // 2, hi - 1):
        for bx, by in ((0, 0), (a, 0), (-a, 0), (0, a), (0, -a), (a, a), (a, -a),
                       (-a, a), (-a, -a)):
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    pts.append((bx + dx, by + dy))
    pts += [(lo, lo), (lo, 0), (0, lo), (lo, hi), (hi, lo), (hi, hi), (lo, -1),
            (-1, lo), (lo, 1)]
    pts = np.array(pts, dtype=np.int64)
    pts = np.concatenate([pts, pts[rng.permutation(len(pts))]])
    assert pts.min() >= lo and pts.max() <= hi and len(pts) <= n
    x, y = iq(rng, n, iw)
    x[:len(pts)], y[:len(pts)] = pts[:, 0], pts[:, 1]
    return x, y


def expected(ocfg, gain, pw, x, y, prev):
    """(mag, freq as int32, ph_(n-1)) for the phase `prev` in front of sample 0"""
    mag, ph = O.topolar(ocfg, x, y)
    if gain is not None:            # o = (o * K) >> 32 (CORDIC_FLAG_UNIT_GAIN)
        mag = ((mag.astype(np.int64) * gain) >> 32).astype(np.int32)
    mask = (1 << pw) - 1
    p = ph.astype(np.int64)
    before = np.concatenate([[prev & mask], p[:-1]]) if p.size else p
    d = (p - before) & mask
    sign = 1 << (pw - 1)
    freq = ((d ^ sign) - sign).astype(np.int64)
    return mag, freq.astype(np.int32), (int(ph[-1]) if ph.size else None)


def run(torch, cfg, work, x, y, phase0=0, last=None, offs=(4, 4, 4, 4), i16=False):
    """one call with x, y, mag, freq at the element offsets `offs` behind an
    aligned start; (mag, freq) after checking the guards and the inputs"""
    n = x.size
    dx = Padded(torch, n, offs[0], i16, src=x)
    dy = Padded(torch, n, offs[1], i16, src=y)
    dm = Padded(torch, n, offs[2], i16)
    df = Padded(torch, n, offs[3], i16)
    ca.fm_demod(cfg, dx.view, dy.view, dm.view, df.view, work, n=n,
                phase0=phase0, last=last)
    torch.cuda.synchronize()
    t = np.int16 if i16 else np.int32
    assert np.array_equal(dx.get(), x.astype(t)) and np.array_equal(dy.get(), y.astype(t))
    return dm.get(), df.get()


def check(torch, name, x, y, work, offs=(4, 4, 4, 4), tag=None):
    """with and without a d_last word, against the oracle; (mag, freq)"""
    cfg, ocfg, gain = both(name)
    pw, n = cfg.pw, x.size
    phase0, preset = 0x9e3779b1, 0x7f4a7c15
    wm, wf, wl = expected(ocfg, gain, pw, x, y, phase0 + preset)
    last = last_word(torch, preset)
    m, f = run(torch, cfg, work, x, y, phase0, last, offs)
    assert np.array_equal(m, wm), (name, n, tag)
    assert np.array_equal(f, wf), (name, n, tag)
    assert last_value(last) == (wl if n else preset), (name, n, tag)
    wm0, wf0, _ = expected(ocfg, gain, pw, x, y, 0)
    m0, f0 = run(torch, cfg, work, x, y, 0, None, offs)
    assert np.array_equal(m0, wm0) and np.array_equal(f0, wf0), (name, n, tag)
    return m, f


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED)
def test_gpu_fused_cores_equal_the_oracle(name):
    import torch
    cfg = both(name)[0]
    fused, T = ca.fm_demod_info(cfg)
    assert fused == 1
    work = work_buffer(torch)
    rng = np.random.default_rng(11)
    # (the sizes of the issue, and 6 and T + 2 for a tail of 2 samples)
    for n in (0, 1, 3, 4, 5, 6, 1023, 1024, 1025, T - 1, T, T + 1, T + 2, T + 4,
              2 * T + 5):
        x, y = iq(rng, n, cfg.iw)
        check(torch, name, x, y, work)
    x, y = hard_points(rng, T + 4, cfg.iw)
    check(torch, name, x, y, work, tag="hard")


def tiles_of(cfg, n):
    """tiles the fused kernel cuts n samples into (whole vectors only)"""
    T = ca.fm_demod_info(cfg)[1]
    return (n // 4 + T // 4 - 1) // (T // 4)


@pytest.mark.gpu
def test_gpu_fused_where_every_block_owns_several_tiles(monkeypatch):
    """n = 2^23 + 4099 is 1026 tiles: fewer than a large device's resident
    blocks, so the grid is capped (CORDIC_FMD_MAX_BLOCKS, cordic_fm_demod.hip) at
    128 and at 37 blocks -- 8 and 27 or 28 tiles per block -- and then left alone;
    every run against the oracle, hence the same bits on every grid"""
    import torch
    name = "cfg3"
    cfg, ocfg, gain = both(name)
    assert tiles_of(cfg, BIG) == 1026
    work = work_buffer(torch)
    x, y = iq(np.random.default_rng(12), BIG, cfg.iw)
    wm, wf, wl = expected(ocfg, gain, cfg.pw, x, y, 0x12345678 + 5)
    for cap in (128, 37, None):
        if cap is None:
            monkeypatch.delenv("CORDIC_FMD_MAX_BLOCKS", raising=False)
        else:
            assert tiles_of(cfg, BIG) >= 3 * cap
            monkeypatch.setenv("CORDIC_FMD_MAX_BLOCKS", str(cap))
        last = last_word(torch, 5)
        m, f = run(torch, cfg, work, x, y, 0x12345678, last)
        assert last_value(last) == wl, cap
        assert np.array_equal(m, wm) and np.array_equal(f, wf), cap


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED)
def test_gpu_fused_on_one_three_and_seven_blocks(name, monkeypatch):
    """24 tiles and a tail of 2 samples on a grid capped at 1, 3 and 7 blocks:
    24, 8 and 3 or 4 tiles per block, the last tile a short one of 3 passes,
    sample 0 in block 0 alone"""
    import torch
    cfg = both(name)[0]
    T = ca.fm_demod_info(cfg)[1]
    n = 23 * T + 2402
    assert n % 4 == 2 and tiles_of(cfg, n) == 24
    work = work_buffer(torch)
    x, y = hard_points(np.random.default_rng(21), n, cfg.iw)
    for cap in (1, 3, 7):
        assert tiles_of(cfg, n) >= 3 * cap
        monkeypatch.setenv("CORDIC_FMD_MAX_BLOCKS", str(cap))
        check(torch, name, x, y, work, tag=cap)


def bank_run(torch, cfg, x, y, phase0, last):
    """the same call as run(), as the one job of a DemodBank"""
    n = x.size
    dx, dy = Padded(torch, n, 4, src=x), Padded(torch, n, 4, src=y)
    dm, df = Padded(torch, n, 4), Padded(torch, n, 4)
    bank = ca.DemodBank(cfg, [(dx.view, dy.view, dm.view, df.view, n, phase0, last)])
    info = bank.info()
    assert info["fused"] == 1 and info["samples"] == n
    bank.run()
    torch.cuda.synchronize()
    bank.close()
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    return dm.get(), df.get()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ww33", "ww34_ow2", "pw20"])
def test_gpu_fused_instances_the_other_cores_do_not_reach(name, monkeypatch):
    """The dynamic-exit instance without unit gain, on the three forms the
    cores of FUSED leave out: stage 1 for WW 33 and for WW 34, the rounding
    outside 2 <= r <= 31 (a 2-bit output) and a PW below 32.  n = 1 is a tail
    without a whole vector, 5 a tail behind one, T + 2 a tile's edge, 2 T + 5 a
    second tile; with and without a d_last word; the grid left alone and capped
    at one block; the single call and a bank of that one job, each against the
    oracle and so against each other."""
    import torch
    cfg, ocfg, gain = both(name)
    assert (cfg.ww, cfg.nlive, cfg.ow, cfg.pw) == {
        "ww33": (33, 29, 25, 32), "ww34_ow2": (34, 20, 2, 32),
        "pw20": (24, 17, 16, 20)}[name]
    fused, T = ca.fm_demod_info(cfg)
    assert (fused, T) == (1, 8188)
    work = work_buffer(torch, 2 * T + 5)
    rng = np.random.default_rng(22)
    phase0, preset = 0x9e3779b1, 0x7f4a7c15
    for n in (1, 5, T + 2, 2 * T + 5):
        x, y = hard_points(rng, n, cfg.iw) if n > T else iq(rng, n, cfg.iw)
        for with_last in (True, False):
            wm, wf, wl = expected(ocfg, gain, cfg.pw, x, y,
                                  phase0 + (preset if with_last else 0))
            for cap in (None, 1):
                if cap is None:
                    monkeypatch.delenv("CORDIC_FMD_MAX_BLOCKS", raising=False)
                else:
                    monkeypatch.setenv("CORDIC_FMD_MAX_BLOCKS", str(cap))
                for path in ("call", "bank"):
                    tag = (name, n, with_last, cap, path)
                    last = last_word(torch, preset) if with_last else None
                    if path == "call":
                        m, f = run(torch, cfg, work, x, y, phase0, last)
                    else:
                        m, f = bank_run(torch, cfg, x, y, phase0, last)
                    assert np.array_equal(m, wm), tag
                    assert np.array_equal(f, wf), tag
                    if with_last:
                        assert last_value(last) == wl, tag


FALLBACK_SIZES = (1, 5, 255, 256, 257, 4099, (1 << 20) + 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["r2p35", "r2p32", "wrap32", "cfg3_no_lj",
                                  "cfg3_generic"])
def test_gpu_fallback_cores_equal_the_oracle(name):
    import torch
    cfg = both(name)[0]
    assert ca.fm_demod_info(cfg) == (0, 0)
    work = work_buffer(torch)
    rng = np.random.default_rng(13)
    for n in FALLBACK_SIZES:
        x, y = iq(rng, n, cfg.iw)
        check(torch, name, x, y, work)


@pytest.mark.gpu
def test_gpu_arrays_off_the_16_byte_grid_take_the_fallback_with_the_same_bits():
    import torch
    work = work_buffer(torch)
    rng = np.random.default_rng(14)
    for n in FALLBACK_SIZES:
        x, y = iq(rng, n, 24)
        m, f = check(torch, "cfg3", x, y, work)         # the fused kernel
        for k in range(4):
            offs = tuple(5 if j == k else 4 for j in range(4))
            m1, f1 = check(torch, "cfg3", x, y, work, offs, tag=offs)
            assert np.array_equal(m1, m) and np.array_equal(f1, f), (n, offs)
    # ... and the flagged cores, word for word
    x, y = iq(rng, 4099, 24)
    m, f = check(torch, "cfg3", x, y, work)
    for name in ("cfg3_no_lj", "cfg3_generic"):
        m1, f1 = check(torch, name, x, y, work)
        assert np.array_equal(m1, m) and np.array_equal(f1, f), name


@pytest.mark.gpu
def test_gpu_16_bit_form_equals_the_32_bit_form_and_the_oracle():
    import torch
    cfg, ocfg, gain = both("io16")
    work = work_buffer(torch)
    rng = np.random.default_rng(15)
    for n in (1, 5, 255, 256, 257, 4099, (1 << 16) + 3):
        x, y = iq(rng, n, 16)
        phase0, preset = 0xbeef1234, 0x1fedc
        wm, wf, wl = expected(ocfg, gain, cfg.pw, x, y, phase0 + preset)
        last = last_word(torch, preset)
        m32, f32 = run(torch, cfg, work, x, y, phase0, last)
        assert np.array_equal(m32, wm) and np.array_equal(f32, wf), n
        assert last_value(last) == wl
        for offs in ((8, 8, 8, 8), (1, 2, 3, 5)):
            last = last_word(torch, preset)
            m, f = run(torch, cfg, work, x, y, phase0, last, offs, True)
            assert np.array_equal(m, m32.astype(np.int16)), (n, offs)
            assert np.array_equal(f, f32.astype(np.int16)), (n, offs)
            assert last_value(last) == wl


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(ca.R2P, 16, 16, 2, 17, -1),
                                  (ca.R2P, 16, 24, 2, 16, -1)])
def test_gpu_16_bit_form_refuses_wide_cores(args):
    import torch
    cfg = ca.Config.from_cli(*args)
    assert cfg.pw == 17 or cfg.ow == 24
    n = 64
    work = work_buffer(torch, n)
    x = Padded(torch, n, 0, True, src=np.arange(n, dtype=np.int16))
    m, f = Padded(torch, n, 0, True), Padded(torch, n, 0, True)
    last = last_word(torch, 9)
    for k in (n, 0):
        with pytest.raises(ca.CordicError) as e:
            ca.fm_demod(cfg, x.view, x.view, m.view, f.view, work, n=k, last=last)
        assert e.value.status == ca.ERR_CONTAINER
    torch.cuda.synchronize()
    assert m.untouched() and f.untouched() and last_value(last) == 9


@pytest.mark.gpu
def test_gpu_consecutive_calls_that_share_the_last_word_equal_one_call():
    import torch
    name = "cfg3"
    cfg, ocfg, gain = both(name)
    T = ca.fm_demod_info(cfg)[1]
    cuts = np.cumsum([0, 1, T - 1, 5, T + 3])
    n = int(cuts[-1])
    work = work_buffer(torch)
    x, y = hard_points(np.random.default_rng(16), n, cfg.iw)
    phase0 = 0x00c0ffee
    wm, wf, wl = expected(ocfg, gain, cfg.pw, x, y, phase0)
    last = last_word(torch, 0)
    m, f = run(torch, cfg, work, x, y, phase0, last)
    assert np.array_equal(m, wm) and np.array_equal(f, wf) and last_value(last) == wl
    last = last_word(torch, 0)
    parts = [run(torch, cfg, work, x[a:b], y[a:b], phase0 if a == 0 else 0, last)
             for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), wm)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), wf)
    assert last_value(last) == wl


@pytest.mark.gpu
def test_gpu_phase0_and_the_last_word_add_mod_2_to_the_pw():
    """a PW-20 core: the bits of phase0 and *d_last above PW are ignored"""
    import torch
    name = "pw20"
    cfg, ocfg, gain = both(name)
    assert cfg.pw == 20
    work = work_buffer(torch)
    rng = np.random.default_rng(17)
    for n in (1, 4, 4101):
        x, y = iq(rng, n, cfg.iw)
        phase0, preset = 0xfff9abcd, 0xabc7fff3
        wm, wf, wl = expected(ocfg, gain, 20, x, y, (phase0 + preset) & 0xfffff)
        assert wl < 1 << 20
        last = last_word(torch, preset)
        m, f = run(torch, cfg, work, x, y, phase0, last)
        assert np.array_equal(m, wm) and np.array_equal(f, wf), n
        assert last_value(last) == wl
        assert f.min() >= -(1 << 19) and f.max() < 1 << 19


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg3", "natr2p24"])
def test_gpu_accumulating_the_steps_gives_back_the_phases(name):
    """cordic_phase_accumulate(freq, phase0 = prev), one sample on, is
    cordic_r2p's phase array in the low PW bits: device against device"""
    import torch
    from gpu_util import DEV, dev_i32, to_np
    cfg = both(name)[0]
    n = ca.fm_demod_info(cfg)[1] * 2 + 7
    mask = np.uint32((1 << cfg.pw) - 1 & 0xffffffff)
    x, y = iq(np.random.default_rng(18), n, cfg.iw)
    dx, dy = dev_i32(x), dev_i32(y)
    mag = torch.zeros(n, dtype=torch.int32, device=DEV)
    freq = torch.zeros(n, dtype=torch.int32, device=DEV)
    ph = torch.zeros(n, dtype=torch.int32, device=DEV)
    acc = torch.zeros(n, dtype=torch.int32, device=DEV)
    prev = 0x0badcafe
    ca.fm_demod(cfg, dx, dy, mag, freq, work_buffer(torch, n), phase0=prev)
    ca.r2p(cfg, dx, dy, mag, ph)
    end = last_word(torch, 0)
    ca.phase_accumulate(freq, acc, phase0=prev, acc=end,
                        work=torch.zeros(ca.fm_workspace(n), dtype=torch.uint8,
                                         device=DEV))
    torch.cuda.synchronize()
    a, p = to_np(acc, np.uint32), to_np(ph, np.uint32)
    assert a[0] & mask == prev & int(mask)
    assert np.array_equal(a[1:] & mask, p[:-1])
    assert last_value(end) & int(mask) == int(p[-1])


@pytest.mark.gpu
def test_gpu_loop_back_through_the_fm_oscillator_equals_the_oracle_chain():
    """cordic_table_fm with a quadrature output (QTR, OW 24, PW 18) into
    cordic_fm_demod on a converter with IW 24"""
    import torch
    from gpu_util import DEV, dev_i32, to_np
    from test_table_fm import TableCore, expected as osc_expected, words
    osc = TableCore(ca.QTR, -1, 24, 18)
    cfg, ocfg, gain = both("cfg3")
    assert cfg.iw == osc.ow == 24
    n = ca.fm_demod_info(cfg)[1] + 9
    fcw = words("random", n, 19)
    p, _ = osc_expected(fcw, None, 0x1234)
    with np.errstate(over="ignore"):
        ws, wc = osc.oracle(p), osc.oracle(p + np.uint32(1 << (osc.pw - 2)))
    wm, wf, wl = expected(ocfg, gain, cfg.pw, wc, ws, 0)
    s = torch.zeros(n, dtype=torch.int32, device=DEV)
    c = torch.zeros(n, dtype=torch.int32, device=DEV)
    osc.h.fm(dev_i32(fcw), s, c, phase0=0x1234,
             work=torch.zeros(ca.fm_workspace(n), dtype=torch.uint8, device=DEV))
    mag = torch.zeros(n, dtype=torch.int32, device=DEV)
    freq = torch.zeros(n, dtype=torch.int32, device=DEV)
    last = last_word(torch, 0)
    ca.fm_demod(cfg, c, s, mag, freq, work_buffer(torch, n), last=last)
    torch.cuda.synchronize()
    assert np.array_equal(to_np(s), ws) and np.array_equal(to_np(c), wc)
    assert np.array_equal(to_np(mag), wm) and np.array_equal(to_np(freq), wf)
    assert last_value(last) == wl
    osc.h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg3", "r2p35"])
def test_gpu_demod_in_a_hip_graph_continues_from_replay_to_replay(name):
    """captured with a shared d_last and replayed three times on new samples
    in the same input buffers: one call over the concatenated samples"""
    import torch
    from gpu_util import DEV, dev_i32
    cfg, ocfg, gain = both(name)
    n = (1 << 18) + 5
    x, y = iq(np.random.default_rng(20), 3 * n, cfg.iw)
    preset = 0x13572468
    wm, wf, wl = expected(ocfg, gain, cfg.pw, x, y, preset)
    work = work_buffer(torch, n)
    last = last_word(torch, preset)
    dx, dy = dev_i32(x[:n]), dev_i32(y[:n])
    mag = torch.zeros(n, dtype=torch.int32, device=DEV)
    freq = torch.zeros(n, dtype=torch.int32, device=DEV)
    # (once outside the capture, on a word of its own)
    ca.fm_demod(cfg, dx, dy, mag, freq, work, last=last_word(torch, 0))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ca.fm_demod(cfg, dx, dy, mag, freq, work, last=last)
    got_m, got_f = [], []
    for k in range(3):
        dx.copy_(dev_i32(x[k * n:(k + 1) * n]))
        dy.copy_(dev_i32(y[k * n:(k + 1) * n]))
        mag.zero_(); freq.zero_()
        g.replay()
        torch.cuda.synchronize()
        got_m.append(mag.cpu().numpy())
        got_f.append(freq.cpu().numpy())
    assert np.array_equal(np.concatenate(got_m), wm)
    assert np.array_equal(np.concatenate(got_f), wf)
    assert last_value(last) == wl
    del g


@pytest.mark.gpu
def test_gpu_bad_arguments_are_refused_and_nothing_is_written():
    import torch
    n = 64
    cfg = both("cfg3")[0]
    work = work_buffer(torch, 1 << 20)      # (longer than need be: a slice will do)
    wbytes = ca.fm_demod_workspace(n)
    ins = Padded(torch, 2 * n, 0, src=np.arange(2 * n, dtype=np.int32))
    outs = Padded(torch, 4 * n, 0)                # outputs cut from one array
    last = last_word(torch, 77)
    x, v = ins.t, outs.t

    def refused(status, a, b, m, f, w, cfg=cfg, last=last):
        with pytest.raises(ca.CordicError) as e:
            ca.fm_demod(cfg, a, b, m, f, w, n=n, last=last)
        assert e.value.status == status

    A = ca.ERR_ARGS
    y, m, f = x[n:], v[:n], v[2 * n:]
    refused(A, None, y, m, f, work)                       # every NULL
    refused(A, x, None, m, f, work)
    refused(A, x, y, None, f, work)
    refused(A, x, y, m, None, work)
    refused(A, x, y, m, f, 0)
    odd = lambda t: t.data_ptr() + 2                      # every misalignment
    refused(A, odd(x), y, m, f, work)
    refused(A, x, odd(y), m, f, work)
    refused(A, x, y, odd(m), f, work)
    refused(A, x, y, m, odd(f), work)
    refused(A, x, y, m, f, work[8:])
    refused(A, x, y, m, f, work, last=last.data_ptr() + 2)
    refused(A, x, y, m, x[n - 1:], work)                  # d_ofreq on d_xval
    refused(A, x, y, m, y[1:], work)                      # d_ofreq on d_yval
    refused(A, x, y, x[1:], f, work)                      # d_omag on d_xval
    refused(A, x, y, m, v[n - 1:], work)                  # d_omag on d_ofreq
    refused(A, x, y, m, f, work, last=work.data_ptr() + wbytes - 4)  # d_last in d_work
    refused(A, x, y, m, f, work, last=v[n - 1:])          # d_last in d_omag
    refused(A, x, y, m, f, work, last=x[3:])              # d_last in d_xval
    refused(A, x, y, m, f, x[n - 4:])                     # d_work on an input
    refused(A, x, y, m, f, v[n - 4:])                     # d_work on d_omag
    p2r = ca.Config.from_cli(ca.P2R, 24, 24, 2, -1, -1)
    refused(ca.ERR_MODE, x, y, m, f, work, cfg=p2r)       # the wrong mode
    # the 16-bit form: odd byte addresses
    c16 = both("io16")[0]
    ptrs = [x.data_ptr(), y.data_ptr(), m.data_ptr(), f.data_ptr()]
    for k in range(4):
        q = [a + (1 if j == k else 0) for j, a in enumerate(ptrs)]
        assert ca.lib().cordic_fm_demod16(c16.ref, n, q[0], q[1], 0, last.data_ptr(),
                                          q[2], q[3], work.data_ptr(), None) == A
    ca.fm_demod(cfg, None, None, None, None, None, n=0, last=last)     # a no-op
    torch.cuda.synchronize()
    assert last_value(last) == 77 and outs.untouched()
    ca.fm_demod(cfg, x, x, m, f, work, n=n, last=last_word(torch, 1))  # inputs may alias
    torch.cuda.synchronize()
    assert np.array_equal(ins.get(), np.arange(2 * n, dtype=np.int32))
    h = outs.t.cpu().numpy()
    assert (h[n:2 * n] == S32).all() and (h[3 * n:] == S32).all()
