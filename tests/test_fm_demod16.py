"""FM demodulation and demodulation banks on int16 I/Q arrays
(cordic_fm_demod16 on its fused kernel, cordic_fm_demod16_info,
cordic_demodbank_create16; include/cordic_amd.h).  Expected values need no
tolerance: expected() of tests/test_fm_demod.py restated -- the oracle's
topolar, a numpy difference mod 2^PW and a sign extension -- on the shorts
taken mod 2^IW, truncated to int16, which loses nothing: the values are
sign-extended OW- and PW-bit numbers, OW, PW <= 16."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O
from test_fm_demod import Padded, last_value, last_word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_fm_demod16_info", "cordic_demodbank_create16")
FIELDS = ["d_xval", "d_yval", "d_omag", "d_ofreq", "d_last", "n", "phase0", "reserved"]
UG = ca.FLAG_UNIT_GAIN
# name: (cli args: mode, iw, ow, xtra, pw, nstages; flags)
CORES = {
    "io16": ((ca.R2P, 16, 16, 2, 16, -1), 0),           # WW 24, 13 stages
    "io16_ug": ((ca.R2P, 16, 16, 2, 16, -1), UG),
    "sr16": ((ca.SR2P, 16, 16, 2, 16, -1), 0),
    "i12": ((ca.R2P, 12, 12, 2, 12, -1), 0),            # junk above bit 11 is ignored
    "pw8": ((ca.R2P, 16, 16, 2, 8, -1), 0),             # sign extension from 8 bits
    "ww34": ((ca.R2P, 16, 16, 7, 16, -1), 0),           # pol_stage1_lj_early
    "ww36": ((ca.R2P, 16, 16, 8, 16, -1), 0),           # not fused
    "ow1": ((ca.R2P, 16, 1, 2, 16, -1), 0),             # wraps: not fused
    "io16_no_lj": ((ca.R2P, 16, 16, 2, 16, -1), ca.FLAG_NO_LJ),
}
FUSED = ("io16", "io16_ug", "sr16", "i12", "pw8", "ww34")
ONE_BY_ONE = ("ww36", "ow1", "io16_no_lj")
T = 8188
PASSES = (1, 2, 4, 8)


def both(name):
    args, flags = CORES[name]
    cfg = ca.Config.from_cli(*args)
    if flags:
        cfg = cfg.with_flags(flags)
    gain = ca.lib().cordic_config_gain_annihilator(cfg.ref) if flags & UG else None
    return cfg, O.config_cli(*args), gain


def assert_named_for(name, cfg):
    """what the cores are named for"""
    if name in ("io16", "io16_ug", "sr16", "io16_no_lj"):
        assert (cfg.ww, cfg.nlive) == (24, 13)
    if name == "ww34":
        assert cfg.ww == 34
    if name == "ww36":
        assert cfg.ww == 36
    if name == "ow1":
        assert cfg.needs_wrap
    if name == "i12":
        assert cfg.iw == 12
    if name == "pw8":
        assert cfg.pw == 8


def tile_of(p):
    return (256 * p - 1) * 4


# ---------------------------------------------------------------- no GPU

def test_the_16_bit_forms_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    c = r"(\s*/\*.*?\*/)?\s*"
    assert re.search(r"int\s+cordic_fm_demod16_info\s*\(\s*const\s+cordic_config\s*\*\s*"
                     r"cfg\s*,\s*int32_t\s*\*\s*fused\s*,\s*int32_t\s*\*\s*tile\s*\)\s*;",
                     text)
    assert re.search(
        r"typedef\s+struct\s+cordic_demod_job16\s*\{\s*"
        r"const\s+int16_t\s*\*\s*d_xval\s*,\s*\*\s*d_yval\s*;" + c +
        r"int16_t\s*\*\s*d_omag\s*,\s*\*\s*d_ofreq\s*;" + c +
        r"uint32_t\s*\*\s*d_last\s*;" + c +
        r"uint64_t\s+n\s*;" + c +
        r"uint32_t\s+phase0\s*;" + c +
        r"uint32_t\s+reserved\s*;" + c +
        r"\}\s*cordic_demod_job16\s*;", text, re.S)
    assert re.search(
        r"int\s+cordic_demodbank_create16\s*\(\s*const\s+cordic_config\s*\*\s*cfg\s*,"
        r"\s*size_t\s+njobs\s*,\s*const\s+cordic_demod_job16\s*\*\s*jobs\s*,\s*"
        r"cordic_demodbank\s*\*\*\s*bank\s*\)\s*;", text)
    assert "There is no 16-bit form" not in text
    from cordic_amd import _native
    for name in NAMES + ("cordic_fm_demod16",):
        getattr(ca.lib(), name)             # AttributeError: not exported
        assert name in _native.ABI
    assert "fm_demod16_info" in ca.__all__ and callable(ca.fm_demod16_info)
    assert "DemodBank16" in ca.__all__ and issubclass(ca.DemodBank16, ca.DemodBank)
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_header_is_plain_c99_and_the_job_is_56_bytes(tmp_path):
    src, lay, exe = tmp_path / "t.c", tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { cordic_config c; cordic_demod_job16 j; int32_t f, t; int rc;\n'
        'cordic_demodbank *b = 0; int16_t *a = 0;\n'
        'char size_is_56[sizeof(cordic_demod_job16) == 56 ? 1 : -1];\n'
        'cordic_config_init(&c, CORDIC_R2P, 16, 16, 2, 16, -1);\n'
        'j.d_xval = j.d_yval = a; j.d_omag = j.d_ofreq = a; j.d_last = 0; j.n = 0;\n'
        'j.phase0 = 0; j.reserved = 0; (void)size_is_56;\n'
        'rc = cordic_fm_demod16_info(&c, &f, &t);\n'
        'rc += cordic_demodbank_create16(&c, 1, &j, &b);\n'
        'rc += cordic_demodbank_run(b, 0); cordic_demodbank_destroy(b);\n'
        'return rc; }\n')
    flags = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
             os.path.join(ROOT, "include")]
    r = subprocess.run(flags + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the layout from a compiled offsetof program: cordic_demod_job's, which the
    # ctypes mirror that DemodBank16 fills has
    lay.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "cordic_amd.h"\n'
        'int main(void) { printf("%zu", sizeof(cordic_demod_job16));\n'
        + "".join('printf(" %%zu %%zu", offsetof(cordic_demod_job16, %s), '
                  'offsetof(cordic_demod_job, %s));\n' % (f, f) for f in FIELDS)
        + 'return 0; }\n')
    r = subprocess.run(flags + [str(lay), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    nums = [int(v) for v in r.stdout.split()]
    mirror = ca._native._CDemodJob
    assert nums[0] == 56 == C.sizeof(mirror)
    assert nums[1::2] == nums[2::2] == [0, 8, 16, 24, 32, 40, 48, 52]
    assert [getattr(mirror, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 52]


def test_nulls_and_a_rotator_are_refused_before_a_handle_is_made():
    L = ca.lib()
    cfg = both("io16")[0]
    p2r = ca.Config.from_cli(ca.P2R, 16, 16, 2, 16, -1)
    h = C.c_void_p(0x5a5a)
    job = ca._native._CDemodJob()
    assert L.cordic_demodbank_create16(None, 0, None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_demodbank_create16(None, 1, C.byref(job), C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_demodbank_create16(cfg.ref, 1, None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_demodbank_create16(cfg.ref, 0, None, None) == ca.ERR_ARGS
    assert L.cordic_demodbank_create16(p2r.ref, 0, None, C.byref(h)) == ca.ERR_MODE
    assert L.cordic_demodbank_create16(p2r.ref, 1, C.byref(job), C.byref(h)) == ca.ERR_MODE
    # the container's rule holds for a bank without jobs as well
    for wide in ((ca.R2P, 16, 16, 2, 17, -1), (ca.R2P, 16, 24, 2, 16, -1)):
        c = ca.Config.from_cli(*wide)
        assert L.cordic_demodbank_create16(c.ref, 0, None, C.byref(h)) == ca.ERR_CONTAINER
        assert L.cordic_demodbank_create16(c.ref, 1, C.byref(job), C.byref(h)) \
            == ca.ERR_CONTAINER
    assert h.value == 0x5a5a                # no handle was made


def test_the_16_bit_path_query_answers_in_the_order_of_the_call():
    L = ca.lib()
    f, t = C.c_int32(-5), C.c_int32(-5)
    ask = lambda cfg: L.cordic_fm_demod16_info(cfg, C.byref(f), C.byref(t))
    assert ask(None) == ca.ERR_ARGS
    assert ask(ca.Config.from_cli(ca.R2P, 16, 16, 2, 17, -1).ref) == ca.ERR_CONTAINER
    assert ask(ca.Config.from_cli(ca.R2P, 16, 24, 2, 16, -1).ref) == ca.ERR_CONTAINER
    assert ask(ca.Config.from_cli(ca.P2R, 16, 16, 2, 16, -1).ref) == ca.ERR_MODE
    assert (f.value, t.value) == (-5, -5)   # untouched on every error
    # either pointer may be NULL
    assert L.cordic_fm_demod16_info(both("io16")[0].ref, None, None) == 0
    for name in CORES:
        cfg = both(name)[0]
        assert_named_for(name, cfg)
        assert ca.fm_demod16_info(cfg) == ((1, T) if name in FUSED else (0, 0)), name
    # the binding takes shorts only
    import torch
    with pytest.raises(TypeError):
        ca.DemodBank16(both("io16")[0], [(torch.zeros(4, dtype=torch.int32), 2, 4, 6, 4,
                                          0, None)])


# ---------------------------------------------------------------- GPU

S16 = 0x5a5b
PHASE0, PRESET = 0x9e3779b1, 0x7f4a7c15     # bits above PW set in both
LENGTHS = (1, 3, 4, 5, 7, 8, 1023, 1024, 1025, T - 1, T, T + 1, T + 4, T + 5, 2 * T + 5)
# element offsets behind an 8-byte boundary (torch allocations sit on 256-byte
# ones): 4 is offset 0 with guards in front
ROT = (4, 1, 2, 3)


def offsets(r):
    """(x, y, mag, freq): every array at each of the offsets 0 .. 3 shorts as r
    runs over 0 .. 3, the four of one call all different"""
    return tuple(ROT[(r + k) % 4] for k in range(4))


def sext(v, bits):
    v = v.astype(np.int64) & ((1 << bits) - 1)
    return ((v ^ (1 << (bits - 1))) - (1 << (bits - 1))).astype(np.int32)


def iq16(rng, n):
    """random over the full range of a short, whatever IW"""
    return (rng.integers(-32768, 32768, n).astype(np.int16),
            rng.integers(-32768, 32768, n).astype(np.int16))


def hard_points(rng, n, iw):
    """x = y = 0, the axes, the diagonals, +/-1 LSB around each and the most
    negative port value, in random order in front of random full-scale samples:
    topolar's phase wraps between such neighbours and the sign extension flips
    (hard_points of tests/test_fm_demod.py, as int16)"""
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
    assert pts.min() >= lo and pts.max() <= hi
    x, y = iq16(rng, n)
    m = min(n, len(pts))
    x[:m], y[:m] = pts[:m, 0], pts[:m, 1]
    return x, y


def expected(ocfg, gain, cfg, x, y, prev):
    """(mag, freq as int16, ph_(n-1)) for the phase `prev` in front of sample 0;
    x, y: the shorts as they lie in memory, taken mod 2^IW"""
    pw = cfg.pw
    mag, ph = O.topolar(ocfg, sext(x, cfg.iw), sext(y, cfg.iw))
    if gain is not None:            # o = (o * K) >> 32 (CORDIC_FLAG_UNIT_GAIN)
        mag = ((mag.astype(np.int64) * gain) >> 32).astype(np.int32)
    mask = (1 << pw) - 1
    p = ph.astype(np.int64)
    before = np.concatenate([[prev & mask], p[:-1]]) if p.size else p
    d = (p - before) & mask
    sign = 1 << (pw - 1)
    freq = ((d ^ sign) - sign).astype(np.int64)
    return (mag.astype(np.int16), freq.astype(np.int16),
            (int(ph[-1]) if ph.size else None))


def work_buffer(torch, n):
    from gpu_util import DEV
    return torch.zeros(max(16, ca.fm_demod_workspace(n)), dtype=torch.uint8, device=DEV)


def run16(torch, cfg, work, x, y, phase0=0, last=None, offs=None):
    """one call with x, y, mag, freq at their element offsets behind an aligned
    start; (mag, freq) after checking the guards and the inputs"""
    offs = offs or offsets(0)
    n = x.size
    dx = Padded(torch, n, offs[0], True, src=x)
    dy = Padded(torch, n, offs[1], True, src=y)
    dm = Padded(torch, n, offs[2], True)
    df = Padded(torch, n, offs[3], True)
    ca.fm_demod(cfg, dx.view, dy.view, dm.view, df.view, work, n=n, phase0=phase0,
                last=last)
    torch.cuda.synchronize()
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    return dm.get(), df.get()


def check16(torch, name, x, y, work, r, tag=None):
    """with a preset d_last word and a phase0 with high bits, and without
    either, against the oracle; (mag, freq, last) of the first"""
    cfg, ocfg, gain = both(name)
    n = x.size
    wm, wf, wl = expected(ocfg, gain, cfg, x, y, PHASE0 + PRESET)
    last = last_word(torch, PRESET)
    m, f = run16(torch, cfg, work, x, y, PHASE0, last, offsets(r))
    assert np.array_equal(m, wm), (name, n, tag, r)
    assert np.array_equal(f, wf), (name, n, tag, r)
    assert last_value(last) == wl, (name, n, tag)       # as a 32-bit word
    wm0, wf0, _ = expected(ocfg, gain, cfg, x, y, 0)
    m0, f0 = run16(torch, cfg, work, x, y, 0, None, offsets(r + 1))
    assert np.array_equal(m0, wm0) and np.array_equal(f0, wf0), (name, n, tag, r)
    return m, f, wl


def wide_call(torch, cfg, work, x, y, phase0, preset):
    """cordic_fm_demod on widened copies: (mag, freq narrowed, last)"""
    from gpu_util import DEV, dev_i32
    n = x.size
    wx, wy = dev_i32(x.astype(np.int32)), dev_i32(y.astype(np.int32))
    m = torch.zeros(n, dtype=torch.int32, device=DEV)
    f = torch.zeros(n, dtype=torch.int32, device=DEV)
    last = last_word(torch, preset)
    ca.fm_demod(cfg, wx, wy, m, f, work, n=n, phase0=phase0, last=last)
    torch.cuda.synchronize()
    return (m.cpu().numpy().astype(np.int16), f.cpu().numpy().astype(np.int16),
            last_value(last))


def test_the_offsets_put_every_array_on_every_alignment():
    for k in range(4):
        assert sorted(offsets(r)[k] % 4 for r in range(4)) == [0, 1, 2, 3]
        assert all(offsets(r)[k] > 0 for r in range(4))
    for r in range(4):
        assert len({o % 4 for o in offsets(r)}) == 4
    # check16 uses r and r + 1 per length, over the lengths every r
    assert {i % 4 for i in range(len(LENGTHS))} == {0, 1, 2, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED)
def test_gpu_fused_cores_equal_the_oracle_and_the_32_bit_call(name):
    import torch
    cfg = both(name)[0]
    assert_named_for(name, cfg)
    assert ca.fm_demod16_info(cfg) == (1, T)
    work = work_buffer(torch, 2 * T + 5)
    rng = np.random.default_rng(16)
    for i, n in enumerate(LENGTHS):
        x, y = iq16(rng, n) if i % 2 else hard_points(rng, n, cfg.iw)
        m, f, l = check16(torch, name, x, y, work, i, "hard" if i % 2 == 0 else None)
        wm, wf, wl = wide_call(torch, cfg, work, x, y, PHASE0, PRESET)
        assert np.array_equal(m, wm) and np.array_equal(f, wf) and l == wl, (name, n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ONE_BY_ONE)
def test_gpu_cores_off_the_fused_path_keep_the_fallback_and_its_bits(name):
    import torch
    cfg = both(name)[0]
    assert_named_for(name, cfg)
    assert ca.fm_demod16_info(cfg) == (0, 0)
    work = work_buffer(torch, T + 5)
    rng = np.random.default_rng(17)
    for i, n in enumerate((1, 5, 1025, T + 5)):
        x, y = hard_points(rng, n, cfg.iw)
        check16(torch, name, x, y, work, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["io16", "ww34"])
def test_gpu_many_tiles_per_block_give_the_uncapped_bits(name, monkeypatch):
    """n = 5 T + 3 on grids capped at 1 and 2 blocks: 5 and 2 or 3 tiles per
    block, so `par` is carried from tile to tile"""
    import torch
    cfg, ocfg, gain = both(name)
    assert ca.fm_demod16_info(cfg) == (1, T)
    n = 5 * T + 3
    work = work_buffer(torch, n)
    x, y = hard_points(np.random.default_rng(18), n, cfg.iw)
    wm, wf, wl = expected(ocfg, gain, cfg, x, y, PHASE0 + PRESET)
    monkeypatch.delenv("CORDIC_FMD_MAX_BLOCKS", raising=False)
    for cap in (None, 1, 2):
        if cap:
            monkeypatch.setenv("CORDIC_FMD_MAX_BLOCKS", str(cap))
        last = last_word(torch, PRESET)
        m, f = run16(torch, cfg, work, x, y, PHASE0, last, offsets(cap or 0))
        assert np.array_equal(m, wm) and np.array_equal(f, wf), cap
        assert last_value(last) == wl, cap


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["io16", "pw8", "ww36"])
def test_gpu_three_calls_that_share_the_last_word_equal_one_call(name):
    import torch
    cfg, ocfg, gain = both(name)
    assert ca.fm_demod16_info(cfg)[0] == (1 if name in FUSED else 0)
    cuts = (0, 1023, 1023 + T + 2, 1023 + T + 2 + 4101)
    n = cuts[-1]
    work = work_buffer(torch, n)
    x, y = iq16(np.random.default_rng(19), n)
    wm, wf, wl = expected(ocfg, gain, cfg, x, y, PHASE0 + PRESET)
    last = last_word(torch, PRESET)
    ms, fs = [], []
    for k in range(3):          # phase0 in the first call only: every call adds it
        a, b = cuts[k], cuts[k + 1]
        m, f = run16(torch, cfg, work, x[a:b], y[a:b], PHASE0 if k == 0 else 0, last,
                     offsets(k))
        ms.append(m)
        fs.append(f)
    assert np.array_equal(np.concatenate(ms), wm)
    assert np.array_equal(np.concatenate(fs), wf)
    assert last_value(last) == wl


@pytest.mark.gpu
def test_gpu_the_call_in_a_graph_continues_on_every_replay():
    """one stream, no parallel branches; once outside the capture first.  Every
    run adds phase0 to the word the run before left, which on unchanged inputs
    is the phase of sample n - 1: replay 1 starts from the preset word, replays
    2 and 3 from that phase."""
    import torch
    name = "io16"
    cfg, ocfg, gain = both(name)
    assert ca.fm_demod16_info(cfg) == (1, T)
    n = T + 7
    work = work_buffer(torch, n)
    x, y = iq16(np.random.default_rng(20), n)
    offs = offsets(1)
    dx = Padded(torch, n, offs[0], True, src=x)
    dy = Padded(torch, n, offs[1], True, src=y)
    dm = Padded(torch, n, offs[2], True)
    df = Padded(torch, n, offs[3], True)
    last = last_word(torch, 0)

    def call():
        ca.fm_demod(cfg, dx.view, dy.view, dm.view, df.view, work, n=n, phase0=PHASE0,
                    last=last)
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    last.copy_(last_word(torch, PRESET))
    prev = PHASE0 + PRESET
    for k in range(3):
        dm.t.fill_(S16)
        df.t.fill_(S16)
        g.replay()
        torch.cuda.synchronize()
        wm, wf, wl = expected(ocfg, gain, cfg, x, y, prev)
        assert np.array_equal(dm.get(), wm), k
        assert np.array_equal(df.get(), wf), k
        assert last_value(last) == wl, k
        prev = PHASE0 + wl
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    del g


# ---------------------------------------------------------------- banks

SENT = np.int16(S16)
SENT32 = -0x5a5a5a5b
SENT_U = SENT32 & 0xffffffff


def ragged_lengths():
    ns = [0, 1, 3, 4, 5, 7, 8, 1019, 1020, 1021, 1024]
    for p in PASSES:
        ns += [tile_of(p) + d for d in (-1, 0, 1, 5)]
    ns += [0, 2, 6, 4099, 2 * T + 3, 12, 1, 1023, 513, 77, 9, 4096, 2051]
    order = np.random.default_rng(32).permutation(len(ns))
    return [ns[i] for i in order]


class Spec:
    """The host side of a 16-bit bank in two arenas of shorts (inputs; outputs
    between sentinels) and an array of d_last words, four per job.  Job k's
    arrays start (k + a) % 4 shorts behind an 8-byte boundary, a = 0 .. 3 for
    x, y, mag, freq; every second job has a d_last."""

    def __init__(self, lengths, iw, seed, phase0=None, every_last=False):
        rng = np.random.default_rng(seed)
        self.ns = list(lengths)
        k = len(self.ns)
        self.has_last = [every_last or j % 2 == 0 for j in range(k)]
        self.phase0 = [int(v) for v in rng.integers(0, 1 << 32, k)] \
            if phase0 is None else [phase0] * k
        self.preset = [int(v) for v in rng.integers(0, 1 << 32, k)]
        self.off = []
        cur_in = cur_out = 4
        for j, n in enumerate(self.ns):
            o = []
            for a in range(4):
                cur = cur_in if a < 2 else cur_out
                at = (cur + 3) // 4 * 4 + (j + a) % 4
                o.append(at)
                if a < 2:
                    cur_in = at + n
                else:
                    cur_out = at + n + 1   # at least one sentinel between
            self.off.append(tuple(o))
        self.in_len, self.out_len = cur_in + 8, cur_out + 8
        self.x, self.y = [], []
        for j, n in enumerate(self.ns):
            x, y = hard_points(rng, n, iw) if j % 3 == 0 else iq16(rng, n)
            self.x.append(x)
            self.y.append(y)

    def renew(self, seed):
        rng = np.random.default_rng(seed)
        for j, n in enumerate(self.ns):
            self.x[j], self.y[j] = iq16(rng, n)

    def tiles(self, passes):
        v = passes * 256 - 1
        return sum((n // 4 + v - 1) // v for n in self.ns)

    def tail_jobs(self):
        return sum(1 for n, l in zip(self.ns, self.has_last) if n and (n % 4 or l))


class DeviceBank:
    """`spec` on the device and a DemodBank16 over it"""

    def __init__(self, torch, cfg, spec):
        from gpu_util import DEV
        self.torch, self.spec = torch, spec
        self.ins = torch.zeros(spec.in_len, dtype=torch.int16, device=DEV)
        self.outs = torch.full((spec.out_len,), S16, dtype=torch.int16, device=DEV)
        self.lasts = torch.full((4 * max(1, len(spec.ns)),), SENT32, dtype=torch.int32,
                                device=DEV)
        self.upload()
        self.preset(spec.preset)
        jobs = []
        for j, n in enumerate(spec.ns):
            ox, oy, om, of = spec.off[j]
            jobs.append((self.ins[ox:], self.ins[oy:], self.outs[om:], self.outs[of:],
                         n, spec.phase0[j],
                         self.lasts[4 * j:] if spec.has_last[j] else None))
        self.bank = ca.DemodBank16(cfg, jobs)

    def preset(self, values):
        from gpu_util import DEV
        h = np.full(self.lasts.numel(), SENT_U, dtype=np.uint32)
        for j, l in enumerate(self.spec.has_last):
            if l:
                h[4 * j] = values[j]
        self.lasts.copy_(self.torch.from_numpy(h.view(np.int32)).to(DEV))

    def upload(self):
        from gpu_util import DEV
        h = np.zeros(self.spec.in_len, dtype=np.int16)
        for j, n in enumerate(self.spec.ns):
            ox, oy = self.spec.off[j][:2]
            h[ox:ox + n] = self.spec.x[j]
            h[oy:oy + n] = self.spec.y[j]
        self.ins.copy_(self.torch.from_numpy(h).to(DEV))
        self.h_ins = h

    def results(self):
        """([(mag, freq)], [last or None]) after checking that the inputs, the
        sentinels and the words of jobs without a d_last are as they were"""
        self.torch.cuda.synchronize()
        spec = self.spec
        assert np.array_equal(self.ins.cpu().numpy(), self.h_ins)
        o = self.outs.cpu().numpy()
        l = self.lasts.cpu().numpy().view(np.uint32)
        written = np.zeros(o.size, dtype=bool)
        got, lasts = [], []
        for j, n in enumerate(spec.ns):
            om, of = spec.off[j][2:]
            written[om:om + n] = True
            written[of:of + n] = True
            got.append((o[om:om + n].copy(), o[of:of + n].copy()))
            lasts.append(int(l[4 * j]) if spec.has_last[j] else None)
            if not spec.has_last[j]:
                assert l[4 * j] == SENT_U, j
            assert (l[4 * j + 1:4 * j + 4] == SENT_U).all(), j
        assert (o[~written] == SENT).all()
        return got, lasts


@functools.lru_cache(maxsize=None)
def ragged_spec(iw):
    return Spec(ragged_lengths(), iw, 200 + iw)


@functools.lru_cache(maxsize=None)
def ragged_expected(name):
    """per job (mag, freq, last after the run) of the ragged bank, once per core"""
    cfg, ocfg, gain = both(name)
    spec = ragged_spec(cfg.iw)
    want = []
    for j, n in enumerate(spec.ns):
        prev = spec.phase0[j] + (spec.preset[j] if spec.has_last[j] else 0)
        m, f, l = expected(ocfg, gain, cfg, spec.x[j], spec.y[j], prev)
        if not spec.has_last[j]:
            l = None
        elif n == 0:
            l = spec.preset[j]
        want.append((m, f, l))
    return want


def assert_equals(got, lasts, want, tag):
    for j, ((m, f), l, (wm, wf, wl)) in enumerate(zip(got, lasts, want)):
        assert np.array_equal(m, wm), (tag, j, m.size)
        assert np.array_equal(f, wf), (tag, j, f.size)
        assert l == wl, (tag, j, m.size)


def single_calls(torch, cfg, spec):
    """one cordic_fm_demod16 call per job on copies of the same data"""
    from gpu_util import DEV
    work = work_buffer(torch, max(spec.ns))
    out = []
    for j, n in enumerate(spec.ns):
        x = torch.from_numpy(spec.x[j]).to(DEV)
        y = torch.from_numpy(spec.y[j]).to(DEV)
        m = torch.zeros(max(n, 1), dtype=torch.int16, device=DEV)
        f = torch.zeros(max(n, 1), dtype=torch.int16, device=DEV)
        last = last_word(torch, spec.preset[j]) if spec.has_last[j] else None
        ca.fm_demod(cfg, x, y, m, f, work, n=n, phase0=spec.phase0[j], last=last)
        torch.cuda.synchronize()
        out.append((m.cpu().numpy()[:n], f.cpu().numpy()[:n],
                    None if last is None else last_value(last)))
    return out


def test_the_ragged_bank_has_the_lengths_and_placements_it_is_meant_to_have():
    spec = ragged_spec(16)
    for n in [0, 1, 3, 4, 5, 7, 8, 1019, 1020, 1021, 1024] + [
            tile_of(p) + d for p in PASSES for d in (-1, 0, 1, 5)]:
        assert n in spec.ns
    assert 36 <= len(spec.ns) <= 44
    assert sum(spec.has_last) == (len(spec.ns) + 1) // 2
    assert any(p >> 24 for p in spec.phase0)
    for o in spec.off:
        assert len({a % 4 for a in o}) == 4          # all four displaced differently
    for a in range(4):                               # every 2-byte alignment mod 8
        assert {o[a] % 4 for o in spec.off} == {0, 1, 2, 3}
    # torch allocations sit on 256-byte boundaries: the offsets are the alignment


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED + ONE_BY_ONE)
def test_gpu_ragged_bank_equals_the_oracle_and_the_single_calls(name, monkeypatch):
    import torch
    monkeypatch.delenv("CORDIC_FMD_BANK_PASSES", raising=False)
    monkeypatch.delenv("CORDIC_FMD_MAX_BLOCKS", raising=False)
    cfg = both(name)[0]
    assert_named_for(name, cfg)
    spec = ragged_spec(cfg.iw)
    d = DeviceBank(torch, cfg, spec)
    info = d.bank.info()
    assert info["samples"] == sum(spec.ns)
    assert info["fused"] == ca.fm_demod16_info(cfg)[0] == (1 if name in FUSED else 0)
    if info["fused"]:
        assert info["tile"] in [tile_of(p) for p in PASSES]
        p = (info["tile"] // 4 + 1) // 256
        assert info["tiles"] == spec.tiles(p)
        assert info["tail_jobs"] == spec.tail_jobs()
    else:
        assert (info["tile"], info["tiles"], info["tail_jobs"]) == (0, 0, 0)
    d.bank.run()
    got, lasts = d.results()
    assert_equals(got, lasts, ragged_expected(name), name)
    assert_equals(got, lasts, single_calls(torch, cfg, spec), name + " single calls")
    d.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["io16", "ww34"])
def test_gpu_forced_tile_sizes_and_grid_caps_give_the_same_bits(name, monkeypatch):
    import torch
    cfg = both(name)[0]
    spec = ragged_spec(cfg.iw)
    want = ragged_expected(name)
    monkeypatch.delenv("CORDIC_FMD_MAX_BLOCKS", raising=False)
    for p in PASSES:
        monkeypatch.setenv("CORDIC_FMD_BANK_PASSES", str(p))
        d = DeviceBank(torch, cfg, spec)
        info = d.bank.info()
        assert info["fused"] == 1 and info["tile"] == tile_of(p)
        assert info["tiles"] == spec.tiles(p) and info["tail_jobs"] == spec.tail_jobs()
        d.bank.run()
        got, lasts = d.results()
        assert_equals(got, lasts, want, "passes %d" % p)
        d.bank.close()
    monkeypatch.delenv("CORDIC_FMD_BANK_PASSES")
    for cap in (1, 3):
        monkeypatch.setenv("CORDIC_FMD_MAX_BLOCKS", str(cap))
        d = DeviceBank(torch, cfg, spec)
        assert d.bank.info()["fused"] == 1 and d.bank.info()["tiles"] >= 3 * cap
        d.bank.run()
        got, lasts = d.results()
        assert_equals(got, lasts, want, "max blocks %d" % cap)
        d.bank.close()


ROUNDS, CHANNELS, BLOCK = 3, 8, 4099


def continuation(name):
    """(spec, [x, y per round], per channel the oracle's pass over the three
    blocks in a row with 0 in front)"""
    cfg, ocfg, gain = both(name)
    spec = Spec([BLOCK] * CHANNELS, cfg.iw, 42, phase0=0, every_last=True)
    spec.preset = [0] * CHANNELS
    rounds = []
    for r in range(ROUNDS):
        spec.renew(50 + r)
        rounds.append(([a.copy() for a in spec.x], [a.copy() for a in spec.y]))
    want = [expected(ocfg, gain, cfg,
                     np.concatenate([rounds[r][0][j] for r in range(ROUNDS)]),
                     np.concatenate([rounds[r][1][j] for r in range(ROUNDS)]), 0)
            for j in range(CHANNELS)]
    return cfg, spec, rounds, want


def check_continuation(name, parts, lasts, want):
    for j in range(CHANNELS):
        assert np.array_equal(np.concatenate([p[j][0] for p in parts]), want[j][0]), (name, j)
        assert np.array_equal(np.concatenate([p[j][1] for p in parts]), want[j][1]), (name, j)
        assert lasts[j] == want[j][2], (name, j)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["io16", "ww36"])
def test_gpu_three_runs_on_new_data_continue_every_channel(name):
    import torch
    cfg, spec, rounds, want = continuation(name)
    d = DeviceBank(torch, cfg, spec)
    assert d.bank.info()["fused"] == (1 if name in FUSED else 0)
    parts = []
    for r in range(ROUNDS):
        spec.x, spec.y = rounds[r]
        d.upload()
        d.bank.run()
        got, lasts = d.results()
        parts.append(got)
    check_continuation(name, parts, lasts, want)
    d.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["io16", "ww36"])
def test_gpu_a_captured_run_replayed_three_times_continues_three_times(name):
    """one stream, no parallel branches; once outside the capture first, on a
    bank with words of its own"""
    import torch
    cfg, spec, rounds, want = continuation(name)
    warm = DeviceBank(torch, cfg, spec)
    warm.bank.run()
    torch.cuda.synchronize()
    warm.bank.close()
    d = DeviceBank(torch, cfg, spec)
    assert d.bank.info()["fused"] == (1 if name in FUSED else 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d.bank.run()
    parts = []
    for r in range(ROUNDS):
        spec.x, spec.y = rounds[r]
        d.upload()
        d.outs.fill_(S16)
        g.replay()
        got, lasts = d.results()
        parts.append(got)
    check_continuation(name, parts, lasts, want)
    del g
    d.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["io16", "pw8", "ww36"])
def test_gpu_phase0_is_added_by_every_run(name):
    import torch
    cfg, ocfg, gain = both(name)
    lengths = [1, 3, 4, 6, 1023, 4101]
    phase0 = 0xfff9abcd
    spec = Spec(lengths, cfg.iw, 61, phase0=phase0, every_last=True)
    d = DeviceBank(torch, cfg, spec)
    assert d.bank.info()["fused"] == (1 if name in FUSED else 0)
    prev = [phase0 + p for p in spec.preset]
    for run in range(2):
        d.outs.fill_(S16)
        d.bank.run()
        got, lasts = d.results()
        want = [expected(ocfg, gain, cfg, spec.x[j], spec.y[j], prev[j])
                for j in range(len(lengths))]
        assert_equals(got, lasts, want, (name, run))
        assert all(l < 1 << cfg.pw for l in lasts)
        prev = [phase0 + l for l in lasts]
    d.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["io16", "ww36"])
def test_gpu_empty_banks_run_and_write_nothing(name):
    import torch
    cfg = both(name)[0]
    for lengths in ([], [0, 0, 0]):
        spec = Spec(lengths, cfg.iw, 71, every_last=True)
        d = DeviceBank(torch, cfg, spec)
        info = d.bank.info()
        assert (info["samples"], info["tiles"], info["tail_jobs"]) == (0, 0, 0)
        d.bank.run()
        got, lasts = d.results()
        assert lasts == spec.preset[:len(lengths)]
        assert (d.outs == S16).all().item()
        d.bank.close()
    # a zero-length job's pointers are not looked at
    b = ca.DemodBank16(cfg, [(3, 5, 7, 9, 0, 0, 11)])
    b.run()
    torch.cuda.synchronize()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["io16", "ww36"])
def test_gpu_create_refuses_overlaps_and_bad_jobs_with_nothing_written(name):
    import torch
    from gpu_util import DEV
    cfg = both(name)[0]
    n = 64
    ins = torch.arange(4 * n, dtype=torch.int16, device=DEV)
    outs = torch.full((6 * n,), S16, dtype=torch.int16, device=DEV)
    lasts = torch.full((8,), SENT32, dtype=torch.int32, device=DEV)
    x0, y0, x1, y1 = (ins[k * n:] for k in range(4))
    m0, f0, m1, f1 = (outs[k * n:] for k in range(4))
    l0, l1 = lasts, lasts[4:]

    def job(x=x0, y=y0, m=m0, f=f0, last=l0):
        return (x, y, m, f, n, 0, last)

    def other(x=x1, y=y1, m=m1, f=f1, last=l1):
        return (x, y, m, f, n, 0, last)

    def refused(*jobs, status=ca.ERR_ARGS, core=cfg):
        with pytest.raises(ca.CordicError) as e:
            ca.DemodBank16(core, list(jobs))
        assert e.value.status == status

    odd = lambda t: t.data_ptr() + 1
    # overlaps by ONE SHORT: output over output of the same job and of another
    # job, output over an input of the same job and of another job
    refused(job(f=outs[n - 1:]))
    refused(job(), other(m=outs[2 * n - 1:], f=outs[4 * n:]))
    refused(job(), other(f=outs[2 * n - 1:], m=outs[4 * n:]))
    refused(job(m=ins[2 * n - 1:]))
    refused(job(y=x0), other(x=x0, y=x0, f=ins[n - 1:]))
    refused(job(m=ins[3 * n:]), other())                # ... and by a whole array
    refused(job(), other(last=l0))                      # a shared d_last
    refused(job(), other(last=outs[n - 2:].data_ptr())) # d_last over an output's last shorts
    refused(job(last=ins[6:].data_ptr()))               # ... inside an input array
    for k in range(4):                                  # an odd byte address
        a = [x0, y0, m0, f0]
        a[k] = odd(a[k])
        refused(job(*a))
    refused(job(last=l0.data_ptr() + 2))                # d_last off the 4-byte grid
    for k in range(4):                                  # a NULL sample pointer
        a = [x0, y0, m0, f0]
        a[k] = None
        refused(job(*a))
    arr = (ca._native._CDemodJob * 1)()                 # reserved != 0
    for k, v in zip(("d_xval", "d_yval", "d_omag", "d_ofreq"), (x0, y0, m0, f0)):
        setattr(arr[0], k, v.data_ptr())
    arr[0].n, arr[0].reserved = n, 1
    h = C.c_void_p(0x5a5a)
    assert ca.lib().cordic_demodbank_create16(cfg.ref, 1, arr, C.byref(h)) == ca.ERR_ARGS
    assert h.value == 0x5a5a
    for wide in ((ca.R2P, 16, 16, 2, 17, -1), (ca.R2P, 16, 24, 2, 16, -1),
                 (ca.R2P, 17, 16, 2, 16, -1)):          # wide cores
        refused(job(), status=ca.ERR_CONTAINER, core=ca.Config.from_cli(*wide))
    torch.cuda.synchronize()
    assert (outs == S16).all().item() and (lasts == SENT32).all().item()
    assert torch.equal(ins, torch.arange(4 * n, dtype=torch.int16, device=DEV))
    # the adjacent case is accepted: m1 begins where m0 ends, at any 2-byte
    # alignment; inputs may alias each other
    b = ca.DemodBank16(cfg, [job(y=x0), other(x=x0, y=x0, m=outs[2 * n:],
                                              f=outs[3 * n + 1:])])
    b.run()
    torch.cuda.synchronize()
    h = outs.cpu().numpy()
    for k in range(3):
        assert (h[k * n:(k + 1) * n] != S16).any(), k
    assert (h[3 * n + 1:4 * n + 1] != S16).any()
    assert h[3 * n] == S16 and (h[4 * n + 1:] == S16).all()
    b.close()


@pytest.mark.gpu
def test_gpu_the_example_builds_and_says_that_nothing_differs(tmp_path):
    """examples/afc_channeliser16.c: a 16-bit mixer bank into a 16-bit
    demodulation bank, three rounds, against the per-channel *16 calls"""
    exe = tmp_path / "afc_channeliser16"
    r = subprocess.run(
        ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
         "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
         "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-o", str(exe),
         os.path.join(ROOT, "examples", "afc_channeliser16.c"),
         "-L", os.path.join(ROOT, "cordic_amd"), "-lcordic_amd", "-L", "/opt/rocm/lib",
         "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "cordic_amd"),
         "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "-c", "8", "-l", "4099", "-r", "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "8 channels x 4099 samples x 3 rounds" in r.stdout
    assert re.search(r"demodulation bank: \d+ tiles of at most \d+, 8 tails \(fused, two "
                     r"launches per round\)", r.stdout), r.stdout
    assert "\n0 shorts or words differ from the chain run channel by channel" in r.stdout
