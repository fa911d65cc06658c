"""The FM mixer and FM mixer banks on int16 I/Q arrays (cordic_plan_fm_mix16,
cordic_plan_fm_mix16_workspace, cordic_mixbank_create16; include/cordic_amd.h).
Expected values need no tolerance: numpy's wrapping cumulative sum (expected()
of tests/test_table_fm.py) feeds the oracle's rotate, as want() of
tests/test_fm_mix.py, and the result is truncated to int16 -- exact, because
the oracle's outputs are sign-extended OW-bit values and OW <= 16."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O
from test_fm_demod import S16, Padded, last_value, last_word
from test_fm_mix import CORES, PHASE0, PRESET, _hip, sext
from test_table_fm import expected as phases, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_plan_fm_mix16_workspace", "cordic_plan_fm_mix16",
         "cordic_mixbank_create16")
FIELDS = ["d_fcw", "d_pm", "d_xval", "d_yval", "d_oxval", "d_oyval", "d_acc", "n",
          "phase0", "reserved"]
UG = ca.FLAG_UNIT_GAIN
# name: (cli args, flags).  nat16, n9: tests/test_fm_mix.py; cfg1:
# tools/bench_common.py
CORES16 = {
    "nat16": CORES["nat16"],                            # WW 19, PW 23, 19 stages
    "cfg1": ((ca.P2R, 16, 16, 2, 16, 16), 0),
    "pw32": ((ca.P2R, 16, 16, 2, 32, 16), 0),
    "nat12": ((ca.P2R, 12, 12, 2, -1, -1), 0),
    "n9": CORES["n9"],                                  # 9 live stages
    "cfg1_ug": ((ca.P2R, 16, 16, 2, 16, 16), UG),
    "sp2r16": ((ca.SP2R, 16, 16, 2, 16, 16), 0),
}
SIZES = (0, 1, 255, 256, 257, 1 << 20, 1 << 33)
M32 = 0xffffffff


def both(name):
    args, flags = CORES16[name]
    cfg = ca.Config.from_cli(*args)
    if flags:
        cfg = cfg.with_flags(flags)
    gain = ca.lib().cordic_config_gain_annihilator(cfg.ref) if flags & UG else None
    return cfg, O.config_cli(*args), gain


# ---------------------------------------------------------------- no GPU

def test_the_16_bit_forms_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    c = r"(\s*/\*.*?\*/)?\s*"
    assert re.search(r"size_t\s+cordic_plan_fm_mix16_workspace\s*\(\s*const\s+cordic_plan"
                     r"\s*\*\s*plan\s*,\s*size_t\s+n\s*\)\s*;", text)
    assert re.search(
        r"int\s+cordic_plan_fm_mix16\s*\(\s*const\s+cordic_plan\s*\*\s*plan\s*,\s*size_t\s+n"
        r"\s*,\s*const\s+uint32_t\s*\*\s*d_fcw\s*,\s*const\s+uint32_t\s*\*\s*d_pm\s*,\s*"
        r"uint32_t\s+phase0\s*,\s*uint32_t\s*\*\s*d_acc\s*,\s*const\s+int16_t\s*\*\s*d_xval"
        r"\s*,\s*const\s+int16_t\s*\*\s*d_yval\s*,\s*int16_t\s*\*\s*d_oxval\s*,\s*int16_t"
        r"\s*\*\s*d_oyval\s*,\s*void\s*\*\s*d_work\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(
        r"typedef\s+struct\s+cordic_fmmix_job16\s*\{\s*"
        r"const\s+uint32_t\s*\*\s*d_fcw\s*;" + c +
        r"const\s+uint32_t\s*\*\s*d_pm\s*;" + c +
        r"const\s+int16_t\s*\*\s*d_xval\s*,\s*\*\s*d_yval\s*;" + c +
        r"int16_t\s*\*\s*d_oxval\s*,\s*\*\s*d_oyval\s*;" + c +
        r"uint32_t\s*\*\s*d_acc\s*;" + c +
        r"uint64_t\s+n\s*;" + c +
        r"uint32_t\s+phase0\s*;" + c +
        r"uint32_t\s+reserved\s*;" + c +
        r"\}\s*cordic_fmmix_job16\s*;", text, re.S)
    assert re.search(
        r"int\s+cordic_mixbank_create16\s*\(\s*const\s+cordic_plan\s*\*\s*plan\s*,"
        r"\s*size_t\s+njobs\s*,\s*const\s+cordic_fmmix_job16\s*\*\s*jobs\s*,\s*"
        r"cordic_mixbank\s*\*\*\s*bank\s*\)\s*;", text)
    # the mixer block no longer denies the int16 form; no second info function
    assert "There is no int16 form" not in text
    assert "have no looked-up-direction kernel" not in text
    assert "cordic_plan_fm_mix16_info" not in text
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
    from cordic_amd import _native
    for name in NAMES:
        assert name in _native.ABI
    for name in ("fm_mix16", "fm_mix16_workspace"):
        assert callable(getattr(ca.Plan, name))
    assert "MixBank16" in ca.__all__ and issubclass(ca.MixBank16, ca.MixBank)
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_header_with_the_16_bit_forms_is_plain_c99_and_the_job_is_72_bytes(tmp_path):
    src, lay, exe = tmp_path / "t.c", tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { const cordic_plan *p = 0; cordic_fmmix_job16 j;\n'
        'cordic_mixbank *b = 0; int16_t *a = 0; uint32_t *w = 0; int rc; size_t s;\n'
        'char size_is_72[sizeof(cordic_fmmix_job16) == 72 ? 1 : -1];\n'
        'j.d_fcw = j.d_pm = 0; j.d_xval = j.d_yval = a; j.d_oxval = j.d_oyval = a;\n'
        'j.d_acc = 0; j.n = 0; j.phase0 = 0; j.reserved = 0; (void)size_is_72;\n'
        's = cordic_plan_fm_mix16_workspace(p, 8);\n'
        'rc = cordic_plan_fm_mix16(p, 0, w, w, 0, w, a, a, a, a, 0, 0);\n'
        'rc += cordic_mixbank_create16(p, 1, &j, &b);\n'
        'rc += cordic_mixbank_run(b, 0); cordic_mixbank_destroy(b);\n'
        'return rc + (int)s; }\n')
    flags = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
             os.path.join(ROOT, "include")]
    r = subprocess.run(flags + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the layout from a compiled offsetof program: cordic_fmmix_job's, which the
    # ctypes mirror that MixBank16 fills has
    lay.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "cordic_amd.h"\n'
        'int main(void) { printf("%zu", sizeof(cordic_fmmix_job16));\n'
        + "".join('printf(" %%zu %%zu", offsetof(cordic_fmmix_job16, %s), '
                  'offsetof(cordic_fmmix_job, %s));\n' % (f, f) for f in FIELDS)
        + 'return 0; }\n')
    r = subprocess.run(flags + [str(lay), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    nums = [int(v) for v in r.stdout.split()]
    assert nums[0] == 72 == C.sizeof(ca._native._CFmMixJob)
    assert nums[1::2] == nums[2::2] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68]


def test_a_null_plan_is_refused_without_a_device():
    L = ca.lib()
    for n in (0, 8):
        assert L.cordic_plan_fm_mix16(None, n, None, None, 0, None, None, None, None,
                                      None, None, None) == ca.ERR_ARGS
    assert L.cordic_plan_fm_mix16_workspace(None, 1 << 20) == 0
    h = C.c_void_p(0x5a5a)
    job = ca._native._CFmMixJob()
    assert L.cordic_mixbank_create16(None, 0, None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_mixbank_create16(None, 1, C.byref(job), C.byref(h)) == ca.ERR_ARGS
    assert h.value == 0x5a5a                # no handle was made
    # (a core with 9 live stages has no direction tables and, with IW 16, no
    # seed table worth a device: its plan is host memory)
    plan = ca.Plan(both("n9")[0])
    assert L.cordic_mixbank_create16(plan._h, 1, None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_mixbank_create16(plan._h, 0, None, None) == ca.ERR_ARGS
    assert L.cordic_plan_fm_mix16(plan._h, 0, None, None, 0, None, None, None, None,
                                  None, None, None) == 0           # n = 0: a no-op
    assert h.value == 0x5a5a
    plan.close()


def workspace_properties(plan, fused):
    last = 0
    for n in SIZES:
        w = plan.fm_mix16_workspace(n)
        assert w % 16 == 0, n
        assert w >= last, n
        assert (w == 0) == (n == 0), n
        if fused:
            assert w == plan.fm_mix_workspace(n), n
        else:
            assert w <= 20 * n + 65536 + 96, n
            assert w >= plan.fm_mix_workspace(n) + 16 * n, n   # four int32 arrays
        last = w


def test_the_workspace_of_a_fallback_plan_holds_the_widened_arrays():
    plan = ca.Plan(both("n9")[0])
    assert plan.fm_mix_info() == (0, 0)
    workspace_properties(plan, False)
    plan.close()
    # not a p2r / sp2r plan, and one whose ports do not fit: 0
    r2p = ca.Plan(ca.Config.from_cli(ca.R2P, 16, 16, 2, -1, 9))
    assert r2p.fm_mix16_workspace(64) == 0
    r2p.close()
    wide = ca.Plan(CORES_WIDE())
    assert wide.fm_mix16_workspace(64) == 0 and wide.fm_mix_workspace(64) > 0
    wide.close()


def CORES_WIDE():
    """ww38 of tests/test_fm_mix.py: IW 32, and a plan that needs no device"""
    return ca.Config.from_cli(*CORES["ww38"][0])


def test_the_binding_refuses_a_short_work_buffer_and_wide_tensors():
    import torch
    plan = ca.Plan(both("n9")[0])
    with pytest.raises(TypeError):
        plan.fm_mix16(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, n=8)
    short = torch.zeros(plan.fm_mix16_workspace(8) - 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        plan.fm_mix16(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, short, n=8)
    # (what serves the 32-bit call is too short for the 16-bit fallback)
    assert plan.fm_mix_workspace(8) < plan.fm_mix16_workspace(8)
    with pytest.raises(ValueError):
        plan.fm_mix16(0x1000, 0x2000, 0x3000, 0x4000, 0x5000,
                      torch.zeros(plan.fm_mix_workspace(8), dtype=torch.uint8), n=8)
    with pytest.raises(TypeError):
        plan.fm_mix16(0x1000, torch.zeros(8, dtype=torch.int32), 0x3000, 0x4000,
                      0x5000, torch.zeros(1 << 17, dtype=torch.uint8), n=8)
    plan.close()


# ---------------------------------------------------------------- GPU

FUSED_CASES = ("nat16", "cfg1", "pw32", "nat12")
FALLBACK = ("n9", "cfg1_ug", "sp2r16")
LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025, 2051, 65539)
# element offsets behind a 16-byte boundary: 8 is offset 0 with guards in front
ROT = (8, 1, 2, 3)


def offsets(r):
    """every sample array at each of the offsets 0 .. 3 as r runs over 0 .. 3;
    fcw and pm at their own"""
    at = lambda k: ROT[(r + k) % 4]
    return dict(x=at(0), y=at(1), ox=at(2), oy=at(3), fcw=(r + 3) % 4 or 4,
                pm=(r + 1) % 4 or 4)


def work_buffer(torch, plan, n):
    from gpu_util import DEV
    return torch.zeros(max(16, plan.fm_mix16_workspace(n)), dtype=torch.uint8,
                       device=DEV)


def iq16(rng, n, bits=16):
    """random over the full range of `bits`, the most negative and the most
    positive value among them, as int16"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    x = rng.integers(lo, hi + 1, n).astype(np.int16)
    y = rng.integers(lo, hi + 1, n).astype(np.int16)
    for k, v in enumerate((lo, hi, hi, lo)):
        if k < n:
            x[k] = v
            y[(k * 7 + 2) % n] = v
    return x, y


def want16(name, x, y, p):
    """what cordic_p2r writes for (x, y sign-extended, phase = p), as int16"""
    cfg, ocfg, gain = both(name)
    mask = np.uint32((1 << cfg.pw) - 1 & M32)
    ox, oy = O.rotate(ocfg, sext(x.astype(np.int32), cfg.iw),
                      sext(y.astype(np.int32), cfg.iw), p & mask)
    if gain is not None:        # o = (o * K) >> 32 (CORDIC_FLAG_UNIT_GAIN)
        ox = ((ox.astype(np.int64) * gain) >> 32).astype(np.int32)
        oy = ((oy.astype(np.int64) * gain) >> 32).astype(np.int32)
    # (truncation loses nothing: sign-extended OW-bit values, OW <= 16)
    assert np.array_equal(ox.astype(np.int16), ox) and np.array_equal(oy.astype(np.int16), oy)
    return ox.astype(np.int16), oy.astype(np.int16)


def run16(torch, plan, work, fcw, pm, x, y, phase0=0, acc=None, offs=None):
    """one call with every array at its element offset behind an aligned
    start; (ox, oy) after checking the guards and the inputs"""
    offs = offs or offsets(0)
    n = x.size
    i32 = lambda a: None if a is None else a.view(np.int32)
    df = Padded(torch, n, offs["fcw"], src=i32(fcw))
    dm = None if pm is None else Padded(torch, n, offs["pm"], src=i32(pm))
    dx = Padded(torch, n, offs["x"], i16=True, src=x)
    dy = Padded(torch, n, offs["y"], i16=True, src=y)
    ox = Padded(torch, n, offs["ox"], i16=True)
    oy = Padded(torch, n, offs["oy"], i16=True)
    plan.fm_mix16(df.view, dx.view, dy.view, ox.view, oy.view, work,
                  pm=None if dm is None else dm.view, n=n, phase0=phase0, acc=acc)
    torch.cuda.synchronize()
    assert np.array_equal(df.get(), i32(fcw))
    assert dm is None or np.array_equal(dm.get(), i32(pm))
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    return ox.get(), oy.get()


def check16(torch, name, plan, work, fcw, pm, x, y, tag=None, r=0):
    """with a preset d_acc word and without one, against the oracle"""
    n = x.size
    p, final = phases(fcw, pm, PHASE0, PRESET)
    wx, wy = want16(name, x, y, p)
    acc = last_word(torch, PRESET)
    gx, gy = run16(torch, plan, work, fcw, pm, x, y, PHASE0, acc, offsets(r))
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (name, n, tag, r, "acc")
    assert last_value(acc) == final, (name, n, tag)
    p, _ = phases(fcw, pm, PHASE0)
    wx, wy = want16(name, x, y, p)
    gx, gy = run16(torch, plan, work, fcw, pm, x, y, PHASE0, None, offsets(r + 1))
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (name, n, tag, r)


def fused16(plan):
    """the rule of the header: the 32-bit form's answer, and WW < 35"""
    return plan.fm_mix_info()[0] == 1 and plan.cfg.ww < 35


def test_the_offsets_put_every_array_on_every_alignment():
    for k in ("x", "y", "ox", "oy"):
        assert sorted(offsets(r)[k] % 8 for r in range(4)) == [0, 1, 2, 3]
    for k in ("fcw", "pm"):
        assert sorted(offsets(r)[k] % 4 for r in range(4)) == [0, 1, 2, 3]
        assert all(offsets(r)[k] > 0 for r in range(4))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED_CASES)
def test_gpu_fused_cores_equal_the_oracle(name):
    import torch
    cfg = both(name)[0]
    assert cfg.iw <= 16 and cfg.ow <= 16
    plan = ca.Plan(cfg)
    fused, tile = plan.fm_mix_info()
    if name == "nat16":
        assert fused == 1 and cfg.ww < 35
    assert tile == (1024 if fused else 0)
    workspace_properties(plan, fused16(plan))
    rng = np.random.default_rng(131)
    r = 0
    for n in LENGTHS:
        work = work_buffer(torch, plan, n)
        x, y = iq16(rng, n, cfg.iw)
        for kind in ("zero", "ones", "random", "fsk"):
            fcw = words(kind, n, 40 + n % 7)
            for pm in (None, words("random", n, 50 + n % 5)):
                check16(torch, name, plan, work, fcw, pm, x, y, tag=kind, r=r)
                r += 2      # (check16 uses r and r + 1)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nat16", "n9"])
def test_gpu_the_call_equals_the_32_bit_call_on_widened_copies(name):
    import torch
    from gpu_util import DEV, dev_i32, to_np
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    assert fused16(plan) == (name == "nat16")
    n = 3 * 1024 + 5
    rng = np.random.default_rng(132)
    x, y = iq16(rng, n)
    fcw, pm = words("random", n, 21), words("random", n, 22)
    w32 = torch.zeros(max(16, plan.fm_mix_workspace(n)), dtype=torch.uint8, device=DEV)
    wx = torch.zeros(n, dtype=torch.int32, device=DEV)
    wy = torch.zeros(n, dtype=torch.int32, device=DEV)
    acc32 = last_word(torch, PRESET)
    plan.fm_mix(dev_i32(fcw), dev_i32(x.astype(np.int32)), dev_i32(y.astype(np.int32)),
                wx, wy, w32, pm=dev_i32(pm), phase0=PHASE0, acc=acc32)
    acc16 = last_word(torch, PRESET)
    gx, gy = run16(torch, plan, work_buffer(torch, plan, n), fcw, pm, x, y, PHASE0,
                   acc16, offsets(1))
    assert np.array_equal(gx.astype(np.int32), to_np(wx))
    assert np.array_equal(gy.astype(np.int32), to_np(wy))
    assert last_value(acc16) == last_value(acc32)
    plan.close()


@pytest.mark.gpu
def test_gpu_many_passes_per_block_give_the_same_bits(monkeypatch):
    """5 * 1024 + 7 samples are 6 passes: on 1 and on 3 blocks
    (CORDIC_FMX_MAX_BLOCKS, cordic_fm_mix.hip) and on the grid the library
    chooses"""
    import torch
    name = "nat16"
    plan = ca.Plan(both(name)[0])
    n = 5 * 1024 + 7
    work = work_buffer(torch, plan, n)
    rng = np.random.default_rng(133)
    x, y = iq16(rng, n)
    fcw, pm = words("random", n, 5), words("random", n, 6)
    p, final = phases(fcw, pm, PHASE0, PRESET)
    wx, wy = want16(name, x, y, p)
    for cap in (1, 3, None):
        if cap is None:
            monkeypatch.delenv("CORDIC_FMX_MAX_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("CORDIC_FMX_MAX_BLOCKS", str(cap))
        acc = last_word(torch, PRESET)
        gx, gy = run16(torch, plan, work, fcw, pm, x, y, PHASE0, acc, offsets(3))
        assert np.array_equal(gx, wx) and np.array_equal(gy, wy), cap
        assert last_value(acc) == final, cap
    plan.close()


@pytest.mark.gpu
def test_gpu_bits_above_the_input_width_are_ignored():
    """the 12-bit core with garbage in bits 12 .. 15 of x and y"""
    import torch
    name = "nat12"
    cfg = both(name)[0]
    assert cfg.iw == 12
    plan = ca.Plan(cfg)
    rng = np.random.default_rng(134)
    n = 1024 + 7
    x, y = iq16(rng, n, 12)
    top = lambda: (rng.integers(0, 16, n) << 12).astype(np.uint16)
    gx = ((x.view(np.uint16) & 0x0fff) | top()).view(np.int16)
    gy = ((y.view(np.uint16) & 0x0fff) | top()).view(np.int16)
    assert not np.array_equal(gx, x) and not np.array_equal(gy, y)
    assert np.array_equal(sext(gx.astype(np.int32), 12), x)
    check16(torch, name, plan, work_buffer(torch, plan, n), words("random", n, 3),
            words("random", n, 4), gx, gy, r=1)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FALLBACK)
def test_gpu_fallback_plans_equal_the_oracle(name):
    import torch
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    assert plan.fm_mix_info() == (0, 0)
    workspace_properties(plan, False)
    rng = np.random.default_rng(135)
    for r, n in enumerate((1, 5, 4099)):
        work = work_buffer(torch, plan, n)
        x, y = iq16(rng, n, cfg.iw)
        for kind, pm in (("random", words("random", n, 9)), ("ones", None)):
            check16(torch, name, plan, work, words(kind, n, 10), pm, x, y, tag=kind, r=r)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nat16", "n9"])
def test_gpu_consecutive_calls_that_share_the_accumulator_equal_one_call(name):
    import torch
    plan = ca.Plan(both(name)[0])
    T = 1024
    n = 2 * T + 7
    cuts = [0, 1, T - 1, T + 2, n]
    work = work_buffer(torch, plan, n)
    rng = np.random.default_rng(137)
    x, y = iq16(rng, n)
    fcw, pm = words("random", n, 13), words("random", n, 14)
    p, final = phases(fcw, pm, PHASE0, PRESET)
    wx, wy = want16(name, x, y, p)
    acc = last_word(torch, PRESET)
    gx, gy = run16(torch, plan, work, fcw, pm, x, y, PHASE0, acc)
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy)
    assert last_value(acc) == final
    acc = last_word(torch, PRESET)
    parts = [run16(torch, plan, work, fcw[a:b], pm[a:b], x[a:b], y[a:b],
                   PHASE0 if a == 0 else 0, acc, offsets(k))
             for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
    assert np.array_equal(np.concatenate([q[0] for q in parts]), wx)
    assert np.array_equal(np.concatenate([q[1] for q in parts]), wy)
    assert last_value(acc) == final
    plan.close()


# ---- banks

BANK_LENGTHS = (0, 1, 3, 4, 1023, 1024, 1025, 3000, 9001)
SENT_U = 0xa5a5a5a5
KNOBS = ("CORDIC_FMXB_MAX_BLOCKS", "CORDIC_FMXB_PASSES", "CORDIC_FMXB_MAX_SPANS")


class Spec16:
    """37 ragged jobs in three arenas: the words (fcw, pm; int32), the input
    samples and the output samples (int16, the outputs between sentinels).
    Every array starts an odd number of elements behind a 16-byte boundary."""

    def __init__(self, seed, lengths=None):
        rng = np.random.default_rng(seed)
        if lengths is None:
            lengths = list(BANK_LENGTHS) * 4 + [9001]
            lengths = [lengths[i] for i in rng.permutation(len(lengths))]
        self.ns = list(lengths)
        k = len(self.ns)
        self.has_pm = [bool(j % 3) for j in range(k)]
        self.has_acc = [bool((j + 1) % 4) for j in range(k)]
        self.phase0 = [int(v) | 0x80000000 for v in rng.integers(0, 1 << 32, k)]
        self.preset = [int(v) | 0x80000000 for v in rng.integers(0, 1 << 32, k)]
        self.off = []               # element offsets of fcw, pm, x, y, ox, oy
        cw = ci = co = 8
        for j, n in enumerate(self.ns):
            odd = lambda cur, per, a: (cur + per - 1) // per * per + 1 + 2 * ((j + a) % 2)
            f = odd(cw, 4, 0); cw = f + n
            m = odd(cw, 4, 1); cw = m + n
            x = odd(ci, 8, 0); ci = x + n
            y = odd(ci, 8, 1); ci = y + n
            ox = odd(co, 8, 1); co = ox + n
            oy = odd(co, 8, 0); co = oy + n
            self.off.append((f, m, x, y, ox, oy))
        self.words, self.ins, self.outs = cw + 8, ci + 8, co + 8
        self.fcw, self.pm, self.x, self.y = [], [], [], []
        for j, n in enumerate(self.ns):
            s = int(rng.integers(0, 1 << 30))
            self.fcw.append(words("random" if j % 5 else "fsk", n, s))
            self.pm.append(words("random", n, s + 1) if self.has_pm[j] else None)
            x, y = iq16(rng, n)
            self.x.append(x)
            self.y.append(y)


class DeviceBank16:
    """`spec` on the device and a MixBank16 over it"""

    def __init__(self, torch, plan, spec):
        from gpu_util import DEV
        self.torch, self.spec = torch, spec
        hw = np.zeros(spec.words, dtype=np.int32)
        hi = np.zeros(spec.ins, dtype=np.int16)
        for j, n in enumerate(spec.ns):
            f, m, x, y = spec.off[j][:4]
            hw[f:f + n] = spec.fcw[j].view(np.int32)
            if spec.has_pm[j]:
                hw[m:m + n] = spec.pm[j].view(np.int32)
            hi[x:x + n] = spec.x[j]
            hi[y:y + n] = spec.y[j]
        self.h_words, self.h_ins = hw, hi
        self.wordsd = torch.from_numpy(hw).to(DEV)
        self.ins = torch.from_numpy(hi).to(DEV)
        self.outs = torch.full((spec.outs,), S16, dtype=torch.int16, device=DEV)
        ha = np.full(4 * len(spec.ns), SENT_U, dtype=np.uint32)
        for j, l in enumerate(spec.has_acc):
            if l:
                ha[4 * j] = spec.preset[j]
        self.accs = torch.from_numpy(ha.view(np.int32)).to(DEV)
        jobs = []
        for j, n in enumerate(spec.ns):
            f, m, x, y, ox, oy = spec.off[j]
            jobs.append((self.wordsd[f:], self.wordsd[m:] if spec.has_pm[j] else None,
                         self.ins[x:], self.ins[y:], self.outs[ox:], self.outs[oy:], n,
                         spec.phase0[j], self.accs[4 * j:] if spec.has_acc[j] else None))
        self.bank = ca.MixBank16(plan, jobs)

    def results(self):
        """([(ox, oy)], [acc or None]) after checking that the inputs, the
        sentinels and the words of jobs without a d_acc are as they were"""
        self.torch.cuda.synchronize()
        spec = self.spec
        assert np.array_equal(self.wordsd.cpu().numpy(), self.h_words)
        assert np.array_equal(self.ins.cpu().numpy(), self.h_ins)
        o = self.outs.cpu().numpy()
        a = self.accs.cpu().numpy().view(np.uint32)
        written = np.zeros(o.size, dtype=bool)
        got, accs = [], []
        for j, n in enumerate(spec.ns):
            ox, oy = spec.off[j][4:]
            assert ox % 2 == 1 and oy % 2 == 1
            assert not written[ox - 1] and not written[oy - 1]
            written[ox:ox + n] = True
            written[oy:oy + n] = True
            got.append((o[ox:ox + n].copy(), o[oy:oy + n].copy()))
            accs.append(int(a[4 * j]) if spec.has_acc[j] else None)
            if not spec.has_acc[j]:
                assert a[4 * j] == SENT_U, j
            assert (a[4 * j + 1:4 * j + 4] == SENT_U).all(), j
        assert (o[~written] == S16).all()
        return got, accs


def single_calls16(torch, plan, spec, runs):
    """one cordic_plan_fm_mix16 call per job and run on copies of the same
    data; per run [(ox, oy, acc or None)]"""
    from gpu_util import DEV, dev_i32
    work = work_buffer(torch, plan, max(spec.ns))
    accs = [dev_i32(np.array([spec.preset[j]] * 4, dtype=np.uint32))
            if spec.has_acc[j] else None for j in range(len(spec.ns))]
    out = []
    for _ in range(runs):
        this = []
        for j, n in enumerate(spec.ns):
            f = dev_i32(spec.fcw[j])
            m = dev_i32(spec.pm[j]) if spec.has_pm[j] else None
            x = torch.from_numpy(spec.x[j]).to(DEV)
            y = torch.from_numpy(spec.y[j]).to(DEV)
            ox = torch.zeros(max(n, 1), dtype=torch.int16, device=DEV)
            oy = torch.zeros(max(n, 1), dtype=torch.int16, device=DEV)
            plan.fm_mix16(f, x, y, ox, oy, work, pm=m, n=n, phase0=spec.phase0[j],
                          acc=accs[j])
            torch.cuda.synchronize()
            this.append((ox.cpu().numpy()[:n], oy.cpu().numpy()[:n],
                         None if accs[j] is None
                         else int(accs[j].cpu().numpy().view(np.uint32)[0])))
        out.append(this)
    return out


def assert_equals(got, accs, wanted, tag):
    for j, ((gx, gy), a, (wx, wy, wa)) in enumerate(zip(got, accs, wanted)):
        assert np.array_equal(gx, wx), (tag, j, gx.size)
        assert np.array_equal(gy, wy), (tag, j, gy.size)
        assert a == wa, (tag, j, gx.size)


def spans_of(n, passes, cap=4096):
    if n == 0:
        return 0
    np_ = -(-n // 1024)
    while -(-np_ // passes) > cap:
        passes *= 2
    return -(-np_ // passes)


@functools.lru_cache(maxsize=None)
def ragged16():
    return Spec16(300)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nat16", "n9"])
def test_gpu_ragged_bank_run_twice_equals_the_single_calls(name, monkeypatch):
    import torch
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    plan = ca.Plan(both(name)[0])
    spec = ragged16()
    assert len(spec.ns) == 37 and set(spec.ns) == set(BANK_LENGTHS)
    assert 0 < sum(spec.has_pm) < 37 and 0 < sum(spec.has_acc) < 37
    d = DeviceBank16(torch, plan, spec)
    info = d.bank.info()
    assert info["samples"] == sum(spec.ns)
    assert info["fused"] == (1 if fused16(plan) else 0) == (1 if name == "nat16" else 0)
    if info["fused"]:
        p = info["tile"] // 1024
        assert info["tile"] == p * 1024 and p >= 1 and p & (p - 1) == 0
        assert info["spans"] == sum(spans_of(n, p) for n in spec.ns)
    else:
        assert (info["tile"], info["spans"]) == (0, 0)
    wanted = single_calls16(torch, plan, spec, 2)
    for run in range(2):            # the second continues every d_acc
        d.outs.fill_(S16)
        d.bank.run()
        got, accs = d.results()
        assert_equals(got, accs, wanted[run], (name, run))
    # ... and the oracle, for the first run
    for j in (0, 5, 36):
        n = spec.ns[j]
        acc0 = spec.preset[j] if spec.has_acc[j] else 0
        p, final = phases(spec.fcw[j], spec.pm[j], spec.phase0[j], acc0)
        wx, wy = want16(name, spec.x[j], spec.y[j], p)
        assert np.array_equal(wanted[0][j][0], wx) and np.array_equal(wanted[0][j][1], wy)
        if spec.has_acc[j]:
            assert wanted[0][j][2] == (final if n else acc0)
    d.bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_one_pass_spans_and_a_span_cap_of_two_give_the_same_bits(monkeypatch):
    """CORDIC_FMXB_PASSES=1 with CORDIC_FMXB_MAX_SPANS=2: a job of 6 passes
    walks two spans of 4 and 2, one of 9 passes two of 8 and 1"""
    import torch
    name = "nat16"
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    plan = ca.Plan(both(name)[0])
    spec = Spec16(301, [5 * 1024 + 7, 1, 9001, 1024, 0, 2049])
    wanted = []
    for j, n in enumerate(spec.ns):
        acc0 = spec.preset[j] if spec.has_acc[j] else 0
        p, final = phases(spec.fcw[j], spec.pm[j], spec.phase0[j], acc0)
        wx, wy = want16(name, spec.x[j], spec.y[j], p)
        wanted.append((wx, wy, None if not spec.has_acc[j] else final if n else acc0))
    for knobs in ({}, {"CORDIC_FMXB_PASSES": "1", "CORDIC_FMXB_MAX_SPANS": "2"}):
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        d = DeviceBank16(torch, plan, spec)
        info = d.bank.info()
        assert info["fused"] == 1
        if knobs:
            assert info["tile"] == 1024
            assert info["spans"] == sum(spans_of(n, 1, 2) for n in spec.ns) == 8
        d.bank.run()
        got, accs = d.results()
        assert_equals(got, accs, wanted, knobs)
        d.bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_the_fused_call_in_a_graph_is_one_chain_and_continues_on_replay():
    """captured once with a d_acc word and replayed three times on the same
    arrays: *d_acc = start + 3 * sum(fcw), the last replay's outputs are the
    oracle's for the phase it started from, and the graph is two kernel nodes
    with one edge between them"""
    import torch
    from gpu_util import DEV, dev_i32, to_np
    name = "nat16"
    plan = ca.Plan(both(name)[0])
    assert fused16(plan)
    n = 3 * 1024 + 5
    rng = np.random.default_rng(138)
    x, y = iq16(rng, n)
    fcw, pm = words("random", n, 15), words("random", n, 16)
    dfcw, dpm = dev_i32(fcw), dev_i32(pm)
    # (one element behind the allocation's start: 2-byte aligned, no more)
    dx = torch.zeros(n + 1, dtype=torch.int16, device=DEV)[1:]
    dy = torch.zeros(n + 1, dtype=torch.int16, device=DEV)[1:]
    dx.copy_(torch.from_numpy(x).to(DEV))
    dy.copy_(torch.from_numpy(y).to(DEV))
    ox = torch.zeros(n + 1, dtype=torch.int16, device=DEV)[1:]
    oy = torch.zeros(n + 3, dtype=torch.int16, device=DEV)[3:]
    work = work_buffer(torch, plan, n)
    acc = last_word(torch, PRESET)
    total = int(np.sum(fcw, dtype=np.uint64)) & M32

    hip = _hip()
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
        plan.fm_mix16(dfcw, dx, dy, ox, oy, work, pm=dpm, phase0=0, acc=acc,
                      stream=stream.cuda_stream)
    finally:
        rc = hip.hipStreamEndCapture(h, C.byref(graph))
    assert rc == 0 and graph.value
    try:
        assert last_value(acc) == PRESET             # captured, not run
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
            for _ in range(3):
                assert hip.hipGraphLaunch(ex, h) == 0
            stream.synchronize()
        finally:
            hip.hipGraphExecDestroy(ex)
    finally:
        hip.hipGraphDestroy(graph)
    # (phase0 = 0: every replay adds it again, and start = the preset word)
    assert last_value(acc) == (PRESET + 3 * total) & M32
    p, final = phases(fcw, pm, 0, (PRESET + 2 * total) & M32)
    assert final == last_value(acc)
    wx, wy = want16(name, x, y, p)
    assert np.array_equal(to_np(ox, np.int16), wx)
    assert np.array_equal(to_np(oy, np.int16), wy)
    plan.close()


@pytest.mark.gpu
def test_gpu_bad_arguments_are_refused_and_nothing_is_written():
    import torch
    from gpu_util import DEV
    n = 64
    plan = ca.Plan(both("nat16")[0])
    assert fused16(plan)
    big = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    work = big[:plan.fm_mix16_workspace(n)]
    wordsd = Padded(torch, 2 * n, 0, src=np.arange(2 * n, dtype=np.int32))
    ins = Padded(torch, 2 * n, 0, i16=True, src=np.arange(2 * n, dtype=np.int16))
    outs = Padded(torch, 4 * n, 0, i16=True)      # outputs cut from one array
    acc = last_word(torch, 77)
    w, i, v = wordsd.t, ins.t, outs.t
    f, m, x, y = w[:n], w[n:], i[:n], i[n:]
    a, b = v[:n], v[2 * n:]

    def refused(status, f, m, x, y, a, b, wk, plan=plan, acc=acc):
        with pytest.raises(ca.CordicError) as e:
            plan.fm_mix16(f, x, y, a, b, wk, pm=m, n=n, acc=acc)
        assert e.value.status == status

    A = ca.ERR_ARGS
    byte = lambda t: t.data_ptr() + 1                     # an odd byte address
    refused(A, f, m, byte(x), y, a, b, work)
    refused(A, f, m, x, byte(y), a, b, work)
    refused(A, f, m, x, y, byte(a), b, work)
    refused(A, f, m, x, y, a, byte(b), work)
    refused(A, f.data_ptr() + 2, m, x, y, a, b, work)     # d_fcw off the 4-byte grid
    refused(A, f, m.data_ptr() + 2, x, y, a, b, work)
    refused(A, f, m, x, y, a, b, work, acc=acc.data_ptr() + 2)
    refused(A, f, m, x, y, a, b, big[8:])                 # d_work off the 16-byte grid
    refused(A, f, m, x, y, i[n - 1:], b, work)            # an output over d_yval by one
    refused(A, f, m, x, y, a, v[n - 1:], work)            # d_oyval over d_oxval by one
    refused(A, None, m, x, y, a, b, work)
    refused(A, f, m, x, y, a, b, 0)
    # 2-byte offsets of the samples and one element behind an input are fine
    cfg2 = ca.Plan(ca.Config.from_cli(*CORES["cfg2"][0]))           # IW 32
    refused(ca.ERR_CONTAINER, f, m, x, y, a, b, work, plan=cfg2)
    r2p = ca.Plan(ca.Config.from_cli(ca.R2P, 16, 16, 2, -1, 16))
    refused(ca.ERR_MODE, f, m, x, y, a, b, work, plan=r2p)
    r2p32 = ca.Plan(ca.Config.from_cli(ca.R2P, 24, 24, 2, -1, 20))  # the mode comes first
    refused(ca.ERR_MODE, f, m, x, y, a, b, work, plan=r2p32)

    def job(f=f, m=m, x=x, y=y, a=a, b=b, acc=None):
        return (f, m, x, y, a, b, n, 0, acc)

    def bank_refused(status, jobs, plan=plan):
        with pytest.raises(ca.CordicError) as e:
            ca.MixBank16(plan, jobs)
        assert e.value.status == status

    other = job(x=y, y=x, a=v[n:2 * n], b=v[3 * n:])
    acc2 = last_word(torch, 78)
    ok = ca.MixBank16(plan, [job(acc=acc), dict(zip(
        ("fcw", "pm", "x", "y", "ox", "oy", "n", "phase0", "acc"), other[:8] + (acc2,)))])
    ok.close()
    bank_refused(ca.ERR_CONTAINER, [job()], plan=cfg2)
    bank_refused(ca.ERR_MODE, [job()], plan=r2p)
    bank_refused(A, [job(acc=acc), other[:8] + (acc,)])           # a shared d_acc
    bank_refused(A, [job(), job(x=y, y=x, a=i[n:], b=v[3 * n:])])  # output on an input
    bank_refused(A, [job(), job(a=v[n - 1:2 * n - 1], b=v[3 * n:])])  # on an output by one
    bank_refused(A, [job(x=byte(x))])
    bank_refused(A, [job(f=f.data_ptr() + 2)])
    plan.fm_mix16(None, None, None, None, None, None, n=0, acc=acc)   # a no-op
    torch.cuda.synchronize()
    assert last_value(acc) == 77 and outs.untouched()
    assert np.array_equal(ins.get(), np.arange(2 * n, dtype=np.int16))
    # 2-byte-aligned sample arrays one element behind each other are served
    plan.fm_mix16(f, i[1:], i[1:], v[1:], v[2 * n + 1:], work, pm=f, n=n,
                  acc=last_word(torch, 1))
    torch.cuda.synchronize()
    h = outs.t.cpu().numpy()
    assert h[0] == S16 and (h[n + 1:2 * n + 1] == S16).all() and (h[3 * n + 1:] == S16).all()
    assert not (h[1:n + 1] == S16).all()
    for q in (plan, cfg2, r2p, r2p32):
        q.close()
