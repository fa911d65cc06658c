"""The FM mixer (cordic_plan_fm_mix, cordic_plan_fm_mix_info,
cordic_plan_fm_mix_workspace; include/cordic_amd.h): the rotator with per-sample
tuning words accumulated inside the kernel.  Expected values need no tolerance:
numpy's wrapping cumulative sum (expected() of tests/test_table_fm.py) feeds the
oracle's rotate."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O
from test_fm_demod import S32, Padded, last_value, last_word
from test_table_fm import expected as phases, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_plan_fm_mix_workspace", "cordic_plan_fm_mix_info",
         "cordic_plan_fm_mix")
UG = ca.FLAG_UNIT_GAIN
CFG2 = (ca.P2R, 32, 32, 2, 32, 16)
# name: (cli args, flags).  cfg2, n20, cfg4, nat32, nat24, nat16:
# tools/bench_common.py; ww38, wrap32: tests/test_jobset_fused.py
CORES = {
    "cfg2": (CFG2, 0),                                  # WW 35, 16 live stages
    "n20": ((ca.P2R, 32, 32, 2, 32, 20), 0),
    "cfg4": ((ca.P2R, 32, 32, 2, 32, 24), 0),
    "nat32": ((ca.P2R, 32, 32, 2, 32, -1), 0),          # 29 stages
    "nat24": ((ca.P2R, 24, 24, 2, -1, -1), 0),          # WW 27, PW 31, 27 stages
    "nat16": ((ca.P2R, 16, 16, 2, -1, -1), 0),          # WW 19, PW 23, 19 stages
    "ww38": ((ca.P2R, 32, 32, 5, 32, 24), 0),
    "n9": ((ca.P2R, 16, 16, 2, -1, 9), 0),              # 9 live stages
    "wrap32": ((ca.P2R, 24, 2, 7, 32, -1), 0),
    "n17": ((ca.P2R, 32, 32, 2, 32, 17), 0),            # 17 is not an instance
    "sp2r": ((ca.SP2R, 32, 32, 2, 32, 16), 0),          # 14 live stages
    "cfg2_ug": (CFG2, UG),
    "cfg2_no_tails": (CFG2, ca.FLAG_NO_TAILS),
    "cfg2_no_lj": (CFG2, ca.FLAG_NO_LJ),
    "cfg2_generic": (CFG2, ca.FLAG_FORCE_GENERIC),
}
FUSED = ("cfg2", "n20", "cfg4", "nat32", "nat24", "nat16")
NOT_FUSED = ("ww38", "n9", "wrap32", "n17", "sp2r", "cfg2_ug", "cfg2_no_tails",
             "cfg2_no_lj", "cfg2_generic")
INSTANCES = (13, 16, 19, 20, 24, 27, 29)
SIZES = (0, 1, 255, 256, 257, 1 << 20, 1 << 33)


def both(name):
    args, flags = CORES[name]
    cfg = ca.Config.from_cli(*args)
    if flags:
        cfg = cfg.with_flags(flags)
    gain = ca.lib().cordic_config_gain_annihilator(cfg.ref) if flags & UG else None
    return cfg, O.config_cli(*args), gain


# ---------------------------------------------------------------- no GPU

def test_the_three_functions_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    assert re.search(r"size_t\s+cordic_plan_fm_mix_workspace\s*\(\s*const\s+cordic_plan"
                     r"\s*\*\s*plan\s*,\s*size_t\s+n\s*\)\s*;", text)
    assert re.search(r"int\s+cordic_plan_fm_mix_info\s*\(\s*const\s+cordic_plan\s*\*\s*"
                     r"plan\s*,\s*int32_t\s*\*\s*fused\s*,\s*int32_t\s*\*\s*tile\s*\)\s*;",
                     text)
    assert re.search(
        r"int\s+cordic_plan_fm_mix\s*\(\s*const\s+cordic_plan\s*\*\s*plan\s*,\s*size_t\s+n"
        r"\s*,\s*const\s+uint32_t\s*\*\s*d_fcw\s*,\s*const\s+uint32_t\s*\*\s*d_pm\s*,\s*"
        r"uint32_t\s+phase0\s*,\s*uint32_t\s*\*\s*d_acc\s*,\s*const\s+int32_t\s*\*\s*d_xval"
        r"\s*,\s*const\s+int32_t\s*\*\s*d_yval\s*,\s*int32_t\s*\*\s*d_oxval\s*,\s*int32_t"
        r"\s*\*\s*d_oyval\s*,\s*void\s*\*\s*d_work\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    # behind the FM demodulation block
    assert text.index("cordic_fm_demod16(") < text.index("cordic_plan_fm_mix_workspace(")
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
    from cordic_amd import _native
    for name in NAMES:
        assert name in _native.ABI
    assert "Plan" in ca.__all__
    for name in ("fm_mix", "fm_mix_info", "fm_mix_workspace"):
        assert callable(getattr(ca.Plan, name))
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_header_with_the_new_block_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { const cordic_plan *p = 0; int32_t f, t; int32_t *a = 0;\n'
        'uint32_t *w = 0; size_t b = cordic_plan_fm_mix_workspace(p, 8);\n'
        'return cordic_plan_fm_mix_info(p, &f, &t) + cordic_plan_fm_mix(p, 0, w, w, 0, w,'
        ' a, a, a, a, 0, 0) + (int)b; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def workspace_properties(plan, fused):
    last = 0
    for n in SIZES:
        w = plan.fm_mix_workspace(n)
        assert w % 16 == 0, n
        assert w >= last, n
        assert w <= (n // 256 + 65536 if fused else 4 * n + 65536 + 16), n
        assert (w == 0) == (n == 0), n
        last = w


def test_the_workspace_of_a_plan_that_is_not_fused_holds_the_phases():
    """(a WW 38 core has no seed table, so its plan needs no device; a fused
    plan's tables live on one: test_gpu_the_workspace_of_a_fused_plan_is_small)"""
    plan = ca.Plan(both("ww38")[0])
    assert plan.fm_mix_info() == (0, 0)
    workspace_properties(plan, False)
    assert plan.fm_mix_workspace(1 << 20) >= 4 << 20
    assert ca.lib().cordic_plan_fm_mix_workspace(None, 1 << 20) == 0
    plan.close()


def test_the_queries_and_the_call_refuse_a_null_plan_without_a_device():
    L = ca.lib()
    f, t = C.c_int32(-5), C.c_int32(-5)
    assert L.cordic_plan_fm_mix_info(None, C.byref(f), C.byref(t)) == ca.ERR_ARGS
    assert (f.value, t.value) == (-5, -5)
    for n in (0, 8):
        assert L.cordic_plan_fm_mix(None, n, None, None, 0, None, None, None, None,
                                    None, None, None) == ca.ERR_ARGS
    plan = ca.Plan(both("ww38")[0])
    assert L.cordic_plan_fm_mix_info(plan._h, None, None) == 0   # either may be NULL
    assert L.cordic_plan_fm_mix(plan._h, 0, None, None, 0, None, None, None, None,
                                None, None, None) == 0           # n = 0: a no-op
    plan.close()


def test_the_binding_asks_the_caller_for_the_scratch():
    import torch
    plan = ca.Plan(both("ww38")[0])
    with pytest.raises(TypeError):
        plan.fm_mix(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, n=8)
    with pytest.raises(TypeError):
        plan.fm_mix(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, None, n=8)
    short = torch.zeros(plan.fm_mix_workspace(8) - 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        plan.fm_mix(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, short, n=8)
    plan.close()


# ---------------------------------------------------------------- GPU

BIG = (1 << 23) + 4099
OFFS = dict(x=1, y=2, fcw=3, pm=1, ox=1, oy=3)   # every array at its own offset
PHASE0, PRESET = 0x9e3779b1, 0x7f4a7c15          # their sum wraps


def work_buffer(torch, plan, n):
    from gpu_util import DEV
    return torch.zeros(max(16, plan.fm_mix_workspace(n)), dtype=torch.uint8,
                       device=DEV)


def iq(rng, n, iw):
    """random over the full IW range, the most negative and the most positive
    value among them"""
    lo, hi = -(1 << (iw - 1)), (1 << (iw - 1)) - 1
    x = rng.integers(lo, hi + 1, n).astype(np.int32)
    y = rng.integers(lo, hi + 1, n).astype(np.int32)
    for k, v in enumerate((lo, hi, hi, lo)):
        if k < n:
            x[k] = v
            y[(k * 7 + 2) % n] = v
    return x, y


def sext(a, w):
    s = 32 - w
    return (a.astype(np.int32) << s) >> s


def want(name, x, y, p):
    """what cordic_p2r writes for (x, y, phase = p): inputs modulo IW and PW"""
    cfg, ocfg, gain = both(name)
    mask = np.uint32((1 << cfg.pw) - 1 & 0xffffffff)
    ox, oy = O.rotate(ocfg, sext(x, cfg.iw), sext(y, cfg.iw), p & mask)
    if gain is not None:        # o = (o * K) >> 32 (CORDIC_FLAG_UNIT_GAIN)
        ox = ((ox.astype(np.int64) * gain) >> 32).astype(np.int32)
        oy = ((oy.astype(np.int64) * gain) >> 32).astype(np.int32)
    return ox, oy


def run(torch, plan, work, fcw, pm, x, y, phase0=0, acc=None, offs=OFFS):
    """one call with every array at its element offset behind an aligned
    start; (ox, oy) after checking the guards and the inputs"""
    n = x.size
    i32 = lambda a: None if a is None else a.view(np.int32)
    df = Padded(torch, n, offs["fcw"], src=i32(fcw))
    dm = None if pm is None else Padded(torch, n, offs["pm"], src=i32(pm))
    dx = Padded(torch, n, offs["x"], src=x)
    dy = Padded(torch, n, offs["y"], src=y)
    ox, oy = Padded(torch, n, offs["ox"]), Padded(torch, n, offs["oy"])
    plan.fm_mix(df.view, dx.view, dy.view, ox.view, oy.view, work,
                pm=None if dm is None else dm.view, n=n, phase0=phase0, acc=acc)
    torch.cuda.synchronize()
    assert np.array_equal(df.get(), i32(fcw))
    assert dm is None or np.array_equal(dm.get(), i32(pm))
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    return ox.get(), oy.get()


def check(torch, name, plan, work, fcw, pm, x, y, tag=None):
    """with a preset d_acc word and without one, against the oracle"""
    n = x.size
    p, final = phases(fcw, pm, PHASE0, PRESET)
    wx, wy = want(name, x, y, p)
    acc = last_word(torch, PRESET)
    gx, gy = run(torch, plan, work, fcw, pm, x, y, PHASE0, acc)
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (name, n, tag, "acc")
    assert last_value(acc) == final, (name, n, tag)
    p, _ = phases(fcw, pm, PHASE0)
    wx, wy = want(name, x, y, p)
    gx, gy = run(torch, plan, work, fcw, pm, x, y, PHASE0)
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (name, n, tag)


def mode_of(name):
    return CORES[name][0][0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED + NOT_FUSED)
def test_gpu_the_path_query_names_the_fused_cores(name):
    plan = ca.Plan(both(name)[0])
    fused, tile = plan.fm_mix_info()
    assert fused == (1 if name in FUSED else 0)
    if fused:
        assert tile > 0 and tile % 4 == 0
    else:
        assert tile == 0
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(ca.P2R, 32, 32, 2, 32, 13), (ca.P2R, 24, 24, 2, 28, 20),
                                  (ca.P2R, 32, 32, 2, 32, 27), (ca.P2R, 12, 12, 2, -1, -1),
                                  (ca.P2R, 32, 32, 3, 32, 22), (ca.SP2R, 24, 24, 2, -1, -1)])
def test_gpu_the_path_query_agrees_with_the_plans_tables_on_any_other_core(args):
    """no claim about these cores but the rule itself: fused needs direction
    tables, WW <= 35, no wrap and a live-stage count with an instance"""
    cfg = ca.Config.from_cli(*args)
    plan = ca.Plan(cfg)
    fused, tile = plan.fm_mix_info()
    assert fused in (0, 1) and (tile > 0) == (fused == 1)
    if fused:
        assert len(plan.dir_groups) > 0 and cfg.ww <= 35 and not cfg.needs_wrap
        assert cfg.nlive in INSTANCES
    if not plan.dir_groups or cfg.ww > 35 or cfg.needs_wrap \
            or cfg.nlive not in INSTANCES:
        assert fused == 0
    plan.close()


@pytest.mark.gpu
def test_gpu_the_workspace_of_a_fused_plan_is_small():
    for name in ("cfg2", "nat16"):
        plan = ca.Plan(both(name)[0])
        assert plan.fm_mix_info()[0] == 1
        workspace_properties(plan, True)
        plan.close()
    plan = ca.Plan(both("wrap32")[0])
    workspace_properties(plan, False)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "n20", "nat32", "nat24", "nat16"])
def test_gpu_fused_cores_equal_the_oracle(name):
    import torch
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    fused, T = plan.fm_mix_info()
    assert fused == 1
    rng = np.random.default_rng(31)
    for n in (1, 3, 4, 5, T - 1, T, T + 1, 2 * T + 3, (1 << 16) + 3):
        work = work_buffer(torch, plan, n)
        x, y = iq(rng, n, cfg.iw)
        for kind in ("zero", "ones", "random", "fsk"):
            fcw = words(kind, n, 40 + n % 7)
            for pm in (None, words("random", n, 50 + n % 5)):
                check(torch, name, plan, work, fcw, pm, x, y, tag=kind)
    plan.close()


@pytest.mark.gpu
def test_gpu_bits_above_the_input_width_are_ignored():
    """nat16 (IW 16) with garbage above bit 15 of x and y"""
    import torch
    name = "nat16"
    cfg = both(name)[0]
    assert cfg.iw == 16
    plan = ca.Plan(cfg)
    rng = np.random.default_rng(32)
    n = plan.fm_mix_info()[1] + 7
    x, y = iq(rng, n, 16)
    gx = (x & 0xffff) | (rng.integers(0, 1 << 16, n).astype(np.int32) << 16)
    gy = (y & 0xffff) | (rng.integers(0, 1 << 16, n).astype(np.int32) << 16)
    assert not np.array_equal(gx, x)
    check(torch, name, plan, work_buffer(torch, plan, n), words("random", n, 3),
          words("random", n, 4), gx.astype(np.int32), gy.astype(np.int32))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "nat24"])
def test_gpu_many_passes_per_block_give_the_same_bits(name, monkeypatch):
    """2^16 + 3 samples are 65 passes: on 1 and on 3 blocks (65, and 22 or 21
    passes per block: CORDIC_FMX_MAX_BLOCKS, cordic_fm_mix.hip) and on the grid
    the library chooses"""
    import torch
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    n = (1 << 16) + 3
    assert -(-n // plan.fm_mix_info()[1]) == 65
    work = work_buffer(torch, plan, n)
    rng = np.random.default_rng(33)
    x, y = iq(rng, n, cfg.iw)
    fcw, pm = words("random", n, 5), words("random", n, 6)
    p, final = phases(fcw, pm, PHASE0, PRESET)
    wx, wy = want(name, x, y, p)
    for cap in (1, 3, None):
        if cap is None:
            monkeypatch.delenv("CORDIC_FMX_MAX_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("CORDIC_FMX_MAX_BLOCKS", str(cap))
        acc = last_word(torch, PRESET)
        gx, gy = run(torch, plan, work, fcw, pm, x, y, PHASE0, acc)
        assert np.array_equal(gx, wx) and np.array_equal(gy, wy), cap
        assert last_value(acc) == final, cap
    plan.close()


@pytest.mark.gpu
def test_gpu_one_long_call_equals_the_oracle_on_every_sample():
    import torch
    name = "cfg2"
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    work = work_buffer(torch, plan, BIG)
    x, y = iq(np.random.default_rng(34), BIG, cfg.iw)
    fcw, pm = words("random", BIG, 7), words("random", BIG, 8)
    p, final = phases(fcw, pm, PHASE0, PRESET)
    wx, wy = want(name, x, y, p)
    acc = last_word(torch, PRESET)
    gx, gy = run(torch, plan, work, fcw, pm, x, y, PHASE0, acc)
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy)
    assert last_value(acc) == final
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ww38", "n9", "wrap32", "sp2r", "cfg2_ug"])
def test_gpu_fallback_cores_equal_the_oracle(name):
    import torch
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    assert plan.fm_mix_info() == (0, 0)
    rng = np.random.default_rng(35)
    for n in (1, 5, 4097, (1 << 16) + 3):
        work = work_buffer(torch, plan, n)
        x, y = iq(rng, n, cfg.iw)
        for kind, pm in (("random", words("random", n, 9)), ("ones", None)):
            check(torch, name, plan, work, words(kind, n, 10), pm, x, y, tag=kind)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "ww38"])
def test_gpu_the_call_equals_the_accumulator_and_the_rotator_and_the_mixer(name):
    """device against device: cordic_phase_accumulate + cordic_plan_p2r, and
    with constant words cordic_plan_mix(phase0, f, 0)"""
    import torch
    from gpu_util import DEV, dev_i32, to_np
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    n = 2 * 1024 + 7
    rng = np.random.default_rng(36)
    x, y = iq(rng, n, cfg.iw)
    dx, dy = dev_i32(x), dev_i32(y)
    work = work_buffer(torch, plan, n)
    new = lambda: torch.zeros(n, dtype=torch.int32, device=DEV)
    f = 0x0123457
    for fcw, pm in ((words("random", n, 11), words("random", n, 12)),
                    (np.full(n, f, dtype=np.uint32), None)):
        dfcw = dev_i32(fcw)
        dpm = None if pm is None else dev_i32(pm)
        ox, oy, ph, rx, ry = new(), new(), new(), new(), new()
        plan.fm_mix(dfcw, dx, dy, ox, oy, work, pm=dpm, phase0=PHASE0)
        ca.phase_accumulate(dfcw, ph, pm=dpm, phase0=PHASE0,
                            work=torch.zeros(ca.fm_workspace(n), dtype=torch.uint8,
                                             device=DEV))
        plan.p2r(dx, dy, ph, rx, ry)
        torch.cuda.synchronize()
        assert np.array_equal(to_np(ox), to_np(rx))
        assert np.array_equal(to_np(oy), to_np(ry))
        if pm is None:
            mx, my = new(), new()
            plan.mix(PHASE0, f, 0, dx, dy, mx, my)
            torch.cuda.synchronize()
            assert np.array_equal(to_np(ox), to_np(mx))
            assert np.array_equal(to_np(oy), to_np(my))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "ww38"])
def test_gpu_consecutive_calls_that_share_the_accumulator_equal_one_call(name):
    import torch
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    T = plan.fm_mix_info()[1] or 1024
    n = 2 * T + 7
    cuts = [0, 1, T - 1, T + 2, n]
    work = work_buffer(torch, plan, n)
    rng = np.random.default_rng(37)
    x, y = iq(rng, n, cfg.iw)
    fcw, pm = words("random", n, 13), words("random", n, 14)
    p, final = phases(fcw, pm, PHASE0, PRESET)
    wx, wy = want(name, x, y, p)
    acc = last_word(torch, PRESET)
    gx, gy = run(torch, plan, work, fcw, pm, x, y, PHASE0, acc)
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy)
    assert last_value(acc) == final
    acc = last_word(torch, PRESET)
    parts = [run(torch, plan, work, fcw[a:b], pm[a:b], x[a:b], y[a:b],
                 PHASE0 if a == 0 else 0, acc) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate([q[0] for q in parts]), wx)
    assert np.array_equal(np.concatenate([q[1] for q in parts]), wy)
    assert last_value(acc) == final
    plan.close()


def _hip():
    for name in ("libamdhip64.so", "libamdhip64.so.6", "libamdhip64.so.7"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    return C.CDLL("/opt/rocm/lib/libamdhip64.so")


@pytest.mark.gpu
def test_gpu_the_fused_call_in_a_graph_is_one_chain_and_continues_on_replay():
    """captured once with a d_acc word and replayed three times on the same
    arrays: *d_acc = start + 3 * sum(fcw), the last replay's outputs are the
    oracle's for the phase it started from, and the graph is two kernel nodes
    with one edge between them"""
    import torch
    from gpu_util import DEV, dev_i32, to_np
    name = "cfg2"
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    assert plan.fm_mix_info()[0] == 1
    n = 3 * 1024 + 5
    rng = np.random.default_rng(38)
    x, y = iq(rng, n, cfg.iw)
    fcw, pm = words("random", n, 15), words("random", n, 16)
    dfcw, dpm, dx, dy = dev_i32(fcw), dev_i32(pm), dev_i32(x), dev_i32(y)
    ox = torch.zeros(n, dtype=torch.int32, device=DEV)
    oy = torch.zeros(n, dtype=torch.int32, device=DEV)
    work = work_buffer(torch, plan, n)
    acc = last_word(torch, PRESET)
    total = int(np.sum(fcw, dtype=np.uint64)) & 0xffffffff

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
        plan.fm_mix(dfcw, dx, dy, ox, oy, work, pm=dpm, phase0=0, acc=acc,
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
    assert last_value(acc) == (PRESET + 3 * total) & 0xffffffff
    p, final = phases(fcw, pm, 0, (PRESET + 2 * total) & 0xffffffff)
    assert final == last_value(acc)
    wx, wy = want(name, x, y, p)
    assert np.array_equal(to_np(ox), wx) and np.array_equal(to_np(oy), wy)
    plan.close()


@pytest.mark.gpu
def test_gpu_bad_arguments_are_refused_and_nothing_is_written():
    import torch
    n = 64
    plan = ca.Plan(both("cfg2")[0])
    assert plan.fm_mix_info()[0] == 1
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    wbytes = plan.fm_mix_workspace(n)
    work = big[:wbytes]
    ins = Padded(torch, 4 * n, 0, src=np.arange(4 * n, dtype=np.int32))
    outs = Padded(torch, 4 * n, 0)                # outputs cut from one array
    acc = last_word(torch, 77)
    i, v = ins.t, outs.t
    f, m, x, y = i[:n], i[n:], i[2 * n:], i[3 * n:]
    a, b = v[:n], v[2 * n:]

    def refused(status, f, m, x, y, a, b, w, plan=plan, acc=acc):
        with pytest.raises(ca.CordicError) as e:
            plan.fm_mix(f, x, y, a, b, w, pm=m, n=n, acc=acc)
        assert e.value.status == status

    A = ca.ERR_ARGS
    refused(A, None, m, x, y, a, b, work)                 # every NULL
    refused(A, f, m, None, y, a, b, work)
    refused(A, f, m, x, None, a, b, work)
    refused(A, f, m, x, y, None, b, work)
    refused(A, f, m, x, y, a, None, work)
    refused(A, f, m, x, y, a, b, 0)
    odd = lambda t: t.data_ptr() + 2                      # every misalignment
    refused(A, odd(f), m, x, y, a, b, work)
    refused(A, f, odd(m), x, y, a, b, work)
    refused(A, f, m, odd(x), y, a, b, work)
    refused(A, f, m, x, odd(y), a, b, work)
    refused(A, f, m, x, y, odd(a), b, work)
    refused(A, f, m, x, y, a, odd(b), work)
    refused(A, f, m, x, y, a, b, big[8:])
    refused(A, f, m, x, y, a, b, work, acc=acc.data_ptr() + 2)
    refused(A, f, m, x, y, x, b, work)                    # d_oxval is d_xval
    refused(A, f, m, x, y, x[1:], b, work)                # d_oxval on d_xval
    refused(A, f, m, x, y, a, i[n - 1:], work)            # d_oyval on d_fcw and d_pm
    refused(A, f, m, x, y, a, v[n - 1:], work)            # d_oyval on d_oxval by one
    refused(A, f, m, x, y, a, b, work, acc=x[3:])         # d_acc inside an input
    refused(A, f, m, x, y, a, b, work, acc=m[n - 1:])
    refused(A, f, m, x, y, a, b, work, acc=v[n - 1:])     # d_acc in d_oxval
    refused(A, f, m, x, y, a, b, work, acc=work.data_ptr() + wbytes - 4)
    refused(A, f, m, x, y, a, b, y[n - 4:].data_ptr())    # d_work on an input
    refused(A, f, m, x, y, a, b, v[n - 4:].data_ptr())    # d_work on d_oxval
    r2p = ca.Plan(ca.Config.from_cli(ca.R2P, 24, 24, 2, -1, 20))
    refused(ca.ERR_MODE, f, m, x, y, a, b, work, plan=r2p)        # the wrong mode
    fq, tq = C.c_int32(-5), C.c_int32(-5)
    assert ca.lib().cordic_plan_fm_mix_info(r2p._h, C.byref(fq), C.byref(tq)) \
        == ca.ERR_MODE and (fq.value, tq.value) == (-5, -5)
    assert r2p.fm_mix_workspace(n) == 0
    assert ca.lib().cordic_plan_fm_mix(None, n, f.data_ptr(), None, 0, acc.data_ptr(),
                                       x.data_ptr(), y.data_ptr(), a.data_ptr(),
                                       b.data_ptr(), work.data_ptr(), None) == A
    plan.fm_mix(None, None, None, None, None, None, n=0, acc=acc)  # a no-op
    torch.cuda.synchronize()
    assert last_value(acc) == 77 and outs.untouched()
    # the same refusals on a plan of the fallback
    slow = ca.Plan(both("ww38")[0])
    w2 = big[:slow.fm_mix_workspace(n)]
    refused(A, f, m, x, y, x[1:], b, w2, plan=slow)
    refused(A, f, m, x, y, a, v[n - 1:], w2, plan=slow)
    refused(A, f, m, x, y, a, b, w2, plan=slow, acc=x[3:])
    refused(A, f, m, x, y, a, b, w2, plan=slow,
            acc=w2.data_ptr() + slow.fm_mix_workspace(n) - 4)     # among the phases
    torch.cuda.synchronize()
    assert last_value(acc) == 77 and outs.untouched()
    plan.fm_mix(f, x, x, a, b, work, pm=f, n=n, acc=last_word(torch, 1))  # inputs may alias
    torch.cuda.synchronize()
    assert np.array_equal(ins.get(), np.arange(4 * n, dtype=np.int32))
    h = outs.t.cpu().numpy()
    assert (h[n:2 * n] == S32).all() and (h[3 * n:] == S32).all()
    assert not (h[:n] == S32).all()
    for q in (plan, r2p, slow):
        q.close()
