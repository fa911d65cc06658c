"""The decimating FM mixer (cordic_plan_fm_mix_decim, _decim16 and their
_workspace; include/cordic_amd.h): cordic_plan_fm_mix with an integrate-and-dump
by R = 2^k behind the rotator.  Expected values need no tolerance: the oracle's
tuned samples for numpy's wrapping running sum (want() of tests/test_fm_mix.py),
summed as int64 over reshape(-1, R) and shifted right by k."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
from test_fm_demod import S16, S32, Padded, last_value, last_word
from test_fm_mix import PHASE0, PRESET, _hip
from test_table_fm import expected as phases, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_plan_fm_mix_decim_workspace", "cordic_plan_fm_mix_decim",
         "cordic_plan_fm_mix_decim16_workspace", "cordic_plan_fm_mix_decim16",
         "cordic_mixbank_create_decim", "cordic_mixbank_create_decim16")
KS = (1, 2, 3, 4, 5, 6, 7, 8)
# one core per unit of the instance chooser: (name, int16 arrays)
UNITS = (("cfg2", False), ("nat24", False), ("nat16", True))
# ports of 16 bits at WW 35 (18 appended bits): LJ 29, for which the int16
# kernels are not instantiated -- cordic_plan_fm_mix16's fallback
WW35_16 = (ca.P2R, 16, 16, 18, 16, 16)


def decimate(a, k):
    """floor(the sum of 2^k consecutive values / 2^k), exactly"""
    s = a.astype(np.int64).reshape(-1, 1 << k).sum(axis=1)
    return (s >> k).astype(a.dtype)


def core(name, i16):
    if name == "ww35_16":
        return ca.Config.from_cli(*WW35_16)
    return (MIX16.both if i16 else MIX.both)(name)[0]


def tuned(name, i16, x, y, p):
    """what cordic_plan_fm_mix (_mix16) writes for the phases p"""
    if name == "ww35_16":       # inputs modulo IW and PW, as want16() takes them
        cfg = core(name, i16)
        mask = np.uint32((1 << cfg.pw) - 1)
        ox, oy = O.rotate(O.config_cli(*WW35_16), MIX.sext(x.astype(np.int32), cfg.iw),
                          MIX.sext(y.astype(np.int32), cfg.iw), p & mask)
        assert np.array_equal(ox.astype(np.int16), ox) and np.array_equal(oy.astype(np.int16), oy)
        return ox.astype(np.int16), oy.astype(np.int16)
    return (MIX16.want16 if i16 else MIX.want)(name, x, y, p)


# ---------------------------------------------------------------- no GPU

def test_the_new_functions_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    for t, tag in (("int32_t", ""), ("int16_t", "16")):
        assert re.search(
            r"size_t\s+cordic_plan_fm_mix_decim%s_workspace\s*\(\s*const\s+cordic_plan\s*\*"
            r"\s*plan\s*,\s*size_t\s+n\s*,\s*uint32_t\s+log2r\s*\)\s*;" % tag, text)
        assert re.search(
            r"int\s+cordic_plan_fm_mix_decim%s\s*\(\s*const\s+cordic_plan\s*\*\s*plan\s*,"
            r"\s*size_t\s+n\s*,\s*uint32_t\s+log2r\s*,\s*const\s+uint32_t\s*\*\s*d_fcw\s*,"
            r"\s*const\s+uint32_t\s*\*\s*d_pm\s*,\s*uint32_t\s+phase0\s*,\s*uint32_t\s*\*"
            r"\s*d_acc\s*,\s*const\s+%s\s*\*\s*d_xval\s*,\s*const\s+%s\s*\*\s*d_yval\s*,"
            r"\s*%s\s*\*\s*d_oxval\s*,\s*%s\s*\*\s*d_oyval\s*,\s*void\s*\*\s*d_work\s*,"
            r"\s*void\s*\*\s*stream\s*\)\s*;" % (tag, t, t, t, t), text)
        assert re.search(
            r"int\s+cordic_mixbank_create_decim%s\s*\(\s*const\s+cordic_plan\s*\*\s*plan\s*,"
            r"\s*uint32_t\s+log2r\s*,\s*size_t\s+njobs\s*,\s*const\s+cordic_fmmix_job%s\s*\*"
            r"\s*jobs\s*,\s*cordic_mixbank\s*\*\*\s*bank\s*\)\s*;" % (tag, tag), text)
    # next to the FM mixer block, in front of the banks
    assert text.index("cordic_plan_fm_mix16(") < text.index("cordic_plan_fm_mix_decim(") \
        < text.index("cordic_mixbank_create(")
    assert text.index("cordic_mixbank_create16(") < text.index("cordic_mixbank_create_decim(")
    from cordic_amd import _native
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
        assert name in _native.ABI
    for name in ("fm_mix_decim", "fm_mix_decim16", "fm_mix_decim_workspace",
                 "fm_mix_decim16_workspace"):
        assert callable(getattr(ca.Plan, name))
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_header_is_still_plain_c99_and_the_jobs_keep_their_72_bytes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { const cordic_plan *p = 0; int32_t *a = 0; int16_t *s = 0;\n'
        'uint32_t *w = 0; cordic_mixbank *b = 0; cordic_fmmix_job *j = 0;\n'
        'cordic_fmmix_job16 *h = 0;\n'
        'char a72[sizeof(cordic_fmmix_job) == 72 ? 1 : -1];\n'
        'char b72[sizeof(cordic_fmmix_job16) == 72 ? 1 : -1];\n'
        'size_t t = cordic_plan_fm_mix_decim_workspace(p, 8, 3)\n'
        ' + cordic_plan_fm_mix_decim16_workspace(p, 8, 3); (void)a72; (void)b72;\n'
        'return cordic_plan_fm_mix_decim(p, 0, 3, w, w, 0, w, a, a, a, a, 0, 0)\n'
        ' + cordic_plan_fm_mix_decim16(p, 0, 3, w, w, 0, w, s, s, s, s, 0, 0)\n'
        ' + cordic_mixbank_create_decim(p, 3, 0, j, &b)\n'
        ' + cordic_mixbank_create_decim16(p, 3, 0, h, &b) + (int)t; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def workspace_properties(plan, fused, i16):
    """0 / a multiple of 16 / non-decreasing over the multiples of R / the
    bounds of the header"""
    ws = plan.fm_mix_decim16_workspace if i16 else plan.fm_mix_decim_workspace
    mix = plan.fm_mix16_workspace if i16 else plan.fm_mix_workspace
    for k in (0, 1, 2, 5, 8):
        R = 1 << k
        last = 0
        for n in sorted({0, R, 3 * R, 256, 1024, 1024 + R, 1 << 20, 1 << 33}):
            w = ws(n, k)
            assert w % 16 == 0 and w >= last, (k, n)
            assert (w == 0) == (n == 0), (k, n)
            if fused or k == 0:
                assert w == mix(n), (k, n)
            else:
                es = 2 if i16 else 4
                each = (n * es + 15) // 16 * 16
                assert w == mix(n) + 2 * each, (k, n)
                assert w <= (24 * n + 65536 + 128 if i16 else 12 * n + 65536 + 48), (k, n)
            last = w
        if k:
            assert ws(R + 1, k) == 0 and ws(R // 2, k) == 0      # not whole groups
    assert ws(1024, 9) == 0 and ws(0, 9) == 0


def test_the_workspace_of_plans_that_are_not_fused_holds_two_more_arrays():
    """(WW 38 and 9 live stages: no seed table, so the plans need no device)"""
    plan = ca.Plan(MIX.both("ww38")[0])
    workspace_properties(plan, False, False)
    assert plan.fm_mix_decim16_workspace(1024, 3) == 0           # IW 32: the container
    plan.close()
    plan = ca.Plan(MIX16.both("n9")[0])
    workspace_properties(plan, False, True)
    workspace_properties(plan, False, False)
    plan.close()
    L = ca.lib()
    assert L.cordic_plan_fm_mix_decim_workspace(None, 1024, 3) == 0
    assert L.cordic_plan_fm_mix_decim16_workspace(None, 1024, 3) == 0


def test_a_null_plan_k_9_and_a_partial_group_are_refused_without_a_device():
    L = ca.lib()
    nul = (None,) * 4
    for fn in (L.cordic_plan_fm_mix_decim, L.cordic_plan_fm_mix_decim16):
        for n in (0, 8):
            assert fn(None, n, 1, None, None, 0, None, *nul, None, None) == ca.ERR_ARGS
    plan = ca.Plan(MIX16.both("n9")[0])
    for fn in (L.cordic_plan_fm_mix_decim, L.cordic_plan_fm_mix_decim16):
        a = 0x10000
        args = (a, None, 0, None, 2 * a, 3 * a, 4 * a, 5 * a, 6 * a, None)
        assert fn(plan._h, 1024, 9, *args) == ca.ERR_ARGS        # k > 8
        assert fn(plan._h, 0, 9, *args) == ca.ERR_ARGS
        assert fn(plan._h, 1020, 3, *args) == ca.ERR_ARGS        # n % R
        assert fn(plan._h, 255, 8, *args) == ca.ERR_ARGS
        assert fn(plan._h, 0, 8, None, None, 0, None, *nul, None, None) == 0   # a no-op
    wide = ca.Plan(MIX.both("ww38")[0])                          # the container first
    assert L.cordic_plan_fm_mix_decim16(wide._h, 1020, 9, None, None, 0, None, *nul,
                                        None, None) == ca.ERR_CONTAINER
    h = C.c_void_p(0x5a5a)
    for fn in (L.cordic_mixbank_create_decim, L.cordic_mixbank_create_decim16):
        assert fn(None, 3, 0, None, C.byref(h)) == ca.ERR_ARGS
        assert fn(plan._h, 9, 0, None, C.byref(h)) == ca.ERR_ARGS
        assert h.value == 0x5a5a
    job = ca._native._CFmMixJob()
    job.d_fcw, job.d_xval, job.d_yval = 0x10000, 0x20000, 0x30000
    job.d_oxval, job.d_oyval, job.n = 0x40000, 0x50000, 1020
    assert L.cordic_mixbank_create_decim(plan._h, 3, 1, C.byref(job), C.byref(h)) \
        == ca.ERR_ARGS and h.value == 0x5a5a
    plan.close()
    wide.close()


def test_the_binding_asks_the_caller_for_the_scratch():
    import torch
    plan = ca.Plan(MIX.both("ww38")[0])
    with pytest.raises(TypeError):
        plan.fm_mix_decim(3, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, n=8)
    short = torch.zeros(plan.fm_mix_decim_workspace(8, 3) - 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        plan.fm_mix_decim(3, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, short, n=8)
    plan.close()


# ---------------------------------------------------------------- GPU

NMAX = 5 * 1024 + 256


@pytest.mark.gpu
@pytest.mark.parametrize("name,i16,fused", [("cfg2", False, True), ("nat24", False, True),
                                            ("nat16", True, True), ("nat16", False, True),
                                            ("ww35_16", True, False)])
def test_gpu_the_workspace_of_a_fused_plan_is_the_mixers(name, i16, fused):
    """(a fused plan's tables live on a device.)  For a fused plan and every k
    the mixer's own workspace; ww35_16 is fused on int32 arrays only"""
    plan = ca.Plan(core(name, i16))
    fused32 = plan.fm_mix_info()[0] == 1
    assert fused == (fused32 and (not i16 or plan.cfg.ww < 35))
    workspace_properties(plan, fused, i16)
    if fused:
        ws = plan.fm_mix_decim16_workspace if i16 else plan.fm_mix_decim_workspace
        for k in (1, 4, 8):
            assert ws(1 << 20, k) == plan.fm_mix_workspace(1 << 20) <= (1 << 20) // 256 + 65536
    else:
        assert plan.cfg.ww == 35
        workspace_properties(plan, fused32, False)  # the same plan on int32 arrays
    plan.close()


def lengths(k):
    R = 1 << k
    return (R, 2 * R, 1024 - R, 1024, 1024 + R, 2048 + R, 5 * 1024 + R)


def work_buffer(torch, plan, n, k, i16=False):
    from gpu_util import DEV
    ws = plan.fm_mix_decim16_workspace if i16 else plan.fm_mix_decim_workspace
    return torch.zeros(max(16, ws(n, k)), dtype=torch.uint8, device=DEV)


def run(torch, plan, k, work, fcw, pm, x, y, phase0=0, acc=None, i16=False):
    """one call with the sample arrays 4 bytes (2 for int16) and the words 4
    bytes behind a 16-byte boundary; (ox, oy), n >> k each, after checking the
    guards around them and the inputs"""
    n = x.size
    off = 9 if i16 else 5
    i32 = lambda a: None if a is None else a.view(np.int32)
    df = Padded(torch, n, 5, src=i32(fcw))
    dm = None if pm is None else Padded(torch, n, 5, src=i32(pm))
    dx = Padded(torch, n, off, i16=i16, src=x)
    dy = Padded(torch, n, off, i16=i16, src=y)
    ox, oy = Padded(torch, n >> k, off, i16=i16), Padded(torch, n >> k, off, i16=i16)
    call = plan.fm_mix_decim16 if i16 else plan.fm_mix_decim
    call(k, df.view, dx.view, dy.view, ox.view, oy.view, work,
         pm=None if dm is None else dm.view, n=n, phase0=phase0, acc=acc)
    torch.cuda.synchronize()
    assert np.array_equal(df.get(), i32(fcw))
    assert dm is None or np.array_equal(dm.get(), i32(pm))
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    return ox.get(), oy.get()


@functools.lru_cache(maxsize=None)
def reference(name, i16, n=NMAX, seed=41):
    """inputs of n samples and the oracle's tuned samples for them, with pm and
    a preset d_acc and with neither; a call of m <= n samples has the first m"""
    cfg = core(name, i16)
    rng = np.random.default_rng(seed)
    x, y = MIX16.iq16(rng, n, cfg.iw) if i16 else MIX.iq(rng, n, cfg.iw)
    fcw, pm = words("random", n, seed + 1), words("random", n, seed + 2)
    p, _ = phases(fcw, pm, PHASE0, PRESET)
    full = tuned(name, i16, x, y, p)
    p, _ = phases(fcw, None, PHASE0)
    bare = tuned(name, i16, x, y, p)
    for a in (x, y, fcw, pm) + full + bare:
        a.setflags(write=False)
    return x, y, fcw, pm, full, bare


def acc_after(fcw, n, start):
    return (start + int(np.sum(fcw[:n], dtype=np.uint64))) & 0xffffffff


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,i16", UNITS)
def test_gpu_every_k_equals_the_oracle_on_one_core_per_unit(name, i16, k):
    import torch
    plan = ca.Plan(core(name, i16))
    assert plan.fm_mix_info()[0] == 1 and (not i16 or plan.cfg.ww < 35)
    x, y, fcw, pm, full, bare = reference(name, i16)
    work = work_buffer(torch, plan, NMAX, k, i16)
    for n in lengths(k):
        acc = last_word(torch, PRESET)
        gx, gy = run(torch, plan, k, work, fcw[:n], pm[:n], x[:n], y[:n], PHASE0, acc, i16)
        assert np.array_equal(gx, decimate(full[0][:n], k)), (n, "pm, acc")
        assert np.array_equal(gy, decimate(full[1][:n], k)), (n, "pm, acc")
        assert last_value(acc) == acc_after(fcw, n, PHASE0 + PRESET), n
        gx, gy = run(torch, plan, k, work, fcw[:n], None, x[:n], y[:n], PHASE0, None, i16)
        assert np.array_equal(gx, decimate(bare[0][:n], k)), n
        assert np.array_equal(gy, decimate(bare[1][:n], k)), n
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ww", [34, 35])
@pytest.mark.parametrize("nlive", MIX.INSTANCES)
def test_gpu_every_rotator_instance_at_k_3_and_k_0_is_the_mixer(nlive, ww):
    """the seven stage counts x LJ 30 (WW 34: two extra bits) / LJ 29 (WW 35)"""
    import torch
    from gpu_util import DEV, dev_i32, to_np
    args = (ca.P2R, 32, 32, ww - 33, 32, nlive)
    cfg = ca.Config.from_cli(*args)
    assert cfg.ww == ww and cfg.nlive == nlive
    plan = ca.Plan(cfg)
    assert plan.fm_mix_info()[0] == 1
    n, k = 2048 + 8, 3
    rng = np.random.default_rng(42 + nlive)
    x, y = MIX.iq(rng, n, cfg.iw)
    fcw, pm = words("random", n, 17), words("random", n, 18)
    p, final = phases(fcw, pm, PHASE0, PRESET)
    wx, wy = O.rotate(O.config_cli(*args), x, y, p)
    acc = last_word(torch, PRESET)
    gx, gy = run(torch, plan, k, work_buffer(torch, plan, n, k), fcw, pm, x, y, PHASE0, acc)
    assert np.array_equal(gx, decimate(wx, k)) and np.array_equal(gy, decimate(wy, k))
    assert last_value(acc) == final
    # k = 0: cordic_plan_fm_mix bit for bit, on every sample
    dfcw, dpm, dx, dy = dev_i32(fcw), dev_i32(pm), dev_i32(x), dev_i32(y)
    new = lambda: torch.zeros(n, dtype=torch.int32, device=DEV)
    ox, oy, mx, my = new(), new(), new(), new()
    work = work_buffer(torch, plan, n, 0)
    assert plan.fm_mix_decim_workspace(n, 0) == plan.fm_mix_workspace(n)
    plan.fm_mix_decim(0, dfcw, dx, dy, ox, oy, work, pm=dpm, phase0=PHASE0)
    plan.fm_mix(dfcw, dx, dy, mx, my, work, pm=dpm, phase0=PHASE0)
    torch.cuda.synchronize()
    assert np.array_equal(to_np(ox), to_np(mx)) and np.array_equal(to_np(oy), to_np(my))
    wx, wy = O.rotate(O.config_cli(*args), x, y, phases(fcw, pm, PHASE0)[0])
    assert np.array_equal(to_np(ox), wx) and np.array_equal(to_np(oy), wy)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 8])
def test_gpu_a_sum_that_overflows_32_bits_is_exact(k):
    """cfg2, all-zero tuning words, constant full-scale positive x"""
    import torch
    name = "cfg2"
    plan = ca.Plan(MIX.both(name)[0])
    n = 1024 + 256
    x = np.full(n, 0x7fffffff, dtype=np.int32)
    y = np.zeros(n, dtype=np.int32)
    fcw = np.zeros(n, dtype=np.uint32)
    p, _ = phases(fcw, None, 0)
    wx, wy = MIX.want(name, x, y, p)
    sums = wx.astype(np.int64).reshape(-1, 1 << k).sum(axis=1)
    assert (np.abs(sums) >= 1 << 31).any()       # a 32-bit accumulator would wrap
    gx, gy = run(torch, plan, k, work_buffer(torch, plan, n, k), fcw, None, x, y)
    assert np.array_equal(gx, decimate(wx, k)) and np.array_equal(gy, decimate(wy, k))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,i16", UNITS)
def test_gpu_the_quotient_is_floored_not_truncated(name, i16):
    """reference()'s seed 41: at every k some group has a negative sum that is
    not a multiple of R (asserted on the oracle's values; checked on the CPU
    when the seed was picked), where truncation toward zero is one too high"""
    import torch
    plan = ca.Plan(core(name, i16))
    x, y, fcw, pm, full, bare = reference(name, i16)
    n = 2048
    for k in (1, 2, 3, 6):
        s = bare[0][:n].astype(np.int64).reshape(-1, 1 << k).sum(axis=1)
        assert ((s < 0) & (s % (1 << k) != 0)).any(), k
        gx, gy = run(torch, plan, k, work_buffer(torch, plan, n, k, i16), fcw[:n], None,
                     x[:n], y[:n], PHASE0, None, i16)
        assert np.array_equal(gx, decimate(bare[0][:n], k)), k
        assert np.array_equal(gy, decimate(bare[1][:n], k)), k
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,i16", UNITS[:1] + UNITS[2:])
def test_gpu_many_passes_per_block_give_the_same_bits(name, i16, monkeypatch):
    """65 passes on 1 block, on 3 and on the grid the library chooses"""
    import torch
    plan = ca.Plan(core(name, i16))
    n = 65 * 1024
    x, y, fcw, pm, full, bare = reference(name, i16, n, 43)
    for cap in (1, 3, None):
        if cap is None:
            monkeypatch.delenv("CORDIC_FMX_MAX_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("CORDIC_FMX_MAX_BLOCKS", str(cap))
        for k in (1, 4, 8):
            acc = last_word(torch, PRESET)
            gx, gy = run(torch, plan, k, work_buffer(torch, plan, n, k, i16), fcw, pm, x, y,
                         PHASE0, acc, i16)
            assert np.array_equal(gx, decimate(full[0], k)), (cap, k)
            assert np.array_equal(gy, decimate(full[1], k)), (cap, k)
            assert last_value(acc) == acc_after(fcw, n, PHASE0 + PRESET), (cap, k)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,i16", [("ww38", False), ("n9", False), ("sp2r", False),
                                      ("cfg2_ug", False), ("ww35_16", True), ("n9", True)])
def test_gpu_fallback_plans_equal_the_oracle(name, i16):
    """plans that cordic_plan_fm_mix (_mix16) does not fuse; ww35_16: ports of
    16 bits at WW 35, which the int16 form does not fuse"""
    import torch
    cfg = core(name, i16)
    plan = ca.Plan(cfg)
    assert cfg.ww == 35 if name == "ww35_16" else plan.fm_mix_info()[0] == 0
    n = 2048 + 128
    rng = np.random.default_rng(44)
    x, y = MIX16.iq16(rng, n, cfg.iw) if i16 else MIX.iq(rng, n, cfg.iw)
    fcw, pm = words("random", n, 19), words("random", n, 20)
    p, final = phases(fcw, pm, PHASE0, PRESET)
    wx, wy = tuned(name, i16, x, y, p)
    ws = plan.fm_mix_decim16_workspace if i16 else plan.fm_mix_decim_workspace
    mix = plan.fm_mix16_workspace if i16 else plan.fm_mix_workspace
    for k in (2, 7):
        assert ws(n, k) == mix(n) + 2 * ((n * (2 if i16 else 4) + 15) // 16 * 16)
        acc = last_word(torch, PRESET)
        gx, gy = run(torch, plan, k, work_buffer(torch, plan, n, k, i16), fcw, pm, x, y,
                     PHASE0, acc, i16)
        assert np.array_equal(gx, decimate(wx, k)) and np.array_equal(gy, decimate(wy, k)), k
        assert last_value(acc) == final
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "ww38"])
def test_gpu_three_calls_cut_at_multiples_of_r_equal_one_call(name):
    import torch
    plan = ca.Plan(MIX.both(name)[0])
    x, y, fcw, pm, full, bare = reference("cfg2", False)
    if name != "cfg2":
        p, _ = phases(fcw, pm, PHASE0, PRESET)
        full = MIX.want(name, x, y, p)
    k, n = 5, 3 * 1024 + 64
    cuts = [0, 32, 1024 + 96, n]
    work = work_buffer(torch, plan, n, k)
    acc = last_word(torch, PRESET)
    parts = [run(torch, plan, k, work, fcw[a:b], pm[a:b], x[a:b], y[a:b],
                 PHASE0 if a == 0 else 0, acc) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate([q[0] for q in parts]), decimate(full[0][:n], k))
    assert np.array_equal(np.concatenate([q[1] for q in parts]), decimate(full[1][:n], k))
    assert last_value(acc) == acc_after(fcw, n, PHASE0 + PRESET)
    plan.close()


@pytest.mark.gpu
def test_gpu_the_fused_call_in_a_graph_is_one_chain_and_continues_on_replay():
    """captured once with a d_acc word and replayed three times: two kernel
    nodes with one edge, *d_acc = start + 3 * sum(fcw), and the last replay's
    outputs are the oracle's for the phase it started from"""
    import torch
    from gpu_util import DEV, dev_i32, to_np
    name, k = "cfg2", 4
    plan = ca.Plan(MIX.both(name)[0])
    assert plan.fm_mix_info()[0] == 1
    n = 3 * 1024 + 16
    x, y, fcw, pm, _, _ = reference(name, False)
    x, y, fcw, pm = x[:n].copy(), y[:n].copy(), fcw[:n].copy(), pm[:n].copy()
    dfcw, dpm, dx, dy = dev_i32(fcw), dev_i32(pm), dev_i32(x), dev_i32(y)
    ox = torch.zeros(n >> k, dtype=torch.int32, device=DEV)
    oy = torch.zeros(n >> k, dtype=torch.int32, device=DEV)
    work = work_buffer(torch, plan, n, k)
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
        plan.fm_mix_decim(k, dfcw, dx, dy, ox, oy, work, pm=dpm, phase0=0, acc=acc,
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
    assert last_value(acc) == (PRESET + 3 * total) & 0xffffffff
    p, final = phases(fcw, pm, 0, (PRESET + 2 * total) & 0xffffffff)
    assert final == last_value(acc)
    wx, wy = MIX.want(name, x, y, p)
    assert np.array_equal(to_np(ox), decimate(wx, k))
    assert np.array_equal(to_np(oy), decimate(wy, k))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "ww38"])
def test_gpu_bad_arguments_are_refused_and_nothing_is_written(name):
    import torch
    n, k = 64, 3
    m = n >> k
    plan = ca.Plan(MIX.both(name)[0])
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    wbytes = plan.fm_mix_decim_workspace(n, k)
    work = big[:wbytes]
    ins = Padded(torch, 4 * n, 0, src=np.arange(4 * n, dtype=np.int32))
    outs = Padded(torch, 4 * n, 0)                # outputs cut from one array
    acc = last_word(torch, 77)
    i, v = ins.t, outs.t
    f, pm, x, y = i[:n], i[n:], i[2 * n:], i[3 * n:]
    a, b = v[:n], v[2 * n:]

    def refused(f, pm, x, y, a, b, w, n=n, k=k, acc=acc):
        with pytest.raises(ca.CordicError) as e:
            plan.fm_mix_decim(k, f, x, y, a, b, w, pm=pm, n=n, acc=acc)
        assert e.value.status == ca.ERR_ARGS

    refused(f, pm, x, y, a, b, work, n=n - 4)             # n % R
    refused(f, pm, x, y, a, b, work, n=n + 1)
    refused(f, pm, x, y, a, b, work, k=9)                 # k > 8
    refused(f, pm, x, y, a, b, work, k=0xffffffff)
    refused(None, pm, x, y, a, b, work)                   # every NULL
    refused(f, pm, None, y, a, b, work)
    refused(f, pm, x, None, a, b, work)
    refused(f, pm, x, y, None, b, work)
    refused(f, pm, x, y, a, None, work)
    refused(f, pm, x, y, a, b, 0)
    odd = lambda t: t.data_ptr() + 2                      # every pointer off its grid
    refused(odd(f), pm, x, y, a, b, work)
    refused(f, odd(pm), x, y, a, b, work)
    refused(f, pm, odd(x), y, a, b, work)
    refused(f, pm, x, odd(y), a, b, work)
    refused(f, pm, x, y, odd(a), b, work)
    refused(f, pm, x, y, a, odd(b), work)
    refused(f, pm, x, y, a, b, big[8:])
    refused(f, pm, x, y, a, b, work, acc=acc.data_ptr() + 2)
    refused(f, pm, x, y, x, b, work)                      # d_oxval is d_xval
    refused(f, f, x, y, i[2 * n - m + 1:], b, work)       # its last element on d_xval
    refused(f, pm, x, y, a, v[m - 1:], work)              # d_oyval on d_oxval by one
    refused(f, pm, x, y, a, b, work, acc=v[m - 1:])       # d_acc in d_oxval
    refused(f, pm, x, y, a, b, work, acc=work.data_ptr() + wbytes - 4)
    refused(f, pm, x, y, a, b, y[n - 4:].data_ptr())      # d_work on an input
    torch.cuda.synchronize()
    assert last_value(acc) == 77 and outs.untouched()
    # by the DECIMATED range: an output that ends where an input begins, and
    # two outputs m elements apart, are accepted; the inputs may alias
    plan.fm_mix_decim(k, f, x, x, i[2 * n - m:], v[m:], work, pm=f, n=n,
                      acc=last_word(torch, 1))
    torch.cuda.synchronize()
    h = ins.get()
    want = np.arange(4 * n, dtype=np.int32)
    assert np.array_equal(h[:2 * n - m], want[:2 * n - m])
    assert np.array_equal(h[2 * n:], want[2 * n:])
    assert not np.array_equal(h[2 * n - m:2 * n], want[2 * n - m:2 * n])
    o = outs.t.cpu().numpy()
    assert (o[:m] == S32).all() and (o[2 * m:] == S32).all() and not (o[m:2 * m] == S32).all()
    plan.close()
