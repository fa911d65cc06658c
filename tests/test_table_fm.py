"""Frequency- and phase-modulated oscillators on the table and quadratic sine
cores (cordic_table_fm, cordic_quad_fm, their int16 forms) and the phase
accumulator alone (cordic_phase_accumulate; include/cordic_amd.h).  The phase
of sample i is an exclusive running sum of per-sample tuning words (+ a phase
word), made on the device.  Expected phases are numpy's cumsum in uint32;
expected values are the oracle's lookup at those phases, the device's own
lookup on them, and -- for constant tuning words -- the pure-tone oscillator."""
import os
import re

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM = ("cordic_table_fm", "cordic_table_fm16", "cordic_quad_fm",
      "cordic_quad_fm16")


# ---------------------------------------------------------------- no GPU

def test_the_six_functions_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    u32p = r"const\s+uint32_t\s*\*\s*"
    for name in FM:
        handle = "cordic_table" if "table" in name else "cordic_quad"
        elem = "int16_t" if name.endswith("16") else "int32_t"
        assert re.search(
            r"int\s+%s\s*\(\s*const\s+%s\s*\*\s*\w+\s*,\s*size_t\s+n\s*,\s*"
            r"%sd_fcw\s*,\s*%sd_pm\s*,\s*uint32_t\s+phase0\s*,\s*"
            r"uint32_t\s*\*\s*d_acc\s*,\s*%s\s*\*\s*d_sin\s*,\s*%s\s*\*\s*d_cos\s*,"
            r"\s*void\s*\*\s*d_work\s*,\s*void\s*\*\s*stream\s*\)\s*;"
            % (name, handle, u32p, u32p, elem, elem), text), name
    assert re.search(
        r"int\s+cordic_phase_accumulate\s*\(\s*size_t\s+n\s*,\s*%sd_fcw\s*,\s*"
        r"%sd_pm\s*,\s*uint32_t\s+phase0\s*,\s*uint32_t\s*\*\s*d_acc\s*,\s*"
        r"uint32_t\s*\*\s*d_phase\s*,\s*void\s*\*\s*d_work\s*,\s*"
        r"void\s*\*\s*stream\s*\)\s*;" % (u32p, u32p), text)
    assert re.search(r"size_t\s+cordic_fm_workspace\s*\(\s*size_t\s+n\s*\)\s*;",
                     text)
    for name in FM + ("cordic_phase_accumulate", "cordic_fm_workspace"):
        getattr(ca.lib(), name)             # AttributeError: not exported
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


@pytest.mark.parametrize("name", FM)
def test_a_null_handle_is_refused(name):
    f = getattr(ca.lib(), name)
    for n in (8, 0):
        assert f(None, n, None, None, 0, None, None, None, None, None) \
            == ca.ERR_ARGS


def test_the_workspace_size_is_small_aligned_and_monotonic():
    assert ca.fm_workspace(0) == 0
    sizes = [0, 1, 2, 5, 511, 512, 513, 4095, 4096, 4097, (1 << 16) + 3,
             1 << 20, (1 << 23) + 4099, 1 << 28, (1 << 32) + 1, 1 << 40]
    last = 0
    for n in sizes:
        w = ca.fm_workspace(n)
        assert w % 16 == 0, n
        assert w >= last, n
        assert w <= n // 512 + 65536, n
        assert n == 0 or w > 0
        last = w


def test_the_binding_asks_the_caller_for_the_scratch():
    with pytest.raises(TypeError):
        ca.phase_accumulate(0x1000, 0x2000, n=8)
    with pytest.raises(TypeError):
        ca.Table(ca.QTR, -1, 16, 17, device=False).fm(0x1000, 0x2000, n=8)


# ---------------------------------------------------------------- GPU

TABLES = [(ca.TBL, -1, 13, 17), (ca.QTR, -1, 24, 18), (ca.TBL, -1, 8, 6),
          (ca.QTR, -1, 16, 17), (ca.QTR, -1, 24, 17), (ca.TBL, -1, 24, 17),
          (ca.TBL, -1, 12, 18)]
QUADS = ["rtl_quadtbl", "o20x4p24"]        # of test_quadtbl's GOOD; OW 13, 20
# (n, element offset of the sine array; the cosine sits at 3 * that)
SIZES = [(0, 0), (1, 1), (5, 2), (4095, 3), (4096, 0), (4097, 1),
         ((1 << 16) + 3, 3)]
BIG = (1 << 23) + 4099
S32, S16 = -0x5a5a5a5b, 0x5a5b        # sentinels
PAD = 16
M32 = 0xffffffff


def words(kind, n, seed):
    """tuning words: the four patterns of the issue"""
    if kind == "zero":
        return np.zeros(n, dtype=np.uint32)
    if kind == "ones":
        return np.full(n, M32, dtype=np.uint32)
    if kind == "random":
        return np.random.default_rng(seed).integers(
            0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    assert kind == "fsk"
    bit = (np.arange(n) // 37) & 1
    return np.where(bit, 0x0123457, 0xfff00001).astype(np.uint32)


def phase_words(kind, n, seed):
    if kind == "none":
        return None
    if kind == "const":
        return np.full(n, 0x40000123, dtype=np.uint32)
    return words("random", n, seed + 1000)


def expected(fcw, pm, phase0, acc0=0):
    """(p_i as uint32, the accumulator after the call)"""
    start = (phase0 + acc0) & M32
    incl = np.cumsum(fcw, dtype=np.uint32)
    a = np.empty(fcw.size, dtype=np.uint32)
    if fcw.size:
        a[0] = 0
        a[1:] = incl[:-1]
    with np.errstate(over="ignore"):
        a = a + np.uint32(start)
        p = a if pm is None else a + pm
    final = (start + (int(incl[-1]) if fcw.size else 0)) & M32
    return p, final


class TableCore:
    def __init__(self, kind, iw, ow, pw):
        self.h = ca.Table(kind, iw, ow, pw)
        self.kind, self.pw, self.ow = kind, self.h.pw, self.h.ow
        self.tbl = O.table_values(kind, self.pw, self.ow)

    def oracle(self, ph):
        ph = ph & np.uint32((1 << self.pw) - 1)
        return O.table_lookup(self.kind, self.pw, self.ow, self.tbl, ph)


class QuadCore:
    def __init__(self, name):
        from test_quadtbl import GOLD, cli_args
        args = cli_args(GOLD[name]["args"])
        self.h = ca.Quad(*args)
        self.q = O.quad_cli(*args)
        self.t = O.quad_tables(self.q)
        self.pw, self.ow = self.h.pw, self.h.ow

    def oracle(self, ph):
        mask = np.uint32(((1 << self.pw) - 1) & M32)
        return O.quad_lookup(self.q, self.t, ph & mask)


class Padded:
    """A sentinel-filled device array with `off` elements in front of and PAD
    behind the n that a call may write"""

    def __init__(self, torch, n, off, i16=False, src=None):
        from gpu_util import DEV
        self.dt, self.sent = (torch.int16, S16) if i16 else (torch.int32, S32)
        self.n, self.off = n, off
        self.t = torch.full((off + n + PAD,), self.sent, dtype=self.dt, device=DEV)
        if src is not None and n:
            self.t[off:off + n].copy_(torch.from_numpy(
                np.ascontiguousarray(src).view(np.int32)).to(DEV))

    @property
    def view(self):
        return self.t[self.off:]

    def get(self, dtype=None):
        """the n values, after checking that nothing around them was written"""
        h = self.t.cpu().numpy()
        assert (h[:self.off] == self.sent).all()
        assert (h[self.off + self.n:] == self.sent).all()
        v = h[self.off:self.off + self.n]
        return v if dtype is None else v.view(dtype)

    def untouched(self):
        return bool((self.t == self.sent).all().item())


def work_buffer(torch, n=BIG):
    from gpu_util import DEV
    return torch.zeros(max(16, ca.fm_workspace(n)), dtype=torch.uint8, device=DEV)


def acc_word(torch, value):
    from gpu_util import DEV
    v = value - (1 << 32) if value >= 1 << 31 else value
    return torch.full((4,), v, dtype=torch.int32, device=DEV)


def acc_value(acc):
    h = acc.cpu().numpy().view(np.uint32)
    assert (h[1:] == h[1]).all()            # only the first word is the call's
    return int(h[0])


def run_fm(core, torch, work, fcw, pm, phase0, off_s, off_c, i16, acc=None):
    """One call with every array at its own element offset (fcw + 1, pm + 3,
    sin + off_s, cos + off_c); off_c None: sine only, with a spare sentinel
    buffer in the cosine's place.  Returns the in-range slices."""
    n = fcw.size
    df = Padded(torch, n, 1, src=fcw)
    dp = None if pm is None else Padded(torch, n, 3, src=pm)
    bs = Padded(torch, n, off_s, i16)
    bc = Padded(torch, n, 0 if off_c is None else off_c, i16)
    core.h.fm(df.view, bs.view, None if off_c is None else bc.view,
              pm=None if dp is None else dp.view, n=n, phase0=phase0, acc=acc,
              work=work)
    torch.cuda.synchronize()
    assert np.array_equal(df.get(np.uint32), fcw)       # inputs are inputs
    if dp is not None:
        assert np.array_equal(dp.get(np.uint32), pm)
    if off_c is None:
        assert bc.untouched()
        return bs.get(), None
    return bs.get(), bc.get()


def run_accumulate(torch, work, fcw, pm, phase0, off, acc=None, in_place=False):
    n = fcw.size
    df = Padded(torch, n, off if in_place else 1, src=fcw)
    dp = None if pm is None else Padded(torch, n, 3, src=pm)
    out = df if in_place else Padded(torch, n, off)
    ca.phase_accumulate(df.view, out.view, pm=None if dp is None else dp.view,
                        n=n, phase0=phase0, acc=acc, work=work)
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(df.get(np.uint32), fcw)
    return out.get(np.uint32), out


def device_lookup(core, torch, ph_dev, n):
    from gpu_util import DEV, to_np
    if n == 0:
        return np.empty(0, dtype=np.int32)
    out = torch.zeros(n, dtype=torch.int32, device=DEV)
    core.h.lookup(ph_dev, out, n=n)
    torch.cuda.synchronize()
    return to_np(out)


def run_nco(core, torch, n, phase0, fcw):
    from gpu_util import DEV, to_np
    s = torch.zeros(max(n, 1), dtype=torch.int32, device=DEV)
    c = torch.zeros(max(n, 1), dtype=torch.int32, device=DEV)
    core.h.nco(s, c, n=n, phase0=phase0, fcw=fcw, index0=0)
    torch.cuda.synchronize()
    return to_np(s)[:n], to_np(c)[:n]


COMBOS = [(f, p) for f in ("zero", "ones", "random", "fsk")
          for p in ("none", "const", "random")]
PHASE0 = 0xdeadbeef


def check_core(core):
    import torch
    work = work_buffer(torch)
    quarter = 1 << (core.pw - 2)
    queues = core.h.queue_info
    for n, off in SIZES:
        for k, (fk, pk) in enumerate(COMBOS):
            fcw, pm = words(fk, n, 7 * n + k), phase_words(pk, n, 7 * n + k)
            p, final = expected(fcw, pm, PHASE0)
            want_s = core.oracle(p)
            with np.errstate(over="ignore"):
                want_c = core.oracle(p + np.uint32(quarter))
            acc = acc_word(torch, 0)
            s, c = run_fm(core, torch, work, fcw, pm, PHASE0, off, 3 * off,
                          False, acc)
            assert np.array_equal(s, want_s), (n, fk, pk)
            assert np.array_equal(c, want_c), (n, fk, pk)
            assert acc_value(acc) == (final if n else 0)
            s1, _ = run_fm(core, torch, work, fcw, pm, PHASE0, off, None, False)
            assert np.array_equal(s1, want_s), (n, fk, pk)
            # the device's own lookup on what cordic_phase_accumulate wrote
            got_p, arr = run_accumulate(torch, work, fcw, pm, PHASE0, off)
            assert np.array_equal(got_p, p), (n, fk, pk)
            assert np.array_equal(
                s, device_lookup(core, torch, arr.view[:n].clone(), n))
            if fk in ("zero", "ones"):
                # constant tuning words: the pure-tone oscillator, bit for bit
                lead = 0 if pm is None else int(pm[0]) if n else 0
                if pk != "random":
                    ns, nc = run_nco(core, torch, n, PHASE0 + lead,
                                     int(fcw[0]) if n else 0)
                    assert np.array_equal(s, ns) and np.array_equal(c, nc)
            if core.ow <= 16:
                # also at an odd element offset: a 2-byte-aligned address
                for o16 in sorted({off, off | 1}):
                    a, b = run_fm(core, torch, work, fcw, pm, PHASE0, o16,
                                  3 * o16, True)
                    assert np.array_equal(a, want_s.astype(np.int16))
                    assert np.array_equal(b, want_c.astype(np.int16))
                    a1, _ = run_fm(core, torch, work, fcw, pm, PHASE0, o16,
                                   None, True)
                    assert np.array_equal(a1, want_s.astype(np.int16))
        if n > 5:
            # the job cut at an odd k and at 2k into three calls that share
            # one accumulator word: the bits, and the final word, of one call
            fcw, pm = words("random", n, n), words("random", n, n + 1)
            p, final = expected(fcw, pm, PHASE0, 0x01020304)
            want_s = core.oracle(p)
            with np.errstate(over="ignore"):
                want_c = core.oracle(p + np.uint32(quarter))
            k = n // 3 | 1
            cuts = [(0, k), (k, 2 * k), (2 * k, n)]
            for i16 in ((False, True) if core.ow <= 16 else (False,)):
                t = np.int16 if i16 else np.int32
                acc = acc_word(torch, 0x01020304)
                s, c = run_fm(core, torch, work, fcw, pm, PHASE0, off, 3 * off,
                              i16, acc)
                assert np.array_equal(s, want_s.astype(t))
                assert np.array_equal(c, want_c.astype(t))
                assert acc_value(acc) == final
                acc = acc_word(torch, 0x01020304)
                parts = [run_fm(core, torch, work, fcw[a:b], pm[a:b],
                                PHASE0 if a == 0 else 0, off, 3 * off, i16, acc)
                         for a, b in cuts]
                assert np.array_equal(np.concatenate([x for x, _ in parts]),
                                      want_s.astype(t))
                assert np.array_equal(np.concatenate([y for _, y in parts]),
                                      want_c.astype(t))
                assert acc_value(acc) == final
    # no tile queue was taken
    assert core.h.queue_info == queues


def check_big(core, with_oracle):
    """every block owns several tiles on any grid of up to 1024 blocks"""
    import torch
    from gpu_util import dev_i32
    n = BIG
    work = work_buffer(torch)
    fcw, pm = words("random", n, 1), words("random", n, 2)
    p, final = expected(fcw, pm, PHASE0, 5)
    with np.errstate(over="ignore"):
        pc = p + np.uint32(1 << (core.pw - 2))
    acc = acc_word(torch, 5)
    s, c = run_fm(core, torch, work, fcw, pm, PHASE0, 1, 3, False, acc)
    assert acc_value(acc) == final
    assert np.array_equal(s, device_lookup(core, torch, dev_i32(p), n))
    assert np.array_equal(c, device_lookup(core, torch, dev_i32(pc), n))
    if with_oracle:
        assert np.array_equal(s, core.oracle(p))
        assert np.array_equal(c, core.oracle(pc))
    if core.ow <= 16:
        a, b = run_fm(core, torch, work, fcw, pm, PHASE0, 1, 5, True,
                      acc_word(torch, 5))
        assert np.array_equal(a, s.astype(np.int16))
        assert np.array_equal(b, c.astype(np.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,iw,ow,pw", TABLES)
def test_gpu_table_fm_equals_oracle_lookup_and_oscillator(kind, iw, ow, pw):
    core = TableCore(kind, iw, ow, pw)
    check_core(core)
    core.h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", QUADS)
def test_gpu_quad_fm_equals_oracle_lookup_and_oscillator(name):
    core = QuadCore(name)
    check_core(core)
    core.h.close()


@pytest.mark.gpu
def test_gpu_table_fm_where_every_block_owns_several_tiles():
    core = TableCore(ca.QTR, -1, 16, 17)
    check_big(core, True)
    core.h.close()


@pytest.mark.gpu
def test_gpu_quad_fm_where_every_block_owns_several_tiles():
    core = QuadCore("rtl_quadtbl")
    check_big(core, False)
    core.h.close()


@pytest.mark.gpu
def test_gpu_phase_accumulate_equals_numpy_also_in_place():
    import torch
    work = work_buffer(torch)
    for n, off in SIZES + [(BIG, 1)]:
        combos = COMBOS if n < BIG else [("random", "random")]
        for k, (fk, pk) in enumerate(combos):
            fcw, pm = words(fk, n, 3 * n + k), phase_words(pk, n, 3 * n + k)
            p, final = expected(fcw, pm, 0x80000001, 0xfffffff0)
            for in_place in (False, True):
                acc = acc_word(torch, 0xfffffff0)
                got, _ = run_accumulate(torch, work, fcw, pm, 0x80000001, off,
                                        acc, in_place)
                assert np.array_equal(got, p), (n, fk, pk, in_place)
                assert acc_value(acc) == (final if n else 0xfffffff0)
            # without an accumulator word: start = phase0
            got, _ = run_accumulate(torch, work, fcw, pm, 0x80000001, off)
            assert np.array_equal(got, expected(fcw, pm, 0x80000001)[0])


@pytest.mark.gpu
def test_gpu_16_bit_forms_refuse_wide_cores():
    import torch
    work = work_buffer(torch, 64)
    fcw = Padded(torch, 16, 0, src=words("random", 16, 1))
    for h in (ca.Table(ca.QTR, -1, 24, 17), ca.Quad(ow=24, pw=32)):
        s, c = Padded(torch, 16, 2, True), Padded(torch, 16, 2, True)
        for cos in (None, c.view):
            with pytest.raises(ca.CordicError) as e:
                h.fm(fcw.view, s.view, cos, n=16, work=work)
            assert e.value.status == ca.ERR_CONTAINER
        # (also with n = 0: the container is the handle's, as for *_nco16)
        with pytest.raises(ca.CordicError) as e:
            h.fm(fcw.view, s.view, None, n=0, work=work)
        assert e.value.status == ca.ERR_CONTAINER
        torch.cuda.synchronize()
        assert s.untouched() and c.untouched()
        h.close()


@pytest.mark.gpu
def test_gpu_bad_arguments_are_refused_and_nothing_is_written():
    import torch
    n = 64
    work = work_buffer(torch, n)
    big = Padded(torch, 4 * n, 0)                # outputs cut from one array
    fcw = Padded(torch, 2 * n, 0, src=words("random", 2 * n, 1))
    acc = acc_word(torch, 77)
    v, f = big.t, fcw.t
    for h in (ca.Table(ca.QTR, -1, 16, 17), ca.Quad(*(-1, 13, 2, 18))):
        def refused(*a, **kw):
            with pytest.raises(ca.CordicError) as e:
                h.fm(*a, n=n, acc=acc, **kw)
            assert e.value.status == ca.ERR_ARGS
        refused(None, v[:n], v[2 * n:], work=work)              # NULL d_fcw
        refused(f, None, v[2 * n:], work=work)                  # NULL d_sin
        refused(f, v[:n], v[2 * n:], work=0)                    # NULL d_work
        refused(f, v[:n], v[2 * n:], work=work[8:])             # misaligned
        refused(f[1:].view(torch.int16)[1:], v[:n], None, work=work)
        refused(f, v[:n], v[n - 1:], work=work)                 # sin over cos
        refused(f, f[n - 1:], None, work=work)                  # sin over fcw
        refused(f, f, None, work=work)          # in place is the accumulator's
        refused(f, v[:n], None, pm=v[n - 1:], work=work)        # sin over pm
        refused(f, v[:n], None, work=v[n - 4:])                 # work over sin
        with pytest.raises(ca.CordicError) as e:                # acc over sin
            h.fm(f, v[:n], None, n=n, acc=v[n - 1:], work=work)
        assert e.value.status == ca.ERR_ARGS
        h.fm(None, None, None, n=0, acc=acc, work=None)         # a no-op
        h.close()
    # the accumulator alone: a shifted overlap is refused, the exact one is not
    for bad in (dict(phase=f[1:]), dict(phase=f[n - 1:]), dict(fcw=None),
                dict(phase=None), dict(work=0), dict(work=work[4:]),
                dict(pm=f, phase=f), dict(acc=f[n - 1:])):
        kw = dict(fcw=f, phase=v, pm=None, acc=acc, work=work)
        kw.update(bad)
        with pytest.raises(ca.CordicError) as e:
            ca.phase_accumulate(kw.pop("fcw"), kw.pop("phase"), n=n, **kw)
        assert e.value.status == ca.ERR_ARGS, bad
    ca.phase_accumulate(None, None, n=0, acc=acc, work=None)    # a no-op
    torch.cuda.synchronize()
    assert big.untouched()
    assert acc_value(acc) == 77
    assert np.array_equal(fcw.get(np.uint32), words("random", 2 * n, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(13, 13, 2, -1, -1), (32, 32, 2, 32, 16)])
def test_gpu_accumulate_then_p2r_equals_the_cordic_oscillator(args):
    """constant tuning words through cordic_phase_accumulate and
    cordic_p2r_const: cordic_nco for the same tuning"""
    import torch
    from gpu_util import DEV, gpu_nco, to_np
    cfg = ca.Config.from_cli(ca.P2R, *args)
    n = (1 << 16) + 3
    phase0, f = 0x00012345, 0x9e3779b1
    x0 = (1 << (args[0] - 1)) - 1
    fcw = torch.full((n,), f - (1 << 32), dtype=torch.int32, device=DEV)
    ph = torch.zeros(n, dtype=torch.int32, device=DEV)
    ca.phase_accumulate(fcw, ph, phase0=phase0, work=work_buffer(torch, n))
    ox = torch.zeros(n, dtype=torch.int32, device=DEV)
    oy = torch.zeros(n, dtype=torch.int32, device=DEV)
    ca.p2r_const(cfg, x0, 0, ph, ox, oy)
    torch.cuda.synchronize()
    wx, wy = gpu_nco(cfg, n, phase0, f, 0, x0, 0)
    assert np.array_equal(to_np(ox), wx) and np.array_equal(to_np(oy), wy)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["qtr16", "qtr24", "quad"])
def test_gpu_fm_in_a_hip_graph_continues_the_waveform(which):
    """A captured quadrature call takes no queue slot; replayed three times
    with new tuning words in the same input buffer it gives one call over the
    concatenated words."""
    import torch
    from gpu_util import DEV, dev_i32
    if which == "quad":
        core = QuadCore("rtl_quadtbl")
    else:
        core = TableCore(ca.QTR, -1, 16 if which == "qtr16" else 24, 17)
    n = (1 << 18) + 5
    fcw = words("random", 3 * n, 11)
    pm = words("random", n, 12)                  # the same phase words each time
    p, final = expected(fcw, np.tile(pm, 3), 0, 0x13572468)
    want_s = core.oracle(p)
    with np.errstate(over="ignore"):
        want_c = core.oracle(p + np.uint32(1 << (core.pw - 2)))
    work = work_buffer(torch, n)
    acc = acc_word(torch, 0x13572468)
    df, dp = dev_i32(fcw[:n]), dev_i32(pm)
    s = torch.zeros(n, dtype=torch.int32, device=DEV)
    c = torch.zeros(n, dtype=torch.int32, device=DEV)
    # (once outside the capture, on an accumulator word of its own)
    core.h.fm(df, s, c, pm=dp, acc=acc_word(torch, 0), work=work)
    used = core.h.queue_info["captured_used"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        core.h.fm(df, s, c, pm=dp, acc=acc, work=work)
    assert core.h.queue_info["captured_used"] == used
    got_s, got_c = [], []
    for k in range(3):
        df.copy_(dev_i32(fcw[k * n:(k + 1) * n]))
        s.zero_(); c.zero_()
        g.replay()
        torch.cuda.synchronize()
        got_s.append(s.cpu().numpy())
        got_c.append(c.cpu().numpy())
    assert np.array_equal(np.concatenate(got_s), want_s)
    assert np.array_equal(np.concatenate(got_c), want_c)
    assert acc_value(acc) == final
    del g
    core.h.close()
