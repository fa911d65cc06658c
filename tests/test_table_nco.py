"""Oscillator forms of the table and quadratic sine cores (cordic_table_nco,
cordic_quad_nco and their int16 forms; include/cordic_amd.h).  The kernel makes
the phases p_i = phase0 + (index0 + i) * fcw itself; sin is the core at p_i,
cos the core a quarter turn ahead.  Every output must be, bit for bit, what the
oracle gives for those phases AND what the device's own lookup gives on the
materialised phase array (the oscillator unit restates the lookups' sample
functions: this pins the two copies to each other on every layout)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_table_nco", "cordic_table_nco16", "cordic_quad_nco",
         "cordic_quad_nco16")


# ---------------------------------------------------------------- no GPU

def test_the_oscillator_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    for name in NAMES:
        handle = "cordic_table" if "table" in name else "cordic_quad"
        elem = "int16_t" if name.endswith("16") else "int32_t"
        assert re.search(
            r"int\s+%s\s*\(\s*const\s+%s\s*\*\s*\w+\s*,\s*size_t\s+n\s*,"
            r"\s*uint32_t\s+phase0\s*,\s*uint32_t\s+fcw\s*,\s*uint64_t\s+index0\s*,"
            r"\s*%s\s*\*\s*d_sin\s*,\s*%s\s*\*\s*d_cos\s*,\s*void\s*\*\s*stream\s*\)\s*;"
            % (name, handle, elem, elem), text), name
        getattr(ca.lib(), name)             # AttributeError: not exported
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


@pytest.mark.parametrize("name", NAMES)
def test_a_null_handle_is_refused(name):
    f = getattr(ca.lib(), name)
    assert f(None, 8, 0, 1, 0, None, None, None) == ca.ERR_ARGS
    assert f(None, 0, 0, 1, 0, None, None, None) == ca.ERR_ARGS


# ---------------------------------------------------------------- GPU

TABLES = [(ca.TBL, -1, 13, 17), (ca.QTR, -1, 24, 18), (ca.TBL, -1, 8, 6),
          (ca.QTR, -1, 16, 17), (ca.QTR, -1, 24, 17), (ca.TBL, -1, 24, 17),
          (ca.QTR, -1, 30, 20), (ca.QTR, -1, 9, 5), (ca.TBL, -1, 12, 18)]
# (phase0, fcw, index0); with n = 2^20 the first is every phase of every core
# with PW <= 20; in the last the sample index crosses 2^32 inside the call
CASES = [(0, 1, 0), (0x12345, 0, 7), (0xdeadbeef, 0x9e3779b1, 0),
         (5, 0x80000001, (1 << 40) + 3), (0, 3, (1 << 32) - 2)]
SIZES = [(0, 0), (5, 0), (1 << 20, 0), ((1 << 16) + 3, 1)]
S32, S16 = -0x5a5a5a5b, 0x5a5b        # sentinels
PAD = 16


def phases(pw, n, phase0, fcw, index0, lead=0):
    """p_i (+ lead) mod 2^PW in uint64 arithmetic"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(index0 % (1 << 64))
    with np.errstate(over="ignore"):
        p = np.uint64(phase0) + i * np.uint64(fcw) + np.uint64(lead)
    return (p & np.uint64((1 << pw) - 1)).astype(np.uint32)


class TableCore:
    def __init__(self, kind, iw, ow, pw):
        self.h = ca.Table(kind, iw, ow, pw)
        self.kind, self.pw, self.ow = kind, self.h.pw, self.h.ow
        self.tbl = O.table_values(kind, self.pw, self.ow)

    def oracle(self, ph):
        return O.table_lookup(self.kind, self.pw, self.ow, self.tbl, ph)


class QuadCore:
    def __init__(self, args):
        self.h = ca.Quad(*args)
        self.q = O.quad_cli(*args)
        self.t = O.quad_tables(self.q)
        self.pw, self.ow = self.h.pw, self.h.ow

    def oracle(self, ph):
        return O.quad_lookup(self.q, self.t, ph)


def run_nco(core, torch, n, case, off_s, off_c, i16):
    """One call into sentinel-filled buffers; off_c None: sine only, with a
    spare sentinel buffer in the cosine's place.  Returns the two in-range
    slices after checking that nothing else was written."""
    from gpu_util import DEV
    dt, sent = (torch.int16, S16) if i16 else (torch.int32, S32)
    npdt = np.int16 if i16 else np.int32
    phase0, fcw, index0 = case
    bs = torch.full((off_s + n + PAD,), sent, dtype=dt, device=DEV)
    oc = 0 if off_c is None else off_c
    bc = torch.full((oc + n + PAD,), sent, dtype=dt, device=DEV)
    core.h.nco(bs[off_s:], None if off_c is None else bc[oc:], n=n,
               phase0=phase0, fcw=fcw, index0=index0)
    torch.cuda.synchronize()
    hs, hc = bs.cpu().numpy(), bc.cpu().numpy()
    assert hs.dtype == npdt
    assert (hs[:off_s] == sent).all() and (hs[off_s + n:] == sent).all()
    if off_c is None:
        assert (hc == sent).all()
        return hs[off_s:off_s + n], None
    assert (hc[:oc] == sent).all() and (hc[oc + n:] == sent).all()
    return hs[off_s:off_s + n], hc[oc:oc + n]


def device_lookup(core, torch, ph):
    from gpu_util import DEV, dev_i32, to_np
    if ph.size == 0:
        return np.empty(0, dtype=np.int32)
    out = torch.zeros(ph.size, dtype=torch.int32, device=DEV)
    core.h.lookup(dev_i32(ph), out, n=ph.size)
    torch.cuda.synchronize()
    return to_np(out)


def check_core(core):
    import torch
    for case in CASES:
        phase0, fcw, index0 = case
        for n, off in SIZES:
            ps = phases(core.pw, n, phase0, fcw, index0)
            pc = phases(core.pw, n, phase0, fcw, index0, 1 << (core.pw - 2))
            want_s, want_c = core.oracle(ps), core.oracle(pc)
            # the cosine array sits differently from the sine array
            s, c = run_nco(core, torch, n, case, off, 3 * off, False)
            assert np.array_equal(s, want_s) and np.array_equal(c, want_c)
            assert np.array_equal(s, device_lookup(core, torch, ps))
            assert np.array_equal(c, device_lookup(core, torch, pc))
            s1, _ = run_nco(core, torch, n, case, off, None, False)
            assert np.array_equal(s1, want_s)
            if core.ow <= 16:
                # also at an odd element offset: a 2-byte-aligned address
                for o16 in sorted({off, off | 1}):
                    a, b = run_nco(core, torch, n, case, o16, 3 * o16, True)
                    assert np.array_equal(a, want_s.astype(np.int16))
                    assert np.array_equal(b, want_c.astype(np.int16))
                    a1, _ = run_nco(core, torch, n, case, o16, None, True)
                    assert np.array_equal(a1, want_s.astype(np.int16))
            if n > 5:
                # the job cut at an odd k into two calls: the bits of one call
                k = n // 3 | 1
                for i16 in ((False, True) if core.ow <= 16 else (False,)):
                    a0, b0 = run_nco(core, torch, k, case, off, 3 * off, i16)
                    a1, b1 = run_nco(core, torch, n - k,
                                     (phase0, fcw, index0 + k), off, 3 * off, i16)
                    t = np.int16 if i16 else np.int32
                    assert np.array_equal(np.concatenate([a0, a1]), want_s.astype(t))
                    assert np.array_equal(np.concatenate([b0, b1]), want_c.astype(t))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,iw,ow,pw", TABLES)
def test_gpu_table_oscillator_equals_oracle_and_lookup(kind, iw, ow, pw):
    core = TableCore(kind, iw, ow, pw)
    check_core(core)
    core.h.close()


def _quad_cores():
    from test_quadtbl import GOLD, GOOD, cli_args
    return [(name, cli_args(GOLD[name]["args"])) for name in GOOD]


@pytest.mark.gpu
@pytest.mark.parametrize("name,args", _quad_cores())
def test_gpu_quad_oscillator_equals_oracle_and_lookup(name, args):
    core = QuadCore(args)
    check_core(core)
    core.h.close()


@pytest.mark.gpu
def test_gpu_16_bit_forms_refuse_wide_cores_and_bad_arguments():
    import torch
    from gpu_util import DEV
    t = ca.Table(ca.QTR, -1, 24, 17)
    q = ca.Quad(ow=24, pw=32)
    o16 = torch.zeros(64, dtype=torch.int16, device=DEV)
    o32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    for h in (t, q):
        with pytest.raises(ca.CordicError) as e:
            h.nco(o16[:16], o16[32:48])
        assert e.value.status == ca.ERR_CONTAINER
        with pytest.raises(ca.CordicError) as e:
            h.nco(None, o32[:16], n=16)                 # no sine array
        assert e.value.status == ca.ERR_ARGS
        h.nco(None, None, n=0)                          # a no-op
        with pytest.raises(ca.CordicError) as e:
            h.nco(o32[:16], o32[8:24])                  # overlapping outputs
        assert e.value.status == ca.ERR_ARGS
    torch.cuda.synchronize()
    assert not o16.any() and not o32.any()
    t.close(); q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["qtr16", "qtr24", "quad"])
def test_gpu_oscillator_in_a_hip_graph(which):
    """A captured quadrature call keeps a tile queue of its own (captured_used
    rises by one) and replays to the same bits."""
    import torch
    from gpu_util import DEV
    if which == "quad":
        core = QuadCore((-1, 13, 2, 18))
    else:
        core = TableCore(ca.QTR, -1, 16 if which == "qtr16" else 24, 17)
    n = (1 << 18) + 5
    case = (0x1234, 0x01234567, 99)
    s = torch.zeros(n, dtype=torch.int32, device=DEV)
    c = torch.zeros(n, dtype=torch.int32, device=DEV)
    core.h.nco(s, c, phase0=case[0], fcw=case[1], index0=case[2])
    torch.cuda.synchronize()
    want_s = core.oracle(phases(core.pw, n, *case))
    want_c = core.oracle(phases(core.pw, n, *case, 1 << (core.pw - 2)))
    assert np.array_equal(s.cpu().numpy(), want_s)
    assert np.array_equal(c.cpu().numpy(), want_c)
    used = core.h.queue_info["captured_used"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        core.h.nco(s, c, phase0=case[0], fcw=case[1], index0=case[2])
    assert core.h.queue_info["captured_used"] == used + 1
    for _ in range(2):
        s.zero_(); c.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(s.cpu().numpy(), want_s)
        assert np.array_equal(c.cpu().numpy(), want_c)
    del g
    core.h.close()
