"""Acceptance statistics of the sine-producing cores, reduced on the device
(cordic_quality_create_quad / _table, cordic_quality_sine*; include/cordic_amd.h).

bench/cpp/quadtbl_tb.cpp:146-179: err = |sin(2 pi p / 2^PW) * (2^(OW-1) - 1) - o|,
its maximum, the extreme outputs, the threshold |TBL_ERR| + 2.  The kernels
read what the engine wrote (*_lookup, *_nco, *_nco16); expected values are
tests/sine_quality.py's numpy restatement on the oracle's outputs, which the
engine's outputs are first checked to equal."""
import numpy as np
import pytest

import sine_quality as S

pytestmark = pytest.mark.gpu

FCW = 0x9E3779B1
N_NCO = (1 << 16) + 37


def check(got, phase, out, pw, ow, judged, tbl_err=0.0):
    want = S.expected(pw, ow, phase, out)
    i = got["max_err_index"]
    print("max_err dev %.17g numpy %.17g rel %.3g | err[index] - max %.3g | "
          "MXVAL %d MNVAL %d" % (got["max_err"], want["max_err"],
                                 abs(got["max_err"] / want["max_err"] - 1),
                                 want["err"][i] - want["max_err"],
                                 got["max_val"], got["min_val"]))
    assert got["n"] == phase.size
    assert got["max_err"] == pytest.approx(want["max_err"], rel=1e-9)
    assert got["max_val"] == want["max_val"] and got["min_val"] == want["min_val"]
    # near-ties may pick another index
    assert abs(want["err"][i] - want["max_err"]) < 1e-6
    assert got["max_err_phase"] == int(phase[i])
    assert got["scale"] == float((1 << (ow - 1)) - 1)
    assert got["judged"] == int(judged)
    if judged:
        assert got["tbl_err"] == tbl_err
        assert got["limit"] == abs(tbl_err) + 2.0
        assert got["pass"] == int(not want["max_err"] > got["limit"])
    else:
        assert got["tbl_err"] == 0.0 and got["limit"] == 0.0 and got["pass"] == 1


@pytest.fixture(scope="module")
def quad13():
    """-o 13 -p 18, the checked-in core: the full sweep through Quad.lookup,
    shared (read-only) by the tests below"""
    import torch
    import cordic_amd as ca
    from gpu_util import DEV, dev_i32, to_np
    core = S.QuadCore(ca, (-1, 13, 2, 18))
    ph = np.arange(1 << 18, dtype=np.uint32)
    dph = dev_i32(ph)
    out = torch.empty(ph.size, dtype=torch.int32, device=DEV)
    core.h.lookup(dph, out)
    torch.cuda.synchronize()
    ref = core.oracle(ph)
    assert np.array_equal(to_np(out), ref)
    return dict(core=core, ph=ph, dph=dph, out=out, ref=ref)


def test_quadratic_core_full_sweep_o13_p18(quad13):
    import cordic_amd as ca
    c = quad13["core"]
    q = c.quality(ca)
    q.sine(quad13["dph"], quad13["out"])
    got = q.sine_result()
    check(got, quad13["ph"], quad13["ref"], c.pw, c.ow, True, c.h.tbl_err)
    assert got["pass"] == 1
    q.close()


def test_quadratic_core_full_sweep_o8_p12():
    import torch
    import cordic_amd as ca
    from gpu_util import DEV, dev_i32, to_np
    c = S.QuadCore(ca, (-1, 8, 2, 12))
    ph = np.arange(1 << 12, dtype=np.uint32)
    dph = dev_i32(ph)
    out = torch.empty(ph.size, dtype=torch.int32, device=DEV)
    c.h.lookup(dph, out)
    torch.cuda.synchronize()
    ref = c.oracle(ph)
    assert np.array_equal(to_np(out), ref)
    q = c.quality(ca)
    q.sine(dph, out)
    check(q.sine_result(), ph, ref, c.pw, c.ow, True, c.h.tbl_err)
    q.close()


@pytest.mark.parametrize("args,index0", [((-1, 24, 2, 32), (1 << 32) + 12345),
                                         ((14, 10, 2, 20), 7)])
def test_quadratic_core_through_the_oscillator(args, index0):
    """odd fcw, n = 2^16 + 37; -o 24 -p 32 is the signed-phase case of the
    bench's (int), with the sample index past 2^32"""
    import torch
    import cordic_amd as ca
    from gpu_util import DEV, to_np
    c = S.QuadCore(ca, args)
    phase0 = 0x1234567
    ph = S.nco_phases(c.pw, N_NCO, phase0, FCW, index0)
    out = torch.empty(N_NCO, dtype=torch.int32, device=DEV)
    c.h.nco(out, None, phase0=phase0, fcw=FCW, index0=index0)
    torch.cuda.synchronize()
    ref = c.oracle(ph)
    assert np.array_equal(to_np(out), ref)
    q = c.quality(ca)
    q.sine_nco(out, phase0=phase0, fcw=FCW, index0=index0)
    check(q.sine_result(), ph, ref, c.pw, c.ow, True, c.h.tbl_err)
    q.close()


@pytest.mark.parametrize("kind,pw,ow,i16", [("tbl", 10, 12, False),
                                            ("qtr", 12, 16, True),
                                            ("qtr", 18, 24, False)])
def test_table_cores_sine_and_quadrature_of_one_nco_call(kind, pw, ow, i16):
    """tbl PW 10 / OW 12; qtr PW 12 / OW 16 through nco16 (the LDS int16
    path); qtr PW 18 / OW 24 (the L2 gather).  The cosine array is judged
    with phase0 + 2^(PW-2)."""
    import torch
    import cordic_amd as ca
    from gpu_util import DEV
    c = S.TableCore(ca, ca.TBL if kind == "tbl" else ca.QTR, ow, pw)
    assert (c.pw, c.ow) == (pw, ow)
    if kind == "qtr":
        assert c.h.lds_mode == (1 if i16 else 0)
    n = max(1 << pw, 4096) + 37
    phase0, fcw, index0 = 5, 3, (1 << 32) - 100
    dt = torch.int16 if i16 else torch.int32
    sn = torch.empty(n, dtype=dt, device=DEV)
    cs = torch.empty(n, dtype=dt, device=DEV)
    c.h.nco(sn, cs, phase0=phase0, fcw=fcw, index0=index0)
    torch.cuda.synchronize()
    q = c.quality(ca)
    for arr, lead in ((sn, 0), (cs, 1 << (pw - 2))):
        ph = S.nco_phases(pw, n, phase0, fcw, index0, lead)
        ref = c.oracle(ph)
        assert np.array_equal(arr.cpu().numpy().astype(np.int32), ref)
        q.reset()
        q.sine_nco(arr, phase0=phase0 + lead, fcw=fcw, index0=index0)
        check(q.sine_result(), ph, ref, pw, ow, False)
    q.close()


def test_pieces_give_the_bytes_of_one_call_and_reset_forgets():
    import torch
    import cordic_amd as ca
    from gpu_util import DEV
    c = S.QuadCore(ca, (-1, 24, 2, 32))
    phase0, index0 = 0x1234567, (1 << 32) + 12345
    out = torch.empty(N_NCO, dtype=torch.int32, device=DEV)
    c.h.nco(out, None, phase0=phase0, fcw=FCW, index0=index0)
    q = c.quality(ca)
    q.sine_nco(out, phase0=phase0, fcw=FCW, index0=index0)
    whole = q.sine_result(raw=True)
    q.reset()
    # a first sweep that must leave nothing behind: huge "errors"
    junk = torch.full((1000,), (1 << 23) - 1, dtype=torch.int32, device=DEV)
    q.sine_nco(junk, phase0=1 << 31, fcw=0, index0=0)
    assert q.sine_result()["max_err"] > 1e6
    q.reset()
    cuts = [0, 1, 4100, N_NCO]              # three ragged pieces: 1, 4099, rest
    for a, b in zip(cuts, cuts[1:]):
        q.sine_nco(out[a:b], phase0=phase0, fcw=FCW, index0=index0 + a)
    pieces = q.sine_result(raw=True)
    assert len(whole) == 72 and pieces == whole
    q.close()


def test_an_8_lsb_excess_at_one_sample_is_found_and_fails(quad13):
    import cordic_amd as ca
    c = quad13["core"]
    at = 123457
    bad = quad13["out"].clone()
    bad[at] += 8
    q = c.quality(ca)
    q.sine(quad13["dph"], bad)
    got = q.sine_result()
    # the altered sample is off by at least 8 minus its own error, a 7-LSB
    # excess, which is above |TBL_ERR| + 2 for this core, while every other
    # sample is below it: the maximum is there and the core fails
    clean = S.sine_err(c.pw, c.ow, quad13["ph"], quad13["ref"])
    assert 8.0 - clean[at] > abs(got["tbl_err"]) + 2.0
    assert got["tbl_err"] == c.h.tbl_err and abs(got["tbl_err"]) + 2.0 < 7.0
    assert np.delete(clean, at).max() < abs(got["tbl_err"]) + 2.0
    assert got["max_err_index"] == at
    assert got["max_err_phase"] == int(quad13["ph"][at])
    assert got["pass"] == 0 and got["judged"] == 1
    q.close()


def test_refusals(quad13):
    import ctypes as C
    import torch
    import cordic_amd as ca
    from gpu_util import DEV
    L = ca.lib()
    ph, out = quad13["dph"], quad13["out"]
    st = torch.cuda.current_stream().cuda_stream
    p2r = ca.Quality(ca.Config.from_cli(ca.P2R, 13, 13, 2))
    sine = quad13["core"].quality(ca)
    n = 64
    a, b = ph.data_ptr(), out.data_ptr()
    assert L.cordic_quality_sine(p2r._h, n, a, b, st) == ca.ERR_ARGS
    assert L.cordic_quality_sine_nco(p2r._h, n, 0, 1, 0, b, st) == ca.ERR_ARGS
    assert L.cordic_quality_p2r(sine._h, n, None, None, 4095, 0, a, b, b, st) == ca.ERR_ARGS
    assert L.cordic_quality_nco(sine._h, n, 0, 1, 0, 4095, 0, b, b, st) == ca.ERR_ARGS
    assert L.cordic_quality_r2p(sine._h, n, b, b, 4095, b, a, st) == ca.ERR_ARGS
    # n == 0: CORDIC_OK, the pointers are not looked at
    assert L.cordic_quality_sine(sine._h, 0, None, None, st) == 0
    assert L.cordic_quality_sine_nco(sine._h, 0, 0, 1, 0, None, st) == 0
    # nothing fed yet
    from cordic_amd._native import _CSineQuality
    r = _CSineQuality()
    assert L.cordic_quality_sine_result(sine._h, C.byref(r)) == ca.ERR_ARGS
    # the 16-bit forms on a core with OW > 16
    wide = ca.Quality.for_quad(ca.Quad(ow=24, pw=32, device=False))
    v16 = torch.zeros(n, dtype=torch.int16, device=DEV)
    assert L.cordic_quality_sine16(wide._h, n, a, v16.data_ptr(), st) == ca.ERR_CONTAINER
    assert L.cordic_quality_sine_nco16(wide._h, n, 0, 1, 0, v16.data_ptr(), st) == ca.ERR_CONTAINER
    for h in (p2r, sine, wide):
        h.close()
