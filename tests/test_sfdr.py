"""cordic_sfdr (include/cordic_amd.h): the device fp64 FFT against numpy, the
two load forms, and the benches' SFDR end to end (bench/cpp/cordic_tb.cpp
:340-371, bench/cpp/quadtbl_tb.cpp:185-219)."""
import numpy as np
import pytest

import oracle_lib as O
import quality as Q
import sine_quality as S

pytestmark = pytest.mark.gpu

# The transform has no size thresholds of its own: one launch per radix-4 stage
# and one radix-2 stage when lgn is odd, so the paths are "radix-2 only" (1),
# "radix-4 only" (2, 4, 10) and "both" (3, 5, 11, 13).  What does change with
# size is the launch: a block holds 256 work items (several blocks from lgn 9
# / 10 / 11 on) and the grid stops at 8 blocks per CU -- 2^19 items on the 256
# CUs of an MI355X -- beyond which the kernels stride.  lgn 19 is the last size
# at which nothing strides, at 20 the load and the spur search do, at 21 the
# radix-2 stage, at 22 the radix-4 stages.
LGNS = [1, 2, 3, 4, 5, 10, 11, 13, 19, 20, 21, 22]


def random_iq(lgn):
    rng = np.random.default_rng(1000 + lgn)
    n = 1 << lgn
    return (rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32),
            rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32))


@pytest.mark.parametrize("lgn", LGNS)
def test_transform_against_numpy(lgn):
    import cordic_amd as ca
    from gpu_util import dev_i32
    re, im = random_iq(lgn)
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    want = np.fft.fft(x)
    s = ca.Sfdr(lgn)
    s.load_iq(dev_i32(re), dev_i32(im))
    r = s.run()
    got = s.bins()
    n = 1 << lgn
    worst = np.abs(got - want).max()
    bound = 1e-12 * np.sqrt(n * np.sum(np.abs(x) ** 2))
    print("lgn %d: max |X_dev - X_np| = %.3g, bound %.3g (ratio %.3g)"
          % (lgn, worst, bound, worst / bound))
    assert worst <= bound
    # the reduction: bin 1 and the largest other bin
    p = np.abs(got) ** 2
    assert r["n"] == n
    assert r["master"] == pytest.approx(p[1], rel=1e-14)
    others = np.delete(p, 1)
    assert r["spur"] == pytest.approx(others.max(), rel=1e-14)
    assert r["spur_bin"] != 1
    assert p[r["spur_bin"]] == pytest.approx(others.max(), rel=1e-14)
    assert r["sfdr_dbc"] == pytest.approx(10 * np.log10(r["master"] / r["spur"]),
                                          abs=1e-9)
    # a slice of the bins
    if lgn >= 4:
        assert np.array_equal(s.bins(3, 7), got[3:10])
    s.close()


def test_ragged_pieces_out_of_order_give_the_bits_of_one_load():
    import cordic_amd as ca
    from gpu_util import dev_i32
    lgn = 13
    re, im = random_iq(lgn)
    dre, dim = dev_i32(re), dev_i32(im)
    s = ca.Sfdr(lgn)
    s.load_iq(dre, dim)
    s.run()
    whole = s.bins()
    cuts = [0, 1, 4100, 4101, 1 << lgn]
    order = [2, 0, 3, 1]
    for k in order:
        a, b = cuts[k], cuts[k + 1]
        s.load_iq(dre[a:b], dim[a:b], index0=a)
    s.run()
    assert np.array_equal(s.bins().view(np.uint64), whole.view(np.uint64))
    s.close()


def test_load_sine_places_the_cores_own_quadrature_pair():
    import cordic_amd as ca
    from gpu_util import dev_i32
    lgn, n = 4, 16
    ramp = np.arange(n, dtype=np.int32)
    k = np.arange(n)
    x = ramp[(k + n // 4) & (n - 1)].astype(np.float64) + 1j * ramp
    assert np.array_equal(x, S.sine_spectrum_input(ramp))
    want = np.fft.fft(x)
    s = ca.Sfdr(lgn)
    d = dev_i32(ramp)
    s.load_sine(d[5:], index0=5)            # in two pieces, the later first
    s.load_sine(d[:5], index0=0)
    s.run()
    got = s.bins()
    assert np.abs(got - want).max() <= 1e-12 * np.sqrt(n * np.sum(np.abs(x) ** 2))
    s.close()


def check_sfdr(r, want_db, spectrum):
    master, spur = S.spur(spectrum)
    print("SFDR dev %.6f dBc, host %.6f dBc; spur bin %d"
          % (r["sfdr_dbc"], want_db, r["spur_bin"]))
    assert abs(r["sfdr_dbc"] - want_db) < 0.01
    assert r["spur_bin"] != 1
    # bins k and N - k can tie to rounding
    assert abs(spectrum[r["spur_bin"]]) ** 2 == pytest.approx(spur, rel=1e-6)
    assert r["master"] == pytest.approx(master, rel=1e-9)


def test_sfdr_of_the_quadratic_core_o13_p18():
    import torch
    import cordic_amd as ca
    from gpu_util import DEV, to_np
    c = S.QuadCore(ca, (-1, 13, 2, 18))
    n = 1 << c.pw
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    c.h.nco(out, None)                      # phase0 0, fcw 1: the full ramp
    ref = c.oracle(np.arange(n, dtype=np.uint32))
    assert np.array_equal(to_np(out), ref)
    k = np.arange(n)
    want = Q.sfdr_dbc(ref[(k + n // 4) & (n - 1)], ref)
    s = ca.Sfdr(c.pw)
    s.load_sine(out)
    check_sfdr(s.run(), want, np.fft.fft(S.sine_spectrum_input(ref)))
    s.close()


def test_sfdr_of_the_rotator_i13_o13_x2():
    import cordic_amd as ca
    from gpu_util import dev_i32, gpu_p2r
    c = O.config_cli(O.P2R, 13, 13, 2)
    cfg = ca.Config.from_cli(ca.P2R, 13, 13, 2)
    ph, x0, y0 = Q.p2r_bench_inputs(c.iw, c.pw)
    rx, ry = O.rotate(c, x0, y0, ph)
    ox, oy = gpu_p2r(cfg, x0, y0, ph)
    assert np.array_equal(ox, rx) and np.array_equal(oy, ry)
    lgn = c.pw
    s = ca.Sfdr(lgn)
    s.load_iq(dev_i32(ox), dev_i32(oy))
    check_sfdr(s.run(), Q.sfdr_dbc(rx, ry),
               np.fft.fft(rx.astype(np.float64) + 1j * ry))
    s.close()


def test_sfdr_of_the_plain_table_p10():
    import torch
    import cordic_amd as ca
    from gpu_util import DEV, to_np
    c = S.TableCore(ca, ca.TBL, 12, 10)
    n = 1 << c.pw
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    c.h.nco(out, None)
    ref = c.oracle(np.arange(n, dtype=np.uint32))
    assert np.array_equal(to_np(out), ref)
    k = np.arange(n)
    s = ca.Sfdr(c.pw)
    s.load_sine(out)
    check_sfdr(s.run(), Q.sfdr_dbc(ref[(k + n // 4) & (n - 1)], ref),
               np.fft.fft(S.sine_spectrum_input(ref)))
    s.close()


def test_refusals():
    import ctypes as C
    import torch
    import cordic_amd as ca
    from cordic_amd._native import _CSfdrResult
    from gpu_util import DEV
    L = ca.lib()
    st = torch.cuda.current_stream().cuda_stream
    s = ca.Sfdr(6)
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = z.data_ptr()
    r = _CSfdrResult()
    out = np.empty(64, dtype=np.complex128)
    # nothing transformed yet
    assert L.cordic_sfdr_bins(s._h, 0, 1, out.ctypes.data) == ca.ERR_ARGS
    # a range past 2^lgn
    assert L.cordic_sfdr_load_iq(s._h, 64, 1, p, p, st) == ca.ERR_ARGS
    assert L.cordic_sfdr_load_iq(s._h, 65, 0, p, p, st) == ca.ERR_ARGS
    assert L.cordic_sfdr_load_sine(s._h, 1, 64, p, st) == ca.ERR_ARGS
    assert L.cordic_sfdr_load_sine(s._h, 2, (1 << 64) - 1, p, st) == ca.ERR_ARGS
    # run before the last sample is there
    assert L.cordic_sfdr_run(s._h, C.byref(r), st) == ca.ERR_ARGS
    assert L.cordic_sfdr_load_iq(s._h, 63, 0, p, p, st) == 0
    assert L.cordic_sfdr_run(s._h, C.byref(r), st) == ca.ERR_ARGS
    assert L.cordic_sfdr_load_iq(s._h, 0, 64, None, None, st) == 0     # n == 0
    assert L.cordic_sfdr_load_iq(s._h, 1, 63, p, p, st) == 0
    assert L.cordic_sfdr_run(s._h, None, st) == ca.ERR_ARGS
    assert L.cordic_sfdr_run(s._h, C.byref(r), st) == 0
    assert r.n == 64
    assert L.cordic_sfdr_bins(s._h, 60, 5, out.ctypes.data) == ca.ERR_ARGS
    assert L.cordic_sfdr_bins(s._h, 0, 64, out.ctypes.data) == 0
    assert not out.any()                    # the transform of zeros
    # the samples were consumed: a second run wants a second sweep
    assert L.cordic_sfdr_run(s._h, C.byref(r), st) == ca.ERR_ARGS
    s.close()
