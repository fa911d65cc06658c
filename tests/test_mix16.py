"""The data-fed single calls on int16 arrays: cordic_mix16 / cordic_plan_mix16
(fused NCO mixer) and cordic_plan_p2r16.  Bit for bit the oracle's values --
O.mix: phases (phase0 + (index0 + i) * fcw) mod 2^PW -- narrowed to int16,
which is the whole value because the ports fit; on the vector kernel of
cordic_p2r16 at any element offset."""
import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
N = (1 << 18) + 3


def dev16(a, offset=0):
    """int16 device view `offset` elements past an aligned allocation"""
    a = np.ascontiguousarray(a).view(np.int16)
    t = torch.zeros(a.size + offset + 8, dtype=torch.int16, device=DEV)
    v = t[offset:offset + a.size]
    v.copy_(torch.from_numpy(a).to(DEV))
    return v


def out16(n, offset=0):
    return torch.zeros(n + offset + 8, dtype=torch.int16,
                       device=DEV)[offset:offset + n]


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV)


def both(mode, iw, ow, xtra=2, pw=-1, ns=-1):
    return (ca.Config.from_cli(mode, iw, ow, xtra, pw, ns),
            O.config_cli(mode, iw, ow, xtra, pw, ns))


def iq16(rng, iw, n):
    """full-range samples, the extremes first (tests/test_gpu_io16.py: rand16)"""
    lo, hi = -(1 << (iw - 1)), (1 << (iw - 1))
    x = rng.randint(lo, hi, n).astype(np.int16)
    y = rng.randint(lo, hi, n).astype(np.int16)
    ext = [lo, hi - 1, 0, -1, 1]
    k = 0
    for a in ext:
        for b in ext:
            x[k], y[k] = a, b
            k += 1
    return x, y


def ncos(pw, index0):
    """(phase0, fcw) pairs: unrelated phases, and a walk along the octant
    boundaries -- sample i has phase i * 2^(PW-3) + i - 1: one below the
    boundary, on it, one above, two above ... octant after octant"""
    mask = (1 << pw) - 1
    q = 1 << (pw - 3)
    fcw = (q + 1) & mask
    return [(0x2545F491 & mask, (0x9E3779B1 & mask) | 1),
            ((-1 - index0 * fcw) & mask, fcw)]


MIX16 = {
    "pw16": (ca.P2R, 16, 16, 2, 16, -1),
    "pw24": (ca.P2R, 16, 16, 2, 24, -1),
    "pw32": (ca.P2R, 16, 16, 2, 32, -1),
    "i12o14": (ca.P2R, 12, 14, 3, 20, -1),
    "i16o8": (ca.P2R, 16, 8, 2, 12, 10),
    "seq": (ca.SP2R, 16, 16, 2, 16, 16),
}
INDEX0 = (1 << 33) + 12345


def test_the_cores_are_the_ones_the_vector_kernel_serves():
    want = {"pw16": 13, "pw24": 19, "pw32": 19, "i12o14": 17}
    for name, args in MIX16.items():
        cfg = ca.Config.from_cli(*args)
        assert 18 <= cfg.ww <= 19 and not cfg.needs_wrap, name
        if name in want:
            assert cfg.nstages == want[name], (name, cfg.nstages)


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("name", sorted(MIX16))
def test_mix16_matches_oracle(name, offset):
    cfg, ocfg = both(*MIX16[name])
    plan = ca.Plan(cfg)
    rng = np.random.RandomState(71)
    x, y = iq16(rng, cfg.iw, N)
    dx, dy = dev16(x, offset), dev16(y, offset)
    x32, y32 = dev32(x), dev32(y)
    for ph0, fcw in ncos(cfg.pw, INDEX0):
        rx, ry = O.mix(ocfg, ph0, fcw, INDEX0, x.astype(np.int32), y.astype(np.int32))
        assert min(rx.min(), ry.min()) >= -32768 and max(rx.max(), ry.max()) <= 32767
        for runner in (lambda *a, **k: ca.mix(cfg, *a, **k), plan.mix):
            ox, oy = out16(N, offset), out16(N, offset)
            runner(ph0, fcw, INDEX0, dx, dy, ox, oy, n=N)
            torch.cuda.synchronize()
            assert ca.last_kernel() == ca.KERNEL_UNROLLED
            assert np.array_equal(ox.cpu().numpy(), rx.astype(np.int16))
            assert np.array_equal(oy.cpu().numpy(), ry.astype(np.int16))
        # the same samples through cordic_mix on int32 arrays
        o32x, o32y = torch.zeros_like(x32), torch.zeros_like(y32)
        ca.mix(cfg, ph0, fcw, INDEX0, x32, y32, o32x, o32y)
        torch.cuda.synchronize()
        assert torch.equal(o32x.to(torch.int16), ox)
        assert torch.equal(o32y.to(torch.int16), oy)
    plan.close()


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("name", ["pw16", "i16o8", "seq"])
def test_plan_p2r16_is_p2r16(name, offset):
    cfg, ocfg = both(*MIX16[name])
    plan = ca.Plan(cfg)
    rng = np.random.RandomState(72)
    x, y = iq16(rng, cfg.iw, N)
    ph = rng.randint(0, 1 << cfg.pw, N).astype(np.uint16)
    q = 1 << (cfg.pw - 3)
    for j, e in enumerate([(i * q + d) & ((1 << cfg.pw) - 1) for i in range(9)
                           for d in (-1, 0, 1)]):
        ph[30 + j] = e
    rx, ry = O.rotate(ocfg, x.astype(np.int32), y.astype(np.int32), ph.astype(np.uint32))
    dx, dy, dph = dev16(x, offset), dev16(y, offset), dev16(ph, offset)
    ax, ay, bx, by = (out16(N, offset) for _ in range(4))
    plan.p2r(dx, dy, dph, ax, ay, n=N)
    torch.cuda.synchronize()
    assert ca.last_kernel() == ca.KERNEL_UNROLLED
    ca.p2r(cfg, dx, dy, dph, bx, by, n=N)
    torch.cuda.synchronize()
    assert torch.equal(ax, bx) and torch.equal(ay, by)
    assert np.array_equal(ax.cpu().numpy(), rx.astype(np.int16))
    assert np.array_equal(ay.cpu().numpy(), ry.astype(np.int16))
    plan.close()


def test_unit_gain_mixer_on_16bit_containers():
    base, ocfg = both(*MIX16["pw32"])
    cfg = base.with_flags(ca.FLAG_UNIT_GAIN)
    k = ca.lib().cordic_config_gain_annihilator(cfg.ref)
    rng = np.random.RandomState(73)
    x, y = iq16(rng, 16, N)

    def scaled(a):
        return ((a.astype(np.int64) * k) >> 32).astype(np.int16)
    plan = ca.Plan(cfg)
    for ph0, fcw in ncos(32, INDEX0):
        rx, ry = O.mix(ocfg, ph0, fcw, INDEX0, x.astype(np.int32), y.astype(np.int32))
        for runner in (lambda *a, **k: ca.mix(cfg, *a, **k), plan.mix):
            ox, oy = out16(N, 1), out16(N, 3)
            runner(ph0, fcw, INDEX0, dev16(x, 3), dev16(y, 1), ox, oy, n=N)
            torch.cuda.synchronize()
            assert ca.last_kernel() == ca.KERNEL_UNROLLED
            assert np.array_equal(ox.cpu().numpy(), scaled(rx))
            assert np.array_equal(oy.cpu().numpy(), scaled(ry))
    plan.close()


def test_container_rule_of_the_plan_forms():
    t = out16(64)
    p17 = ca.Plan(ca.Config.from_cli(ca.P2R, 16, 16, 2, 17, 16))
    with pytest.raises(ca.CordicError) as e:        # reads a phase array
        p17.p2r(t, t, t, t, t, n=16)
    assert e.value.status == ca.ERR_CONTAINER
    p17.mix(1, 3, 0, t[:16], t[16:32], t[32:48], t[48:], n=16)   # PW-bit scalars
    p32 = ca.Plan(ca.Config.from_cli(ca.P2R, 16, 16, 2, 32, -1))
    p32.mix(1, 3, 0, t[:16], t[16:32], t[32:48], t[48:], n=16)
    torch.cuda.synchronize()
    for iw, ow in ((17, 16), (16, 17)):
        with pytest.raises(ca.CordicError) as e:
            ca.Plan(ca.Config.from_cli(ca.P2R, iw, ow, 2, 16, 16)).mix(
                1, 3, 0, t[:16], t[16:32], t[32:48], t[48:], n=16)
        assert e.value.status == ca.ERR_CONTAINER
    # mixed widths are refused before the library sees them
    w = torch.zeros(16, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError):
        p32.mix(1, 3, 0, t[:16], t[16:32], w, t[48:], n=16)
    with pytest.raises(TypeError):
        ca.mix(p32.cfg, 1, 3, 0, w, t[16:32], t[32:48], t[48:], n=16)
