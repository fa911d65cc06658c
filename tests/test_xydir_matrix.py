"""Every instance and every port geometry of the per-sample-vector rotator with
looked-up directions (cordic_xydir.h: rotator_xydir<LJ, N>, its tile-reading
form and fm_mix_xydir<LJ, N> of cordic_fm_mix.hip) against the oracle, bit for
bit: integer arithmetic, no tolerance.

The inputs put a residual phase of exactly -1, 0 and +1 in front of EVERY
stage -- the fold's, the looked-up ones and those that recur on what the last
group leaves -- in all four quadrants, under extreme and ordinary vectors, with
junk above the port widths, at lengths that are no multiple of 4 and in arrays
that start 1, 2 and 3 words behind a 16-byte boundary."""
import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O

INSTANCES = (13, 16, 19, 20, 24, 27, 29)    # tile-reading and fm_mix instances
JOB_SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1027, 8191, 8193, 12]
OFFS = dict(x=1, y=2, phase=3, out=1)       # words behind a 16-byte boundary
POOL = 997      # vectors cycled over the tie phases: a prime, so that the 36
                # extreme pairs in front of them meet every stage and quadrant


# ------------------------------------------------ shared inputs (numpy only)

def split(n):
    """stages per looked-up group of an n-stage core: stage 1 is the fold's,
    at most 24 more are looked up, in the fewest groups of at most 5, the
    larger ones last (a restatement of cordic_internal.h: dx_size)"""
    c = min(n - 1, 24)
    g = -(-c // 5)
    return [c // g + (i >= g - c % g) for i in range(g)]


def tie_walks(angle, pw, nlive, walks=64, seed=1):
    """Per stage k = 0 .. nlive - 1 the folded phases (PW-bit units, signed)
    that leave a residual of exactly 0 in front of stage k: from 0, walk back
    through the stages i = k-1 .. 0 with a random direction s, q = p + s
    angle[i], kept where the recurrence (rtl/cordic.v:262-280) would have
    taken that direction on q, else with the other direction, else dropped."""
    rng = np.random.RandomState(seed)
    ang = [int(a) for a in angle[:nlive]]
    lim = 1 << (pw - 3)
    out = []
    for k in range(nlive):
        p = np.zeros(walks, dtype=np.int64)
        alive = np.ones(walks, dtype=bool)
        for i in range(k - 1, -1, -1):
            s = np.where(rng.randint(0, 2, walks) == 1, 1, -1).astype(np.int64)
            q = p + s * ang[i]
            ok = (q >= 0) == (s > 0)
            q2 = p - s * ang[i]
            ok2 = (q2 >= 0) == (s < 0)
            p = np.where(ok, q, np.where(ok2, q2, p))
            alive &= ok | ok2
        out.append(p[alive & (p >= -lim + 2) & (p < lim - 2)])
    return out


def tie_folded(angle, pw, nlive, walks=64, seed=1):
    """the walks' phases + d, d = -2 .. 2, of all stages in one array"""
    return np.concatenate([(p[:, None] + np.arange(-2, 3)[None, :]).ravel()
                           for p in tie_walks(angle, pw, nlive, walks, seed)])


def tie_ports(folded, pw):
    """the folded phases in all four quadrants as port phases (uint32 below
    2^PW), then the fold's own edges (2j + 1) 2^(PW-3) + d"""
    quad = (np.arange(4, dtype=np.int64) << (pw - 2))[None, :]
    ph = (folded[:, None] + quad).ravel()
    edges = [(2 * j + 1) * (1 << (pw - 3)) + d for j in range(4) for d in range(-2, 3)]
    ph = np.concatenate([ph, np.array(edges, dtype=np.int64)])
    return (ph & ((1 << pw) - 1)).astype(np.uint32)


def fold(ports, pw):
    """the octant fold of cordic_xydir.h on port phases: the signed phase left
    within +/- 45 degrees of its quadrant's axis"""
    t = (ports.astype(np.int64) + (1 << (pw - 3))) & ((1 << pw) - 1)
    return (t & ((1 << (pw - 2)) - 1)) - (1 << (pw - 3))


def residuals_met(angle, pw, nlive, ports):
    """per stage k, which of the residuals -1, 0, +1 the forward recurrence
    meets in front of it on these port phases: [nlive][3] booleans"""
    p = fold(ports, pw)
    met = []
    for k in range(nlive):
        met.append([bool((p == d).any()) for d in (-1, 0, 1)])
        a = int(angle[k])
        p = np.where(p >= 0, p - a, p + a)
    return met


def sext(a, w):
    s = 32 - w
    return (a.astype(np.int32) << s) >> s


def make_inputs(cfg, ocfg, seed):
    """dict(ties: port tie phases; x, y, ph: what the device reads; wx, wy,
    wph: the same as the ports take them (sign-extended from IW, masked to
    PW), which is what the oracle is fed).  Ties first, under POOL vectors
    cycled, then at least 8192 random samples, then 3 more: n % 4 == 3."""
    from test_gpu_parity import rand_inputs
    iw, pw = cfg.iw, cfg.pw
    angle = [int(ocfg.angle[i]) for i in range(cfg.nlive)]
    ties = tie_ports(tie_folded(angle, pw, cfg.nlive), pw)
    met = residuals_met(angle, pw, cfg.nlive, ties)
    assert all(all(m) for m in met), [k for k, m in enumerate(met) if not all(m)]
    rng = np.random.RandomState(seed)
    px, py, _ = rand_inputs(rng, iw, pw, POOL)
    cyc = np.arange(ties.size) % POOL
    nr = 8192 + (-ties.size) % 4 + 3
    rx, ry, rph = rand_inputs(rng, iw, pw, nr)
    x = np.concatenate([px[cyc], rx])
    y = np.concatenate([py[cyc], ry])
    ph = np.concatenate([ties, rph])
    n = ph.size
    assert n % 4 == 3 and n <= 50000
    if iw < 32:     # junk above bit IW-1 of every second x and y
        for a in (x, y):
            junk = rng.randint(0, 1 << (32 - iw), n // 2, dtype=np.int64) << iw
            a[1::2] = ((a[1::2].astype(np.int64) & ((1 << iw) - 1)) | junk) \
                .astype(np.uint32).view(np.int32)
    if pw < 32:     # junk above bit PW-1 of every second phase
        junk = rng.randint(0, 1 << (32 - pw), (n + 1) // 2, dtype=np.int64) << pw
        ph[0::2] = (ph[0::2].astype(np.int64) & ((1 << pw) - 1)) | junk
    return dict(ties=ties, x=x, y=y, ph=ph, wx=sext(x, iw), wy=sext(y, iw),
                wph=ph & np.uint32((1 << pw) - 1), rng=rng)


# ------------------------------------------------ no GPU

def test_the_restated_split():
    assert split(13) == [4, 4, 4] and split(14) == [4, 4, 5]
    assert split(15) == [4, 5, 5] and split(16) == [5, 5, 5]
    assert split(17) == [4, 4, 4, 4] and split(18) == [4, 4, 4, 5]
    assert split(21) == [5, 5, 5, 5] and split(22) == [4, 4, 4, 4, 5]
    assert split(23) == [4, 4, 4, 5, 5] and split(24) == [4, 4, 5, 5, 5]
    for n in range(25, 30):
        assert split(n) == [4, 5, 5, 5, 5]


@pytest.mark.parametrize("args", [(ca.P2R, 32, 32, 2, 32, 29), (ca.P2R, 31, 31, 2, 32, 13),
                                  (ca.P2R, 24, 24, 2, 20, 20), (ca.P2R, 16, 16, 2, 16, 16),
                                  (ca.P2R, 5, 32, 2, 32, 20)])
def test_the_inputs_are_what_they_claim(args):
    """-1, 0 and +1 in front of every stage (asserted inside), junk only above
    the ports, and the oracle's view free of it"""
    cfg, ocfg = ca.Config.from_cli(*args), O.config_cli(*args)
    inp = make_inputs(cfg, ocfg, 5)
    n = inp["ph"].size
    # 64 walks of 5 phases per stage in 4 quadrants, less the walks that end
    # beyond 45 degrees, and the fold's 20 edges
    assert 3 * 320 * cfg.nlive < inp["ties"].size - 20 <= 4 * 320 * cfg.nlive
    assert np.array_equal(inp["ph"][:inp["ties"].size] & np.uint32((1 << cfg.pw) - 1),
                          inp["ties"])
    lo, hi = -(1 << (cfg.iw - 1)), (1 << (cfg.iw - 1)) - 1
    for w in (inp["wx"], inp["wy"]):
        assert w.min() == lo and w.max() == hi and w.size == n
    if cfg.iw < 32:
        assert not np.array_equal(inp["x"][1::2], inp["wx"][1::2])
        assert np.array_equal(inp["x"][0::2], inp["wx"][0::2])
    if cfg.pw < 32:
        nt = inp["ties"].size   # (the random phases behind are 32-bit anyway)
        assert not np.array_equal(inp["ph"][0:nt:2], inp["wph"][0:nt:2])
        assert np.array_equal(inp["ph"][1:nt:2], inp["wph"][1:nt:2])
    # a stage's ties are consecutive samples, about as many as the pool has
    # vectors: nearly every stage meets nearly every one of the 36 extreme pairs
    assert inp["ties"].size // cfg.nlive > POOL * 3 // 4


# ------------------------------------------------ GPU

def _padded(torch, n, off, src=None):
    from test_fm_demod import Padded
    return Padded(torch, n, off, src=None if src is None else src.view(np.int32))


def _rotate(torch, plan, x, y, ph):
    """cordic_plan_p2r on arrays at OFFS with guard words around: the outputs,
    after checking the guards and that the inputs are intact"""
    n = ph.size
    dx, dy = _padded(torch, n, OFFS["x"], x), _padded(torch, n, OFFS["y"], y)
    dp = _padded(torch, n, OFFS["phase"], ph)
    ox, oy = _padded(torch, n, OFFS["out"]), _padded(torch, n, OFFS["out"])
    plan.p2r(dx.view, dy.view, dp.view, ox.view, oy.view, n=n)
    torch.cuda.synchronize()
    kernel = ca.last_kernel()
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    assert np.array_equal(dp.get().view(np.uint32), ph)
    return ox.get(), oy.get(), kernel


def _mixer(torch, plan, phase0, fcw, index0, x, y):
    n = x.size
    dx, dy = _padded(torch, n, OFFS["x"], x), _padded(torch, n, OFFS["y"], y)
    ox, oy = _padded(torch, n, OFFS["out"]), _padded(torch, n, OFFS["out"])
    plan.mix(phase0, fcw, index0, dx.view, dy.view, ox.view, oy.view, n=n)
    torch.cuda.synchronize()
    kernel = ca.last_kernel()
    assert np.array_equal(dx.get(), x) and np.array_equal(dy.get(), y)
    return ox.get(), oy.get(), kernel


def check_p2r(torch, cfg, ocfg, plan, inp, family):
    gx, gy, kernel = _rotate(torch, plan, inp["x"], inp["y"], inp["ph"])
    assert kernel == family, kernel
    wx, wy = O.rotate(ocfg, inp["wx"], inp["wy"], inp["wph"])
    bad = np.flatnonzero((gx != wx) | (gy != wy))
    assert bad.size == 0, (bad.size, bad[:8], inp["wph"][bad[:8]])


def check_mix(torch, cfg, ocfg, plan, inp):
    """the phase ramp through a tie of the deepest looked-up stage, upwards
    one unit per sample from 2048 below it with an index that wraps 2^32, the
    same with the word -1, downwards through the same tie, and a random odd
    word on 8195 samples"""
    pw, rng = cfg.pw, inp["rng"]
    deep = min(cfg.nlive - 1, 24)
    angle = [int(ocfg.angle[i]) for i in range(cfg.nlive)]
    tie = int(tie_walks(angle, pw, cfg.nlive)[deep][0])
    p = tie
    for k in range(deep):
        p = p - angle[k] if p >= 0 else p + angle[k]
    assert p == 0
    mask = (1 << pw) - 1
    odd = int(rng.randint(0, 1 << 31)) * 2 + 1
    cases = [(tie - 2048, 1, (1 << 32) - 1000, 4099),
             (tie - 2048, mask, (1 << 32) - 1000, 4099),
             (tie + 2048 - 1000, mask, (1 << 32) - 1000, 4099),
             (int(rng.randint(0, 1 << 31)), odd & mask, int(rng.randint(0, 1 << 31)), 8195)]
    for phase0, fcw, index0, n in cases:
        phase0 &= mask
        gx, gy, kernel = _mixer(torch, plan, phase0, fcw, index0, inp["x"][:n],
                                inp["y"][:n])
        assert kernel == ca.KERNEL_DIRECTIONS, (kernel, fcw)
        wx, wy = O.mix(ocfg, phase0, fcw, index0, inp["wx"][:n], inp["wy"][:n])
        assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (phase0, fcw, n)


def check_jobsets(torch, cfg, ocfg, plan, inp, family):
    """job sets of both data-fed kinds over JOB_SIZES, the phases of the two
    longest P2R_XY jobs replaced by tie phases; returns the families reported"""
    import test_jobset_fused as F
    from gpu_util import dev_i32
    ties, rng = inp["ties"], inp["rng"]
    seen = []
    for kind in (ca.JOBS_P2R_XY, ca.JOBS_MIX):
        jobs, host, outs, bigs = F._ragged_set(kind, cfg, 71 + kind, JOB_SIZES)
        if kind == ca.JOBS_P2R_XY:
            perm, at = rng.permutation(ties.size), 0
            for k in sorted(range(len(jobs)), key=lambda k: -jobs[k]["n"])[:2]:
                n = jobs[k]["n"]
                tp = ties[perm[np.arange(at, at + n) % ties.size]]
                at += n
                jobs[k]["phase"].copy_(dev_i32(tp))
                host[k] = (host[k][0], host[k][1], tp)
        js = ca.Jobset(plan, kind, jobs)
        for b in bigs:
            b.fill_(0x5a5a5a5a)
        js.run()
        torch.cuda.synchronize()
        assert js.path == ca.JOBS_PATH_FUSED, kind
        seen.append(ca.last_kernel())
        if family is not None:
            assert seen[-1] == family, (kind, seen[-1])
        F._check_outputs(kind, ocfg, jobs, host, outs, None, kind)
        total = sum(jb["n"] for jb in jobs)
        for b in bigs:              # guard words and gaps untouched
            assert int((b == 0x5a5a5a5a).sum().item()) == b.numel() - total
        js.close()
    ca.jobset_reap()
    return seen


def check_fm_mix(torch, cfg, ocfg, plan, inp):
    """cordic_plan_fm_mix on the fused kernel around its tile size with random
    words, and rotating by exactly the tie set"""
    from test_fm_demod import last_value, last_word
    from test_fm_mix import PHASE0, PRESET, run, work_buffer
    from test_table_fm import expected as phases, words
    fused, T = plan.fm_mix_info()
    assert fused == 1 and T > 0
    mask = np.uint32((1 << cfg.pw) - 1)

    def check(fcw, pm, n, preset, tag):
        x, y = inp["x"][:n], inp["y"][:n]
        p, final = phases(fcw, pm, PHASE0, preset or 0)
        wx, wy = O.rotate(ocfg, inp["wx"][:n], inp["wy"][:n], p & mask)
        acc = None if preset is None else last_word(torch, preset)
        gx, gy = run(torch, plan, work_buffer(torch, plan, n), fcw, pm, x, y, PHASE0,
                     acc)
        assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (tag, n)
        assert acc is None or last_value(acc) == final, (tag, n)

    for n in (T - 1, T + 1, 2 * T + 3):
        fcw = words("random", n, 40 + n % 7)
        for pm in (None, words("random", n, 50 + n % 5)):
            check(fcw, pm, n, PRESET, "random")
            check(fcw, pm, n, None, "random, no accumulator word")
    ties = inp["ties"]
    n = ties.size + 3
    fcw = words("random", n, 44)
    p0, _ = phases(fcw, None, PHASE0, PRESET)
    want = np.concatenate([ties, ties[:3]])
    with np.errstate(over="ignore"):
        pm = want - p0
    check(fcw, pm, n, PRESET, "ties")


def exercise(args, expect, family=ca.KERNEL_DIRECTIONS, seed=0, sets_anyway=False):
    """One core through every call that reaches the family.  expect: values of
    the configuration, asserted first; family: what cordic_plan_p2r must
    report; sets_anyway: job sets also where the stage count has no
    tile-reading instance (the family they report is printed, not asserted)."""
    import torch
    cfg, ocfg = ca.Config.from_cli(*args), O.config_cli(*args)
    have = dict(ww=cfg.ww, pw=cfg.pw, nlive=cfg.nlive, in_shl=cfg.ww - cfg.iw - 1,
                r=cfg.ww - cfg.ow)
    for key, value in expect.items():
        assert have[key] == value, (key, have[key], value)
    assert not cfg.needs_wrap
    plan = ca.Plan(cfg)
    assert plan.dir_groups == split(cfg.nlive)
    inp = make_inputs(cfg, ocfg, 100 + seed)
    check_p2r(torch, cfg, ocfg, plan, inp, family)
    fused = plan.fm_mix_info()[0]
    if family != ca.KERNEL_DIRECTIONS:      # a core the launcher refuses
        assert fused == 0
    else:
        check_mix(torch, cfg, ocfg, plan, inp)
        if cfg.nlive in INSTANCES:
            check_jobsets(torch, cfg, ocfg, plan, inp, ca.KERNEL_DIRECTIONS)
            check_fm_mix(torch, cfg, ocfg, plan, inp)
        else:
            assert fused == 0
            if sets_anyway:
                seen = check_jobsets(torch, cfg, ocfg, plan, inp, None)
                print("job sets of %s, %d live stages, report the kernel families %s"
                      % (args[1:], cfg.nlive, seen))
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(13, 30))
@pytest.mark.parametrize("lj", [29, 30])
def test_gpu_every_instance_equals_the_oracle(lj, n):
    """rotator_xydir<LJ, N> for all 34 (LJ, N), and where N has them the
    tile-reading instance and fm_mix_xydir<LJ, N>"""
    args = (ca.P2R, 32, 32, 2, 32, n) if lj == 29 else (ca.P2R, 31, 31, 2, 32, n)
    exercise(args, dict(ww=64 - lj, nlive=n, in_shl=2, r=3), seed=lj * 100 + n,
             sets_anyway=n in (17, 22))


# (iw, ow, xtra): WW, in_shl, r -- mode P2R, PW 32, 20 stages.  Rounding
# branches of the kernel: r + LJ == 32; r + LJ > 32 and r < 31; general
GEOMETRY = [
    ((32, 16, 2), 35, 2, 19),       # LJ 29, second branch, shift 16
    ((32, 5, 2), 35, 2, 30),        # second branch, its last r
    ((32, 4, 2), 35, 2, 31),        # general
    ((32, 3, 2), 35, 2, 32),        # general, r >= 32
    ((16, 32, 2), 35, 18, 3),
    ((5, 32, 2), 35, 29, 3),
    ((4, 32, 2), 35, 30, 3),        # in_shl at its upper edge
    ((32, 32, 1), 34, 1, 2),        # LJ 30, full ports, in_shl at its lower edge
    ((31, 31, 1), 33, 1, 2),
    ((31, 16, 2), 34, 2, 18),       # second branch, shift 16
    ((31, 3, 2), 34, 2, 31),        # general
    ((3, 31, 2), 34, 30, 3),        # second branch
    ((3, 32, 1), 34, 30, 2),
    ((16, 32, 0), 33, 16, 1),       # r = 1: no rounding, general
    ((30, 32, 0), 33, 2, 1),
    ((2, 32, 0), 33, 30, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("ports,ww,in_shl,r", GEOMETRY,
                         ids=["%d-%d-x%d" % g[0] for g in GEOMETRY])
def test_gpu_every_port_geometry_equals_the_oracle(ports, ww, in_shl, r):
    iw, ow, xtra = ports
    exercise((ca.P2R, iw, ow, xtra, 32, 20),
             dict(ww=ww, in_shl=in_shl, r=r, nlive=20, pw=32), seed=iw * 64 + ow)


@pytest.mark.gpu
@pytest.mark.parametrize("args,pw,nlive", [((ca.P2R, 24, 24, 2, 20, 20), 20, 17),
                                           ((ca.P2R, 16, 16, 2, 16, 16), 16, 13)],
                         ids=["pw20", "pw16"])
def test_gpu_narrow_phase_cores_equal_the_oracle(args, pw, nlive):
    """phase words scaled up to 32 bits in the kernel, junk above PW"""
    exercise(args, dict(pw=pw, nlive=nlive), seed=pw, sets_anyway=True)


@pytest.mark.gpu
@pytest.mark.parametrize("ports,ww,in_shl,family", [
    ((32, 32, 0), 33, 0, "unrolled"),       # nothing appended below the input
    ((2, 32, 1), 34, 31, "generic"),        # 2^31 is no 32-bit multiplier
    ((1, 32, 0), 33, 31, "generic"),
], ids=["32-32-x0", "2-32-x1", "1-32-x0"])
def test_gpu_cores_the_launcher_refuses_equal_the_oracle(ports, ww, in_shl, family):
    """the tables exist and the oracle's bits hold: only the launch rule
    1 <= in_shl <= 30 keeps these cores out, and the path queries say so"""
    iw, ow, xtra = ports
    args = (ca.P2R, iw, ow, xtra, 32, 20)
    assert ca.dir_table(ca.Config.from_cli(*args)) is not None
    exercise(args, dict(ww=ww, in_shl=in_shl, nlive=20),
             family=ca.KERNEL_UNROLLED if family == "unrolled" else ca.KERNEL_GENERIC,
             seed=ww + in_shl)
