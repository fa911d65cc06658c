"""Every tile kernel of the data-fed job sets (CORDIC_JOBS_R2P / _P2R_XY / _MIX)
against the oracle: rotator_xy_tiles in its eight containers, topolar_ljw_tiles
at its six widths, topolar_lj_tiles, topolar_narrow_tiles (cordic_jobs_kernels.h,
each with and without unit gain), the four instances on int16 arrays
(cordic_jobs_io16.hip), topolar_lj_jobs in its three instances
(cordic_inst_pol_lj.hip) and the rounding branches, port geometries and stage
counts inside them.

Every row runs the same ragged set twice: on the tiles and the grid that the
library chooses (one pass of 256 vectors a tile at this size, one block a
tile), and with CORDIC_JOBS_TILE_PASSES=8 and CORDIC_JOBS_MAX_BLOCKS=2, where a
tile is eight passes -- the prefetched loads of a pass are handed over to the
next seven times -- and a block walks several tiles of several jobs.  The job
lengths are the edges of both tiles.  Every output word of every job must equal
what the oracle computes for that job alone (unit gain: (o * K) >> 32; int16
arrays: narrowed as Set16.want narrows), and no word outside the jobs' outputs
may change.  The helpers are the job-set tests' own.  Nothing has a tolerance.

Rounding ties are not constructed: with r bits dropped a random register lies
on a tie with probability 2^-r, bit r either way, so the r <= 9 of the rows
below meet each kind some 30 times or more in the 2^15 random samples of a
set.  At r >= 31 ties are not reached; the output there is a few bits.

CORDIC_JOBS_MAX_BLOCKS caps the grid of launch_xy_jobs_fused and
launch_xy_jobs16.  launch_xy_jobs (topolar_lj_jobs and the looked-up-direction
instances of cordic_inst_xydir_*) keeps min(tiles, CUs * 8), see
cordic_jobs_fused.h: on those kernels the rows and sweeps below vary the tile
only, and a block's step to its next tile is reached the other way round --
tiles are cut per job, so a set of more small jobs than the device has
resident blocks, with the long jobs behind them, has more tiles than blocks
and the blocks' second tiles are the long jobs' (crowd below)."""
import collections
import contextlib
import os
import re

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O
import test_jobset as JS
import test_jobset16 as J16
import test_jobset_fused as F
import test_xydir_matrix as XM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")
P2R, SP2R, R2P, SR2P = ca.P2R, ca.SP2R, ca.R2P, ca.SR2P
UG, NT = ca.FLAG_UNIT_GAIN, ca.FLAG_NO_TAILS
FUSED, EACH = ca.JOBS_PATH_FUSED, ca.JOBS_PATH_ONE_BY_ONE
UNROLLED, LEFT, DIRS = ca.KERNEL_UNROLLED, ca.KERNEL_LEFT_JUSTIFIED, ca.KERNEL_DIRECTIONS
KNOBS = ("CORDIC_JOBS_TILE_PASSES", "CORDIC_JOBS_MAX_BLOCKS")
PASS = 1024             # samples of a pass: kJobPassVecs vectors of four
GUARD = 0x5a5a5a5a
BLOCK = 64              # samples of each block of special vectors in a job
FORCED = (8, 2)         # the second setting: passes a tile, blocks


def lengths(P):
    """an empty job, jobs of trailing samples only, a vector, a pass less a
    sample, a pass, a pass and three samples; a tile of P passes one vector
    short, a full one, one that spills a vector into a second tile and two
    samples behind it; three tiles (four of one pass), the last a pass and a
    vector, which a block of a capped grid reaches in its second step"""
    T = PASS * P
    return [0, 1, 3, 4, 5, 1023, 1024, 1027, T - 4, T, T + 6, 2 * T + 1029, 12]


def crowd(blocks, P):
    """more one-tile jobs (one or two vectors, 0 .. 3 samples behind) than a
    grid of `blocks` has blocks, then the jobs of lengths(P): in the table's
    order every tile of the long jobs lies behind tile `blocks`, so it is some
    block's second tile"""
    return [4 + k % 5 for k in range(blocks + 40)] + lengths(P)


# ---------------------------------------------------------------- the matrix
#
# args: (mode, iw, ow, xtra, pw, nstages) of the command line; kind: rot / pol
# (32-bit arrays), rot16 / pol16 (int16 arrays), mix16 (int16, CORDIC_JOBS_MIX
# only); inst: the `lj` that launch_rot_xy_tiles / launch_pol_tiles switch on
# (0: Narrow32), "jobs:20" / "jobs:29" / "jobs:dyn" for topolar_lj_jobs, "dirs"
# for a looked-up-direction instance, None for a set that runs one by one;
# then what Config.from_cli must give.  Rotators: WW = max(iw, ow) + xtra + 1,
# in_shl = WW - iw - 1; converters: WW = max(iw, ow) + 2 (xtra + 2), in_shl =
# WW - iw - 2; r = WW - ow.

Row = collections.namedtuple(
    "Row", "args flags kind path family inst ww in_shl r nlive pw wrap junk_phase")


def row(kind, args, flags, inst, ww, in_shl, r, nlive, pw=32, wrap=False, path=FUSED,
        family=UNROLLED, junk_phase=False):
    return Row(args, flags, kind, path, family, inst, ww, in_shl, r, nlive, pw, wrap,
               junk_phase)


def _rotators():
    rows = []
    for ug in (0, UG):
        # Narrow32: WW 32, wrapping; the second with nothing appended below
        rows.append(row("rot", (P2R, 24, 2, 7, 32, -1), ug, 0, 32, 7, 30, 29, wrap=True))
        rows.append(row("rot", (P2R, 31, 1, 0, 32, 20), ug, 0, 32, 0, 31, 20, wrap=True))
        # WideLJ<30>.  27 stages at WW 27 have a looked-up-direction instance,
        # which unit gain keeps the set off, and FLAG_NO_TAILS where there is
        # none; 17 and 22 stages have no such instance
        rows.append(row("rot", (P2R, 24, 24, 2, -1, -1), ug or NT, 30, 27, 2, 3, 27, pw=31))
        rows.append(row("rot", (P2R, 31, 31, 2, 32, 17), ug, 30, 34, 2, 3, 17))
        rows.append(row("rot", (P2R, 32, 32, 0, 32, 22), ug, 30, 33, 0, 1, 22))  # fold1 false
        # WideLJ<29>
        rows.append(row("rot", (P2R, 32, 32, 2, 32, 17), ug, 29, 35, 2, 3, 17))
        rows.append(row("rot", (P2R, 32, 32, 2, 32, 16), ug | NT, 29, 35, 2, 3, 16))
        # WideLJ<28> .. <24>: no direction tables above WW 35
        for x in range(3, 8):
            rows.append(row("rot", (P2R, 32, 32, x, 32, 20), ug, 31 - x, 33 + x, x, x + 1, 20))
    # the rounding branches of rotator_xy_tiles by r_lj = r + LJ: == 32; > 32
    # with r < 31 (shifts 1 and 15); the general one at r = 31 and at r >= 32
    for ww in range(35, 41):
        n = 17 if ww == 35 else 20
        for ow in (32, 31, 17, ww - 31, 3):
            rows.append(row("rot", (P2R, 32, ow, ww - 33, 32, n), 0, 64 - ww, ww, ww - 33,
                            ww - ow, n))
    rows.append(row("rot", (P2R, 32, 32, 1, 32, 17), 0, 30, 34, 1, 2, 17))     # r_lj == 32
    rows.append(row("rot", (P2R, 31, 16, 2, 32, 17), 0, 30, 34, 2, 18, 17))    # second
    rows.append(row("rot", (P2R, 31, 3, 2, 32, 17), 0, 30, 34, 2, 31, 17))     # general
    rows.append(row("rot", (P2R, 16, 32, 0, 32, 17), 0, 30, 33, 16, 1, 17))    # no rounding
    # edges: in_shl 30 is the last 32-bit multiplier of the fold, 31 is none
    rows.append(row("rot", (P2R, 9, 32, 7, 32, 20), 0, 24, 40, 30, 8, 20))
    rows.append(row("rot", (P2R, 8, 32, 7, 32, 20), 0, None, 40, 31, 8, 20, path=EACH,
                    family=None))
    for n in (1, 2, 12):
        rows.append(row("rot", (P2R, 32, 32, 2, 32, n), 0, 29, 35, 2, 3, n))
        rows.append(row("rot", (P2R, 32, 32, 5, 32, n), 0, 26, 38, 5, 6, n))
    # kDynStages = 40 live stages, and one more
    rows.append(row("rot", (SP2R, 32, 32, 3, 32, 42), 0, 28, 36, 3, 4, 40))
    rows.append(row("rot", (SP2R, 32, 32, 3, 32, 43), 0, None, 36, 3, 4, 41, path=EACH,
                    family=None))
    # PW 20: junk above bit 19 of every second phase word
    rows.append(row("rot", (P2R, 24, 24, 2, 20, 17), 0, 30, 27, 2, 3, 17, pw=20,
                    junk_phase=True))
    return rows


def _converters():
    rows = []
    # topolar_ljw_tiles<64 - WW, UG>; round_hi: r + LJ >= 32 and r <= 31, sh = r + LJ - 32
    for ww, iw, x in ((35, 31, 0), (36, 32, 0), (37, 31, 1), (38, 32, 1), (39, 31, 2),
                      (40, 32, 2)):
        lj, shl = 64 - ww, ww - iw - 2
        for ug in (0, UG):
            rows.append(row("pol", (R2P, iw, iw, x, 32, 24), ug, lj, ww, shl, ww - iw, 24,
                            family=LEFT))
        for ow in (16, ww - 31, ww - 32):      # sh = 16; r = 31, the last round_hi; r = 32
            rows.append(row("pol", (R2P, iw, ow, x, 32, 24), 0, lj, ww, shl, ww - ow, 24,
                            family=LEFT))
        # a 16-bit input port under the full output port: up = 16
        rows.append(row("pol", (R2P, 16, iw, x, 32, 24), 0, lj, ww, ww - 18, ww - iw, 24,
                        family=LEFT))
    # topolar_lj_tiles<true>: unit gain at WW <= 34
    rows.append(row("pol", (R2P, 24, 24, 2, -1, 20), UG, 30, 32, 6, 8, 20, family=LEFT))
    rows.append(row("pol", (R2P, 25, 25, 2, 32, 20), UG, 30, 33, 6, 8, 20, family=LEFT))
    rows.append(row("pol", (R2P, 26, 26, 2, 32, 24), UG, 30, 34, 6, 8, 24, family=LEFT))
    rows.append(row("pol", (R2P, 26, 2, 2, 24, 16), UG, 30, 34, 6, 32, 16, pw=24, family=LEFT))
    # topolar_lj_jobs: the static instances on a plain geometry, the dynamic-exit
    # one on another count and on the two geometries that are not plain
    rows.append(row("pol", (R2P, 24, 24, 2, -1, 20), 0, "jobs:20", 32, 6, 8, 20, family=LEFT))
    rows.append(row("pol", (R2P, 24, 24, 2, -1, -1), 0, "jobs:29", 32, 6, 8, 29, family=LEFT))
    rows.append(row("pol", (R2P, 16, 16, 2, -1, -1), 0, "jobs:dyn", 24, 6, 8, 21, pw=24,
                    family=LEFT))
    rows.append(row("pol", (R2P, 26, 26, 2, 32, 20), 0, "jobs:dyn", 34, 6, 8, 20, family=LEFT))
    rows.append(row("pol", (R2P, 26, 2, 2, 24, 20), 0, "jobs:dyn", 34, 6, 32, 20, pw=24,
                    family=LEFT))
    # topolar_narrow_tiles<UG>: wrap at WW 32
    for ug in (0, UG):
        rows.append(row("pol", (R2P, 24, 1, 2, 32, -1), ug, 0, 32, 6, 31, 29, wrap=True))
        rows.append(row("pol", (R2P, 28, 1, 0, 32, 20), ug, 0, 32, 2, 31, 20, wrap=True))
    rows.append(row("pol", (SR2P, 32, 32, 2, 32, 40), 0, 24, 40, 6, 8, 40, family=LEFT))
    rows.append(row("pol", (SR2P, 32, 32, 2, 32, 41), 0, None, 40, 6, 8, 41, path=EACH,
                    family=None))
    return rows


def _shorts():
    rows = []
    for ug in (0, UG):
        rows.append(row("rot16", (P2R, 16, 16, 15, 16, -1), ug, 0, 32, 15, 16, 13, pw=16))
        rows.append(row("rot16", (P2R, 16, 2, 15, 16, -1), ug, 0, 32, 15, 30, 13, pw=16,
                        wrap=True))
        rows.append(row("rot16", (P2R, 2, 16, 2, 16, -1), ug, 0, 19, 16, 3, 13, pw=16))
        rows.append(row("mix16", (P2R, 16, 16, 15, 32, -1), ug, 0, 32, 15, 16, 29))
        rows.append(row("pol16", (R2P, 16, 16, 6, 16, -1), ug, 0, 32, 14, 16, 13, pw=16))
        rows.append(row("pol16", (R2P, 16, 1, 6, 16, -1), ug, 0, 32, 14, 31, 13, pw=16,
                        wrap=True))
    return rows


def _unique(rows):
    seen, out = set(), []
    for r in rows:
        if (r.kind, r.args, r.flags) not in seen:   # (a rounding row that is a container's)
            seen.add((r.kind, r.args, r.flags))
            out.append(r)
    return out


ROT_ROWS = _unique(_rotators())
POL_ROWS = _unique(_converters())
SHORT_ROWS = _unique(_shorts())
# one named core per family for the sweeps over the tile and the grid
SWEEPS = {
    "rot": row("rot", (P2R, 32, 32, 5, 32, 20), 0, 26, 38, 5, 6, 20),
    "pol": row("pol", (R2P, 32, 32, 1, 32, 24), 0, 26, 38, 4, 6, 24, family=LEFT),
    "io16": row("rot16", (P2R, 16, 16, 15, 16, -1), 0, 0, 32, 15, 16, 13, pw=16),
    # looked-up directions: 16 stages through launch_xy_jobs (no grid cap), 20
    # through launch_xy_jobs_fused (cordic_jobs_xydir.hip), the same kernel
    "dirs16": row("rot", (P2R, 32, 32, 2, 32, 16), 0, "dirs", 35, 2, 3, 16, family=DIRS),
    "dirs20": row("rot", (P2R, 32, 32, 2, 32, 20), 0, "dirs", 35, 2, 3, 20, family=DIRS),
    "lj_jobs": row("pol", (R2P, 24, 24, 2, -1, 20), 0, "jobs:20", 32, 6, 8, 20, family=LEFT),
}
# the two whose kernels launch_xy_jobs starts: no grid cap, a crowd instead
UNCAPPED = ("dirs16", "lj_jobs")
# (family, passes a tile, blocks or None: the library's grid)
SWEEP_CASES = [(f, p, b) for f in sorted(SWEEPS) for p in (1, 2, 4, 8)
               for b in ((None,) if f in UNCAPPED else (1, 3))]


def row_id(r):
    a = r.args
    return "%s-%d-%d-x%d-pw%d-n%d-f%x" % (
        {P2R: "p2r", SP2R: "sp2r", R2P: "r2p", SR2P: "sr2p"}[a[0]] + r.kind[3:],
        a[1], a[2], a[3], a[4], a[5], r.flags)


def config_of(r):
    cfg, ocfg = JS.both(*r.args, flags=r.flags)
    return cfg, ocfg


def pol_lj_jobs_class(cfg):
    """launch_pol_lj_jobs (cordic_inst_pol_lj.hip): the static instances serve
    PLAIN cores only"""
    in_shl = cfg.ww - cfg.iw - 2
    r = cfg.ww - cfg.ow
    plain = (32 - cfg.iw) - in_shl >= 2 and 2 <= r <= 31
    return ("jobs:%d" % cfg.nlive if plain and cfg.nlive in (20, 29) else "jobs:dyn"), plain


# ---------------------------------------------------------------- no GPU

def _body(text, head):
    """the body of the function whose definition begins with `head`"""
    m = re.search(re.escape(head) + r"[^{;]*\{(.*?)\n\}", text, re.S)
    assert m, head
    return m.group(1)


def _cases(body):
    labels = [int(v) for v in re.findall(r"\bcase (\d+):", body)]
    assert len(labels) == len(set(labels)) == body.count("case ")
    return set(labels)


def test_the_matrix_is_the_launchers_containers_and_the_rows_are_what_they_claim():
    def src(name):
        return open(os.path.join(CSRC, name)).read()
    rot, rotw, pol = src("cordic_jobs_rot.hip"), src("cordic_jobs_rotw.hip"), src("cordic_jobs_pol.hip")
    rot_lj = _cases(_body(rot, "bool launch_rot_xy_tiles(")) \
        | _cases(_body(rotw, "bool launch_rot_xy_tiles_w("))
    assert rot_lj == {0, 30, 29, 28, 27, 26, 25, 24}
    # both launch helpers choose the unit-gain instance by kp.post_mul
    for text, head in ((rot, "void launch_c("), (rotw, "void launch_w(")):
        b = _body(text, head)
        assert "kp.post_mul != 0" in b and b.count("hipLaunchKernelGGL") == 2
        assert re.search(r"rotator_xy_tiles<[^;]*, true>", b) \
            and re.search(r"rotator_xy_tiles<[^;]*, false>", b)
    body = _body(pol, "bool launch_pol_tiles(")
    pol_lj = _cases(body)
    assert pol_lj == {0, 30, 29, 28, 27, 26, 25, 24}
    assert re.search(r"case 30:[^\n]*\n\s*if \(kp\.post_mul == 0\)\s*return false;", body)
    assert "topolar_narrow_tiles<true>" in body and "topolar_narrow_tiles<false>" in body
    b = _body(pol, "void launch_ljw(")
    assert "topolar_ljw_tiles<LJ, true>" in b and "topolar_ljw_tiles<LJ, false>" in b

    fused = lambda rows: {(r.inst, bool(r.flags & UG)) for r in rows if isinstance(r.inst, int)}
    assert fused(ROT_ROWS) == {(lj, ug) for lj in rot_lj for ug in (False, True)}
    assert fused(POL_ROWS) == {(lj, ug) for lj in pol_lj - {30} for ug in (False, True)} \
        | {(30, True)}
    # the four instances of launch_xy_jobs16
    io16 = _body(src("cordic_jobs_io16.hip"), "int launch_xy_jobs16(")
    assert io16.count("hipLaunchKernelGGL") == 4
    assert {(r.kind[:3], bool(r.flags & UG)) for r in SHORT_ROWS} \
        == {(k, ug) for k in ("rot", "mix", "pol") for ug in (False, True)}

    classes = []
    for r in ROT_ROWS + POL_ROWS + SHORT_ROWS + list(SWEEPS.values()):
        cfg, _ = config_of(r)
        rotator = r.args[0] in (P2R, SP2R)
        assert rotator == (r.kind[:3] in ("rot", "mix")), r
        have = (cfg.ww, cfg.ww - cfg.iw - (1 if rotator else 2), cfg.ww - cfg.ow, cfg.nlive,
                cfg.pw, bool(cfg.needs_wrap))
        assert have == (r.ww, r.in_shl, r.r, r.nlive, r.pw, r.wrap), (row_id(r), have)
        # rotators do not wrap from ow 3, converters from ow 2
        assert r.wrap == (cfg.ow < (3 if rotator else 2)), row_id(r)
        if isinstance(r.inst, int):
            # the container launch_xy_jobs_fused / launch_xy_jobs16 picks
            assert r.inst == (0 if r.wrap or r.kind.endswith("16") else 30 if r.ww <= 34
                              else 64 - r.ww), row_id(r)
            assert r.path == FUSED and 1 <= r.nlive <= 40
            assert r.family == (UNROLLED if rotator or r.inst == 0 else LEFT)
            if rotator and r.inst != 0:
                assert r.in_shl <= 30
                # no looked-up directions: unit gain, FLAG_NO_TAILS, nothing
                # appended, WW > 35 or a stage count without an instance
                assert (r.flags & (UG | NT)) or r.in_shl == 0 or r.ww > 35 \
                    or r.nlive not in XM.INSTANCES, row_id(r)
            if not rotator and r.inst == 30:
                assert r.flags & UG
        elif r.inst is None:
            assert r.path == EACH and (r.nlive == 41 or r.in_shl == 31)
        elif r.inst == "dirs":
            assert r.nlive in XM.INSTANCES and r.ww <= 35 and not r.flags
        else:
            assert not rotator and r.ww <= 34 and not r.flags and not r.wrap
            cls, plain = pol_lj_jobs_class(cfg)
            assert cls == r.inst, row_id(r)
            classes.append((cls, plain, r.nlive, r.r > 31))
    assert set(classes) == {("jobs:20", True, 20, False), ("jobs:29", True, 29, False),
                            ("jobs:dyn", True, 21, False), ("jobs:dyn", False, 20, False),
                            ("jobs:dyn", False, 20, True)}
    # the branches the rows name: r_lj of the rotators, sh of the converters
    rl = {(r.inst, r.r + r.inst) for r in ROT_ROWS if isinstance(r.inst, int) and r.inst
          and not r.flags}
    for lj in (29, 28, 27, 26, 25, 24):
        assert {(lj, 32), (lj, 33), (lj, 47), (lj, 31 + lj)} <= rl
        assert any(i == lj and v - lj >= 32 for i, v in rl)
        sh = {r.r + lj - 32 for r in POL_ROWS if r.inst == lj and r.r <= 31}
        assert {16, lj - 1} <= sh and any(r.inst == lj and r.r == 32 for r in POL_ROWS)
        assert any(r.inst == lj and r.args[1] == 16 for r in POL_ROWS)      # up = 16
    assert {(30, 32), (30, 48), (30, 61), (30, 31)} <= rl
    assert any(r.in_shl == 0 and r.inst == 30 for r in ROT_ROWS)            # fold1 false
    assert any(r.in_shl == 30 and r.path == FUSED for r in ROT_ROWS)
    assert {r.nlive for r in ROT_ROWS if r.inst == 29} >= {1, 2, 12} \
        and {r.nlive for r in ROT_ROWS if r.inst == 26} >= {1, 2, 12}
    assert any(r.junk_phase and r.pw == 20 for r in ROT_ROWS)
    # a set has 2^(r + 6) random samples for every r <= 9 that a row rounds at
    most = max(r.r for r in ROT_ROWS + POL_ROWS if r.r <= 9)
    assert most == 9 and sum(lengths(FORCED[0])) - 5 * BLOCK * len(lengths(1)) >= 1 << (most + 6)

    # the knobs are the names the sources read
    tile = _body(src("cordic_abi.cpp"), "uint32_t xy_tile_vecs(")
    assert re.search(r'bank_forced_passes\(\s*std::getenv\("%s"\),\s*kJobTileVecs / kJobPassVecs,'
                     % KNOBS[0], tile)
    assert re.search(r"xy \? xy_tile_vecs\(vecs\) : kJobTileVecs", src("cordic_abi.cpp"))
    fused_src = src("cordic_jobs_fused.hip")
    assert 'env_block_cap("%s"' % KNOBS[1] in _body(fused_src, "int jobs_grid(")
    assert "jobs_grid(tabs.ntiles)" in _body(fused_src, "int launch_xy_jobs_fused(")
    assert "jobs_grid(tabs.ntiles)" in io16
    # launch_xy_jobs (cordic_kernels.hip) reads no knob; the sweeps' families
    # that it serves -- topolar_lj_jobs, and the direction instances that
    # cordic_jobs_xydir.hip does not carry -- are the ones run as a crowd
    assert KNOBS[1] not in src("cordic_kernels.hip")
    more = {int(lj): {int(v) for v in re.findall(r"X\((\d+)\)", body)} for lj, body in
            re.findall(r"#define CORDIC_XYDIR_MORE_LJ(\d+)\(X\)(.*)", src("cordic_jobs_xydir.hip"))}
    assert sorted(more) == [29, 30]
    assert {name for name, r in SWEEPS.items() if str(r.inst).startswith("jobs:")
            or (r.inst == "dirs" and r.nlive not in more[29 if r.ww == 35 else 30])} \
        == set(UNCAPPED)
    assert {(f, b) for f, _, b in SWEEP_CASES} == {(f, b) for f in SWEEPS for b in
                                                   ((None,) if f in UNCAPPED else (1, 3))}
    # ... and the helper holds the only copy of the rule in these two units
    assert fused_src.count("cus * 8") == 1 and "cus * 8" not in src("cordic_jobs_io16.hip")


def test_the_job_lengths_are_the_edges_of_a_pass_and_of_a_tile():
    for P in (1, 2, 4, 8):
        L, tv = lengths(P), 256 * P
        vecs = [n // 4 for n in L]
        tiles = [-(-v // tv) for v in vecs]
        last = [v - (t - 1) * tv if t else 0 for v, t in zip(vecs, tiles)]
        assert L[0] == 0 and [n for n in L if 0 < n < 4] == [1, 3]      # no vector
        assert L[5:8] == [1023, 1024, 1027]
        assert [(v, n % 4) for v, n in zip(vecs[5:8], L[5:8])] == [(255, 3), (256, 0), (256, 3)]
        k = 8
        assert L[k] == PASS * P - 4
        assert (vecs[k], tiles[k], L[k] % 4) == (tv - 1, 1, 0)
        assert (vecs[k + 1], tiles[k + 1], L[k + 1] % 4) == (tv, 1, 0)
        assert (tiles[k + 2], last[k + 2], L[k + 2] % 4) == (2, 1, 2)
        assert (tiles[k + 3], last[k + 3], L[k + 3] % 4) == (3 if P > 1 else 4, 257 - 256 * (P == 1), 1)
        # every block of a grid of 1, 2 or 3 takes a second tile, on another job
        assert sum(tiles) >= 8 and max(tiles) <= 4
        # jobs with 1, 2 and 3 trailing samples (xy_job_tails16 with kp.wrap)
        assert {n % 4 for n in L} == {0, 1, 2, 3}
    assert sum(lengths(8)) < 70000
    # a full tile is P passes of the block; the unforced rule gives one pass
    # to a set of this size on any device of two CUs or more
    assert sum(n // 4 for n in lengths(8)) // (2 * 8 * 4) < 256
    # the crowd: one tile a small job, all four counts of trailing samples,
    # and every tile of the long jobs behind the grid's last block
    for cus in (64, 256, 304):
        for P in (1, 8):
            L, tv, blocks = crowd(cus * 8, P), 256 * P, cus * 8
            tiles = [-(-(n // 4) // tv) for n in L]
            small = len(L) - len(lengths(P))
            assert small > blocks and set(tiles[:small]) == {1}
            assert {n % 4 for n in L[:small]} == {0, 1, 2, 3}
            assert L[small:] == lengths(P) and sum(tiles) > small + 8
            assert sum(L) < 70000 and sum(n // 4 for n in L) // (cus * 8 * 4) < 256


# ---------------------------------------------------------------- GPU

def set_knobs(monkeypatch, passes=None, blocks=None):
    for name, v in zip(KNOBS, (passes, blocks)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def edge_vectors(rng, iw, pw, n):
    """random vectors within IW behind the 36 extreme pairs (and, for those
    that read them, random phases with the octant edges) of rand_inputs; from
    sample 128 a block of vectors in [-8, 8), one with y = 0 and one of words
    with junk above bit IW-1"""
    from test_gpu_parity import rand_inputs
    x, y, ph = rand_inputs(rng, iw, pw, n)
    ph &= np.uint32((1 << pw) - 1)
    if n < 12:      # (a crowd's small jobs: not the same few pairs in all of them)
        x, y = JS._iq(rng, n, iw), JS._iq(rng, n, iw)
    if n >= 128 + 3 * BLOCK:
        a = 128
        x[a:a + BLOCK] = rng.randint(-8, 8, BLOCK)
        y[a:a + BLOCK] = rng.randint(-8, 8, BLOCK)
        a += BLOCK
        y[a:a + BLOCK] = 0
        a += BLOCK
        x[a:a + BLOCK] = JS._iq(rng, BLOCK, iw, full=True)
        y[a:a + BLOCK] = JS._iq(rng, BLOCK, iw, full=True)
    return x, y, ph


def tie_phases(cfg, ocfg):
    angle = [int(ocfg.angle[i]) for i in range(cfg.nlive)]
    return XM.tie_ports(XM.tie_folded(angle, cfg.pw, cfg.nlive), cfg.pw)


def check_info(js, sizes, passes, min_tiles=0):
    tv = JS.xy_tile_vecs(sum(n // 4 for n in sizes))
    assert tv == 256 * (passes or 1)
    assert js.info["tiles"] >= min_tiles
    assert js.info == dict(samples=sum(sizes), tiles=sum(-(-(n // 4) // tv) for n in sizes),
                           tail_samples=sum(n % 4 for n in sizes))


def check_run(js, r, tag):
    assert js.path == r.path, (tag, js.path)
    if r.family is not None:
        assert ca.last_kernel() == r.family, (tag, ca.last_kernel())


def run_words(torch, plan, cfg, ocfg, r, kind, seed, sizes, settings, monkeypatch,
              min_tiles=0):
    """a set of `kind` on 32-bit arrays at odd word offsets between guard words"""
    from gpu_util import dev_i32
    jobs, host, outs, bigs = F._ragged_set(kind, cfg, seed, sizes)
    rng = np.random.RandomState(seed + 1)
    for k, jb in enumerate(jobs):
        if jb["n"]:
            hx, hy, hp = edge_vectors(rng, cfg.iw, cfg.pw, jb["n"])
            jb["x"].copy_(dev_i32(hx))
            jb["y"].copy_(dev_i32(hy))
            host[k] = (hx, hy, hp)
    if kind == ca.JOBS_P2R_XY:
        # the two longest jobs rotate by -1, 0 and +1 in front of every stage
        ties = tie_phases(cfg, ocfg)
        perm, at = rng.permutation(ties.size), 0
        for k in sorted(range(len(jobs)), key=lambda k: -jobs[k]["n"])[:2]:
            n = jobs[k]["n"]
            host[k] = host[k][:2] + (ties[perm[np.arange(at, at + n) % ties.size]],)
            at += n
        for k, jb in enumerate(jobs):
            if not jb["n"]:
                continue
            words = host[k][2].copy()
            if r.junk_phase:    # the port takes the low PW bits
                junk = rng.randint(1, 1 << (32 - cfg.pw), (jb["n"] + 1) // 2, dtype=np.int64)
                words[0::2] |= (junk << cfg.pw).astype(np.uint32)
                assert np.array_equal(words & np.uint32((1 << cfg.pw) - 1), host[k][2])
            jb["phase"].copy_(dev_i32(words))
    gain = F._gain(cfg, r.flags)
    want = [F._want(kind, ocfg, jb, host[k], gain) if jb["n"] else None
            for k, jb in enumerate(jobs)]
    total = sum(sizes)
    for passes, blocks in settings:
        set_knobs(monkeypatch, passes, blocks)
        with contextlib.closing(ca.Jobset(plan, kind, jobs)) as js:
            check_info(js, sizes, passes, min_tiles)
            for b in bigs:
                b.fill_(GUARD)
            js.run()
            torch.cuda.synchronize()
            check_run(js, r, (kind, passes, blocks))
            F._check_outputs(kind, ocfg, jobs, host, outs, gain, (passes, blocks), want)
            for b in bigs:          # exactly the jobs' words were written
                assert int((b == GUARD).sum().item()) == b.numel() - total, (passes, blocks)


def run_shorts(torch, plan, cfg, ocfg, r, kind, seed, sizes, settings, monkeypatch,
               min_tiles=0):
    """the same on int16 arrays at odd element offsets (Set16)"""
    s = J16.Set16(kind, cfg, seed, sizes=sizes)
    s.fill(seed)
    rng = np.random.RandomState(seed + 1)
    for k, n in enumerate(sizes):
        if not n:
            continue
        hx, hy, _ = edge_vectors(rng, cfg.iw, min(cfg.pw, 16), n)
        hx, hy = hx.astype(np.int16), hy.astype(np.int16)
        s.host[k] = (hx, hy, s.host[k][2])
        J16.put(s.xv[k], hx)
        J16.put(s.yv[k], hy)
    if kind == ca.JOBS_P2R_XY:      # PW <= 16: the tie phases fit the uint16 words
        ties = tie_phases(cfg, ocfg)
        perm, at = rng.permutation(ties.size), 0
        for k in sorted(range(len(sizes)), key=lambda k: -sizes[k])[:2]:
            hp = ties[perm[np.arange(at, at + sizes[k]) % ties.size]].astype(np.uint16)
            at += sizes[k]
            s.host[k] = s.host[k][:2] + (hp,)
            J16.put(s.phv[k], hp)
    gain = F._gain(cfg, r.flags)
    want = [s.want(ocfg, k, gain) if n else None for k, n in enumerate(sizes)]
    for passes, blocks in settings:
        set_knobs(monkeypatch, passes, blocks)
        with contextlib.closing(ca.Jobset(plan, s.kind, s.jobs)) as js:
            assert js.io16
            check_info(js, sizes, passes, min_tiles)
            s.abig.fill_(J16.GUARD)
            s.bbig.fill_(J16.GUARD)
            js.run()
            torch.cuda.synchronize()
            check_run(js, r, (kind, passes, blocks))
            s.check(ocfg, gain, (passes, blocks), want)


KINDS = {"rot": (ca.JOBS_P2R_XY, ca.JOBS_MIX), "pol": (ca.JOBS_R2P,),
         "rot16": (ca.JOBS_P2R_XY, ca.JOBS_MIX), "mix16": (ca.JOBS_MIX,),
         "pol16": (ca.JOBS_R2P,)}


def run_row(r, seed, sizes, settings, monkeypatch, min_tiles=0):
    import torch
    cfg, ocfg = config_of(r)
    run = run_shorts if r.kind.endswith("16") else run_words
    with contextlib.closing(ca.Plan(cfg)) as plan:
        for kind in KINDS[r.kind]:
            run(torch, plan, cfg, ocfg, r, kind, seed + kind, sizes, settings, monkeypatch,
                min_tiles)
    ca.jobset_reap()


BOTH = ((None, None), FORCED)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROT_ROWS, ids=row_id)
def test_gpu_every_rotator_tile_instance_equals_the_oracle(r, monkeypatch):
    """rotator_xy_tiles<C, NGEN, UG>: CORDIC_JOBS_P2R_XY and CORDIC_JOBS_MIX on
    every row, on the library's tiles and grid and on eight-pass tiles walked
    by two blocks"""
    run_row(r, 1000 + ROT_ROWS.index(r), lengths(FORCED[0]), BOTH, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("r", POL_ROWS, ids=row_id)
def test_gpu_every_converter_tile_instance_equals_the_oracle(r, monkeypatch):
    """topolar_ljw_tiles<LJ, UG>, topolar_lj_tiles<true>, topolar_narrow_tiles<UG>
    and the three instances of topolar_lj_jobs, as the rotators above"""
    run_row(r, 2000 + POL_ROWS.index(r), lengths(FORCED[0]), BOTH, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("r", SHORT_ROWS, ids=row_id)
def test_gpu_every_int16_tile_instance_equals_the_oracle(r, monkeypatch):
    """the four instances of launch_xy_jobs16 and xy_job_tails16, with the
    wrap at WW 32 on the trailing samples too"""
    run_row(r, 3000 + SHORT_ROWS.index(r), lengths(FORCED[0]), BOTH, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("family,passes,blocks", SWEEP_CASES,
                         ids=["%s-%d-%s" % (f, p, "b%d" % b if b else "grid")
                              for f, p, b in SWEEP_CASES])
def test_gpu_every_tile_length_equals_the_oracle(family, passes, blocks, monkeypatch):
    """tiles of 1, 2, 4 and 8 passes at their own edges: where the launcher
    reads CORDIC_JOBS_MAX_BLOCKS, one block walking all of them and three
    blocks taking every third; on the kernels of launch_xy_jobs the library's
    grid, a block a tile (their blocks' second tiles: the crowd below)"""
    assert (blocks is None) == (family in UNCAPPED)
    run_row(SWEEPS[family], 4000 + 8 * passes + (blocks or 0), lengths(passes),
            ((passes, blocks),), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 8])
@pytest.mark.parametrize("family", UNCAPPED)
def test_gpu_more_tiles_than_blocks_on_the_kernels_of_launch_xy_jobs(family, passes, monkeypatch):
    """topolar_lj_jobs<20> and rotator_xydir<29, 16, true> on a grid that
    nothing caps: more small jobs than CUs * 8 and the long jobs behind them,
    so that the blocks that step on take the long jobs' tiles, of one pass and
    of eight; every job against the oracle"""
    import torch
    blocks = torch.cuda.get_device_properties(0).multi_processor_count * 8
    run_row(SWEEPS[family], 5000 + passes, crowd(blocks, passes), ((passes, None),),
            monkeypatch, min_tiles=blocks + 40 + 8)
