"""FM demodulation banks (cordic_demodbank_create, _destroy, _info, _run;
include/cordic_amd.h): many cordic_fm_demod jobs of one core in at most two
launches.  Expected values need no tolerance: per job the oracle's topolar, a
numpy difference mod 2^PW and a sign extension (`expected`, restated from
test_fm_demod.py); in addition the bank's bits must equal those of one
cordic_fm_demod call per job on copies of the same data."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_demodbank_create", "cordic_demodbank_destroy",
         "cordic_demodbank_info", "cordic_demodbank_run")
UG = ca.FLAG_UNIT_GAIN
# the cores of tests/test_fm_demod.py, and cfg3 with a 20-bit phase
CORES = {
    "cfg3": ((ca.R2P, 24, 24, 2, -1, 20), 0),
    "natr2p24": ((ca.R2P, 24, 24, 2, -1, -1), 0),
    "ug_lj": ((ca.R2P, 24, 24, 2, -1, 20), UG),
    "sr2p": ((ca.SR2P, 24, 24, 2, -1, 20), 0),
    "cfg3_pw20": ((ca.R2P, 24, 24, 2, 20, 20), 0),
    "r2p35": ((ca.R2P, 27, 27, 2, 32, 20), 0),
    "wrap32": ((ca.R2P, 24, 1, 2, 32, -1), 0),
    "cfg3_no_lj": ((ca.R2P, 24, 24, 2, -1, 20), ca.FLAG_NO_LJ),
    "pw20": ((ca.R2P, 16, 16, 2, 20, -1), 0),
}
FUSED = ("cfg3", "natr2p24", "ug_lj", "sr2p")
ONE_BY_ONE = ("r2p35", "wrap32", "cfg3_no_lj")
# pw20 (IW 16, WW 24, no wrap) is a core for which cordic_fm_demod_info answers
# 1, so by the rule of the header its bank is a fused one: it runs with the
# others for its 20-bit phase, and its path is checked against that query
PW20 = ("pw20",)
PASSES = (1, 2, 4, 8)


def both(name):
    args, flags = CORES[name]
    cfg = ca.Config.from_cli(*args)
    if flags:
        cfg = cfg.with_flags(flags)
    gain = ca.lib().cordic_config_gain_annihilator(cfg.ref) if flags & UG else None
    return cfg, O.config_cli(*args), gain


def tile_of(passes):
    return (passes * 256 - 1) * 4


# ---------------------------------------------------------------- no GPU

def test_the_bank_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    assert re.search(
        r"typedef\s+struct\s+cordic_demod_job\s*\{\s*"
        r"const\s+int32_t\s*\*\s*d_xval\s*,\s*\*\s*d_yval\s*;(\s*/\*.*?\*/)?\s*"
        r"int32_t\s*\*\s*d_omag\s*,\s*\*\s*d_ofreq\s*;(\s*/\*.*?\*/)?\s*"
        r"uint32_t\s*\*\s*d_last\s*;(\s*/\*.*?\*/)?\s*"
        r"uint64_t\s+n\s*;(\s*/\*.*?\*/)?\s*"
        r"uint32_t\s+phase0\s*;(\s*/\*.*?\*/)?\s*"
        r"uint32_t\s+reserved\s*;(\s*/\*.*?\*/)?\s*"
        r"\}\s*cordic_demod_job\s*;", text, re.S)
    assert re.search(r"typedef\s+struct\s+cordic_demodbank\s+cordic_demodbank\s*;", text)
    assert re.search(
        r"int\s+cordic_demodbank_create\s*\(\s*const\s+cordic_config\s*\*\s*cfg\s*,"
        r"\s*size_t\s+njobs\s*,\s*const\s+cordic_demod_job\s*\*\s*jobs\s*,\s*"
        r"cordic_demodbank\s*\*\*\s*bank\s*\)\s*;", text)
    assert re.search(r"void\s+cordic_demodbank_destroy\s*\(\s*cordic_demodbank\s*\*\s*"
                     r"bank\s*\)\s*;", text)
    assert re.search(
        r"int\s+cordic_demodbank_info\s*\(\s*const\s+cordic_demodbank\s*\*\s*bank\s*,"
        r"\s*uint64_t\s*\*\s*samples\s*,\s*uint32_t\s*\*\s*tiles\s*,\s*uint32_t\s*\*\s*"
        r"tail_jobs\s*,\s*int32_t\s*\*\s*fused\s*,\s*int32_t\s*\*\s*tile\s*\)\s*;", text)
    assert re.search(r"int\s+cordic_demodbank_run\s*\(\s*const\s+cordic_demodbank\s*\*"
                     r"\s*bank\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    from cordic_amd import _native
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
        assert name in _native.ABI
    assert "DemodBank" in ca.__all__ and callable(ca.DemodBank)
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_ctypes_mirror_has_the_layout_of_the_header():
    from cordic_amd._native import _CDemodJob
    assert C.sizeof(_CDemodJob) == 56
    assert [f[0] for f in _CDemodJob._fields_] == [
        "d_xval", "d_yval", "d_omag", "d_ofreq", "d_last", "n", "phase0", "reserved"]
    assert [getattr(_CDemodJob, f[0]).offset for f in _CDemodJob._fields_] == [
        0, 8, 16, 24, 32, 40, 48, 52]


def test_the_header_with_the_bank_block_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { cordic_config c; cordic_demod_job j; cordic_demodbank *b = 0;\n'
        'uint64_t s; uint32_t t, u; int32_t f, l; int rc;\n'
        'char size_is_56[sizeof(cordic_demod_job) == 56 ? 1 : -1];\n'
        'cordic_config_init(&c, CORDIC_R2P, 24, 24, 2, -1, 20);\n'
        'j.d_xval = j.d_yval = 0; j.d_omag = j.d_ofreq = 0; j.d_last = 0; j.n = 0;\n'
        'j.phase0 = 0; j.reserved = 0; (void)size_is_56;\n'
        'rc = cordic_demodbank_create(&c, 1, &j, &b);\n'
        'rc += cordic_demodbank_info(b, &s, &t, &u, &f, &l);\n'
        'rc += cordic_demodbank_run(b, 0); cordic_demodbank_destroy(b); return rc; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_create_refuses_nulls_and_a_rotator_before_anything_is_allocated():
    L = ca.lib()
    cfg = both("cfg3")[0]
    h = C.c_void_p(0x5a5a)
    job = ca._native._CDemodJob()
    assert L.cordic_demodbank_create(None, 0, None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_demodbank_create(cfg.ref, 0, None, None) == ca.ERR_ARGS
    assert L.cordic_demodbank_create(cfg.ref, 1, None, C.byref(h)) == ca.ERR_ARGS
    p2r = ca.Config.from_cli(ca.P2R, 24, 24, 2, -1, -1)
    assert L.cordic_demodbank_create(p2r.ref, 1, C.byref(job), C.byref(h)) == ca.ERR_MODE
    assert L.cordic_demodbank_create(p2r.ref, 0, None, C.byref(h)) == ca.ERR_MODE
    assert h.value == 0x5a5a                # no handle was made


def test_info_run_and_destroy_on_a_null_handle():
    L = ca.lib()
    s, t, u = C.c_uint64(7), C.c_uint32(7), C.c_uint32(7)
    f, l = C.c_int32(7), C.c_int32(7)
    assert L.cordic_demodbank_info(None, C.byref(s), C.byref(t), C.byref(u),
                                   C.byref(f), C.byref(l)) == ca.ERR_ARGS
    assert (s.value, t.value, u.value, f.value, l.value) == (7, 7, 7, 7, 7)
    assert L.cordic_demodbank_run(None, None) == ca.ERR_ARGS
    L.cordic_demodbank_destroy(None)        # a no-op


CUTTER = r"""
#include <cstdio>
#include <cstring>
#include "cordic_fm_demod_bank.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced: job k's four arrays in four regions
static cordic_demod_job job_at(size_t k, uint64_t n, bool last)
{
	cordic_demod_job j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t base = 0x10000000u + (uintptr_t)k * 0x100000u + 4 * (k % 4);
	j.d_xval = (const int32_t *)(base);
	j.d_yval = (const int32_t *)(base + 0x1000000000u);
	j.d_omag = (int32_t *)(base + 0x2000000000u);
	j.d_ofreq = (int32_t *)(base + 0x3000000000u);
	j.d_last = last ? (uint32_t *)(0x6000000000u + 16 * k) : nullptr;
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u + 1);
	return j;
}

static void check_cut(const std::vector<cordic_demod_job> &jobs, int passes)
{
	const uint32_t tv = fmd_bank_tile_vecs(passes);
	EXPECT(tv == (uint32_t)passes * 256 - 1);
	std::vector<DemodTile> tiles;
	std::vector<DemodTail> tails;
	fmd_bank_cut(jobs.size(), jobs.data(), tv, &tiles, &tails);
	EXPECT(tiles.size() == fmd_bank_count_tiles(jobs.size(), jobs.data(), tv));
	size_t at = 0, tail_at = 0;
	for (size_t k = 0; k < jobs.size(); k++) {
		const cordic_demod_job &jb = jobs[k];
		const uint64_t x = (uintptr_t)jb.d_xval, y = (uintptr_t)jb.d_yval,
			m = (uintptr_t)jb.d_omag, f = (uintptr_t)jb.d_ofreq,
			l = (uintptr_t)jb.d_last;
		// the tiles cover the job's n / 4 vectors exactly and in order
		const uint64_t nvec = jb.n / 4;
		uint64_t v = 0;
		while (v < nvec) {
			EXPECT(at < tiles.size());
			if (at >= tiles.size())
				return;
			const DemodTile &t = tiles[at++];
			EXPECT(t.x == x + v * 16 && t.y == y + v * 16);
			EXPECT(t.mag == m + v * 16 && t.freq == f + v * 16);
			EXPECT(t.nvec >= 1 && t.nvec <= tv && t.nvec <= nvec - v);
			// only a job's last tile is shorter
			EXPECT(t.nvec == tv || v + t.nvec == nvec);
			EXPECT(t.first == (v == 0 ? 1u : 0u));
			EXPECT(t.phase0 == (v == 0 ? jb.phase0 : 0u));
			EXPECT(t.last == (v == 0 ? l : 0));
			EXPECT(t.pad == 0);
			v += t.nvec ? t.nvec : 1;
		}
		EXPECT(v == nvec);
		// a tail exactly when the length is no multiple of 4 or there is a d_last
		if (jb.n == 0 || (jb.n % 4 == 0 && !l))
			continue;
		EXPECT(tail_at < tails.size());
		if (tail_at >= tails.size())
			return;
		const DemodTail &t = tails[tail_at++];
		const uint64_t s0 = nvec ? nvec * 4 - 1 : 0;
		EXPECT(t.x == x + s0 * 4 && t.y == y + s0 * 4);
		EXPECT(t.mag == m + s0 * 4 && t.freq == f + s0 * 4);
		EXPECT(t.last == l && t.phase0 == jb.phase0 && t.pad == 0);
		EXPECT(t.count == jb.n - s0 && t.count >= 1 && t.count <= 4);
		EXPECT(t.first == (nvec == 0 ? 1u : 0u));
	}
	EXPECT(at == tiles.size() && tail_at == tails.size());
}

int main()
{
	std::vector<uint64_t> lens = {0, 1, 3, 4, 5, 7, 8, 1019, 1020, 1021, 1024};
	for (uint64_t p = 1; p <= 8; p *= 2) {
		const uint64_t t = (p * 256 - 1) * 4;	// samples of a full tile
		for (uint64_t n : {t - 1, t, t + 1, t + 4, t + 5})
			lens.push_back(n);
	}
	lens.push_back(40003);
	std::vector<cordic_demod_job> jobs;
	for (size_t k = 0; k < lens.size(); k++)
		jobs.push_back(job_at(k, lens[k], k % 2 == 1));
	EXPECT(fmd_bank_jobs_valid(jobs.size(), jobs.data()));
	for (int p = 1; p <= 8; p *= 2)
		check_cut(jobs, p);
	// ... the other jobs with a d_last, and no job at all
	for (size_t k = 0; k < jobs.size(); k++)
		jobs[k] = job_at(k, lens[k], k % 2 == 0);
	EXPECT(fmd_bank_jobs_valid(jobs.size(), jobs.data()));
	for (int p = 1; p <= 8; p *= 2) {
		check_cut(jobs, p);
		check_cut(std::vector<cordic_demod_job>(), p);
	}
	{	// a job of the greatest length: 2^58 vectors, counted without a cut
		const cordic_demod_job big = job_at(0, ~(size_t)0 >> 4, false);
		EXPECT(fmd_bank_count_tiles(1, &big, fmd_bank_tile_vecs(8))
			== (((uint64_t)1 << 58) - 1 + 2046) / 2047);
	}

	// P by the bank's size: the longest tile that leaves 4 per resident block
	// (8 per CU): total / (cus * 32) / 256, in the steps 1, 2, 4, 8
	const int cuses[] = {256, 0, -1};
	for (int cus : cuses) {
		EXPECT(fmd_bank_passes(0, cus) == 1 && fmd_bank_passes(4194303, cus) == 1);
		EXPECT(fmd_bank_passes(4194304, cus) == 2 && fmd_bank_passes(8388607, cus) == 2);
		EXPECT(fmd_bank_passes(8388608, cus) == 4 && fmd_bank_passes(16777215, cus) == 4);
		EXPECT(fmd_bank_passes(16777216, cus) == 8);
		EXPECT(fmd_bank_passes(~(uint64_t)0, cus) == 8);
	}
	EXPECT(fmd_bank_passes(16383, 1) == 1 && fmd_bank_passes(16384, 1) == 2);
	EXPECT(fmd_bank_passes(65536, 1) == 8 && fmd_bank_passes(65536, 64) == 1);

	// the overlap rules
	const uint64_t n = 64;
	const cordic_demod_job a = job_at(0, n, true), b = job_at(1, n, true);
	auto valid = [](cordic_demod_job x, cordic_demod_job y) {
		const cordic_demod_job two[2] = {x, y};
		return fmd_bank_jobs_valid(2, two);
	};
	EXPECT(valid(a, b));
	// output on output
	{ cordic_demod_job c = b; c.d_omag = a.d_omag + n - 1; EXPECT(!valid(a, c)); }
	{ cordic_demod_job c = b; c.d_omag = a.d_omag + n; EXPECT(valid(a, c)); }
	{ cordic_demod_job c = b; c.d_ofreq = a.d_omag; EXPECT(!valid(a, c)); }
	{ cordic_demod_job c = a; c.d_ofreq = c.d_omag + 1; EXPECT(!valid(c, b)); }
	// output over input: of the same job, of another, each kind of input
	{ cordic_demod_job c = b; c.d_omag = (int32_t *)a.d_xval + n - 1; EXPECT(!valid(a, c)); }
	{ cordic_demod_job c = b; c.d_ofreq = (int32_t *)a.d_yval; EXPECT(!valid(a, c)); }
	{ cordic_demod_job c = b; c.d_omag = (int32_t *)a.d_yval + 3; EXPECT(!valid(a, c)); }
	{ cordic_demod_job c = a; c.d_ofreq = (int32_t *)c.d_yval; EXPECT(!valid(c, b)); }
	{ cordic_demod_job c = a; c.d_omag = (int32_t *)c.d_xval; EXPECT(!valid(c, b)); }
	{ cordic_demod_job c = b; c.d_omag = (int32_t *)a.d_xval + n; EXPECT(valid(a, c)); }
	{ cordic_demod_job c = b; c.d_omag = (int32_t *)a.d_xval - n; EXPECT(valid(a, c)); }
	{ cordic_demod_job c = b; c.d_omag = (int32_t *)a.d_xval - n + 1; EXPECT(!valid(a, c)); }
	// d_last: shared, inside an output, inside an input
	{ cordic_demod_job c = b; c.d_last = a.d_last; EXPECT(!valid(a, c)); }
	{ cordic_demod_job c = b; c.d_last = a.d_last + 1; EXPECT(valid(a, c)); }
	{ cordic_demod_job c = b; c.d_last = (uint32_t *)a.d_ofreq + 5; EXPECT(!valid(a, c)); }
	{ cordic_demod_job c = b; c.d_last = (uint32_t *)a.d_xval + n - 1; EXPECT(!valid(a, c)); }
	{ cordic_demod_job c = a; c.d_last = (uint32_t *)c.d_yval; EXPECT(!valid(c, b)); }
	{ cordic_demod_job c = a; c.d_last = (uint32_t *)c.d_omag + n; EXPECT(valid(c, b)); }
	// inputs may alias, within a job and between jobs
	{ cordic_demod_job c = b; c.d_xval = a.d_xval; c.d_yval = a.d_xval + 1;
	  EXPECT(valid(a, c)); }
	{ cordic_demod_job c = a; c.d_yval = c.d_xval; EXPECT(valid(c, b)); }
	// a job alone: NULLs, the 4-byte grid, reserved, the length
	auto one = [](cordic_demod_job x) { return fmd_bank_jobs_valid(1, &x); };
	EXPECT(one(a));
	{ cordic_demod_job c = a; c.d_last = nullptr; EXPECT(one(c)); }
	{ cordic_demod_job c = a; c.d_xval = nullptr; EXPECT(!one(c)); }
	{ cordic_demod_job c = a; c.d_yval = nullptr; EXPECT(!one(c)); }
	{ cordic_demod_job c = a; c.d_omag = nullptr; EXPECT(!one(c)); }
	{ cordic_demod_job c = a; c.d_ofreq = nullptr; EXPECT(!one(c)); }
#define ODD(field, type) { cordic_demod_job c = a; \
	c.field = (type)((uintptr_t)c.field + 2); EXPECT(!one(c)); }
	ODD(d_xval, const int32_t *) ODD(d_yval, const int32_t *) ODD(d_omag, int32_t *)
	ODD(d_ofreq, int32_t *) ODD(d_last, uint32_t *)
	{ cordic_demod_job c = a; c.reserved = 1; EXPECT(!one(c)); }
	{ cordic_demod_job c = a; c.n = (~(size_t)0 >> 4) + 1; EXPECT(!one(c)); }
	{ cordic_demod_job c = a; c.n = ~(size_t)0 >> 4; EXPECT(!one(c)); }	// its arrays reach over each other
	// a zero-length job's pointers are not looked at
	{ cordic_demod_job c = a; c.n = 0; c.d_xval = nullptr; c.reserved = 9;
	  c.d_omag = (int32_t *)3; c.d_last = b.d_last; EXPECT(valid(c, b)); }
	EXPECT(fmd_bank_jobs_valid(0, nullptr));
	if (!failures)
		std::printf("cutter ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_host_cutter_under_address_and_ub_sanitizers(tmp_path):
    """cordic_fm_demod_bank.h in a stand-alone program with its own main: no
    GPU, no Python in the checked process"""
    src, exe = tmp_path / "cutter.cpp", tmp_path / "cutter"
    src.write_text(CUTTER)
    csrc = os.path.join(ROOT, "cordic_amd", "csrc")
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", csrc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "cutter ok" in r.stdout


# ---------------------------------------------------------------- GPU

SENT = -0x5a5a5a5b
SENT_U = SENT & 0xffffffff


def iq(rng, n, iw):
    lo, hi = -(1 << (iw - 1)), (1 << (iw - 1)) - 1
    return (rng.integers(lo, hi + 1, n).astype(np.int32),
            rng.integers(lo, hi + 1, n).astype(np.int32))


def hard_points(iw):
    """x = y = 0, the axes, the diagonals, +/-1 LSB around each, +/- full scale"""
    lo, hi = -(1 << (iw - 1)), (1 << (iw - 1)) - 1
    pts = []
    for a in (1, 2, 1000, hi // 2, hi - 1):
        for bx, by in ((0, 0), (a, 0), (-a, 0), (0, a), (0, -a), (a, a), (a, -a),
                       (-a, a), (-a, -a)):
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    pts.append((bx + dx, by + dy))
    pts += [(lo, lo), (lo, 0), (0, lo), (lo, hi), (hi, lo), (hi, hi), (lo, -1),
            (-1, lo), (lo, 1)]
    return np.array(pts, dtype=np.int32)


def expected(ocfg, gain, pw, x, y, prev):
    """(mag, freq as int32, ph_(n-1)) for the phase `prev` in front of sample 0"""
    mag, ph = O.topolar(ocfg, x, y)
    if gain is not None:            # o = (o * K) >> 32 (CORDIC_FLAG_UNIT_GAIN)
        mag = ((mag.astype(np.int64) * gain) >> 32).astype(np.int32)
    mask = (1 << pw) - 1
    p = ph.astype(np.int64)
    before = np.concatenate([[prev & mask], p[:-1]]) if p.size else p
    d = (p - before) & mask
    sign = 1 << (pw - 1)
    freq = ((d ^ sign) - sign).astype(np.int64)
    return mag, freq.astype(np.int32), (int(ph[-1]) if ph.size else None)


def ragged_lengths():
    rng = np.random.default_rng(31)
    ns = [0, 1, 2, 3, 4, 5, 7, 8]
    for p in PASSES:
        ns += [tile_of(p) + d for d in (-4, -1, 0, 1, 4)]
    ns.append(2 * 8188 + 3)
    ns += [int(v) for v in rng.integers(9, 20001, 6)]
    ns += [0, 6]
    order = rng.permutation(len(ns))
    return [ns[i] for i in order]


class Spec:
    """The host side of a bank in two arenas (inputs; outputs between sentinel
    words) and an array of d_last words, four per job: job k's arrays start
    (k + a) % 4 words behind a 16-byte boundary, a = 0 .. 3 for x, y, mag,
    freq, so the four sit differently and every job has one aligned array."""

    def __init__(self, lengths, iw, seed, with_last=None, phase0=None, hard=True):
        rng = np.random.default_rng(seed)
        self.ns = list(lengths)
        k = len(self.ns)
        self.has_last = [bool(rng.integers(0, 2)) for _ in range(k)] \
            if with_last is None else [with_last] * k
        self.phase0 = [int(v) for v in rng.integers(0, 1 << 32, k)] \
            if phase0 is None else [phase0] * k
        self.preset = [int(v) for v in rng.integers(0, 1 << 32, k)]
        self.off = []                      # (x, y, mag, freq) word offsets
        cur_in = cur_out = 4
        for j, n in enumerate(self.ns):
            o = []
            for a in range(4):
                cur = cur_in if a < 2 else cur_out
                at = (cur + 3) // 4 * 4 + (j + a) % 4
                o.append(at)
                if a < 2:
                    cur_in = at + n
                else:
                    cur_out = at + n + 1   # at least one sentinel word between
            self.off.append(tuple(o))
        self.in_words, self.out_words = cur_in + 8, cur_out + 8
        self.x, self.y = [], []
        pts = hard_points(iw)
        for j, n in enumerate(self.ns):
            x, y = iq(rng, n, iw)
            if hard and n:                  # a slice of the hard points in front
                m = min(n, 40)
                s = (j * 37) % (len(pts) - m)
                x[:m], y[:m] = pts[s:s + m, 0], pts[s:s + m, 1]
            self.x.append(x)
            self.y.append(y)

    def renew(self, iw, seed):
        """new random samples in the same places"""
        rng = np.random.default_rng(seed)
        for j, n in enumerate(self.ns):
            self.x[j], self.y[j] = iq(rng, n, iw)

    def tiles(self, passes):
        v = passes * 256 - 1
        return sum((n // 4 + v - 1) // v for n in self.ns)

    def tail_jobs(self):
        return sum(1 for n, l in zip(self.ns, self.has_last) if n and (n % 4 or l))


class DeviceBank:
    """`spec` on the device and a DemodBank over it"""

    def __init__(self, torch, cfg, spec):
        from gpu_util import DEV
        self.torch, self.spec = torch, spec
        self.ins = torch.zeros(spec.in_words, dtype=torch.int32, device=DEV)
        self.outs = torch.full((spec.out_words,), SENT, dtype=torch.int32, device=DEV)
        self.lasts = torch.full((4 * max(1, len(spec.ns)),), SENT, dtype=torch.int32,
                                device=DEV)
        self.upload()
        h = np.full(self.lasts.numel(), SENT_U, dtype=np.uint32)
        for j, l in enumerate(spec.has_last):
            if l:
                h[4 * j] = spec.preset[j]
        self.lasts.copy_(torch.from_numpy(h.view(np.int32)).to(DEV))
        jobs = []
        for j, n in enumerate(spec.ns):
            ox, oy, om, of = spec.off[j]
            jobs.append((self.ins[ox:], self.ins[oy:], self.outs[om:], self.outs[of:],
                         n, spec.phase0[j],
                         self.lasts[4 * j:] if spec.has_last[j] else None))
        self.bank = ca.DemodBank(cfg, jobs)

    def upload(self):
        from gpu_util import DEV
        h = np.zeros(self.spec.in_words, dtype=np.int32)
        for j, n in enumerate(self.spec.ns):
            ox, oy = self.spec.off[j][:2]
            h[ox:ox + n] = self.spec.x[j]
            h[oy:oy + n] = self.spec.y[j]
        self.ins.copy_(self.torch.from_numpy(h).to(DEV))
        self.h_ins = h

    def results(self):
        """([(mag, freq)], [last or None]) after checking that the inputs, the
        sentinels and the words of jobs without a d_last are as they were"""
        self.torch.cuda.synchronize()
        spec = self.spec
        assert np.array_equal(self.ins.cpu().numpy(), self.h_ins)
        o = self.outs.cpu().numpy()
        l = self.lasts.cpu().numpy().view(np.uint32)
        written = np.zeros(o.size, dtype=bool)
        got, lasts = [], []
        for j, n in enumerate(spec.ns):
            om, of = spec.off[j][2:]
            written[om:om + n] = True
            written[of:of + n] = True
            got.append((o[om:om + n].copy(), o[of:of + n].copy()))
            lasts.append(int(l[4 * j]) if spec.has_last[j] else None)
            if not spec.has_last[j]:
                assert l[4 * j] == SENT_U, j
            assert (l[4 * j + 1:4 * j + 4] == SENT_U).all(), j
        assert (o[~written] == SENT).all()
        return got, lasts


@functools.lru_cache(maxsize=None)
def ragged_spec(iw):
    return Spec(ragged_lengths(), iw, 100 + iw)


@functools.lru_cache(maxsize=None)
def ragged_expected(name):
    """per job (mag, freq, last after the run) of the ragged bank, once per core"""
    cfg, ocfg, gain = both(name)
    spec = ragged_spec(cfg.iw)
    want = []
    for j, n in enumerate(spec.ns):
        prev = spec.phase0[j] + (spec.preset[j] if spec.has_last[j] else 0)
        m, f, l = expected(ocfg, gain, cfg.pw, spec.x[j], spec.y[j], prev)
        if not spec.has_last[j]:
            l = None
        elif n == 0:
            l = spec.preset[j]
        want.append((m, f, l))
    return want


def assert_equals(got, lasts, want, tag):
    for j, ((m, f), l, (wm, wf, wl)) in enumerate(zip(got, lasts, want)):
        assert np.array_equal(m, wm), (tag, j, m.size)
        assert np.array_equal(f, wf), (tag, j, f.size)
        assert l == wl, (tag, j, m.size)


def single_calls(torch, cfg, spec):
    """one cordic_fm_demod call per job on copies of the same data"""
    from gpu_util import DEV, dev_i32
    work = torch.zeros(max(16, ca.fm_demod_workspace(max(spec.ns))), dtype=torch.uint8,
                       device=DEV)
    out = []
    for j, n in enumerate(spec.ns):
        x, y = dev_i32(spec.x[j]), dev_i32(spec.y[j])
        m = torch.zeros(max(n, 1), dtype=torch.int32, device=DEV)
        f = torch.zeros(max(n, 1), dtype=torch.int32, device=DEV)
        last = None
        if spec.has_last[j]:
            last = dev_i32(np.array([spec.preset[j]] * 4, dtype=np.uint32))
        ca.fm_demod(cfg, x, y, m, f, work, n=n, phase0=spec.phase0[j], last=last)
        torch.cuda.synchronize()
        out.append((m.cpu().numpy()[:n], f.cpu().numpy()[:n],
                    None if last is None else int(last.cpu().numpy().view(np.uint32)[0])))
    return out


def check_ragged_spec(spec):
    """the lengths and placements the ragged bank is meant to have"""
    ns = spec.ns
    for n in [0, 1, 2, 3, 4, 5, 7, 8, 2 * 8188 + 3] + [
            tile_of(p) + d for p in PASSES for d in (-4, -1, 0, 1, 4)]:
        assert n in ns
    assert 36 <= len(ns) <= 44 and max(ns) <= 20000
    assert 0 < sum(spec.has_last) < len(ns)
    assert any(p >> 24 for p in spec.phase0)
    for o in spec.off:
        assert len({a % 4 for a in o}) == 4          # all four displaced differently
    assert {o[0] % 4 for o in spec.off} == {0, 1, 2, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED + ONE_BY_ONE + PW20)
def test_gpu_ragged_bank_equals_the_oracle_and_the_single_calls(name):
    import torch
    cfg = both(name)[0]
    spec = ragged_spec(cfg.iw)
    check_ragged_spec(spec)
    d = DeviceBank(torch, cfg, spec)
    info = d.bank.info()
    assert info["samples"] == sum(spec.ns)
    assert info["fused"] == ca.fm_demod_info(cfg)[0]
    assert info["fused"] == (0 if name in ONE_BY_ONE else 1)
    if info["fused"]:
        assert info["tile"] in [tile_of(p) for p in PASSES]
        p = (info["tile"] // 4 + 1) // 256
        assert info["tiles"] == spec.tiles(p)
        assert info["tail_jobs"] == spec.tail_jobs()
    else:
        assert (info["tile"], info["tiles"], info["tail_jobs"]) == (0, 0, 0)
    d.bank.run()
    got, lasts = d.results()
    assert_equals(got, lasts, ragged_expected(name), name)
    assert_equals(got, lasts, single_calls(torch, cfg, spec), name + " single calls")
    d.bank.close()


@pytest.mark.gpu
def test_gpu_forced_tile_sizes_and_grid_caps_give_the_same_bits(monkeypatch):
    import torch
    name = "cfg3"
    cfg = both(name)[0]
    spec = ragged_spec(cfg.iw)
    want = ragged_expected(name)
    monkeypatch.delenv("CORDIC_FMD_BANK_PASSES", raising=False)
    monkeypatch.delenv("CORDIC_FMD_MAX_BLOCKS", raising=False)
    d = DeviceBank(torch, cfg, spec)
    d.bank.run()
    ref, ref_lasts = d.results()
    assert_equals(ref, ref_lasts, want, "default")
    ref = [(m, f, l) for (m, f), l in zip(ref, ref_lasts)]
    d.bank.close()
    for p in PASSES:
        monkeypatch.setenv("CORDIC_FMD_BANK_PASSES", str(p))
        d = DeviceBank(torch, cfg, spec)
        info = d.bank.info()
        assert info["fused"] == 1 and info["tile"] == tile_of(p)
        assert info["tiles"] == spec.tiles(p) and info["tail_jobs"] == spec.tail_jobs()
        d.bank.run()
        got, lasts = d.results()
        assert_equals(got, lasts, ref, "passes %d" % p)
        d.bank.close()
    monkeypatch.delenv("CORDIC_FMD_BANK_PASSES")
    for cap in (1, 3, 7):
        monkeypatch.setenv("CORDIC_FMD_MAX_BLOCKS", str(cap))
        d = DeviceBank(torch, cfg, spec)
        assert d.bank.info()["tiles"] >= 3 * cap
        d.bank.run()
        got, lasts = d.results()
        assert_equals(got, lasts, ref, "max blocks %d" % cap)
        d.bank.close()


ROUNDS, CHANNELS, BLOCK = 3, 8, 4100


def continuation(name):
    """(spec of round 0, [x, y per round], per channel the oracle's pass over
    the 12300 samples with 0 in front)"""
    cfg, ocfg, gain = both(name)
    spec = Spec([BLOCK] * CHANNELS, cfg.iw, 41, with_last=True, phase0=0, hard=False)
    spec.preset = [0] * CHANNELS
    rounds = []
    for r in range(ROUNDS):
        spec.renew(cfg.iw, 50 + r)
        rounds.append(([a.copy() for a in spec.x], [a.copy() for a in spec.y]))
    want = [expected(ocfg, gain, cfg.pw,
                     np.concatenate([rounds[r][0][j] for r in range(ROUNDS)]),
                     np.concatenate([rounds[r][1][j] for r in range(ROUNDS)]), 0)
            for j in range(CHANNELS)]
    return cfg, spec, rounds, want


def check_continuation(name, parts, lasts, want):
    for j in range(CHANNELS):
        assert np.array_equal(np.concatenate([p[j][0] for p in parts]), want[j][0]), (name, j)
        assert np.array_equal(np.concatenate([p[j][1] for p in parts]), want[j][1]), (name, j)
        assert lasts[j] == want[j][2], (name, j)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg3", "r2p35"])
def test_gpu_three_runs_on_new_data_continue_every_channel(name):
    import torch
    cfg, spec, rounds, want = continuation(name)
    d = DeviceBank(torch, cfg, spec)
    assert d.bank.info()["fused"] == (1 if name == "cfg3" else 0)
    parts = []
    for r in range(ROUNDS):
        spec.x, spec.y = rounds[r]
        d.upload()
        d.bank.run()
        got, lasts = d.results()
        parts.append(got)
    check_continuation(name, parts, lasts, want)
    d.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg3", "r2p35"])
def test_gpu_a_captured_run_replayed_three_times_continues_three_times(name):
    """one stream, no parallel branches; once outside the capture first, on a
    bank with words of its own"""
    import torch
    cfg, spec, rounds, want = continuation(name)
    warm = DeviceBank(torch, cfg, spec)
    warm.bank.run()
    torch.cuda.synchronize()
    warm.bank.close()
    d = DeviceBank(torch, cfg, spec)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d.bank.run()
    parts = []
    for r in range(ROUNDS):
        spec.x, spec.y = rounds[r]
        d.upload()
        d.outs.fill_(SENT)
        g.replay()
        got, lasts = d.results()
        parts.append(got)
    check_continuation(name, parts, lasts, want)
    del g
    d.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg3", "cfg3_pw20", "pw20", "r2p35"])
def test_gpu_phase0_and_the_last_word_add_mod_2_to_the_pw_on_every_run(name):
    import torch
    cfg, ocfg, gain = both(name)
    lengths = [1, 3, 4, 6, 1023, 4101]
    phase0 = 0xfff9abcd
    spec = Spec(lengths, cfg.iw, 61, with_last=True, phase0=phase0)
    d = DeviceBank(torch, cfg, spec)
    assert d.bank.info()["fused"] == (0 if name == "r2p35" else 1)
    prev = [phase0 + p for p in spec.preset]
    for run in range(2):
        d.outs.fill_(SENT)
        d.bank.run()
        got, lasts = d.results()
        want = [expected(ocfg, gain, cfg.pw, spec.x[j], spec.y[j], prev[j])
                for j in range(len(lengths))]
        assert_equals(got, lasts, want, (name, run))
        assert all(l < 1 << cfg.pw for l in lasts)
        prev = [phase0 + l for l in lasts]      # phase0 is added by every run
    d.bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg3", "r2p35"])
def test_gpu_empty_banks_run_and_write_nothing(name):
    import torch
    cfg = both(name)[0]
    for lengths in ([], [0, 0, 0]):
        spec = Spec(lengths, cfg.iw, 71, with_last=True)
        d = DeviceBank(torch, cfg, spec)
        info = d.bank.info()
        assert (info["samples"], info["tiles"], info["tail_jobs"]) == (0, 0, 0)
        d.bank.run()
        got, lasts = d.results()
        assert lasts == spec.preset[:len(lengths)]
        assert (d.outs == SENT).all().item()
        d.bank.close()
    # a zero-length job's pointers are not looked at
    b = ca.DemodBank(cfg, [(3, 5, 7, 9, 0, 0, 11)])
    b.run()
    torch.cuda.synchronize()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg3", "r2p35"])
def test_gpu_create_refuses_overlaps_and_bad_jobs_with_nothing_written(name):
    import torch
    from gpu_util import DEV
    cfg = both(name)[0]
    n = 64
    ins = torch.arange(4 * n, dtype=torch.int32, device=DEV)
    outs = torch.full((6 * n,), SENT, dtype=torch.int32, device=DEV)
    lasts = torch.full((8,), SENT, dtype=torch.int32, device=DEV)
    x0, y0, x1, y1 = (ins[k * n:] for k in range(4))
    m0, f0, m1, f1 = (outs[k * n:] for k in range(4))
    l0, l1 = lasts, lasts[4:]

    def job(x=x0, y=y0, m=m0, f=f0, last=l0):
        return (x, y, m, f, n, 0, last)

    def other(x=x1, y=y1, m=m1, f=f1, last=l1):
        return (x, y, m, f, n, 0, last)

    def refused(*jobs, reserved=None):
        if reserved is None:
            with pytest.raises(ca.CordicError) as e:
                ca.DemodBank(cfg, list(jobs))
            assert e.value.status == ca.ERR_ARGS
            return
        arr = (ca._native._CDemodJob * 1)()
        for k, v in zip(("d_xval", "d_yval", "d_omag", "d_ofreq"), (x0, y0, m0, f0)):
            setattr(arr[0], k, v.data_ptr())
        arr[0].n, arr[0].reserved = n, reserved
        h = C.c_void_p()
        assert ca.lib().cordic_demodbank_create(cfg.ref, 1, arr, C.byref(h)) == ca.ERR_ARGS

    odd = lambda t: t.data_ptr() + 2
    refused(job(), other(m=outs[n - 1:]))               # output over output
    refused(job(f=outs[n - 1:]))                        # ... of the same job
    refused(job(), other(f=outs[2 * n - 1:], m=outs[4 * n:]))
    refused(job(), other(m=ins[n - 1:]))                # output over another job's input
    refused(job(), other(f=ins[1:]))
    refused(job(m=ins[3 * n:]), other())
    refused(job(), other(last=l0))                      # a shared d_last
    refused(job(), other(last=outs[n - 1:]))            # d_last inside an output array
    refused(job(last=outs[n:]))
    refused(job(last=ins[5:]))                          # ... inside an input array
    for k in range(4):                                  # off the 4-byte grid
        a = [x0, y0, m0, f0]
        a[k] = odd(a[k])
        refused(job(*a))
    refused(job(last=odd(l0)))
    refused(reserved=1)
    for k in range(4):                                  # a NULL sample pointer
        a = [x0, y0, m0, f0]
        a[k] = None
        refused(job(*a))
    torch.cuda.synchronize()
    assert (outs == SENT).all().item() and (lasts == SENT).all().item()
    assert torch.equal(ins, torch.arange(4 * n, dtype=torch.int32, device=DEV))
    # inputs may alias each other, within a job and between jobs
    b = ca.DemodBank(cfg, [job(y=x0), other(x=x0, y=x0)])
    b.run()
    torch.cuda.synchronize()
    h = outs.cpu().numpy()
    assert (h[4 * n:] == SENT).all() and (h[:4 * n] != SENT).any()
    b.close()
