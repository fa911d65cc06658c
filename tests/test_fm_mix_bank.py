"""FM mixer banks (cordic_mixbank_create, _destroy, _info, _run;
include/cordic_amd.h): many cordic_plan_fm_mix jobs of one plan in two launches.
Expected values need no tolerance: per job numpy's wrapping cumulative sum
(expected() of tests/test_table_fm.py) feeds the oracle's rotate, as in
tests/test_fm_mix.py; in addition the bank's bits must equal those of one
cordic_plan_fm_mix call per job on copies of the same data."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
from test_fm_mix import both, iq, want, _hip
from test_table_fm import expected as phases, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")
NAMES = ("cordic_mixbank_create", "cordic_mixbank_destroy", "cordic_mixbank_info",
         "cordic_mixbank_run")
FIELDS = ["d_fcw", "d_pm", "d_xval", "d_yval", "d_oxval", "d_oyval", "d_acc", "n",
          "phase0", "reserved"]
FUSED = ("cfg2", "nat24", "nat16")          # LJ 29 / 16 stages, LJ 30 / 27, LJ 30 / 19
ONE_BY_ONE = ("ww38", "sp2r", "cfg2_ug")
PASS = 1024
MAX_SPANS = 4096
KNOBS = ("CORDIC_FMXB_MAX_BLOCKS", "CORDIC_FMXB_PASSES", "CORDIC_FMXB_MAX_SPANS")
M32 = 0xffffffff


def spans_of(n, passes, cap=MAX_SPANS):
    """the cutter's rule (cordic_fm_mix_bank.h) restated: spans of `passes`
    passes, doubled for this job alone until it has at most `cap` of them"""
    if n == 0:
        return 0
    np_ = -(-n // PASS)
    while -(-np_ // passes) > cap:
        passes *= 2
    return -(-np_ // passes)


# ---------------------------------------------------------------- no GPU

def test_the_bank_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    c = r"(\s*/\*.*?\*/)?\s*"
    assert re.search(
        r"typedef\s+struct\s+cordic_fmmix_job\s*\{\s*"
        r"const\s+uint32_t\s*\*\s*d_fcw\s*;" + c +
        r"const\s+uint32_t\s*\*\s*d_pm\s*;" + c +
        r"const\s+int32_t\s*\*\s*d_xval\s*,\s*\*\s*d_yval\s*;" + c +
        r"int32_t\s*\*\s*d_oxval\s*,\s*\*\s*d_oyval\s*;" + c +
        r"uint32_t\s*\*\s*d_acc\s*;" + c +
        r"uint64_t\s+n\s*;" + c +
        r"uint32_t\s+phase0\s*;" + c +
        r"uint32_t\s+reserved\s*;" + c +
        r"\}\s*cordic_fmmix_job\s*;", text, re.S)
    assert re.search(r"typedef\s+struct\s+cordic_mixbank\s+cordic_mixbank\s*;", text)
    assert re.search(
        r"int\s+cordic_mixbank_create\s*\(\s*const\s+cordic_plan\s*\*\s*plan\s*,"
        r"\s*size_t\s+njobs\s*,\s*const\s+cordic_fmmix_job\s*\*\s*jobs\s*,\s*"
        r"cordic_mixbank\s*\*\*\s*bank\s*\)\s*;", text)
    assert re.search(r"void\s+cordic_mixbank_destroy\s*\(\s*cordic_mixbank\s*\*\s*bank"
                     r"\s*\)\s*;", text)
    assert re.search(
        r"int\s+cordic_mixbank_info\s*\(\s*const\s+cordic_mixbank\s*\*\s*bank\s*,"
        r"\s*uint64_t\s*\*\s*samples\s*,\s*uint32_t\s*\*\s*spans\s*,\s*int32_t\s*\*\s*"
        r"fused\s*,\s*int32_t\s*\*\s*tile\s*\)\s*;", text)
    assert re.search(r"int\s+cordic_mixbank_run\s*\(\s*const\s+cordic_mixbank\s*\*"
                     r"\s*bank\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    # behind the FM mixer block, which no longer denies it
    assert text.index("cordic_plan_fm_mix(") < text.index("cordic_mixbank_create(")
    assert "no job-set kind" not in text
    from cordic_amd import _native
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
        assert name in _native.ABI
    assert "MixBank" in ca.__all__ and callable(ca.MixBank)
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_ctypes_mirror_has_the_layout_of_the_header(tmp_path):
    """72 bytes, the field offsets from a compiled offsetof program"""
    from cordic_amd._native import _CFmMixJob
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "cordic_amd.h"\n'
        'int main(void) { printf("%zu", sizeof(cordic_fmmix_job));\n'
        + "".join('printf(" %%zu", offsetof(cordic_fmmix_job, %s));\n' % f for f in FIELDS)
        + 'return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    nums = [int(v) for v in r.stdout.split()]
    assert nums[0] == 72 == C.sizeof(_CFmMixJob)
    assert [f[0] for f in _CFmMixJob._fields_] == FIELDS
    assert [getattr(_CFmMixJob, f).offset for f in FIELDS] == nums[1:]
    assert nums[1:] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68]


def test_the_header_with_the_bank_block_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { const cordic_plan *p = 0; cordic_fmmix_job j;\n'
        'cordic_mixbank *b = 0; uint64_t s; uint32_t t; int32_t f, l; int rc;\n'
        'char size_is_72[sizeof(cordic_fmmix_job) == 72 ? 1 : -1];\n'
        'j.d_fcw = j.d_pm = 0; j.d_xval = j.d_yval = 0; j.d_oxval = j.d_oyval = 0;\n'
        'j.d_acc = 0; j.n = 0; j.phase0 = 0; j.reserved = 0; (void)size_is_72;\n'
        'rc = cordic_mixbank_create(p, 1, &j, &b);\n'
        'rc += cordic_mixbank_info(b, &s, &t, &f, &l);\n'
        'rc += cordic_mixbank_run(b, 0); cordic_mixbank_destroy(b); return rc; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_create_refuses_nulls_before_anything_is_allocated():
    """(a WW 38 core has no seed table, so its plan needs no device)"""
    L = ca.lib()
    plan = ca.Plan(both("ww38")[0])
    h = C.c_void_p(0x5a5a)
    job = ca._native._CFmMixJob()
    assert L.cordic_mixbank_create(None, 0, None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_mixbank_create(None, 1, C.byref(job), C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_mixbank_create(plan._h, 0, None, None) == ca.ERR_ARGS
    assert L.cordic_mixbank_create(plan._h, 1, None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_mixbank_create(plan._h, 1 << 28, C.byref(job), C.byref(h)) \
        == ca.ERR_ARGS                      # (the count is refused unread)
    assert h.value == 0x5a5a                # no handle was made
    plan.close()


def test_info_run_and_destroy_on_a_null_handle():
    L = ca.lib()
    s, t = C.c_uint64(7), C.c_uint32(7)
    f, l = C.c_int32(7), C.c_int32(7)
    assert L.cordic_mixbank_info(None, C.byref(s), C.byref(t), C.byref(f),
                                 C.byref(l)) == ca.ERR_ARGS
    assert (s.value, t.value, f.value, l.value) == (7, 7, 7, 7)
    assert L.cordic_mixbank_run(None, None) == ca.ERR_ARGS
    L.cordic_mixbank_destroy(None)          # a no-op


CUTTER = r"""
#include <cstdio>
#include <cstring>
#include "cordic_fm_mix_bank.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced: job k's six arrays in six regions
static cordic_fmmix_job job_at(size_t k, uint64_t n, bool pm, bool acc)
{
	cordic_fmmix_job j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t base = 0x10000000u + (uintptr_t)k * 0x100000u + 4 * (k % 4);
	j.d_fcw = (const uint32_t *)(base);
	j.d_pm = pm ? (const uint32_t *)(base + 0x1000000000u) : nullptr;
	j.d_xval = (const int32_t *)(base + 0x2000000000u);
	j.d_yval = (const int32_t *)(base + 0x3000000000u);
	j.d_oxval = (int32_t *)(base + 0x4000000000u);
	j.d_oyval = (int32_t *)(base + 0x5000000000u);
	j.d_acc = acc ? (uint32_t *)(0x6000000000u + 16 * k) : nullptr;
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u);
	return j;
}

static void check_cut(const std::vector<cordic_fmmix_job> &jobs, uint32_t passes,
		uint32_t cap)
{
	std::vector<MixSpan> spans;
	uint32_t live = 0;
	span_cut(kFmxbRule, jobs.size(), MixJobs(jobs.data()), passes, cap, &spans, &live);
	EXPECT(spans.size() == span_count(kFmxbRule, jobs.size(), MixJobs(jobs.data()), passes, cap));
	size_t at = 0;
	uint32_t seen = 0;
	for (size_t k = 0; k < jobs.size(); k++) {
		const cordic_fmmix_job &jb = jobs[k];
		if (!jb.n)
			continue;
		const size_t first = at;
		uint64_t done = 0;
		uint64_t full = 0;		// the length of this job's whole spans
		while (done < jb.n) {
			EXPECT(at < spans.size());
			if (at >= spans.size())
				return;
			const MixSpan &s = spans[at];
			// the spans tile [0, n) exactly, in order
			EXPECT(s.fcw == (uintptr_t)jb.d_fcw + done * 4);
			EXPECT(s.pm == (jb.d_pm ? (uintptr_t)jb.d_pm + done * 4 : 0));
			EXPECT(s.x == (uintptr_t)jb.d_xval + done * 4);
			EXPECT(s.y == (uintptr_t)jb.d_yval + done * 4);
			EXPECT(s.ox == (uintptr_t)jb.d_oxval + done * 4);
			EXPECT(s.oy == (uintptr_t)jb.d_oyval + done * 4);
			EXPECT(s.acc == (uintptr_t)jb.d_acc);
			EXPECT(s.phase0 == jb.phase0 && s.pad == 0);
			EXPECT(s.n >= 1 && s.n <= jb.n - done);
			EXPECT(s.start == seen && s.part0 == first && s.idx == at - first);
			const bool is_first = done == 0, is_last = done + s.n == jb.n;
			EXPECT(s.flags == ((is_first ? kSpanFirst : 0u)
				| (is_last ? kSpanLast : 0u)));
			if (!is_last) {		// whole passes, all of one length
				EXPECT(s.n % kFmxbRule.unit == 0);
				EXPECT(full == 0 || s.n == full);
				full = s.n;
			} else {
				EXPECT(full == 0 || s.n <= full);
			}
			if (full) {		// P, or P doubled
				const uint64_t p = full / kFmxbRule.unit;
				EXPECT(p >= passes && p % passes == 0 && !((p / passes) & (p / passes - 1)));
			}
			done += s.n;
			at++;
		}
		EXPECT(done == jb.n);
		const size_t count = at - first;
		EXPECT(count <= cap);
		// doubled only as far as the cap asks
		const uint64_t np = span_units_of(kFmxbRule, jb.n);
		const uint64_t pj = span_job_units(kFmxbRule, jb.n, passes, cap);
		EXPECT(count == (np + pj - 1) / pj);
		EXPECT(pj == passes || (np + pj / 2 - 1) / (pj / 2) > cap);
		seen++;
	}
	EXPECT(at == spans.size() && seen == live);
}

int main()
{
	const uint64_t lens[] = {0, 1, 3, 4, 5, 255, 1023, 1024, 1025, 2047, 2048, 2049,
		4095, 4096, 4097, 8191, 8192, 8193, 40 * 1024 + 3, 0, 7, 3000, 12345,
		16 * 1024 - 1, 16 * 1024, 16 * 1024 + 1, 100 * 1024};
	std::vector<cordic_fmmix_job> jobs;
	for (size_t k = 0; k < sizeof lens / sizeof *lens; k++)
		jobs.push_back(job_at(k, lens[k], k % 2 == 0, k % 3 != 0));
	EXPECT(fmxb_jobs_valid(jobs.size(), jobs.data()));
	for (uint32_t p = 1; p <= 64; p *= 2) {		// every forced P
		check_cut(jobs, p, kFmxbRule.max_spans);
		check_cut(jobs, p, 3);			// a forced span cap of 3
		check_cut(jobs, p, 1);
	}
	check_cut(jobs, 1, 7);
	check_cut(std::vector<cordic_fmmix_job>(), 1, kFmxbRule.max_spans);
	{	// a job of the greatest length stays within the cap
		std::vector<cordic_fmmix_job> big(1, job_at(0, ~(size_t)0 >> 4, false, true));
		EXPECT(span_count(kFmxbRule, 1, MixJobs(big.data()), 1, kFmxbRule.max_spans)
			<= kFmxbRule.max_spans);
		EXPECT(span_count(kFmxbRule, 1, MixJobs(big.data()), 1, 3) <= 3);
	}

	// P by the bank's size: the longest span that leaves 4 per resident block
	auto fmxb_passes = [](uint64_t total_passes, int cus) {
		return span_base_units(kFmxbRule, total_passes, cus, kFmxbBlocksPerCu);
	};
	EXPECT(fmxb_passes(0, 256) == 1 && fmxb_passes(4095, 256) == 1);
	EXPECT(fmxb_passes(4096, 256) == 1 && fmxb_passes(8191, 256) == 1);
	EXPECT(fmxb_passes(8192, 256) == 2 && fmxb_passes(65536, 256) == 16);
	EXPECT(fmxb_passes(65536, 0) == 16 && fmxb_passes(65536, 64) == 64);
	EXPECT(fmxb_passes(~(uint64_t)0, 1) == kFmxbRule.max_units);
	// the knobs
	EXPECT(span_forced_base(kFmxbRule, nullptr, 4) == 4 && span_forced_base(kFmxbRule, "8", 4) == 8);
	EXPECT(span_forced_base(kFmxbRule, "3", 4) == 4 && span_forced_base(kFmxbRule, "0", 4) == 4);
	EXPECT(span_forced_base(kFmxbRule, "-2", 4) == 4 && span_forced_base(kFmxbRule, "x", 4) == 4);
	EXPECT(span_forced_base(kFmxbRule, "1048576", 4) == 1048576);
	EXPECT(span_forced_base(kFmxbRule, "2097152", 4) == 4);
	EXPECT(span_forced_cap(kFmxbRule, nullptr) == 4096 && span_forced_cap(kFmxbRule, "3") == 3);
	EXPECT(span_forced_cap(kFmxbRule, "0") == 4096 && span_forced_cap(kFmxbRule, "4096") == 4096);
	EXPECT(span_forced_cap(kFmxbRule, "99999") == 4096 && span_forced_cap(kFmxbRule, "4095") == 4095);

	// the overlap rules
	const uint64_t n = 64;
	const cordic_fmmix_job a = job_at(0, n, true, true), b = job_at(1, n, true, true);
	auto valid = [](cordic_fmmix_job x, cordic_fmmix_job y) {
		const cordic_fmmix_job two[2] = {x, y};
		return fmxb_jobs_valid(2, two);
	};
	EXPECT(valid(a, b));
	{ cordic_fmmix_job c = b; c.d_oxval = a.d_oxval + n - 1; EXPECT(!valid(a, c)); }
	{ cordic_fmmix_job c = b; c.d_oxval = a.d_oxval + n; EXPECT(valid(a, c)); }
	{ cordic_fmmix_job c = b; c.d_oyval = a.d_oxval; EXPECT(!valid(a, c)); }
	{ cordic_fmmix_job c = a; c.d_oyval = c.d_oxval + 1; EXPECT(!valid(c, b)); }
	// output over input: of the same job, of another, each kind of input
	{ cordic_fmmix_job c = b; c.d_oxval = (int32_t *)a.d_fcw + n - 1; EXPECT(!valid(a, c)); }
	{ cordic_fmmix_job c = b; c.d_oyval = (int32_t *)a.d_pm; EXPECT(!valid(a, c)); }
	{ cordic_fmmix_job c = b; c.d_oxval = (int32_t *)a.d_xval + 3; EXPECT(!valid(a, c)); }
	{ cordic_fmmix_job c = a; c.d_oyval = (int32_t *)c.d_yval; EXPECT(!valid(c, b)); }
	{ cordic_fmmix_job c = b; c.d_oxval = (int32_t *)a.d_fcw + n; EXPECT(valid(a, c)); }
	{ cordic_fmmix_job c = b; c.d_oxval = (int32_t *)a.d_fcw - n; EXPECT(valid(a, c)); }
	{ cordic_fmmix_job c = b; c.d_oxval = (int32_t *)a.d_fcw - n + 1; EXPECT(!valid(a, c)); }
	// d_acc: shared, inside an output, inside an input
	{ cordic_fmmix_job c = b; c.d_acc = a.d_acc; EXPECT(!valid(a, c)); }
	{ cordic_fmmix_job c = b; c.d_acc = a.d_acc + 1; EXPECT(valid(a, c)); }
	{ cordic_fmmix_job c = b; c.d_acc = (uint32_t *)a.d_oyval + 5; EXPECT(!valid(a, c)); }
	{ cordic_fmmix_job c = b; c.d_acc = (uint32_t *)a.d_xval + n - 1; EXPECT(!valid(a, c)); }
	{ cordic_fmmix_job c = a; c.d_acc = (uint32_t *)c.d_pm; EXPECT(!valid(c, b)); }
	// inputs may alias, within a job and between jobs
	{ cordic_fmmix_job c = b; c.d_fcw = a.d_fcw; c.d_pm = a.d_fcw + 1;
	  c.d_xval = a.d_xval; c.d_yval = a.d_xval; EXPECT(valid(a, c)); }
	// a job alone: NULLs, the 4-byte grid, reserved, the length
	auto one = [](cordic_fmmix_job x) { return fmxb_jobs_valid(1, &x); };
	EXPECT(one(a));
	{ cordic_fmmix_job c = a; c.d_pm = nullptr; c.d_acc = nullptr; EXPECT(one(c)); }
	{ cordic_fmmix_job c = a; c.d_fcw = nullptr; EXPECT(!one(c)); }
	{ cordic_fmmix_job c = a; c.d_xval = nullptr; EXPECT(!one(c)); }
	{ cordic_fmmix_job c = a; c.d_yval = nullptr; EXPECT(!one(c)); }
	{ cordic_fmmix_job c = a; c.d_oxval = nullptr; EXPECT(!one(c)); }
	{ cordic_fmmix_job c = a; c.d_oyval = nullptr; EXPECT(!one(c)); }
#define ODD(field, type) { cordic_fmmix_job c = a; \
	c.field = (type)((uintptr_t)c.field + 2); EXPECT(!one(c)); }
	ODD(d_fcw, const uint32_t *) ODD(d_pm, const uint32_t *) ODD(d_xval, const int32_t *)
	ODD(d_yval, const int32_t *) ODD(d_oxval, int32_t *) ODD(d_oyval, int32_t *)
	ODD(d_acc, uint32_t *)
	{ cordic_fmmix_job c = a; c.reserved = 1; EXPECT(!one(c)); }
	{ cordic_fmmix_job c = a; c.n = (~(size_t)0 >> 4) + 1; EXPECT(!one(c)); }
	{ cordic_fmmix_job c = a; c.n = ~(size_t)0 >> 4; EXPECT(!one(c)); }	// its arrays reach over each other
	// a zero-length job's pointers are not looked at
	{ cordic_fmmix_job c = a; c.n = 0; c.d_fcw = nullptr; c.reserved = 9;
	  c.d_oxval = (int32_t *)3; c.d_acc = b.d_acc; EXPECT(valid(c, b)); }
	EXPECT(fmxb_jobs_valid(0, nullptr));
	if (!failures)
		std::printf("cutter ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_host_cutter_under_address_and_ub_sanitizers(tmp_path):
    """cordic_fm_mix_bank.h in a stand-alone program with its own main: no GPU,
    no Python in the checked process"""
    src, exe = tmp_path / "cutter.cpp", tmp_path / "cutter"
    src.write_text(CUTTER)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "cutter ok" in r.stdout


def test_the_pass_loop_is_shared_not_pasted():
    """one definition, in cordic_fm_mix.h, called by both kernels"""
    head = open(os.path.join(CSRC, "cordic_fm_mix.h")).read()
    assert len(re.findall(r"\bvoid\s+pass_loop\s*\(", head)) == 1
    for unit in ("cordic_fm_mix.hip", "cordic_fm_mix_bank.hip"):
        body = open(os.path.join(CSRC, unit)).read()
        assert re.search(r"\bpass_loop<LJ, NLIVE>\(", body), unit
        assert "wave_scan(" not in body and "__builtin_amdgcn_update_dpp" not in body, unit
    stamp = open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert "cordic_fm_mix_bank" not in stamp


# ---------------------------------------------------------------- GPU

SENT = -0x5a5a5a5b
SENT_U = SENT & M32
ARRAYS = ("fcw", "pm", "x", "y", "ox", "oy")


def ragged_lengths():
    """the lengths of the issue -- P * 1024 - 1, P * 1024, P * 1024 + 1 for
    every P that the geometry test forces, 1 among them -- and random ones"""
    rng = np.random.default_rng(31)
    ns = [0, 1, 3, 4, 5, 255, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
          8191, 8192, 8193, 40 * 1024 + 3]
    ns += [int(v) for v in rng.integers(2, 3001, 17)]
    ns += [0, 2, 7, 257]
    order = rng.permutation(len(ns))
    return [ns[i] for i in order]


class Spec:
    """The host side of a bank in two arenas (inputs; outputs between sentinel
    words) and an array of d_acc words, four per job.  Every array starts 1, 2
    or 3 words behind a 16-byte boundary: job k's a-th array at 1 + (k + a) % 3,
    so an output has at least one sentinel word in front of it and behind it."""

    def __init__(self, lengths, iw, seed, with_acc=None, phase0=None, with_pm=None):
        rng = np.random.default_rng(seed)
        self.ns = list(lengths)
        k = len(self.ns)
        pick = lambda forced: [bool(rng.integers(0, 2)) for _ in range(k)] \
            if forced is None else [forced] * k
        self.has_acc, self.has_pm = pick(with_acc), pick(with_pm)
        self.phase0 = [int(v) | 0x80000000 for v in rng.integers(0, 1 << 32, k)] \
            if phase0 is None else [phase0] * k
        # a preset whose sum with phase0 wraps
        self.preset = [(int(v) | 0x80000000) for v in rng.integers(0, 1 << 32, k)]
        self.off = []                      # word offsets of ARRAYS
        cur_in = cur_out = 4
        for j, n in enumerate(self.ns):
            o = []
            for a in range(6):
                cur = cur_in if a < 4 else cur_out
                at = (cur + 3) // 4 * 4 + 1 + (j + a) % 3
                o.append(at)
                if a < 4:
                    cur_in = at + n
                else:
                    cur_out = at + n
            self.off.append(tuple(o))
        self.in_words, self.out_words = cur_in + 8, cur_out + 8
        self.iw = iw
        self.renew(seed + 1)

    def renew(self, seed):
        """new random words and samples in the same places"""
        rng = np.random.default_rng(seed)
        self.fcw, self.pm, self.x, self.y = [], [], [], []
        for j, n in enumerate(self.ns):
            s = int(rng.integers(0, 1 << 30))
            self.fcw.append(words("random" if j % 5 else "fsk", n, s))
            self.pm.append(words("random", n, s + 1) if self.has_pm[j] else None)
            x, y = iq(rng, n, self.iw)
            self.x.append(x)
            self.y.append(y)

    def spans(self, passes, cap=MAX_SPANS):
        return sum(spans_of(n, passes, cap) for n in self.ns)


class DeviceBank:
    """`spec` on the device and a MixBank over it"""

    def __init__(self, torch, plan, spec):
        from gpu_util import DEV
        self.torch, self.spec = torch, spec
        self.ins = torch.zeros(spec.in_words, dtype=torch.int32, device=DEV)
        self.outs = torch.full((spec.out_words,), SENT, dtype=torch.int32, device=DEV)
        self.accs = torch.full((4 * max(1, len(spec.ns)),), SENT, dtype=torch.int32,
                               device=DEV)
        self.upload()
        h = np.full(self.accs.numel(), SENT_U, dtype=np.uint32)
        for j, l in enumerate(spec.has_acc):
            if l:
                h[4 * j] = spec.preset[j]
        self.accs.copy_(torch.from_numpy(h.view(np.int32)).to(DEV))
        jobs = []
        for j, n in enumerate(spec.ns):
            f, m, x, y, ox, oy = spec.off[j]
            jobs.append((self.ins[f:], self.ins[m:] if spec.has_pm[j] else None,
                         self.ins[x:], self.ins[y:], self.outs[ox:], self.outs[oy:], n,
                         spec.phase0[j], self.accs[4 * j:] if spec.has_acc[j] else None))
        self.bank = ca.MixBank(plan, jobs)

    def upload(self):
        from gpu_util import DEV
        spec = self.spec
        h = np.zeros(spec.in_words, dtype=np.int32)
        for j, n in enumerate(spec.ns):
            f, m, x, y = spec.off[j][:4]
            h[f:f + n] = spec.fcw[j].view(np.int32)
            if spec.has_pm[j]:
                h[m:m + n] = spec.pm[j].view(np.int32)
            h[x:x + n] = spec.x[j]
            h[y:y + n] = spec.y[j]
        self.ins.copy_(self.torch.from_numpy(h).to(DEV))
        self.h_ins = h

    def results(self):
        """([(ox, oy)], [acc or None]) after checking that the inputs, the
        sentinels and the words of jobs without a d_acc are as they were"""
        self.torch.cuda.synchronize()
        spec = self.spec
        assert np.array_equal(self.ins.cpu().numpy(), self.h_ins)
        o = self.outs.cpu().numpy()
        a = self.accs.cpu().numpy().view(np.uint32)
        written = np.zeros(o.size, dtype=bool)
        got, accs = [], []
        for j, n in enumerate(spec.ns):
            ox, oy = spec.off[j][4:]
            assert not written[ox - 1] and not written[oy - 1]
            written[ox:ox + n] = True
            written[oy:oy + n] = True
            got.append((o[ox:ox + n].copy(), o[oy:oy + n].copy()))
            accs.append(int(a[4 * j]) if spec.has_acc[j] else None)
            if not spec.has_acc[j]:
                assert a[4 * j] == SENT_U, j
            assert (a[4 * j + 1:4 * j + 4] == SENT_U).all(), j
        assert (o[~written] == SENT).all()
        return got, accs


def expected_of(name, spec, starts=None):
    """per job (ox, oy, acc after the run); starts: the words in front of the
    run, the presets by default"""
    out = []
    for j, n in enumerate(spec.ns):
        acc0 = (spec.preset[j] if starts is None else starts[j]) if spec.has_acc[j] else 0
        p, final = phases(spec.fcw[j], spec.pm[j], spec.phase0[j], acc0)
        wx, wy = want(name, spec.x[j], spec.y[j], p)
        if not spec.has_acc[j]:
            final = None
        elif n == 0:
            final = acc0
        out.append((wx, wy, final))
    return out


@functools.lru_cache(maxsize=None)
def ragged_spec(iw):
    return Spec(ragged_lengths(), iw, 100 + iw)


@functools.lru_cache(maxsize=None)
def ragged_expected(name):
    """the ragged bank's oracle values, once per core"""
    return expected_of(name, ragged_spec(both(name)[0].iw))


def assert_equals(got, accs, wanted, tag):
    for j, ((gx, gy), a, (wx, wy, wa)) in enumerate(zip(got, accs, wanted)):
        assert np.array_equal(gx, wx), (tag, j, gx.size)
        assert np.array_equal(gy, wy), (tag, j, gy.size)
        assert a == wa, (tag, j, gx.size)


def single_calls(torch, plan, spec):
    """one cordic_plan_fm_mix call per job on copies of the same data"""
    from gpu_util import DEV, dev_i32
    work = torch.zeros(max(16, plan.fm_mix_workspace(max(spec.ns))), dtype=torch.uint8,
                       device=DEV)
    out = []
    for j, n in enumerate(spec.ns):
        f, x, y = dev_i32(spec.fcw[j]), dev_i32(spec.x[j]), dev_i32(spec.y[j])
        m = dev_i32(spec.pm[j]) if spec.has_pm[j] else None
        ox = torch.zeros(max(n, 1), dtype=torch.int32, device=DEV)
        oy = torch.zeros(max(n, 1), dtype=torch.int32, device=DEV)
        acc = None
        if spec.has_acc[j]:
            acc = dev_i32(np.array([spec.preset[j]] * 4, dtype=np.uint32))
        plan.fm_mix(f, x, y, ox, oy, work, pm=m, n=n, phase0=spec.phase0[j], acc=acc)
        torch.cuda.synchronize()
        out.append((ox.cpu().numpy()[:n], oy.cpu().numpy()[:n],
                    None if acc is None else int(acc.cpu().numpy().view(np.uint32)[0])))
    return out


def check_ragged_spec(spec):
    """the lengths and placements the ragged bank is meant to have"""
    ns = spec.ns
    for n in [0, 1, 3, 4, 5, 255, 1023, 1024, 1025, 2047, 2048, 4097, 40 * 1024 + 3] + [
            p * 1024 + d for p in (1, 2, 4, 8) for d in (-1, 0, 1)]:
        assert n in ns
    assert 36 <= len(ns) <= 44
    assert 0 < sum(spec.has_acc) < len(ns) and 0 < sum(spec.has_pm) < len(ns)
    for j in range(len(ns)):
        if spec.has_acc[j]:
            assert spec.phase0[j] + spec.preset[j] > M32     # the sum wraps
    for o in spec.off:
        assert all(a % 4 in (1, 2, 3) for a in o)
    assert {o[k] % 4 for o in spec.off for k in (4, 5)} == {1, 2, 3}


def clear_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED + ONE_BY_ONE)
def test_gpu_ragged_bank_equals_the_oracle_and_the_single_calls(name, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    spec = ragged_spec(cfg.iw)
    check_ragged_spec(spec)
    d = DeviceBank(torch, plan, spec)
    info = d.bank.info()
    assert info["samples"] == sum(spec.ns)
    assert info["fused"] == plan.fm_mix_info()[0]
    assert info["fused"] == (1 if name in FUSED else 0)
    if info["fused"]:
        p = info["tile"] // PASS
        assert info["tile"] == p * PASS and p >= 1 and p & (p - 1) == 0
        assert info["spans"] == spec.spans(p)
        # P * 1024 - 1, P * 1024 and P * 1024 + 1 for the P in force
        assert p in (1, 2, 4, 8)
    else:
        assert (info["tile"], info["spans"]) == (0, 0)
    d.bank.run()
    got, accs = d.results()
    assert_equals(got, accs, ragged_expected(name), name)
    assert_equals(got, accs, single_calls(torch, plan, spec), name + " single calls")
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", (13, 16, 19, 20, 24, 27, 29))
@pytest.mark.parametrize("lj", [29, 30])
def test_gpu_every_instance_equals_the_oracle(lj, n, monkeypatch):
    """fm_mixbank_xydir<LJ, N> for all 14 (LJ, N): the cores of
    tests/test_xydir_matrix.py's instance sweep"""
    import torch
    import oracle_lib as O
    clear_knobs(monkeypatch)
    args = (ca.P2R, 32, 32, 2, 32, n) if lj == 29 else (ca.P2R, 31, 31, 2, 32, n)
    cfg, ocfg = ca.Config.from_cli(*args), O.config_cli(*args)
    assert cfg.ww == 64 - lj and cfg.nlive == n and cfg.pw == 32
    plan = ca.Plan(cfg)
    spec = Spec([1, 1023, 1025, 3 * 1024 + 2, 0], cfg.iw, 200 + lj * 100 + n)
    spec.has_acc[3] = spec.has_pm[3] = True
    spec.renew(7)
    d = DeviceBank(torch, plan, spec)
    info = d.bank.info()
    assert info["fused"] == 1 and info["samples"] == sum(spec.ns)
    d.bank.run()
    got, accs = d.results()
    for j, m in enumerate(spec.ns):
        acc0 = spec.preset[j] if spec.has_acc[j] else 0
        p, final = phases(spec.fcw[j], spec.pm[j], spec.phase0[j], acc0)
        wx, wy = O.rotate(ocfg, spec.x[j], spec.y[j], p)
        assert np.array_equal(got[j][0], wx) and np.array_equal(got[j][1], wy), (j, m)
        assert accs[j] == (None if not spec.has_acc[j] else final if m else acc0), (j, m)
    d.bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_forced_spans_grid_caps_and_span_caps_give_the_same_bits(monkeypatch):
    import torch
    name = "cfg2"
    clear_knobs(monkeypatch)
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    spec = ragged_spec(cfg.iw)
    wanted = ragged_expected(name)

    def run(tag, passes=None, cap=MAX_SPANS):
        d = DeviceBank(torch, plan, spec)
        info = d.bank.info()
        assert info["fused"] == 1
        if passes is not None:
            assert info["tile"] == passes * PASS
        assert info["spans"] == spec.spans(info["tile"] // PASS, cap)
        d.bank.run()
        got, accs = d.results()
        assert_equals(got, accs, wanted, tag)
        d.bank.close()
        return info

    run("default")
    for p in (1, 2, 4, 8):
        monkeypatch.setenv("CORDIC_FMXB_PASSES", str(p))
        run("passes %d" % p, p)
    monkeypatch.delenv("CORDIC_FMXB_PASSES")
    for cap in (1, 2, 3):       # one block walks spans of many jobs back to back
        monkeypatch.setenv("CORDIC_FMXB_MAX_BLOCKS", str(cap))
        assert run("max blocks %d" % cap)["spans"] >= 20 * cap
    monkeypatch.delenv("CORDIC_FMXB_MAX_BLOCKS")
    monkeypatch.setenv("CORDIC_FMXB_MAX_SPANS", "3")
    monkeypatch.setenv("CORDIC_FMXB_PASSES", "1")
    assert spans_of(40 * 1024 + 3, 1, 3) == 3       # 41 passes: spans of 16
    assert spans_of(8193, 1, 3) == 3 and spans_of(4097, 1, 3) == 3
    info = run("max spans 3", 1, 3)
    assert info["spans"] < spec.spans(1)
    monkeypatch.setenv("CORDIC_FMXB_MAX_BLOCKS", "2")
    run("max spans 3 on 2 blocks", 1, 3)
    plan.close()


ROUNDS = 3
CONT_LENGTHS = [1, 1023, 1025, 3 * 1024 + 2, 0, 5, 2048, 4097]


def continuation(name, phase0):
    """(spec, per round the spec's data, per round the oracle's values)"""
    cfg = both(name)[0]
    spec = Spec(CONT_LENGTHS, cfg.iw, 41, with_acc=True, phase0=phase0)
    rounds, wanted = [], []
    starts = list(spec.preset)
    for r in range(ROUNDS):
        spec.renew(50 + r)
        rounds.append((spec.fcw, spec.pm, spec.x, spec.y))
        w = expected_of(name, spec, starts)     # phase0 is added by every run
        wanted.append(w)
        starts = [q[2] for q in w]
    if phase0 == 0:     # one long computation per job from the preset word
        for j, n in enumerate(spec.ns):
            cat = lambda k: None if rounds[0][k][j] is None else \
                np.concatenate([rounds[r][k][j] for r in range(ROUNDS)])
            p, final = phases(cat(0), cat(1), 0, spec.preset[j])
            wx, wy = want(name, cat(2), cat(3), p)
            for r in range(ROUNDS):
                assert np.array_equal(wanted[r][j][0], wx[r * n:(r + 1) * n])
                assert np.array_equal(wanted[r][j][1], wy[r * n:(r + 1) * n])
            assert wanted[-1][j][2] == final
    return cfg, spec, rounds, wanted


def set_round(spec, data):
    spec.fcw, spec.pm, spec.x, spec.y = data


@pytest.mark.gpu
@pytest.mark.parametrize("phase0", [0, 0x9e3779b1])
@pytest.mark.parametrize("name", ["cfg2", "ww38"])
def test_gpu_three_runs_on_new_data_continue_every_job(name, phase0, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    cfg, spec, rounds, wanted = continuation(name, phase0)
    plan = ca.Plan(cfg)
    d = DeviceBank(torch, plan, spec)
    assert d.bank.info()["fused"] == (1 if name == "cfg2" else 0)
    for r in range(ROUNDS):
        set_round(spec, rounds[r])
        d.upload()
        d.outs.fill_(SENT)
        d.bank.run()
        got, accs = d.results()
        assert_equals(got, accs, wanted[r], (name, phase0, r))
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "ww38"])
def test_gpu_a_captured_run_replayed_three_times_continues_three_times(name, monkeypatch):
    """one stream; once outside the capture first, on a bank with words of its
    own.  On the fused path the graph is two kernel nodes with one edge between
    them, counted as tests/test_fm_mix.py counts"""
    import torch
    clear_knobs(monkeypatch)
    cfg, spec, rounds, wanted = continuation(name, 0)
    plan = ca.Plan(cfg)
    set_round(spec, rounds[0])
    warm = DeviceBank(torch, plan, spec)
    warm.bank.run()
    torch.cuda.synchronize()
    warm.bank.close()
    d = DeviceBank(torch, plan, spec)
    fused = d.bank.info()["fused"]
    assert fused == (1 if name == "cfg2" else 0)

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
        d.bank.run(stream=stream.cuda_stream)
    finally:
        rc = hip.hipStreamEndCapture(h, C.byref(graph))
    assert rc == 0 and graph.value
    try:
        assert (d.outs == SENT).all().item()         # captured, not run
        cnt = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(cnt)) == 0
        if fused:
            assert cnt.value == 2
            nodes = (C.c_void_p * 2)()
            assert hip.hipGraphGetNodes(graph, nodes, C.byref(cnt)) == 0
            for i in range(2):
                t = C.c_int(-1)
                assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
                assert t.value == 0                  # hipGraphNodeTypeKernel
            edges = C.c_size_t(0)
            assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0
            assert edges.value == 1                  # two nodes, one chain
        ex = C.c_void_p()
        assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
        try:
            for r in range(ROUNDS):
                set_round(spec, rounds[r])
                d.upload()
                d.outs.fill_(SENT)
                torch.cuda.synchronize()
                assert hip.hipGraphLaunch(ex, h) == 0
                stream.synchronize()
                got, accs = d.results()
                assert_equals(got, accs, wanted[r], (name, r))
        finally:
            hip.hipGraphExecDestroy(ex)
    finally:
        hip.hipGraphDestroy(graph)
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "ww38"])
def test_gpu_empty_banks_run_and_write_nothing(name, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    for lengths in ([], [0, 0, 0]):
        spec = Spec(lengths, cfg.iw, 71, with_acc=True)
        d = DeviceBank(torch, plan, spec)
        info = d.bank.info()
        assert (info["samples"], info["spans"]) == (0, 0)
        assert info["fused"] == (1 if name == "cfg2" else 0)
        d.bank.run()
        got, accs = d.results()
        assert accs == spec.preset[:len(lengths)]
        assert (d.outs == SENT).all().item()
        d.bank.close()
    # a zero-length job's pointers are not looked at
    b = ca.MixBank(plan, [(3, 5, 7, 9, 11, 13, 0, 0, 15)])
    b.run()
    torch.cuda.synchronize()
    b.close()
    assert ca.lib().cordic_mixbank_run(None, None) == ca.ERR_ARGS
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "ww38"])
def test_gpu_create_refuses_overlaps_and_bad_jobs_with_nothing_written(name, monkeypatch):
    import torch
    from gpu_util import DEV
    clear_knobs(monkeypatch)
    cfg = both(name)[0]
    plan = ca.Plan(cfg)
    n = 64
    ins = torch.arange(8 * n, dtype=torch.int32, device=DEV)
    outs = torch.full((6 * n,), SENT, dtype=torch.int32, device=DEV)
    accs = torch.full((8,), SENT, dtype=torch.int32, device=DEV)
    f0, m0, x0, y0, f1, m1, x1, y1 = (ins[k * n:] for k in range(8))
    a0, b0, a1, b1 = (outs[k * n:] for k in range(4))
    c0, c1 = accs, accs[4:]

    def job(f=f0, m=m0, x=x0, y=y0, a=a0, b=b0, acc=c0):
        return (f, m, x, y, a, b, n, 0, acc)

    def other(f=f1, m=m1, x=x1, y=y1, a=a1, b=b1, acc=c1):
        return (f, m, x, y, a, b, n, 0, acc)

    def refused(*jobs, status=ca.ERR_ARGS, plan=plan):
        with pytest.raises(ca.CordicError) as e:
            ca.MixBank(plan, list(jobs))
        assert e.value.status == status

    odd = lambda t: t.data_ptr() + 2
    refused(job(), other(a=outs[n - 1:]))               # output over output
    refused(job(b=outs[n - 1:]))                        # ... of the same job
    refused(job(), other(b=outs[2 * n - 1:], a=outs[4 * n:]))
    refused(job(), other(a=ins[n - 1:]))                # output over another job's input
    refused(job(), other(b=ins[1:]))
    refused(job(a=ins[7 * n:]), other())
    refused(job(a=ins[n:]))                             # ... over its own d_pm
    refused(job(), other(acc=c0))                       # a shared d_acc
    refused(job(), other(acc=outs[n - 1:]))             # d_acc inside an output array
    refused(job(acc=outs[n:]))
    refused(job(acc=ins[5:]))                           # ... inside an input array
    for k in range(6):                                  # off the 4-byte grid
        a = [f0, m0, x0, y0, a0, b0]
        a[k] = odd(a[k])
        refused(job(*a))
    refused(job(acc=odd(c0)))
    for k in (0, 2, 3, 4, 5):                           # a NULL pointer that is needed
        a = [f0, m0, x0, y0, a0, b0]
        a[k] = None
        refused(job(*a))
    L = ca.lib()
    arr = (ca._native._CFmMixJob * 1)()
    for k, v in zip(FIELDS[:7], (f0, m0, x0, y0, a0, b0, c0)):
        setattr(arr[0], k, v.data_ptr())
    arr[0].n = n
    h = C.c_void_p(0x5a5a)
    for field, value in (("reserved", 1), ("n", (1 << 60) + 1)):
        setattr(arr[0], field, value)
        assert L.cordic_mixbank_create(plan._h, 1, arr, C.byref(h)) == ca.ERR_ARGS
        setattr(arr[0], field, 0 if field == "reserved" else n)
    assert L.cordic_mixbank_create(plan._h, 1 << 28, arr, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_mixbank_create(None, 1, arr, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_mixbank_create(plan._h, 1, None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_mixbank_create(plan._h, 1, arr, None) == ca.ERR_ARGS
    r2p = ca.Plan(ca.Config.from_cli(ca.R2P, 24, 24, 2, -1, 20))
    refused(job(), status=ca.ERR_MODE, plan=r2p)        # the wrong mode
    assert L.cordic_mixbank_create(r2p._h, 0, None, C.byref(h)) == ca.ERR_MODE
    r2p.close()
    assert h.value == 0x5a5a                            # no handle was made
    torch.cuda.synchronize()
    assert (outs == SENT).all().item() and (accs == SENT).all().item()
    assert torch.equal(ins, torch.arange(8 * n, dtype=torch.int32, device=DEV))
    # inputs may alias each other, within a job and between jobs; d_pm may be NULL
    b = ca.MixBank(plan, [job(y=x0, m=f0), other(f=f0, m=None, x=x0, y=x0)])
    accs.zero_()
    b.run()
    torch.cuda.synchronize()
    hh = outs.cpu().numpy()
    assert (hh[4 * n:] == SENT).all() and (hh[:4 * n] != SENT).any()
    b.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_create_refuses_two_to_the_32_spans_and_a_captured_legacy_stream(
        monkeypatch):
    """2^20 + 1 jobs of 4096 passes are 2^32 + 4096 spans of one pass (addresses
    that nothing dereferences: create refuses before it uploads)"""
    import torch
    clear_knobs(monkeypatch)
    plan = ca.Plan(both("cfg2")[0])
    L = ca.lib()
    k = (1 << 20) + 1
    n = MAX_SPANS * PASS
    dt = np.dtype([(f, "<u8") for f in FIELDS[:8]] + [("phase0", "<u4"), ("reserved", "<u4")])
    assert dt.itemsize == 72
    jobs = np.zeros(k, dtype=dt)
    at = np.arange(k, dtype=np.uint64) * np.uint64(4 * n)
    for i, f in enumerate(("d_fcw", "d_xval", "d_yval", "d_oxval", "d_oyval")):
        jobs[f] = np.uint64((i + 1) << 48) + at
    jobs["n"] = n
    h = C.c_void_p(0x5a5a)
    monkeypatch.setenv("CORDIC_FMXB_PASSES", "1")
    assert L.cordic_mixbank_create(plan._h, k, jobs.ctypes.data, C.byref(h)) == ca.ERR_ARGS
    assert h.value == 0x5a5a
    monkeypatch.delenv("CORDIC_FMXB_PASSES")

    # blocking uploads: not while the legacy stream is being captured -- which a
    # capture in the global mode on a BLOCKING stream amounts to (torch's own
    # streams are non-blocking: they do not take the legacy stream with them)
    spec = Spec([5, 1025], 32, 81)
    t = torch.zeros(8 * 64, dtype=torch.int32, device="cuda:0")
    one = (ca._native._CFmMixJob * 1)()
    for i, f in enumerate(("d_fcw", "d_xval", "d_yval", "d_oxval", "d_oyval")):
        setattr(one[0], f, t[64 * i:].data_ptr())
    one[0].n = 64
    hip = _hip()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hs = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(hs)) == 0     # (default flags: blocking)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(hs, 0) == 0     # hipStreamCaptureModeGlobal
    graph = C.c_void_p()
    try:
        rc = L.cordic_mixbank_create(plan._h, 1, one, C.byref(h))
    finally:
        hip.hipStreamEndCapture(hs, C.byref(graph))
        hip.hipGetLastError()
    if graph.value:
        hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(hs)
    print("create under a global capture: status %d" % rc)
    if rc == 0:
        L.cordic_mixbank_destroy(h)
    assert rc == ca.ERR_UNSUPPORTED and h.value == 0x5a5a
    assert (t == 0).all().item()
    d = DeviceBank(torch, plan, spec)                # and afterwards all is well
    d.bank.run()
    got, accs = d.results()
    assert_equals(got, accs, expected_of("cfg2", spec), "after the refusals")
    d.bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_run_from_another_device_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    plan = ca.Plan(both("cfg2")[0])
    b = ca.MixBank(plan, [])
    with torch.cuda.device(1):
        assert ca.lib().cordic_mixbank_run(b._h, None) == ca.ERR_ARGS
    b.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_the_example_builds_and_exits_0(tmp_path):
    """examples/afc_channeliser.c: one mixer bank into one demodulation bank,
    three rounds, against the per-channel calls"""
    exe = tmp_path / "afc_channeliser"
    r = subprocess.run(
        ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
         "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
         "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-o", str(exe),
         os.path.join(ROOT, "examples", "afc_channeliser.c"),
         "-L", os.path.join(ROOT, "cordic_amd"), "-lcordic_amd", "-L", "/opt/rocm/lib",
         "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "cordic_amd"),
         "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "256 channels" in r.stdout and "x 3 rounds" in r.stdout
    assert "0 words differ" in r.stdout and "fused, two launches" in r.stdout
