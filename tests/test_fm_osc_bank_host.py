"""The host side of the FM oscillator banks (cordic_table_fm_bank.h): the
cutter and the job checks in a stand-alone C++ program with its own main, under
the address and undefined-behaviour sanitizers.  No Python in the checked
process and no GPU, as in tests/test_bank_host.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "cordic_table_fm_bank.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced: job k's arrays in regions of their own
template <typename J> static J job_at(size_t k, uint64_t n, bool pm, bool cos, bool acc)
{
	J j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t base = 0x10000000u + (uintptr_t)k * 0x100000u + 4 * (k % 4);
	j.d_fcw = (const uint32_t *)(base);
	j.d_pm = pm ? (const uint32_t *)(base + 0x1000000000u) : nullptr;
	j.d_sin = (decltype(j.d_sin))(base + 0x2000000000u + 2 * (sizeof *j.d_sin == 2));
	j.d_cos = cos ? (decltype(j.d_cos))(base + 0x3000000000u) : nullptr;
	j.d_acc = acc ? (uint32_t *)(0x6000000000u + 16 * k) : nullptr;
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u);
	return j;
}

template <typename J>
static void check_cut(const std::vector<J> &jobs, uint32_t tiles, uint32_t cap)
{
	const uint64_t es = sizeof *jobs.data()->d_sin;
	std::vector<FmSpan> spans;
	uint32_t live = 0;
	span_cut(kFmobRule, jobs.size(), FmJobs(jobs.data()), tiles, cap, &spans, &live);
	EXPECT(spans.size() == span_count(kFmobRule, jobs.size(), FmJobs(jobs.data()), tiles, cap));
	size_t at = 0;
	uint32_t seen = 0;
	for (size_t k = 0; k < jobs.size(); k++) {
		const J &jb = jobs[k];
		if (!jb.n)
			continue;
		const size_t first = at;
		uint64_t done = 0;
		uint64_t full = 0;		// the length of this job's whole spans
		while (done < jb.n) {
			EXPECT(at < spans.size());
			if (at >= spans.size())
				return;
			const FmSpan &s = spans[at];
			// the spans tile [0, n) exactly, in order: byte addresses
			EXPECT(s.fcw == (uintptr_t)jb.d_fcw + done * 4);
			EXPECT(s.pm == (jb.d_pm ? (uintptr_t)jb.d_pm + done * 4 : 0));
			EXPECT(s.sin == (uintptr_t)jb.d_sin + done * es);
			EXPECT(s.cos == (jb.d_cos ? (uintptr_t)jb.d_cos + done * es : 0));
			EXPECT(s.acc == (uintptr_t)jb.d_acc);
			EXPECT(s.phase0 == jb.phase0 && s.pad == 0);
			EXPECT(s.n >= 1 && s.n <= jb.n - done);
			EXPECT(s.start == seen && s.part0 == first && s.idx == at - first);
			const bool is_first = done == 0, is_last = done + s.n == jb.n;
			EXPECT(s.flags == ((is_first ? kSpanFirst : 0u)
				| (is_last ? kSpanLast : 0u)));
			if (!is_last) {		// whole tiles, all of one length
				EXPECT(s.n % kFmobRule.unit == 0);
				EXPECT(full == 0 || s.n == full);
				full = s.n;
			} else {
				EXPECT(full == 0 || s.n <= full);
			}
			if (full) {		// T, or T doubled
				const uint64_t p = full / kFmobRule.unit;
				EXPECT(p >= tiles && p % tiles == 0
					&& !((p / tiles) & (p / tiles - 1)));
			}
			done += s.n;
			at++;
		}
		EXPECT(done == jb.n);
		const size_t count = at - first;
		EXPECT(count <= cap);
		// doubled only as far as the cap asks
		const uint64_t nt = span_units_of(kFmobRule, jb.n);
		const uint64_t tj = span_job_units(kFmobRule, jb.n, tiles, cap);
		EXPECT(count == (nt + tj - 1) / tj);
		EXPECT(tj == tiles || (nt + tj / 2 - 1) / (tj / 2) > cap);
		seen++;
	}
	EXPECT(at == spans.size() && seen == live);
}

// the span counts of the lengths of the issue, by hand
static void check_counts()
{
	const uint64_t lens[] = {0, 1, 4095, 4096, 4097, 5 * 4096 + 3};
	const uint64_t t1[] = {0, 1, 1, 1, 2, 6}, t2[] = {0, 1, 1, 1, 1, 3};
	// cap 3 at T = 1: 6 tiles -> spans of 2 tiles; 2 tiles stay 2 spans
	const uint64_t c3[] = {0, 1, 1, 1, 2, 3};
	for (int i = 0; i < 6; i++) {
		const cordic_fmosc_job j = job_at<cordic_fmosc_job>(0, lens[i], true, true, true);
		EXPECT(span_count(kFmobRule, 1, FmJobs(&j), 1, kFmobRule.max_spans) == t1[i]);
		EXPECT(span_count(kFmobRule, 1, FmJobs(&j), 2, kFmobRule.max_spans) == t2[i]);
		EXPECT(span_count(kFmobRule, 1, FmJobs(&j), 1, 3) == c3[i]);
	}
	auto fmob_job_tiles = [](uint64_t n, uint32_t tiles, uint32_t cap) {
		return span_job_units(kFmobRule, n, tiles, cap);
	};
	EXPECT(fmob_job_tiles(5 * 4096 + 3, 1, 3) == 2 && fmob_job_tiles(9 * 4096, 1, 3) == 4);
	EXPECT(fmob_job_tiles(9 * 4096, 1, 1024) == 1 && fmob_job_tiles(4097, 2, 1) == 2);
	EXPECT(fmob_job_tiles(1025 * 4096, 1, 1024) == 2);
	EXPECT(fmob_job_tiles(1024 * 4096, 1, 1024) == 1);
}

template <typename J> static void check_container()
{
	const uint64_t lens[] = {0, 1, 4095, 4096, 4097, 5 * 4096 + 3, 0, 7, 3 * 4096 + 7,
		(1 << 16) + 3, 9 * 4096, 2 * 4096, 12345};
	std::vector<J> jobs;
	for (size_t k = 0; k < sizeof lens / sizeof *lens; k++)
		jobs.push_back(job_at<J>(k, lens[k], k % 2 == 0, k % 3 != 1, k % 3 != 0));
	EXPECT(fmob_jobs_valid(jobs.size(), jobs.data()));
	for (uint32_t t = 1; t <= 16; t *= 2) {		// every forced T
		check_cut(jobs, t, kFmobRule.max_spans);
		check_cut(jobs, t, 3);			// a forced span cap of 3
		check_cut(jobs, t, 1);
	}
	check_cut(jobs, 1, 7);
	check_cut(std::vector<J>(), 1, kFmobRule.max_spans);
	{	// a job of the greatest length stays within the cap
		std::vector<J> big(1, job_at<J>(0, ~(size_t)0 >> 4, false, false, true));
		EXPECT(span_count(kFmobRule, 1, FmJobs(big.data()), 1, kFmobRule.max_spans)
			<= kFmobRule.max_spans);
		EXPECT(span_count(kFmobRule, 1, FmJobs(big.data()), 1, 3) <= 3);
	}

	// every refusal of the job check
	const uint64_t n = 64, es = sizeof *jobs.data()->d_sin;
	typedef decltype(jobs.data()->d_sin) out_t;
	const J a = job_at<J>(0, n, true, true, true), b = job_at<J>(1, n, true, true, true);
	auto valid = [](J x, J y) {
		const J two[2] = {x, y};
		return fmob_jobs_valid(2, two);
	};
	auto one = [](J x) { return fmob_jobs_valid(1, &x); };
	EXPECT(valid(a, b) && one(a));
	// output over output: of another job, of the same, by the TRUE byte ranges
	{ J c = b; c.d_sin = a.d_sin + n - 1; EXPECT(!valid(a, c)); }
	{ J c = b; c.d_sin = a.d_sin + n; EXPECT(valid(a, c)); }
	{ J c = b; c.d_cos = a.d_sin; EXPECT(!valid(a, c)); }
	{ J c = a; c.d_cos = c.d_sin + 1; EXPECT(!valid(c, b)); }
	{ J c = a; c.d_cos = c.d_sin + n; EXPECT(valid(c, b)); }
	// output over input: of the same job, of another, each kind of input
	{ J c = b; c.d_sin = (out_t)((uintptr_t)a.d_fcw + 4 * n - es); EXPECT(!valid(a, c)); }
	{ J c = b; c.d_sin = (out_t)((uintptr_t)a.d_fcw + 4 * n); EXPECT(valid(a, c)); }
	{ J c = b; c.d_cos = (out_t)a.d_pm; EXPECT(!valid(a, c)); }
	{ J c = a; c.d_sin = (out_t)c.d_fcw; EXPECT(!valid(c, b)); }
	{ J c = b; c.d_sin = (out_t)((uintptr_t)a.d_fcw - n * es); EXPECT(valid(a, c)); }
	{ J c = b; c.d_sin = (out_t)((uintptr_t)a.d_fcw - n * es + es); EXPECT(!valid(a, c)); }
	// d_acc: shared by two jobs, inside an output, inside an input
	{ J c = b; c.d_acc = a.d_acc; EXPECT(!valid(a, c)); }
	{ J c = b; c.d_acc = a.d_acc + 1; EXPECT(valid(a, c)); }
	{ J c = b; c.d_acc = (uint32_t *)((uintptr_t)a.d_cos + 8); EXPECT(!valid(a, c)); }
	{ J c = b; c.d_acc = (uint32_t *)a.d_fcw + n - 1; EXPECT(!valid(a, c)); }
	{ J c = a; c.d_acc = (uint32_t *)c.d_pm; EXPECT(!valid(c, b)); }
	// inputs may alias, within a job and between jobs
	{ J c = b; c.d_fcw = a.d_fcw; c.d_pm = a.d_fcw + 1; EXPECT(valid(a, c)); }
	{ J c = a; c.d_pm = c.d_fcw; EXPECT(valid(c, b)); }
	// a job alone: NULLs, the grids, reserved, the length
	{ J c = a; c.d_pm = nullptr; c.d_cos = nullptr; c.d_acc = nullptr; EXPECT(one(c)); }
	{ J c = a; c.d_fcw = nullptr; EXPECT(!one(c)); }
	{ J c = a; c.d_sin = nullptr; EXPECT(!one(c)); }
#define OFF(field, type, by, ok) { J c = a; \
	c.field = (type)((uintptr_t)c.field + by); EXPECT(one(c) == ok); }
	OFF(d_fcw, const uint32_t *, 2, false) OFF(d_pm, const uint32_t *, 2, false)
	OFF(d_acc, uint32_t *, 2, false) OFF(d_fcw, const uint32_t *, 1, false)
	OFF(d_sin, out_t, 1, false) OFF(d_cos, out_t, 1, false)
	// 2 bytes off: the 16-bit container's own grid
	OFF(d_sin, out_t, 2, (es == 2)) OFF(d_cos, out_t, 2, (es == 2))
	OFF(d_sin, out_t, 4, true) OFF(d_fcw, const uint32_t *, 4, true)
	{ J c = a; c.reserved = 1; EXPECT(!one(c)); }
	{ J c = a; c.n = (~(size_t)0 >> 4) + 1; EXPECT(!one(c)); }
	// a zero-length job's pointers are not looked at
	{ J c = a; c.n = 0; c.d_fcw = nullptr; c.reserved = 9;
	  c.d_sin = (out_t)3; c.d_acc = b.d_acc; EXPECT(valid(c, b)); }
	EXPECT(fmob_jobs_valid(0, nullptr));
}

int main()
{
	static_assert(sizeof(cordic_fmosc_job) == 56 && sizeof(cordic_fmosc_job16) == 56, "");
	check_counts();
	check_container<cordic_fmosc_job>();
	check_container<cordic_fmosc_job16>();

	// T by the bank's size: the longest span that leaves 4 per resident block
	auto fmob_tiles = [](uint64_t total_tiles, int cus, int blocks_per_cu) {
		return span_base_units(kFmobRule, total_tiles, cus, blocks_per_cu);
	};
	EXPECT(fmob_tiles(0, 256, 2) == 1 && fmob_tiles(4095, 256, 2) == 1);
	EXPECT(fmob_tiles(4096, 256, 2) == 2 && fmob_tiles(4096, 256, 1) == 4);
	EXPECT(fmob_tiles(16384, 256, 2) == 8 && fmob_tiles(16384, 0, 2) == 8);
	EXPECT(fmob_tiles(16384, 256, 0) == 16);	// (no count: one block per CU)
	EXPECT(fmob_tiles(~(uint64_t)0, 1, 1) == kFmobRule.max_units);
	// the knobs
	EXPECT(span_forced_base(kFmobRule, nullptr, 4) == 4 && span_forced_base(kFmobRule, "8", 4) == 8);
	EXPECT(span_forced_base(kFmobRule, "3", 4) == 4 && span_forced_base(kFmobRule, "0", 4) == 4);
	EXPECT(span_forced_base(kFmobRule, "-2", 4) == 4 && span_forced_base(kFmobRule, "x", 4) == 4);
	EXPECT(span_forced_base(kFmobRule, "262144", 4) == 262144);
	EXPECT(span_forced_base(kFmobRule, "524288", 4) == 4);
	EXPECT(span_forced_cap(kFmobRule, nullptr) == 1024 && span_forced_cap(kFmobRule, "3") == 3);
	EXPECT(span_forced_cap(kFmobRule, "0") == 1024 && span_forced_cap(kFmobRule, "1024") == 1024);
	EXPECT(span_forced_cap(kFmobRule, "99999") == 1024 && span_forced_cap(kFmobRule, "1023") == 1023);
	if (!failures)
		std::printf("cutter ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_cutter_and_the_job_checks_under_address_and_ub_sanitizers(tmp_path):
    src, exe = tmp_path / "fmob_host.cpp", tmp_path / "fmob_host"
    src.write_text(PROGRAM)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "cutter ok" in r.stdout
