"""cordic_amd/csrc/cordic_fm_mix_bank.h on 16-bit jobs: the validity check and
the cutter of cordic_mixbank_create16, which serve both job structs through one
implementation (MixJobs), in a stand-alone program with its own main under the
address and undefined-behaviour sanitizers.  No GPU, no Python in the checked
process, nothing preloaded."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "cordic_fm_mix_bank.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced: job k's six arrays in six regions, the
// sample arrays at an odd element offset for odd k
template <typename Job, typename In, typename Out>
static Job job_at(size_t k, uint64_t n, bool pm, bool acc)
{
	Job j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t base = 0x10000000u + (uintptr_t)k * 0x10000000u;
	const uintptr_t odd = sizeof(In) * (k % 4);
	j.d_fcw = (const uint32_t *)(base + 4 * (k % 3));
	j.d_pm = pm ? (const uint32_t *)(base + 0x1000000000u) : nullptr;
	j.d_xval = (const In *)(base + 0x2000000000u + odd);
	j.d_yval = (const In *)(base + 0x3000000000u + odd);
	j.d_oxval = (Out *)(base + 0x4000000000u + odd);
	j.d_oyval = (Out *)(base + 0x5000000000u + odd);
	j.d_acc = acc ? (uint32_t *)(0x6000000000u + 16 * k) : nullptr;
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u);
	return j;
}
static cordic_fmmix_job16 job16(size_t k, uint64_t n, bool pm = true, bool acc = true)
{
	return job_at<cordic_fmmix_job16, int16_t, int16_t>(k, n, pm, acc);
}
static cordic_fmmix_job job32(size_t k, uint64_t n, bool pm = true, bool acc = true)
{
	return job_at<cordic_fmmix_job, int32_t, int32_t>(k, n, pm, acc);
}

// the spans of `jobs` tile every job exactly, in order: ES bytes per sample in
// the four sample arrays, 4 in fcw / pm
template <typename Job>
static void check_cut(const std::vector<Job> &jobs, uint32_t passes, uint32_t cap,
		uint64_t ES)
{
	std::vector<MixSpan> spans;
	uint32_t live = 0;
	span_cut(kFmxbRule, jobs.size(), MixJobs(jobs.data()), passes, cap, &spans, &live);
	EXPECT(spans.size() == span_count(kFmxbRule, jobs.size(), MixJobs(jobs.data()), passes, cap));
	size_t at = 0;
	uint32_t seen = 0;
	for (size_t k = 0; k < jobs.size(); k++) {
		const Job &jb = jobs[k];
		if (!jb.n)
			continue;
		const size_t first = at;
		const uint64_t pj = span_job_units(kFmxbRule, jb.n, passes, cap);
		uint64_t done = 0;
		while (done < jb.n) {
			EXPECT(at < spans.size());
			if (at >= spans.size())
				return;
			const MixSpan &s = spans[at];
			EXPECT(s.fcw == (uintptr_t)jb.d_fcw + done * 4);
			EXPECT(s.pm == (jb.d_pm ? (uintptr_t)jb.d_pm + done * 4 : 0));
			EXPECT(s.x == (uintptr_t)jb.d_xval + done * ES);
			EXPECT(s.y == (uintptr_t)jb.d_yval + done * ES);
			EXPECT(s.ox == (uintptr_t)jb.d_oxval + done * ES);
			EXPECT(s.oy == (uintptr_t)jb.d_oyval + done * ES);
			EXPECT(s.acc == (uintptr_t)jb.d_acc);
			EXPECT(s.phase0 == jb.phase0 && s.pad == 0);
			EXPECT(s.start == seen && s.part0 == first && s.idx == at - first);
			const bool is_first = done == 0;
			const bool is_last = jb.n - done <= pj * kFmxbRule.unit;
			EXPECT(s.n == (is_last ? jb.n - done : pj * kFmxbRule.unit));
			EXPECT(s.flags == ((is_first ? kSpanFirst : 0u)
				| (is_last ? kSpanLast : 0u)));
			done += s.n;
			at++;
		}
		EXPECT(done == jb.n);
		EXPECT(at - first <= cap);
		EXPECT(at - first == (span_units_of(kFmxbRule, jb.n) + pj - 1) / pj);
		seen++;
	}
	EXPECT(at == spans.size() && seen == live);
}

template <typename Job> static bool valid2(Job x, Job y)
{
	const Job two[2] = {x, y};
	return fmxb_jobs_valid(2, two);
}

int main()
{
	// exactly one pass, one more sample, and more than 4096 spans' worth
	const uint64_t huge = (uint64_t)4096 * 1024 + 1, more = (uint64_t)3 * 4096 * 1024 + 5;
	const uint64_t lens[] = {0, 1, 3, 4, 5, 1023, 1024, 1025, 2048, 2049, 3000, 9001,
		0, 4096 * 1024, huge, more};
	std::vector<cordic_fmmix_job16> j16;
	std::vector<cordic_fmmix_job> j32;
	for (size_t k = 0; k < sizeof lens / sizeof *lens; k++) {
		j16.push_back(job16(k, lens[k], k % 2 == 0, k % 3 != 0));
		j32.push_back(job32(k, lens[k], k % 2 == 0, k % 3 != 0));
	}
	EXPECT(fmxb_jobs_valid(j16.size(), j16.data()));
	EXPECT(fmxb_jobs_valid(j32.size(), j32.data()));
	EXPECT(MixJobs(j16.data()).esize() == 2 && MixJobs(j32.data()).esize() == 4);
	for (uint32_t p = 1; p <= 8; p *= 2) {
		check_cut(j16, p, kFmxbRule.max_spans, 2);
		check_cut(j32, p, kFmxbRule.max_spans, 4);
		check_cut(j16, p, 2, 2);
		check_cut(j32, p, 2, 4);
	}
	check_cut(std::vector<cordic_fmmix_job16>(), 1, kFmxbRule.max_spans, 2);
	{	// the three lengths by hand, P = 1
		std::vector<MixSpan> s;
		uint32_t live = 0;
		const cordic_fmmix_job16 a[3] = {job16(0, 1024), job16(1, 1025), job16(2, huge)};
		span_cut(kFmxbRule, 3, MixJobs(a), 1, kFmxbRule.max_spans, &s, &live);
		EXPECT(live == 3 && s.size() == 1 + 2 + 2049);
		EXPECT(s[0].n == 1024 && s[0].flags == (kSpanFirst | kSpanLast));
		EXPECT(s[1].n == 1024 && s[1].flags == kSpanFirst && s[1].idx == 0);
		EXPECT(s[2].n == 1 && s[2].flags == kSpanLast && s[2].idx == 1);
		EXPECT(s[2].part0 == 1 && s[2].start == 1);
		EXPECT(s[2].x == (uintptr_t)a[1].d_xval + 2048);	// 1024 shorts on
		EXPECT(s[2].oy == (uintptr_t)a[1].d_oyval + 2048);
		EXPECT(s[2].fcw == (uintptr_t)a[1].d_fcw + 4096);	// 1024 words on
		EXPECT(s[2].pm == (uintptr_t)a[1].d_pm + 4096);
		// 4097 passes: spans of two, 2048 whole ones and one sample behind them
		EXPECT(s[3].n == 2048 && s[3].part0 == 3 && s[3].start == 2);
		EXPECT(s[4].x == (uintptr_t)a[2].d_xval + 4096 && s[4].idx == 1);
		EXPECT(s[4].fcw == (uintptr_t)a[2].d_fcw + 8192);
		EXPECT(s.back().n == 1 && s.back().idx == 2048
			&& s.back().flags == kSpanLast);
		// the same jobs as 32-bit ones: 4 bytes per sample everywhere
		std::vector<MixSpan> w;
		const cordic_fmmix_job b[3] = {job32(0, 1024), job32(1, 1025), job32(2, huge)};
		span_cut(kFmxbRule, 3, MixJobs(b), 1, kFmxbRule.max_spans, &w, &live);
		EXPECT(live == 3 && w.size() == s.size());
		EXPECT(w[2].x == (uintptr_t)b[1].d_xval + 4096);
		EXPECT(w[2].fcw == (uintptr_t)b[1].d_fcw + 4096);
		for (size_t i = 0; i < w.size() && i < s.size(); i++)
			EXPECT(w[i].n == s[i].n && w[i].idx == s[i].idx && w[i].flags == s[i].flags
				&& w[i].part0 == s[i].part0 && w[i].start == s[i].start);
	}

	// the overlap rule over the true byte ranges: n shorts are 2 n bytes
	const uint64_t n = 64;
	const cordic_fmmix_job16 a = job16(0, n), b = job16(1, n);
	EXPECT(valid2(a, b));
	{ cordic_fmmix_job16 c = b; c.d_oxval = a.d_oxval + n - 1; EXPECT(!valid2(a, c)); }
	{ cordic_fmmix_job16 c = b; c.d_oxval = a.d_oxval + n; EXPECT(valid2(a, c)); }
	{ cordic_fmmix_job16 c = b; c.d_oxval = (int16_t *)a.d_xval + n - 1; EXPECT(!valid2(a, c)); }
	{ cordic_fmmix_job16 c = b; c.d_oxval = (int16_t *)a.d_xval + n; EXPECT(valid2(a, c)); }
	{ cordic_fmmix_job16 c = b; c.d_oyval = (int16_t *)a.d_yval - n + 1; EXPECT(!valid2(a, c)); }
	{ cordic_fmmix_job16 c = b; c.d_oyval = (int16_t *)a.d_yval - n; EXPECT(valid2(a, c)); }
	{ cordic_fmmix_job16 c = a; c.d_oyval = c.d_oxval + 1; EXPECT(!valid2(c, b)); }
	// ... and n * 4 for fcw / pm: an output 2 n bytes into them is still inside
	{ cordic_fmmix_job16 c = b; c.d_oxval = (int16_t *)a.d_fcw + n; EXPECT(!valid2(a, c)); }
	{ cordic_fmmix_job16 c = b; c.d_oxval = (int16_t *)a.d_fcw + 2 * n - 1; EXPECT(!valid2(a, c)); }
	{ cordic_fmmix_job16 c = b; c.d_oxval = (int16_t *)a.d_fcw + 2 * n; EXPECT(valid2(a, c)); }
	{ cordic_fmmix_job16 c = b; c.d_oyval = (int16_t *)a.d_pm + 2 * n - 1; EXPECT(!valid2(a, c)); }
	// d_acc: shared, inside an output's last short, clear behind it
	{ cordic_fmmix_job16 c = b; c.d_acc = a.d_acc; EXPECT(!valid2(a, c)); }
	{ cordic_fmmix_job16 c = a, d = b; c.d_oxval = (int16_t *)0x7000000000u;
	  d.d_acc = (uint32_t *)(0x7000000000u + 2 * n - 4); EXPECT(!valid2(c, d));
	  d.d_acc = (uint32_t *)(0x7000000000u + 2 * n); EXPECT(valid2(c, d)); }
	// inputs may alias
	{ cordic_fmmix_job16 c = b; c.d_xval = a.d_xval; c.d_yval = a.d_xval + 1;
	  c.d_fcw = a.d_fcw; EXPECT(valid2(a, c)); }
	// a job alone: the sample pointers on the 2-byte grid, the words on that of 4
	auto one = [](cordic_fmmix_job16 x) { return fmxb_jobs_valid(1, &x); };
	EXPECT(one(a));
#define OFF(field, type, by, ok) { cordic_fmmix_job16 c = a; \
	c.field = (type)((uintptr_t)c.field + by); EXPECT(one(c) == ok); }
	OFF(d_xval, const int16_t *, 2, true) OFF(d_yval, const int16_t *, 6, true)
	OFF(d_oxval, int16_t *, 2, true) OFF(d_oyval, int16_t *, 2, true)
	OFF(d_xval, const int16_t *, 1, false) OFF(d_yval, const int16_t *, 1, false)
	OFF(d_oxval, int16_t *, 1, false) OFF(d_oyval, int16_t *, 3, false)
	OFF(d_fcw, const uint32_t *, 2, false) OFF(d_pm, const uint32_t *, 2, false)
	OFF(d_acc, uint32_t *, 2, false) OFF(d_fcw, const uint32_t *, 4, true)
	{ cordic_fmmix_job16 c = a; c.d_xval = nullptr; EXPECT(!one(c)); }
	{ cordic_fmmix_job16 c = a; c.d_oyval = nullptr; EXPECT(!one(c)); }
	{ cordic_fmmix_job16 c = a; c.d_pm = nullptr; c.d_acc = nullptr; EXPECT(one(c)); }
	{ cordic_fmmix_job16 c = a; c.reserved = 1; EXPECT(!one(c)); }
	{ cordic_fmmix_job16 c = a; c.n = (~(size_t)0 >> 4) + 1; EXPECT(!one(c)); }
	{ cordic_fmmix_job16 c = a; c.n = 0; c.d_fcw = nullptr; c.reserved = 9;
	  c.d_oxval = (int16_t *)1; c.d_acc = b.d_acc; EXPECT(valid2(c, b)); }

	// the 32-bit job type answers as before: the 4-byte grid, n * 4 bytes
	const cordic_fmmix_job p = job32(0, n), q = job32(1, n);
	EXPECT(valid2(p, q));
	{ cordic_fmmix_job c = q; c.d_oxval = p.d_oxval + n - 1; EXPECT(!valid2(p, c)); }
	{ cordic_fmmix_job c = q; c.d_oxval = p.d_oxval + n; EXPECT(valid2(p, c)); }
	{ cordic_fmmix_job c = q; c.d_oxval = (int32_t *)p.d_xval + n - 1; EXPECT(!valid2(p, c)); }
	{ cordic_fmmix_job c = q; c.d_oxval = (int32_t *)((uintptr_t)p.d_xval + 2 * n);
	  EXPECT(!valid2(p, c)); }			// inside n * 4, behind n * 2
	{ cordic_fmmix_job c = p; c.d_xval = (const int32_t *)((uintptr_t)c.d_xval + 2);
	  EXPECT(!fmxb_jobs_valid(1, &c)); }		// off the 4-byte grid
	{ cordic_fmmix_job c = q; c.d_acc = p.d_acc; EXPECT(!valid2(p, c)); }
	EXPECT(fmxb_jobs_valid(0, nullptr));
	if (!failures)
		std::printf("cutter16 ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_host_cutter_on_16_bit_jobs_under_address_and_ub_sanitizers(tmp_path):
    src, exe = tmp_path / "cutter16.cpp", tmp_path / "cutter16"
    src.write_text(PROGRAM)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "cutter16 ok" in r.stdout


def test_one_implementation_serves_both_job_structs():
    """no second copy of the checks or the cutter, and the cutter touches no
    device"""
    text = open(os.path.join(CSRC, "cordic_fm_mix_bank.h")).read()
    assert len(re.findall(r"\binline\s+\w+\s+fmxb_jobs_valid\s*\(", text)) == 1
    assert "#include <hip" not in text and "hipMalloc" not in text
    # the span count and the cutter: the prefix-sum banks' shared layer
    assert '#include "cordic_span_bank.h"' in text
    text = open(os.path.join(CSRC, "cordic_span_bank.h")).read()
    for fn in ("span_count", "span_cut"):
        assert len(re.findall(r"\binline\s+\w+\s+%s\s*\(" % fn, text)) == 1, fn
    assert "#include <hip" not in text and "hipMalloc" not in text
