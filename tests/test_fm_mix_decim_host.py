"""The host layer of the decimating FM mixer banks (cordic_fm_mix_bank.h over
cordic_span_bank.h) and the single call's range check (cordic_hostargs.h), in a
stand-alone C++ program with its own main under the address and
undefined-behaviour sanitizers, in the style of tests/test_span_bank_host.py: no
Python in the checked process and no GPU.  k = 0, 1, 2, 5, 8 on both job
structs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "cordic_fm_mix_bank.h"
#include "cordic_hostargs.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced: every array of job j in a region of its own
template <typename J> static J job_at(size_t j, uint64_t n)
{
	J b;
	std::memset(&b, 0, sizeof b);
	const uintptr_t base = 0x100000000u * (j + 1);
	typedef decltype(b.d_oxval) out_t;
	typedef decltype(b.d_xval) in_t;
	b.d_fcw = (const uint32_t *)(base + 0x04);
	b.d_pm = j % 2 ? (const uint32_t *)(base + 0x10000008) : nullptr;
	b.d_xval = (in_t)(base + 0x20000000 + sizeof *b.d_xval);
	b.d_yval = (in_t)(base + 0x30000000);
	b.d_oxval = (out_t)(base + 0x40000000 + sizeof *b.d_oxval);
	b.d_oyval = (out_t)(base + 0x50000000);
	b.d_acc = j % 3 ? (uint32_t *)(base + 0x60000000) : nullptr;
	b.n = n;
	b.phase0 = (uint32_t)(j * 0x9e3779b1u);
	return b;
}

// every span's ox / oy at (s0 >> k) * esize, x / y at s0 * esize, fcw / pm at
// s0 * 4; the spans tile each job; the same spans as at k = 0
template <typename J> static void check_cut(uint32_t k, uint32_t passes, uint32_t cap)
{
	const uint64_t es = sizeof *J().d_xval, R = (uint64_t)1 << k;
	const uint64_t lens[] = {0, R, 2 * R, 1024 - R, 1024, 1024 + R, 2048 + R, 0,
		5 * 1024 + R, 40 * 1024, 40 * 1024 + 3 * R};
	std::vector<J> jobs;
	for (size_t j = 0; j < sizeof lens / sizeof *lens; j++)
		jobs.push_back(job_at<J>(j, lens[j]));
	EXPECT(fmxb_jobs_valid(jobs.size(), MixJobs(jobs.data(), k)));
	std::vector<MixSpan> spans, plain;
	uint32_t live = 0, live0 = 0;
	span_cut(kFmxbRule, jobs.size(), MixJobs(jobs.data(), k), passes, cap, &spans, &live);
	span_cut(kFmxbRule, jobs.size(), MixJobs(jobs.data()), passes, cap, &plain, &live0);
	EXPECT(spans.size() == plain.size() && live == live0 && live == 9);
	EXPECT(spans.size() == span_count(kFmxbRule, jobs.size(), MixJobs(jobs.data(), k),
		passes, cap));
	size_t at = 0;
	for (size_t j = 0; j < jobs.size(); j++) {
		const J &jb = jobs[j];
		uint64_t s0 = 0;
		while (s0 < jb.n) {
			EXPECT(at < spans.size());
			if (at >= spans.size())
				return;
			const MixSpan &s = spans[at], &p = plain[at];
			EXPECT(s.fcw == (uintptr_t)jb.d_fcw + s0 * 4);
			EXPECT(s.pm == (jb.d_pm ? (uintptr_t)jb.d_pm + s0 * 4 : 0));
			EXPECT(s.x == (uintptr_t)jb.d_xval + s0 * es);
			EXPECT(s.y == (uintptr_t)jb.d_yval + s0 * es);
			EXPECT(s.ox == (uintptr_t)jb.d_oxval + (s0 >> k) * es);
			EXPECT(s.oy == (uintptr_t)jb.d_oyval + (s0 >> k) * es);
			EXPECT(s.n >= 1 && s.n <= jb.n - s0 && s.n % R == 0 && s0 % 1024 == 0);
			EXPECT(s.n == p.n && s.idx == p.idx && s.flags == p.flags && s.start == p.start
				&& s.part0 == p.part0 && s.fcw == p.fcw && s.x == p.x && s.acc == p.acc);
			EXPECT(k ? (s0 ? s.ox != p.ox : s.ox == p.ox) : s.ox == p.ox);
			s0 += s.n;
			at++;
		}
		EXPECT(s0 == jb.n);
	}
	EXPECT(at == spans.size());
}

template <typename J> static void check_jobs(uint32_t k)
{
	const uint64_t es = sizeof *J().d_xval, R = (uint64_t)1 << k, n = 8 * R;
	typedef decltype(J().d_oxval) out_t;
	auto valid = [&](J a, J b, uint32_t kk) {
		const J two[2] = {a, b};
		return fmxb_jobs_valid(2, MixJobs(two, kk));
	};
	const J a = job_at<J>(0, n), b = job_at<J>(1, n);
	EXPECT(valid(a, b, k));
	// a job whose n is not a multiple of R
	J t = b;
	if (k) {
		t.n = n + 1; EXPECT(!valid(a, t, k)); EXPECT(valid(a, t, 0));
		t.n = n + R / 2; EXPECT(!valid(a, t, k));
		t.n = R - 1; EXPECT(!valid(a, t, k));
	}
	t = b; t.n = 0; t.reserved = 7; t.d_fcw = nullptr; EXPECT(valid(a, t, k));
	EXPECT(!valid(a, b, 9) && !fmxb_jobs_valid(0, MixJobs((const J *)nullptr, 9)));
	// outputs (n >> k) elements apart: their full-rate ranges would overlap,
	// the decimated ones do not -- and the converse, one element closer
	t = b; t.d_oxval = (out_t)((uintptr_t)a.d_oxval + (n >> k) * es);
	EXPECT(valid(a, t, k));
	if (k)
		EXPECT(!valid(a, t, 0));
	t.d_oxval = (out_t)((uintptr_t)a.d_oxval + ((n >> k) - 1) * es);
	EXPECT(!valid(a, t, k));
	// an output that ends where an input begins, and one element over it
	t = b; t.d_oyval = (out_t)((uintptr_t)a.d_xval - (n >> k) * es);
	EXPECT(valid(a, t, k));
	t.d_oyval = (out_t)((uintptr_t)a.d_xval - ((n >> k) - 1) * es);
	EXPECT(!valid(a, t, k));
	// the rest of cordic_mixbank_create's rules, word for word
	t = b; t.reserved = 1; EXPECT(!valid(a, t, k));
	t = b; t.d_acc = a.d_acc ? a.d_acc : (uint32_t *)a.d_oxval; EXPECT(!valid(a, t, k));
	t = b; t.d_oxval = nullptr; EXPECT(!valid(a, t, k));
	t = b; t.d_oxval = (out_t)((uintptr_t)b.d_oxval + es / 2); EXPECT(!valid(a, t, k));
	t = b; t.d_fcw = (const uint32_t *)((uintptr_t)b.d_fcw + 2); EXPECT(!valid(a, t, k));
}

// the single call's check: the outputs are (n >> k) elements long
static void check_call()
{
	const size_t n = 64, m = 8;
	const uintptr_t f = 0x10000, x = 0x20000, y = 0x30000, o0 = 0x40000, o1 = 0x50000,
		w = 0x60000, acc = 0x70000;
	auto ok = [&](uintptr_t a, uintptr_t b, unsigned k, uintptr_t ac) {
		return iq_call_ok(n, (void *)ac, nullptr, (void *)f, nullptr, (void *)x, (void *)y,
			(void *)a, (void *)b, 4, (void *)w, 64, k);
	};
	EXPECT(ok(o0, o1, 0, acc) && ok(o0, o1, 3, acc));
	EXPECT(ok(o0, o0 + 4 * m, 3, acc) && !ok(o0, o0 + 4 * m, 0, acc)
		&& !ok(o0, o0 + 4 * m - 4, 3, acc));
	EXPECT(ok(x - 4 * m, o1, 3, acc) && !ok(x - 4 * m + 4, o1, 3, acc)
		&& !ok(x - 4 * m, o1, 2, acc));
	EXPECT(!ok(o0, o1, 3, o0 + 4 * m - 4) && ok(o0, o1, 3, o0 + 4 * m));
}

int main()
{
	const uint32_t ks[] = {0, 1, 2, 5, 8};
	for (uint32_t k : ks) {
		for (uint32_t passes = 1; passes <= 4; passes *= 2) {
			check_cut<cordic_fmmix_job>(k, passes, kFmxbRule.max_spans);
			check_cut<cordic_fmmix_job16>(k, passes, 3);
		}
		check_jobs<cordic_fmmix_job>(k);
		check_jobs<cordic_fmmix_job16>(k);
	}
	check_call();
	EXPECT(sizeof(cordic_fmmix_job) == 72 && sizeof(cordic_fmmix_job16) == 72);
	if (!failures)
		std::printf("decim host ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_cutter_and_the_checks_at_k_0_1_2_5_8_under_address_and_ub_sanitizers(tmp_path):
    src, exe = tmp_path / "decim_host.cpp", tmp_path / "decim_host"
    src.write_text(PROGRAM)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "decim host ok" in r.stdout


def test_the_host_layer_touches_no_device():
    for head in ("cordic_fm_mix_bank.h", "cordic_span_bank.h", "cordic_hostargs.h"):
        text = open(os.path.join(CSRC, head)).read()
        assert "#include <hip" not in text and "hipMalloc" not in text, head
