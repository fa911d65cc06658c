"""The host side of the decimating receiver and its banks under AddressSanitizer
and UBSan: the call check with decimated output ranges, the workspace rule, the
single call's span and the span cutter with halo = max(4, R), in a stand-alone
C++ program with its own main (as tests/test_fm_rx_host.py): no Python and no
GPU in the checked process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "cordic_fm_rx_decim.h"
#include "cordic_fm_rx_bank.h"
#include "cordic_hostargs.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced: job k's arrays lie 2^24 bytes apart
static const uintptr_t kBase = 0x100000000u;
template <typename J> static J rx_job(size_t k, uint64_t n)
{
	J j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t b = kBase + (uintptr_t)k * 0x10000000u;
	const uintptr_t es = sizeof *j.d_xval;
	j.d_fcw = (const uint32_t *)(b + 4 * (k % 4));
	j.d_pm = k % 2 ? (const uint32_t *)(b + 0x1000000u + 4 * (k % 3)) : nullptr;
	j.d_xval = (decltype(j.d_xval))(b + 0x2000000u + es * (k % 5));
	j.d_yval = (decltype(j.d_yval))(b + 0x3000000u + es * (k % 7));
	j.d_omag = (decltype(j.d_omag))(b + 0x4000000u + es * (k % 3));
	j.d_ofreq = (decltype(j.d_ofreq))(b + 0x5000000u + es * (k % 2));
	j.d_acc = k % 3 ? (uint32_t *)(0x6000000000u + 32 * k) : nullptr;
	j.d_last = k % 4 ? (uint32_t *)(0x6000000000u + 32 * k + 16) : nullptr;
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u);
	j.dphase0 = (uint32_t)(k * 0x85ebca77u);
	return j;
}

// every span yields a multiple of R, consecutive spans tile the job exactly,
// a span that is not the first has its halo inside the job, and the outputs
// are placed at s0 >> k
template <typename J>
static void check_cut(const std::vector<J> &jobs, uint32_t k, uint32_t base, uint32_t cap)
{
	const SpanRule r = fmrxb_rule(k);
	const uint64_t R = (uint64_t)1 << k, halo = R > 4 ? R : 4;
	EXPECT(r.halo == halo && r.unit == 1024 && r.words == 1 && r.max_spans == 4096);
	EXPECT(r.halo == fmrxd_halo(k) || k == 0);
	const uint64_t es = sizeof *jobs.data()->d_xval;
	std::vector<RxSpan> spans;
	uint32_t live = 0;
	const RxJobs view(jobs.data(), k);
	EXPECT(fmrxb_jobs_valid(jobs.size(), view));
	span_cut(r, jobs.size(), view, base, cap, &spans, &live);
	EXPECT(spans.size() == span_count(r, jobs.size(), view, base, cap));
	size_t at = 0;
	uint32_t seen = 0;
	for (size_t q = 0; q < jobs.size(); q++) {
		const J &jb = jobs[q];
		if (!jb.n)
			continue;
		const uint64_t uj = span_job_units(r, jb.n, base, cap);
		const uint64_t yield = uj * 1024 - halo;
		EXPECT(yield % R == 0);
		EXPECT(span_spans_of(r, jb.n, uj) <= cap);
		uint64_t s0 = 0;
		for (uint32_t idx = 0; s0 < jb.n; idx++, at++) {
			EXPECT(at < spans.size());
			if (at >= spans.size())
				return;
			const RxSpan &d = spans[at];
			const bool last = s0 + d.n == jb.n;
			EXPECT(d.n >= 1 && d.n % R == 0 && d.n <= yield && s0 + d.n <= jb.n);
			EXPECT(last || d.n == yield);
			EXPECT(s0 % R == 0 && (s0 == 0 || s0 >= halo));
			EXPECT(d.fcw == (uintptr_t)jb.d_fcw + 4 * s0);
			EXPECT(d.pm == (jb.d_pm ? (uintptr_t)jb.d_pm + 4 * s0 : 0));
			EXPECT(d.x == (uintptr_t)jb.d_xval + es * s0);
			EXPECT(d.y == (uintptr_t)jb.d_yval + es * s0);
			EXPECT(d.mag == (uintptr_t)jb.d_omag + es * (s0 >> k));
			EXPECT(d.freq == (uintptr_t)jb.d_ofreq + es * (s0 >> k));
			EXPECT(d.acc == (uintptr_t)jb.d_acc && d.last == (uintptr_t)jb.d_last);
			EXPECT(d.phase0 == jb.phase0 && d.dphase0 == jb.dphase0);
			EXPECT(d.start == seen && d.idx == idx);
			EXPECT(d.flags == ((s0 ? 0u : kSpanFirst) | (last ? kSpanLast : 0u)));
			s0 += d.n;
		}
		EXPECT(s0 == jb.n);
		seen++;
	}
	EXPECT(at == spans.size() && live == seen);
}

template <typename J> static void cuts()
{
	for (uint32_t k : {0u, 1u, 2u, 5u, 8u}) {
		const uint64_t R = (uint64_t)1 << k, halo = R > 4 ? R : 4, y1 = 1024 - halo;
		// one span; exactly one; a last span that is only a halo's worth longer;
		// several; an empty job; one group; a job that needs longer spans
		const uint64_t ns[] = {R, y1, y1 + halo, 2 * y1, 0, 2 * y1 + halo, 5 * 1024 + 3 * R,
			3 * (2048 - halo), 3 * (2048 - halo) + halo, 4096 * y1 + R, 65536};
		std::vector<J> jobs;
		for (uint64_t n : ns)
			jobs.push_back(rx_job<J>(jobs.size(), n));
		for (uint32_t base : {1u, 2u, 16u})
			for (uint32_t cap : {4096u, 2u, 1u, 7u})
				check_cut(jobs, k, base, cap);
		// the single call's span on 1, 2 and 1000 blocks
		for (size_t cap : {(size_t)1, (size_t)2, (size_t)1000})
			for (uint64_t n : ns) {
				if (!n || !k)
					continue;
				const CallSpan cs = call_span((size_t)n, cap, kFmrxPass, fmrxd_halo(k));
				EXPECT(cs.grid >= 1 && cs.grid <= cap && cs.span % R == 0);
				EXPECT((cs.span + fmrxd_halo(k)) % kFmrxPass == 0);
				EXPECT(cs.span * cs.grid >= n && cs.span * (cs.grid - 1) < n);
			}
		// a job that is no multiple of R, and k = 9
		if (k) {
			std::vector<J> odd = {rx_job<J>(1, 3 * R), rx_job<J>(2, 3 * R + R / 2)};
			EXPECT(!fmrxb_jobs_valid(odd.size(), RxJobs(odd.data(), k)));
			EXPECT(fmrxb_jobs_valid(1, RxJobs(odd.data(), k)));
		}
	}
	std::vector<J> one = {rx_job<J>(1, 512)};
	EXPECT(!fmrxb_jobs_valid(1, RxJobs(one.data(), 9)));
	EXPECT(fmrxb_jobs_valid(1, RxJobs(one.data(), 8)));
}

// the job check takes the outputs' (n >> k) range
template <typename J> static void ranges()
{
	const uint64_t n = 2048;
	const uint32_t k = 3;
	const J a = rx_job<J>(1, n);
	const uintptr_t es = sizeof *a.d_xval;
	auto valid = [&](std::vector<J> v, uint32_t kk) {
		return fmrxb_jobs_valid(v.size(), RxJobs(v.data(), kk));
	};
	J t = a;
	t.d_ofreq = (decltype(t.d_ofreq))((uintptr_t)a.d_omag + es * (n >> k));
	EXPECT(valid({t}, k) && !valid({t}, 0));	// behind n >> k elements, inside n
	t.d_ofreq = (decltype(t.d_ofreq))((uintptr_t)a.d_omag + es * ((n >> k) - 1));
	EXPECT(!valid({t}, k));
	t = a;		// an output that ends where an input begins
	t.d_omag = (decltype(t.d_omag))((uintptr_t)a.d_xval - es * (n >> k));
	EXPECT(valid({t}, k) && !valid({t}, 0));
	t.d_omag = (decltype(t.d_omag))((uintptr_t)a.d_xval - es * ((n >> k) - 1));
	EXPECT(!valid({t}, k));
	J b = rx_job<J>(2, n);
	b.d_last = a.d_last;
	EXPECT(!valid({a, b}, k));			// two jobs sharing a word
}

// the single call's check and workspace rule
static void call()
{
	const size_t n = 4096;
	const uintptr_t f = 0x100000, x = 0x200000, y = 0x300000, o0 = 0x400000, w = 0x800000,
		ac = 0x700000, la = 0x700010;
	auto ok = [&](uintptr_t mag, uintptr_t freq, size_t es, unsigned k, uintptr_t last) {
		return iq_call_ok(n, (void *)ac, (void *)last, (void *)f, nullptr, (void *)x,
			(void *)y, (void *)mag, (void *)freq, es, (void *)w, kFmrxWorkBytes, k);
	};
	for (size_t es : {(size_t)4, (size_t)2})
		for (unsigned k : {1u, 3u, 8u}) {
			const size_t m = n >> k;
			EXPECT(ok(o0, o0 + m * es, es, k, la));		// back to back
			EXPECT(!ok(o0, o0 + m * es - es, es, k, la));
			EXPECT(!ok(o0, o0 + m * es, es, 0, la));	// n elements each: overlap
			EXPECT(ok(x - m * es, o0, es, k, la));		// up to an input
			EXPECT(!ok(x - m * es + es, o0, es, k, la));
			EXPECT(ok(o0, o0 + 0x10000, es, k, o0 + ((m * es + 3) & ~(size_t)3)));
			EXPECT(!ok(o0, o0 + 0x10000, es, k, o0 + (((m - 1) * es) & ~(size_t)3)));
			EXPECT(!ok(o0 + 1, o0 + 0x10000, es, k, la));	// off its grid
		}
	// the workspace: fused is the receiver's; the fallback's parts on the grid
	EXPECT(fmrxd_work_bytes(true, 123, 4096, 3, 4) == kFmrxWorkBytes);
	EXPECT(fmrxd_work_bytes(true, 123, 0, 3, 4) == 0 && fmrxd_work_bytes(false, 160, 0, 3, 2) == 0);
	for (size_t es : {(size_t)4, (size_t)2}) {
		size_t last = 0;
		for (uint32_t k : {1u, 2u, 5u, 8u})
			for (size_t q = 1; q < 70; q += 3) {
				const size_t nn = q << k, m = q;
				const size_t wb = fmrxd_work_bytes(false, 160, nn, k, es);
				EXPECT(wb % 16 == 0);
				EXPECT(wb == 160 + 2 * ((m * es + 15) / 16 * 16) + fmd_work_bytes(m));
				EXPECT(wb <= 160 + (es == 4 ? 9 : 5) * m + 96);
				if (q > 1)
					EXPECT(wb >= last);
				last = wb;
			}
	}
	EXPECT(fmrxd_halo(1) == 4 && fmrxd_halo(2) == 4 && fmrxd_halo(3) == 8
		&& fmrxd_halo(8) == 256);
	EXPECT(fmxd_shape_ok(1024, 8) && !fmxd_shape_ok(1024, 9) && !fmxd_shape_ok(1020, 3));
	// the ring holds what a flush left and a pass adds
	EXPECT(kFmrxdRing >= kFmrxdFlush - 1 + 512 + 1 && !(kFmrxdRing & (kFmrxdRing - 1)));
}

int main()
{
	cuts<cordic_fmrx_job>();
	cuts<cordic_fmrx_job16>();
	ranges<cordic_fmrx_job>();
	ranges<cordic_fmrx_job16>();
	call();
	if (!failures)
		std::printf("rx decim host ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_call_check_the_workspace_and_the_cutter_under_address_and_ub_sanitizers(tmp_path):
    src, exe = tmp_path / "rx_decim.cpp", tmp_path / "rx_decim"
    src.write_text(PROGRAM)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "rx decim host ok" in r.stdout


def test_the_host_headers_need_no_hip():
    for name in ("cordic_fm_rx_decim.h", "cordic_fm_rx_bank.h"):
        text = open(os.path.join(CSRC, name)).read()
        head = text.split("#ifdef __HIPCC__")[0]
        assert "#include <hip" not in head and "hipMalloc" not in head, name
