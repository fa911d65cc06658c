// cordic_span_bank.h -- the host layer of the FM banks, written once.
//   - For all three (cordic_fm_demod_bank.h, cordic_fm_mix_bank.h,
//     cordic_table_fm_bank.h): JobView, the jobs of a create as either job
//     struct, and bank_jobs_valid, the argument checks that need no device.
//   - For the two PREFIX-SUM banks (FM mixer, FM oscillator), which are one
//     two-launch scheme: the host cuts every job into spans of whole units (a
//     pass of 1024 samples, a tile of 4096), never across a job's end; launch 1
//     (span_reduce, cordic_span_reduce.h) sums each span's tuning words into a
//     workspace word; launch 2, the bank's own kernel, adds the job's partials
//     in front of a span to the job's start word and runs the single call's
//     loop.  A bank is a SpanRule, a descriptor struct with the common head
//     below and a span_place that sets the descriptor's sample addresses.
// Plain C++ that touches no device, so that a stand-alone program can run it
// under a sanitizer (tests/test_span_bank_host.py and the banks' own).
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_SPAN_BANK_H
#define CORDIC_SPAN_BANK_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "cordic_bank_host.h"

namespace cordic_amd {

// ---- the jobs of a create

// Field f sits at the same place, with the same size, in job structs A and B.
// A bank states it for every field next to its JobView.
#define CORDIC_SAME_FIELD(A, B, f) \
	(offsetof(A, f) == offsetof(B, f) && sizeof(A::f) == sizeof(B::f))

// The jobs of a create, of either struct: J16 is J32 field for field but for
// the element type behind the sample pointers, which the host never
// dereferences.  jobs[k] is job k as a J32; esize() the bytes of a sample, which
// is all the checks and the cutters know of the container -- by the pointer's
// type: a NULL one still names its container.  (A plain pointer to either
// struct converts.)
template <typename J32, typename J16> struct JobView {
	static_assert(sizeof(J16) == sizeof(J32) && alignof(J16) == alignof(J32)
		&& std::is_trivially_copyable<J32>::value
		&& std::is_trivially_copyable<J16>::value,
		"operator[] copies a J16 into a J32 byte for byte");
	const J32 *j32 = nullptr;
	const J16 *j16 = nullptr;
	uint64_t es = 4;
	JobView(const J32 *j) : j32(j) {}
	JobView(const J16 *j) : j16(j), es(2) {}
	JobView(std::nullptr_t) {}
	bool	none() const { return !j32 && !j16; }
	uint64_t esize() const { return es; }
	uint64_t n(size_t k) const { return j16 ? j16[k].n : j32[k].n; }
	J32	operator[](size_t k) const
	{
		if (!j16)
			return j32[k];
		J32 b;
		std::memcpy(&b, j16 + k, sizeof b);
		return b;
	}
};

// One array of a job: its address, the bytes a sample takes in it (4 for
// tuning and phase words, esize for a sample array), whether it has to be
// there and whether the bank writes it.  shift: the array holds n >> shift
// elements, not n (the outputs of a decimating mixer bank).
struct JobArray {
	const void *p;
	uint64_t bytes;
	bool	required, is_output;
	uint32_t shift = 0;
};

// The argument checks of a bank's create that need no device.  list(jb, es,
// word) names the arrays of job jb, inputs before outputs, and the optional
// 4-byte words the job reads and writes: word[0] (d_acc, d_last) and, for a
// bank whose jobs name two, word[1] (the receiver banks' d_last).  Every job
// with n > 0 has its required pointers non-NULL, each pointer on the grid of its
// element, the words on the 4-byte grid, reserved == 0 and a length within
// SIZE_MAX >> 4; no output range (the words among them, so two jobs -- or one
// job twice -- naming the same word) overlaps another output range or any
// input range of the bank (BankRanges, cordic_bank_host.h), by the true byte
// ranges, n * bytes ((n >> shift) * bytes for an array that says so).  A job of
// no samples is not looked at.
template <typename Jobs, typename List>
inline bool bank_jobs_valid(size_t njobs, Jobs jobs, List list)
{
	BankRanges r;
	for (size_t k = 0; k < njobs; k++) {
		const auto jb = jobs[k];
		if (jb.n == 0)
			continue;
		const void *word[2] = {nullptr, nullptr};
		const auto arrays = list(jb, jobs.esize(), word);
		if ((((uintptr_t)word[0] | (uintptr_t)word[1]) & 3u) || jb.reserved != 0
				|| jb.n > (~(size_t)0 >> 4))
			return false;
		for (const JobArray &a : arrays)
			if ((a.required && !a.p) || ((uintptr_t)a.p & (a.bytes - 1)))
				return false;
		for (const JobArray &a : arrays)
			if (a.p && !r.add((uintptr_t)a.p, (jb.n >> a.shift) * a.bytes, a.is_output))
				return false;
		for (const void *w : word)
			if (w && !r.add((uintptr_t)w, 4, true))
				return false;
	}
	return r.outputs_clear();
}

// ---- the prefix-sum banks

// unit: the samples of a pass or tile; max_spans: the most spans of one job
// (what a span of launch 2 sums in front of itself, the single call's bound);
// max_units: the most units of a base span.  halo: the samples at the head of
// a span's units that belong to the span in front and are made again, not
// stored (the receiver banks: 4; a span of u units yields u * unit - halo
// samples).  words: further latched words per job in the run's workspace,
// behind the partial sums (the receiver banks: 1, the phase in front of sample
// 0).  Both are 0 for the mixer and the oscillator banks.
struct SpanRule {
	uint64_t unit;
	uint32_t max_spans;
	uint32_t max_units;
	uint32_t halo = 0;
	uint32_t words = 0;
};

// a span's flags: its job's first, its job's last
constexpr uint32_t kSpanFirst = 1, kSpanLast = 2;

// A span descriptor is a struct of the bank's own layout (launch 2 reads it as
// scalar words) with these fields, which span_cut fills and span_reduce reads:
//	uint64_t fcw, pm;	// addresses at the span's first sample (pm 0: none)
//	uint64_t acc;		// the job's d_acc, or 0
//	uint64_t n;		// samples: >= 1
//	uint32_t start;		// index of the job's start word
//	uint32_t part0;		// index of the job's first partial sum
//	uint32_t idx;		// this span's index within its job
//	uint32_t flags;		// kSpanFirst | kSpanLast
//	uint32_t phase0;	// the job's (the first span latches the start)
//	uint32_t pad;
// and, between pm and acc, the addresses of its sample arrays.  A span is a run
// of whole units of ONE job, never across the job's end; only a job's last
// span may end in a partial unit.

inline uint64_t span_units_of(const SpanRule &r, uint64_t n)
{
	return n / r.unit + (n % r.unit ? 1 : 0);
}

// The units of a base span for a bank of `total_units` on `cus` CUs with
// `blocks_per_cu` (none: 1) resident blocks each: the tile-length rule
// (cordic_bank_host.h), the longest span, in the steps 1, 2, 4, ..., that still
// gives every resident block four.
inline uint32_t span_base_units(const SpanRule &r, uint64_t total_units, int cus,
		int blocks_per_cu)
{
	return bank_passes(total_units, cus, blocks_per_cu > 0 ? blocks_per_cu : 1, 1,
		r.max_units);
}

// The two knobs of a create, as the environment variable's value `e` (NULL:
// not set): a power of two within 1 .. max_units replaces the base length; a
// value within 1 .. max_spans - 1 lowers the span cap.
inline uint32_t span_forced_base(const SpanRule &r, const char *e, uint32_t base)
{
	return bank_forced_passes(e, r.max_units, base);
}
inline uint32_t span_forced_cap(const SpanRule &r, const char *e)
{
	const long v = e ? std::strtol(e, nullptr, 10) : 0;
	return (v >= 1 && v < (long)r.max_spans) ? (uint32_t)v : r.max_spans;
}

// spans of ONE job of n samples at uj units per span (without a halo: its
// units over uj, rounded up)
inline uint64_t span_spans_of(const SpanRule &r, uint64_t n, uint64_t uj)
{
	const uint64_t yield = uj * r.unit - r.halo;
	return n / yield + (n % yield ? 1 : 0);
}

// units per span of ONE job of n samples: the base length, doubled until the
// job has at most `cap` spans
inline uint64_t span_job_units(const SpanRule &r, uint64_t n, uint32_t base, uint32_t cap)
{
	uint64_t uj = base;
	while (span_spans_of(r, n, uj) > cap)
		uj *= 2;
	return uj;
}

// spans the jobs cut into (saturating at 2^63)
template <typename Jobs>
inline uint64_t span_count(const SpanRule &r, size_t njobs, Jobs jobs, uint32_t base,
		uint32_t cap)
{
	uint64_t t = 0;
	for (size_t k = 0; k < njobs; k++) {
		const uint64_t n = jobs.n(k);
		if (!n)
			continue;
		t += span_spans_of(r, n, span_job_units(r, n, base, cap));
		if (t >> 63)
			break;
	}
	return t;
}

// Cuts valid jobs (the bank's *_jobs_valid; fewer than 2^32 spans) into spans,
// in the jobs' order.  Start words are numbered by non-empty job, partial sums
// by span: the workspace of the run has *njobs_live * (1 + r.words) +
// spans->size() words.  A
// span's addresses are byte addresses: its first sample is 4 bytes per sample
// into d_fcw / d_pm and esize into the sample arrays, which the bank's
// span_place(&span, job, s0 * esize) sets.
template <typename SPAN, typename Jobs>
inline void span_cut(const SpanRule &r, size_t njobs, Jobs jobs, uint32_t base,
		uint32_t cap, std::vector<SPAN> *spans, uint32_t *njobs_live)
{
	const uint64_t es = jobs.esize();
	uint32_t live = 0;
	for (size_t k = 0; k < njobs; k++) {
		const auto jb = jobs[k];
		if (jb.n == 0)
			continue;
		const uint64_t len = span_job_units(r, jb.n, base, cap) * r.unit - r.halo;
		const uint32_t part0 = (uint32_t)spans->size();
		uint32_t idx = 0;
		for (uint64_t s0 = 0; s0 < jb.n; s0 += len, idx++) {
			const uint64_t cnt = jb.n - s0 < len ? jb.n - s0 : len;
			SPAN d{};
			d.fcw = (uintptr_t)jb.d_fcw + s0 * 4;
			d.pm = jb.d_pm ? (uintptr_t)jb.d_pm + s0 * 4 : 0;
			span_place(&d, jb, s0 * es);
			d.acc = (uintptr_t)jb.d_acc;
			d.n = cnt;
			d.start = live;
			d.part0 = part0;
			d.idx = idx;
			d.flags = (s0 ? 0u : kSpanFirst) | (s0 + cnt == jb.n ? kSpanLast : 0u);
			d.phase0 = jb.phase0;
			spans->push_back(d);
		}
		live++;
	}
	if (njobs_live)
		*njobs_live = live;
}

} // namespace cordic_amd
#endif
