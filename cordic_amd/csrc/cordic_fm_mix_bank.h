// cordic_fm_mix_bank.h -- FM mixer banks: many cordic_plan_fm_mix jobs of one
// p2r / sp2r plan in TWO launches (include/cordic_amd.h, "FM mixer banks"), on
// int32 or on int16 I/Q arrays (cordic_fmmix_job / cordic_fmmix_job16).  The
// span descriptors the host cuts at create, the cutter itself -- plain C++ that
// touches no device, so that a stand-alone program can run it under a
// sanitizer -- and the launcher of the two kernels that walk the descriptors
// (cordic_fm_mix_bank.hip).  Host-visible types only; the handle and its four
// entry points live with the plan, in cordic_abi.cpp.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_FM_MIX_BANK_H
#define CORDIC_FM_MIX_BANK_H

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "cordic_amd.h"
#include "cordic_bank_host.h"

namespace cordic_amd {

// A run of whole passes (1024 samples, kFmxPass) of ONE job, never across the
// job's end; only a job's last span may end in a partial pass.
struct MixSpan {
	uint64_t fcw, pm;	// addresses at the span's first sample (pm 0: none)
	uint64_t x, y, ox, oy;
	uint64_t acc;		// the job's d_acc, or 0
	uint64_t n;		// samples: >= 1
	uint32_t start;		// index of the job's start word
	uint32_t part0;		// index of the job's first partial sum
	uint32_t idx;		// this span's index within its job
	uint32_t flags;		// kMixSpanFirst | kMixSpanLast
	uint32_t phase0;	// the job's (the first span latches the start)
	uint32_t pad;
};				// 88 bytes
constexpr uint32_t kMixSpanFirst = 1, kMixSpanLast = 2;

constexpr uint64_t kFmxbPass = 1024;		// = kFmxPass
constexpr uint32_t kFmxbMaxSpans = 4096;	// per job; = kFmxMaxBlocks
constexpr uint32_t kFmxbMaxPasses = 1u << 20;	// a base span's: 2^30 samples
constexpr int	   kFmxbBlocksPerCu = 4;	// = kFmxBlocksPerCu

inline uint64_t fmxb_passes_of(uint64_t n)
{
	return n / kFmxbPass + (n % kFmxbPass ? 1 : 0);
}

// P, the passes of a base span, for a bank of `total_passes` on `cus` CUs: the
// tile-length rule (cordic_bank_host.h), 4 resident blocks per CU, steps 1, 2, 4, ...
inline uint32_t fmxb_passes(uint64_t total_passes, int cus)
{
	return bank_passes(total_passes, cus, kFmxbBlocksPerCu, 1, kFmxbMaxPasses);
}

// CORDIC_FMXB_PASSES / CORDIC_FMXB_MAX_SPANS (read at create): a power of two
// within 1 .. 2^20 replaces P; a value within 1 .. 4095 lowers the span cap.
inline uint32_t fmxb_forced_passes(const char *e, uint32_t p)
{
	return bank_forced_passes(e, kFmxbMaxPasses, p);
}
inline uint32_t fmxb_forced_cap(const char *e)
{
	const long v = e ? std::strtol(e, nullptr, 10) : 0;
	return (v >= 1 && v < (long)kFmxbMaxSpans) ? (uint32_t)v : kFmxbMaxSpans;
}

// passes per span of ONE job of n samples: P, doubled until the job has at
// most `cap` spans -- the single call's bound on what a span sums in front of
// itself
inline uint64_t fmxb_job_passes(uint64_t n, uint32_t passes, uint32_t cap)
{
	const uint64_t np = fmxb_passes_of(n);
	uint64_t pj = passes;
	while ((np + pj - 1) / pj > cap)
		pj *= 2;
	return pj;
}

// The jobs of a create, of either struct: cordic_fmmix_job16 is
// cordic_fmmix_job field for field but for the element type behind the four
// sample pointers, which the host never dereferences.  jobs[k] is job k as a
// cordic_fmmix_job; esize() the bytes of a sample, which is all the checks and
// the cutter know of the container.
struct MixJobs {
	const cordic_fmmix_job *j32 = nullptr;
	const cordic_fmmix_job16 *j16 = nullptr;
	MixJobs(const cordic_fmmix_job *j) : j32(j) {}
	MixJobs(const cordic_fmmix_job16 *j) : j16(j) {}
	MixJobs(std::nullptr_t) {}
	uint64_t esize() const { return j16 ? 2 : 4; }
	uint64_t n(size_t k) const { return j16 ? j16[k].n : j32[k].n; }
	cordic_fmmix_job operator[](size_t k) const
	{
		if (!j16)
			return j32[k];
		const cordic_fmmix_job16 &a = j16[k];
		cordic_fmmix_job b;
		b.d_fcw = a.d_fcw;
		b.d_pm = a.d_pm;
		b.d_xval = reinterpret_cast<const int32_t *>(a.d_xval);
		b.d_yval = reinterpret_cast<const int32_t *>(a.d_yval);
		b.d_oxval = reinterpret_cast<int32_t *>(a.d_oxval);
		b.d_oyval = reinterpret_cast<int32_t *>(a.d_oyval);
		b.d_acc = a.d_acc;
		b.n = a.n;
		b.phase0 = a.phase0;
		b.reserved = a.reserved;
		return b;
	}
};

// The argument checks of cordic_mixbank_create / _create16 that need no device:
// every job with n > 0 has non-NULL d_fcw, d_xval, d_yval, d_oxval, d_oyval, the
// four sample pointers on the grid of their element (4 or 2 bytes), d_fcw, d_pm
// and d_acc on the 4-byte grid, reserved == 0 and a length within SIZE_MAX >>
// 4; no output range (d_oxval, d_oyval, the word at d_acc) overlaps another
// output range or any input range of the bank (BankRanges, cordic_bank_host.h),
// by the true byte ranges: n * esize for a sample array, n * 4 for d_fcw / d_pm.
inline bool fmxb_jobs_valid(size_t njobs, MixJobs jobs)
{
	const uint64_t es = jobs.esize();
	BankRanges r;
	for (size_t k = 0; k < njobs; k++) {
		const cordic_fmmix_job jb = jobs[k];
		if (jb.n == 0)
			continue;
		// inputs, then outputs; pm is optional.  p[0], p[3]: words
		const uintptr_t p[6] = {(uintptr_t)jb.d_fcw, (uintptr_t)jb.d_xval,
			(uintptr_t)jb.d_yval, (uintptr_t)jb.d_pm, (uintptr_t)jb.d_oxval,
			(uintptr_t)jb.d_oyval};
		const uintptr_t a = (uintptr_t)jb.d_acc;
		if (!p[0] || !p[1] || !p[2] || !p[4] || !p[5]
				|| ((p[0] | p[3] | a) & 3u)
				|| ((p[1] | p[2] | p[4] | p[5]) & (es - 1))
				|| jb.reserved != 0 || jb.n > (~(size_t)0 >> 4))
			return false;
		for (int i = 0; i < 6; i++)
			if (p[i] && !r.add(p[i], jb.n * (i == 0 || i == 3 ? 4 : es), i >= 4))
				return false;
		if (a && !r.add(a, 4, true))
			return false;
	}
	return r.outputs_clear();
}

// spans the jobs cut into (saturating at 2^63)
inline uint64_t fmxb_count_spans(size_t njobs, MixJobs jobs, uint32_t passes,
		uint32_t cap)
{
	uint64_t t = 0;
	for (size_t k = 0; k < njobs; k++) {
		const uint64_t n = jobs.n(k);
		if (!n)
			continue;
		const uint64_t pj = fmxb_job_passes(n, passes, cap);
		t += (fmxb_passes_of(n) + pj - 1) / pj;
		if (t >> 63)
			break;
	}
	return t;
}

// Cuts valid jobs (fmxb_jobs_valid; fewer than 2^32 spans) into spans, in the
// jobs' order.  Start words are numbered by non-empty job, partial sums by
// span: the workspace of the run has *njobs_live + spans->size() words.  A
// span's addresses are byte addresses: its first sample is esize bytes per
// sample into the four sample arrays and 4 into d_fcw / d_pm.
inline void fmxb_cut(size_t njobs, MixJobs jobs, uint32_t passes, uint32_t cap,
		std::vector<MixSpan> *spans, uint32_t *njobs_live)
{
	const uint64_t es = jobs.esize();
	uint32_t live = 0;
	for (size_t k = 0; k < njobs; k++) {
		const cordic_fmmix_job jb = jobs[k];
		if (jb.n == 0)
			continue;
		const uint64_t len = fmxb_job_passes(jb.n, passes, cap) * kFmxbPass;
		const uint32_t part0 = (uint32_t)spans->size();
		uint32_t idx = 0;
		for (uint64_t s0 = 0; s0 < jb.n; s0 += len, idx++) {
			const uint64_t cnt = jb.n - s0 < len ? jb.n - s0 : len;
			const uint64_t at = s0 * 4, sat = s0 * es;
			spans->push_back(MixSpan{(uintptr_t)jb.d_fcw + at,
				jb.d_pm ? (uintptr_t)jb.d_pm + at : 0,
				(uintptr_t)jb.d_xval + sat, (uintptr_t)jb.d_yval + sat,
				(uintptr_t)jb.d_oxval + sat, (uintptr_t)jb.d_oyval + sat,
				(uintptr_t)jb.d_acc, cnt, live, part0, idx,
				(s0 ? 0u : kMixSpanFirst)
					| (s0 + cnt == jb.n ? kMixSpanLast : 0u),
				jb.phase0, 0u});
		}
		live++;
	}
	if (njobs_live)
		*njobs_live = live;
}

// The two launches, for a plan of which fmx_is_fused (cordic_fm_mix.h) is true
// -- fmx_is_fused16 where the spans were cut from 16-bit jobs (io16).
// d_start / d_part: the bank's workspace (one word per non-empty job, one per
// span).  cus: the device's, at create.  An empty table launches nothing.
// CORDIC_OK or CORDIC_ERR_DEVICE.
struct DxInfo;		// (cordic_internal.h)
int	launch_fmx_bank(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		const MixSpan *d_spans, uint32_t nspans, uint32_t *d_start,
		uint32_t *d_part, int cus, bool io16, void *stream);

} // namespace cordic_amd
#endif
