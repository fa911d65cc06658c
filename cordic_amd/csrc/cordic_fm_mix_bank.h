// cordic_fm_mix_bank.h -- FM mixer banks: many cordic_plan_fm_mix jobs of one
// p2r / sp2r plan in TWO launches (include/cordic_amd.h, "FM mixer banks"), on
// int32 or on int16 I/Q arrays (cordic_fmmix_job / cordic_fmmix_job16).  What
// the bank adds to the prefix-sum banks' shared host layer (cordic_span_bank.h:
// the cutter, the span counts, the knobs) -- its rule, its span descriptor, its
// job check; plain C++ that touches no device, so that a stand-alone program
// can run it under a sanitizer -- and the launcher of the two kernels that walk
// the descriptors (cordic_fm_mix_bank.hip).  Host-visible types only; the
// handle and its entry points live in cordic_abi_fm.cpp.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_FM_MIX_BANK_H
#define CORDIC_FM_MIX_BANK_H

#include <array>
#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_bank_host.h"
#include "cordic_span_bank.h"

namespace cordic_amd {

// The bank's descriptor: the common head of a span (cordic_span_bank.h) around
// the addresses of the four sample arrays at the span's first sample.  A pass
// is 1024 samples (kFmxPass).
struct MixSpan {
	uint64_t fcw, pm;
	uint64_t x, y, ox, oy;
	uint64_t acc;
	uint64_t n;
	uint32_t start;
	uint32_t part0;
	uint32_t idx;
	uint32_t flags;
	uint32_t phase0;
	uint32_t pad;
};				// 88 bytes
static_assert(sizeof(MixSpan) == 88, "the descriptor is read as scalar words");

// passes of 1024 samples (= kFmxPass); at most 4096 spans per job (=
// kFmxMaxBlocks); a base span of at most 2^20 passes, 2^30 samples.  The knobs,
// read at create: CORDIC_FMXB_PASSES, CORDIC_FMXB_MAX_SPANS.
constexpr SpanRule kFmxbRule = {1024, 4096, 1u << 20};
constexpr int	   kFmxbBlocksPerCu = 4;	// = kFmxBlocksPerCu

// The jobs of a create, of either struct (JobView, cordic_span_bank.h), and the
// bank's k = log2r (0: cordic_mixbank_create; cordic_mixbank_create_decim: the
// outputs hold n >> k sums of R = 2^k tuned samples), which every job of the
// view carries to the checks and to span_place.
// iq: the jobs of a cordic_mixbank_create_c16 (fmxb_from_c16 below) -- 16-bit
// jobs whose d_xval is the job's d_iq and whose d_oxval is its d_oiq, interleaved
// int16 I/Q of 2 n and 2 (n >> k) shorts on the 4-byte grid; d_yval and d_oyval
// are NULL and not looked at.
struct MixJob : cordic_fmmix_job {
	uint32_t log2r = 0;
	bool	iq = false;
};
struct MixJobs : JobView<cordic_fmmix_job, cordic_fmmix_job16> {
	typedef JobView<cordic_fmmix_job, cordic_fmmix_job16> View;
	uint32_t log2r = 0;
	bool	iq = false;
	MixJobs(const cordic_fmmix_job *j, uint32_t k = 0) : View(j), log2r(k) {}
	MixJobs(const cordic_fmmix_job16 *j, uint32_t k = 0, bool interleaved = false)
		: View(j), log2r(k), iq(interleaved) {}
	MixJobs(std::nullptr_t) : View(nullptr) {}
	MixJob	operator[](size_t k) const
	{
		MixJob m;
		static_cast<cordic_fmmix_job &>(m) = View::operator[](k);
		m.log2r = log2r;
		m.iq = iq;
		return m;
	}
};

// a cordic_fmmix_job_c16 as the 16-bit job the bank's host layer works on
inline cordic_fmmix_job16 fmxb_from_c16(const cordic_fmmix_job_c16 &c)
{
	cordic_fmmix_job16 j{};
	j.d_fcw = c.d_fcw;
	j.d_pm = c.d_pm;
	j.d_xval = c.d_iq;
	j.d_oxval = c.d_oiq;
	j.d_acc = c.d_acc;
	j.n = c.n;
	j.phase0 = c.phase0;
	j.reserved = c.reserved;
	return j;
}
static_assert(sizeof(cordic_fmmix_job_c16) == 56, "as include/cordic_amd.h documents it");
#define F(f) CORDIC_SAME_FIELD(cordic_fmmix_job, cordic_fmmix_job16, f)
static_assert(sizeof(cordic_fmmix_job) == 72 && F(d_fcw) && F(d_pm) && F(d_xval)
	&& F(d_yval) && F(d_oxval) && F(d_oyval) && F(d_acc) && F(n) && F(phase0)
	&& F(reserved), "cordic_fmmix_job16 is cordic_fmmix_job with 16-bit sample pointers");
#undef F

// The argument checks of cordic_mixbank_create / _create16 that need no device
// (bank_jobs_valid, cordic_span_bank.h): d_fcw, the four sample arrays
// required, d_pm and d_acc optional; the outputs are d_oxval, d_oyval and the
// word at d_acc.  A decimating bank (jobs.log2r = k > 0): k <= 8, every n a
// multiple of 2^k, and the two outputs are n >> k elements long.  Interleaved
// jobs: d_iq and d_oiq required, on the 4-byte grid, 4 n and 4 (n >> k) bytes.
inline bool fmxb_jobs_valid(size_t njobs, MixJobs jobs)
{
	if (jobs.log2r > 8)
		return false;
	for (size_t k = 0; k < njobs; k++)
		if (jobs.n(k) & (((uint64_t)1 << jobs.log2r) - 1))
			return false;
	return bank_jobs_valid(njobs, jobs,
		[](const MixJob &jb, uint64_t es, const void **word) {
			*word = jb.d_acc;
			// (interleaved: one array of 2 * es bytes per sample on either side)
			if (jb.iq)
				return std::array<JobArray, 6>{{{jb.d_fcw, 4, true, false},
					{jb.d_xval, 2 * es, true, false}, {nullptr, es, false, false},
					{jb.d_pm, 4, false, false},
					{jb.d_oxval, 2 * es, true, true, jb.log2r},
					{nullptr, es, false, true, jb.log2r}}};
			return std::array<JobArray, 6>{{{jb.d_fcw, 4, true, false},
				{jb.d_xval, es, true, false}, {jb.d_yval, es, true, false},
				{jb.d_pm, 4, false, false}, {jb.d_oxval, es, true, true, jb.log2r},
				{jb.d_oyval, es, true, true, jb.log2r}}};
		});
}

// what span_cut (cordic_span_bank.h) leaves to the bank: the sample arrays,
// `at` = s0 * esize bytes in.  s0 is whole passes of 1024, a multiple of R = 2^k
// <= 256, so the outputs of a decimating bank begin (s0 >> k) * esize = at >> k
// bytes in.  An interleaved job's x carries d_iq, 2 * at = 4 s0 bytes in, its ox
// d_oiq, 4 (s0 >> k) bytes in, and its y and oy are unused.
inline void span_place(MixSpan *d, const MixJob &jb, uint64_t at)
{
	if (jb.iq) {
		d->x = (uintptr_t)jb.d_xval + 2 * at;
		d->ox = (uintptr_t)jb.d_oxval + 2 * (at >> jb.log2r);
		d->y = d->oy = 0;
		return;
	}
	d->x = (uintptr_t)jb.d_xval + at;
	d->y = (uintptr_t)jb.d_yval + at;
	d->ox = (uintptr_t)jb.d_oxval + (at >> jb.log2r);
	d->oy = (uintptr_t)jb.d_oyval + (at >> jb.log2r);
}

// The two launches, for a plan of which fmx_is_fused (cordic_fm_mix.h) is true
// -- fmx_is_fused16 where the spans were cut from 16-bit jobs (io16).
// d_start / d_part: the bank's workspace (one word per non-empty job, one per
// span).  cus: the device's, at create.  An empty table launches nothing.
// log2r = k in 1 .. 8: the spans were cut for a decimating bank, and launch 2 is
// fm_mixbank_decim_xydir (cordic_fm_mix_bank_decim.hip).
// iq: they were cut from interleaved jobs (MixJobs::iq), for the <30, IoC16io>
// instances.
// CORDIC_OK or CORDIC_ERR_DEVICE.
struct DxInfo;		// (cordic_internal.h)
int	launch_fmx_bank(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		const MixSpan *d_spans, uint32_t nspans, uint32_t *d_start,
		uint32_t *d_part, int cus, bool io16, void *stream, uint32_t log2r = 0,
		bool iq = false);

// what the create of the plan-side banks (plan_bank_create, cordic_abi_fm.cpp)
// asks of a bank besides its view of the jobs
struct MixBankTraits {
	static bool jobs_valid(size_t njobs, MixJobs jobs) { return fmxb_jobs_valid(njobs, jobs); }
	static SpanRule rule_of(const MixJobs &) { return kFmxbRule; }
	static constexpr const char *passes = "CORDIC_FMXB_PASSES";
	static constexpr const char *max_spans = "CORDIC_FMXB_MAX_SPANS";
	static constexpr int blocks_per_cu = kFmxbBlocksPerCu;
};

#ifdef __HIPCC__
// Launch 2 of a decimating bank, for launch_fmx_bank
// (cordic_fm_mix_bank_decim.hip); unit: an fmx::Unit (cordic_fm_mix.h); false: no
// instance.
namespace dev { struct CoreParams; struct DirArgs; }
bool	launch_fmx_bank_decim_walk(int unit, int nlive, int ngroups, unsigned grid,
		size_t lds, void *stream, const dev::CoreParams &kp, const dev::DirArgs &da,
		const MixSpan *d_spans, uint32_t nspans, const uint32_t *d_start,
		const uint32_t *d_part, uint32_t xw, uint32_t log2r);

// Launch 2 of a bank of interleaved jobs (fmx::kUnitC16): the <30, N, IoC16io>
// instances of the two bank kernels, each in an object of its own (the source
// compiled with -DCORDIC_FMX_C16; see cordic_fm_mix.h).  The plain form ignores
// log2r.  false: no instance.
typedef bool FmxWalkC16(int nlive, int ngroups, unsigned grid, size_t lds, void *stream,
		const dev::CoreParams &kp, const dev::DirArgs &da, const MixSpan *d_spans,
		uint32_t nspans, const uint32_t *d_start, const uint32_t *d_part, uint32_t xw,
		uint32_t log2r);
FmxWalkC16 launch_fmx_bank_walk_c16, launch_fmx_bank_decim_walk_c16;
#endif

} // namespace cordic_amd
#endif
