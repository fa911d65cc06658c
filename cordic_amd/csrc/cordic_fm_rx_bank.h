// cordic_fm_rx_bank.h -- receiver banks: many cordic_plan_fm_rx jobs of one
// plan and one converter in TWO launches (include/cordic_amd.h, "Tuned FM
// receiver"), on int32 or on int16 arrays (cordic_fmrx_job / cordic_fmrx_job16).
// What the bank adds to the prefix-sum banks' shared host layer
// (cordic_span_bank.h) -- its rule, with a halo and a second latched word per
// job, its span descriptor, its job check; plain C++ that touches no device, so
// that a stand-alone program can run it under a sanitizer
// (tests/test_fm_rx_host.py) -- and the launcher of the two kernels that walk
// the descriptors (cordic_fm_rx_bank.hip).  Host-visible types only; the handle
// and its entry points live in cordic_abi_fm.cpp.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_FM_RX_BANK_H
#define CORDIC_FM_RX_BANK_H

#include <array>
#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_bank_host.h"
#include "cordic_span_bank.h"

namespace cordic_amd {

// The bank's descriptor: a mixer bank's (the common head of a span around the
// addresses of the four sample arrays at the span's first sample) and, behind
// it, the job's d_last and dphase0, which the job's first span latches and its
// last span writes.  A span's first vector is the halo (fmrx::pass_loop): a span
// of P passes has 1024 P - 4 samples, and what lies in front of a span that is
// not its job's first is inside the job.
struct RxSpan {
	uint64_t fcw, pm;
	uint64_t x, y, mag, freq;
	uint64_t acc;
	uint64_t n;
	uint32_t start;
	uint32_t part0;
	uint32_t idx;
	uint32_t flags;
	uint32_t phase0;
	uint32_t pad;
	uint64_t last;
	uint32_t dphase0;
	uint32_t pad2;
};				// 104 bytes
static_assert(sizeof(RxSpan) == 104, "the descriptor is read as scalar words");

// passes of 1024 samples (= kFmrxPass) with a halo of 4 (= kFmrxHalo); at most
// 4096 spans per job; a base span of at most 2^20 passes; one further latched
// word per job.  The knobs, read at create: CORDIC_FMRXB_PASSES,
// CORDIC_FMRXB_MAX_SPANS.
constexpr SpanRule kFmrxbRule = {1024, 4096, 1u << 20, 4, 1};
constexpr int	   kFmrxbBlocksPerCu = 3;	// by its registers (cordic_fm_rx_bank.hip)

// A decimating bank (cordic_rxbank_create_decim, k = log2r in 1 .. 8): the halo
// is the R = 2^k input samples of the decimated sample in front, max(4, R) --
// a multiple of R, so every span begins and ends on a multiple of R.  k = 0:
// kFmrxbRule.
constexpr SpanRule fmrxb_rule(uint32_t log2r)
{
	return SpanRule{1024, 4096, 1u << 20, log2r > 2 ? 1u << log2r : 4u, 1};
}

// The jobs of a create, of either struct (JobView, cordic_span_bank.h), and the
// bank's k = log2r (0: cordic_rxbank_create), which every job of the view
// carries to the checks and to span_place (as MixJobs, cordic_fm_mix_bank.h).
// iq: the jobs of a cordic_rxbank_create_c16 (fmrxb_from_c16 below) -- 16-bit
// jobs whose d_xval is the job's d_iq, interleaved int16 I/Q of 2 n shorts on
// the 4-byte grid, and whose d_yval is NULL and not looked at.
struct RxJob : cordic_fmrx_job {
	uint32_t log2r = 0;
	bool	iq = false;
};
struct RxJobs : JobView<cordic_fmrx_job, cordic_fmrx_job16> {
	typedef JobView<cordic_fmrx_job, cordic_fmrx_job16> View;
	uint32_t log2r = 0;
	bool	iq = false;
	RxJobs(const cordic_fmrx_job *j, uint32_t k = 0) : View(j), log2r(k) {}
	RxJobs(const cordic_fmrx_job16 *j, uint32_t k = 0, bool interleaved = false)
		: View(j), log2r(k), iq(interleaved) {}
	RxJobs(std::nullptr_t) : View(nullptr) {}
	RxJob	operator[](size_t k) const
	{
		RxJob m;
		static_cast<cordic_fmrx_job &>(m) = View::operator[](k);
		m.log2r = log2r;
		m.iq = iq;
		return m;
	}
};

// a cordic_fmrx_job_c16 as the 16-bit job the bank's host layer works on
inline cordic_fmrx_job16 fmrxb_from_c16(const cordic_fmrx_job_c16 &c)
{
	cordic_fmrx_job16 j{};
	j.d_fcw = c.d_fcw;
	j.d_pm = c.d_pm;
	j.d_xval = c.d_iq;
	j.d_omag = c.d_omag;
	j.d_ofreq = c.d_ofreq;
	j.d_acc = c.d_acc;
	j.d_last = c.d_last;
	j.n = c.n;
	j.phase0 = c.phase0;
	j.dphase0 = c.dphase0;
	j.reserved = c.reserved;
	return j;
}
static_assert(sizeof(cordic_fmrx_job_c16) == 80, "as include/cordic_amd.h documents it");
#define F(f) CORDIC_SAME_FIELD(cordic_fmrx_job, cordic_fmrx_job16, f)
static_assert(sizeof(cordic_fmrx_job) == 88 && F(d_fcw) && F(d_pm) && F(d_xval)
	&& F(d_yval) && F(d_omag) && F(d_ofreq) && F(d_acc) && F(d_last) && F(n)
	&& F(phase0) && F(dphase0) && F(reserved),
	"cordic_fmrx_job16 is cordic_fmrx_job with 16-bit sample pointers");
#undef F

// The argument checks of cordic_rxbank_create / _create16 that need no device
// (bank_jobs_valid, cordic_span_bank.h): d_fcw and the four sample arrays
// required (of an interleaved job: d_iq, on the 4-byte grid, 4 n bytes), d_pm,
// d_acc and d_last optional; the outputs are d_omag, d_ofreq
// and the words at d_acc and d_last.  A decimating bank (jobs.log2r = k > 0): k
// <= 8, every n a multiple of 2^k, and the two outputs are n >> k elements long.
inline bool fmrxb_jobs_valid(size_t njobs, RxJobs jobs)
{
	if (jobs.log2r > 8)
		return false;
	for (size_t k = 0; k < njobs; k++)
		if (jobs.n(k) & (((uint64_t)1 << jobs.log2r) - 1))
			return false;
	return bank_jobs_valid(njobs, jobs,
		[](const RxJob &jb, uint64_t es, const void **word) {
			word[0] = jb.d_acc;
			word[1] = jb.d_last;
			// (interleaved: one input array of 2 * es bytes per sample)
			if (jb.iq)
				return std::array<JobArray, 6>{{{jb.d_fcw, 4, true, false},
					{jb.d_xval, 2 * es, true, false}, {nullptr, es, false, false},
					{jb.d_pm, 4, false, false},
					{jb.d_omag, es, true, true, jb.log2r},
					{jb.d_ofreq, es, true, true, jb.log2r}}};
			return std::array<JobArray, 6>{{{jb.d_fcw, 4, true, false},
				{jb.d_xval, es, true, false}, {jb.d_yval, es, true, false},
				{jb.d_pm, 4, false, false}, {jb.d_omag, es, true, true, jb.log2r},
				{jb.d_ofreq, es, true, true, jb.log2r}}};
		});
}

// what span_cut (cordic_span_bank.h) leaves to the bank: the sample arrays,
// `at` = s0 * esize bytes in, and the discriminator's word.  s0 is a multiple
// of R = 2^k (fmrxb_rule), so the outputs of a decimating bank begin (s0 >> k) *
// esize = at >> k bytes in.
// An interleaved job's x carries d_iq, 2 * at bytes in, and its y is unused.
inline void span_place(RxSpan *d, const RxJob &jb, uint64_t at)
{
	d->x = (uintptr_t)jb.d_xval + (jb.iq ? 2 * at : at);
	d->y = jb.iq ? 0 : (uintptr_t)jb.d_yval + at;
	d->mag = (uintptr_t)jb.d_omag + (at >> jb.log2r);
	d->freq = (uintptr_t)jb.d_ofreq + (at >> jb.log2r);
	d->last = (uintptr_t)jb.d_last;
	d->dphase0 = jb.dphase0;
}

// The converter's kernel parameters on the device, for launch 2 to fetch by
// scalar loads (fmrx::conv_params); the bank frees them with hipFree.
// CORDIC_OK or CORDIC_ERR_DEVICE.
int	fmrxb_upload_conv(const cordic_config &conv, uint32_t **d_conv);

// The two launches, for a plan and a converter of which the single call is
// fused (cordic_fm_rx.h), in the form the spans were cut for: the container of
// the jobs' arrays, form.iq where they were interleaved jobs (RxJobs::iq: the
// <30, IoC16> instances), form.log2r = k in 1 .. 8 for a decimating bank
// (fmrxb_rule(k); launch 2 is fm_rxbank_decim_xydir,
// cordic_fm_rx_bank_decim.hip).  d_start / d_part / d_prev: the bank's workspace
// (one word per non-empty job, one per span, one per non-empty job).  cus: the
// device's, at create.  An empty table launches nothing.  CORDIC_OK or
// CORDIC_ERR_DEVICE.
struct DxInfo;		// (cordic_internal.h)
struct FmForm;		// (cordic_fm_mix.h)
int	launch_fmrx_bank(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		const uint32_t *d_conv, const RxSpan *d_spans, uint32_t nspans,
		uint32_t *d_start, uint32_t *d_part, uint32_t *d_prev, int cus, FmForm form,
		void *stream);

// (as MixBankTraits, cordic_fm_mix_bank.h; the rule depends on the bank's k)
struct RxBankTraits {
	static bool jobs_valid(size_t njobs, RxJobs jobs) { return fmrxb_jobs_valid(njobs, jobs); }
	static SpanRule rule_of(const RxJobs &jobs) { return fmrxb_rule(jobs.log2r); }
	static constexpr const char *passes = "CORDIC_FMRXB_PASSES";
	static constexpr const char *max_spans = "CORDIC_FMRXB_MAX_SPANS";
	static constexpr int blocks_per_cu = kFmrxbBlocksPerCu;
};

} // namespace cordic_amd
#endif
