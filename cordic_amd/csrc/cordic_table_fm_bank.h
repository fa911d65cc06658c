// cordic_table_fm_bank.h -- FM oscillator banks: many cordic_table_fm /
// cordic_quad_fm jobs of one sine core in TWO launches (include/cordic_amd.h,
// "FM oscillator banks"), on int32 or on int16 outputs (cordic_fmosc_job /
// cordic_fmosc_job16).  What the bank adds to the prefix-sum banks' shared host
// layer (cordic_span_bank.h: the cutter, the span counts, the knobs) -- its
// rule, its span descriptor, its job check; plain C++ that touches no device,
// so that a stand-alone program can run it under a sanitizer
// (tests/test_fm_osc_bank_host.py) -- and the launcher of the two kernels that
// walk the descriptors (cordic_table_fm_bank.hip).  Host-visible types only;
// the handle and its seven entry points live with the cores, in
// cordic_abi_table.cpp.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_TABLE_FM_BANK_H
#define CORDIC_TABLE_FM_BANK_H

#include <array>
#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_bank_host.h"
#include "cordic_span_bank.h"

namespace cordic_amd {

// The bank's descriptor: the common head of a span (cordic_span_bank.h) around
// the addresses of the outputs at the span's first sample (cos 0: sine only).
// A tile is 4096 samples (kFmTile).
struct FmSpan {
	uint64_t fcw, pm;
	uint64_t sin, cos;
	uint64_t acc;
	uint64_t n;
	uint32_t start;
	uint32_t part0;
	uint32_t idx;
	uint32_t flags;
	uint32_t phase0;
	uint32_t pad;
};				// 72 bytes
static_assert(sizeof(FmSpan) == 72, "the descriptor is read as scalar words");

// tiles of 4096 samples (= kFmTile); at most 1024 spans per job (=
// kFmMaxBlocks: one partial per thread of launch 2); a base span of at most
// 2^18 tiles, 2^30 samples.  The knobs, read at create: CORDIC_FMOB_TILES,
// CORDIC_FMOB_MAX_SPANS.
constexpr SpanRule kFmobRule = {4096, 1024, 1u << 18};

// The jobs of a create, of either struct (JobView, cordic_span_bank.h)
struct FmJobs : JobView<cordic_fmosc_job, cordic_fmosc_job16> {
	using JobView::JobView;
	bool	quadrature(size_t k) const
	{
		return j16 ? j16[k].d_cos != nullptr : j32[k].d_cos != nullptr;
	}
};
#define F(f) CORDIC_SAME_FIELD(cordic_fmosc_job, cordic_fmosc_job16, f)
static_assert(sizeof(cordic_fmosc_job) == 56 && F(d_fcw) && F(d_pm) && F(d_sin)
	&& F(d_cos) && F(d_acc) && F(n) && F(phase0) && F(reserved),
	"cordic_fmosc_job16 is cordic_fmosc_job with 16-bit output pointers");
#undef F

// The argument checks of the four creates that need no device
// (bank_jobs_valid, cordic_span_bank.h): d_fcw and d_sin required, d_pm, d_cos
// and d_acc optional; the outputs are d_sin, d_cos and the word at d_acc.
inline bool fmob_jobs_valid(size_t njobs, FmJobs jobs)
{
	return bank_jobs_valid(njobs, jobs,
		[](const cordic_fmosc_job &jb, uint64_t es, const void **word) {
			*word = jb.d_acc;
			return std::array<JobArray, 4>{{{jb.d_fcw, 4, true, false},
				{jb.d_pm, 4, false, false}, {jb.d_sin, es, true, true},
				{jb.d_cos, es, false, true}}};
		});
}

// what span_cut (cordic_span_bank.h) leaves to the bank: the outputs, `at`
// bytes in
inline void span_place(FmSpan *d, const cordic_fmosc_job &jb, uint64_t at)
{
	d->sin = (uintptr_t)jb.d_sin + at;
	d->cos = jb.d_cos ? (uintptr_t)jb.d_cos + at : 0;
}

// ---- the launcher (cordic_table_fm_bank.hip)
struct SineCore;	// (cordic_table_nco.h)

// What a create asks of the core: the blocks of launch 2 that one CU holds at a
// time on the layout that with_layout (cordic_table_nco.h) chooses for `c` --
// its fall-back to the L2 gather included -- into *blocks_per_cu.  CORDIC_OK;
// CORDIC_ERR_UNSUPPORTED: a quadratic core whose tables exceed 64 KiB;
// CORDIC_ERR_DEVICE: no layout serves the core.  The caller has checked
// c.sane() and the container.
int	fmob_resident(const SineCore &c, bool io16, int *blocks_per_cu);

// The two launches.  d_start / d_part: the bank's workspace (one word per
// non-empty job, one per span).  cus: the device's, at create.  An empty table
// launches nothing.  CORDIC_OK, CORDIC_ERR_DEVICE, or what fmob_resident
// answers.
int	launch_fmosc_bank(const SineCore &c, const FmSpan *d_spans, uint32_t nspans,
		uint32_t *d_start, uint32_t *d_part, int cus, bool io16, void *stream);

} // namespace cordic_amd
#endif
