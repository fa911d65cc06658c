// cordic_fm_mix.h -- the FM mixer (cordic_plan_fm_mix, cordic_plan_fm_mix_info,
// cordic_plan_fm_mix_workspace; include/cordic_amd.h): the rotator with
// looked-up directions whose phase is the running sum of per-sample tuning
// words, made in the kernel,
//   p_i = start + fcw[0] + .. + fcw[i-1] + pm[i]      (mod 2^32)
//   (ox_i, oy_i) = cordic_p2r(x_i, y_i, p_i).
// The launcher and the host checks for cordic_abi.cpp, where the plan and with
// it the three entry points live; the fallback (cordic_phase_accumulate into
// the workspace, then cordic_plan_p2r) is put together there.
//
// Neither unit holds a kernel of the DESIGN section 4.4 sweep (no swept
// workload has per-sample tuning words), so tools/build_stamp.py does not hash
// them.
#ifndef CORDIC_FM_MIX_H
#define CORDIC_FM_MIX_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_internal.h"
#include "cordic_table_fm.h"

namespace cordic_amd {

// Fused kernel: a block of 256 threads makes kFmxPass consecutive samples per
// pass, 4 per lane, and owns a contiguous span of whole passes; a launch has
// at most kFmxMaxBlocks blocks.  Its workspace is fm_reduce's: one word for
// the latched start (in a 16-byte slot) and one partial sum per block.
constexpr size_t kFmxPass = 1024;
constexpr size_t kFmxMaxBlocks = 4096;
constexpr size_t kFmxBlocksPerCu = 4;	// by its registers (cordic_fm_mix.hip)
constexpr size_t kFmxWorkBytes = 16 + 4 * kFmxMaxBlocks;

// Fallback: [cordic_phase_accumulate's own scratch | n phases]
constexpr size_t kFmxPhaseAt = kFmWorkBytes;
static_assert(kFmxPhaseAt % 16 == 0, "the phases sit on the 16-byte grid");

constexpr size_t fmx_work_bytes(bool fused, size_t n)
{
	return !n ? 0 : fused ? kFmxWorkBytes
		: kFmxPhaseAt + ((n * 4 + 15) & ~(size_t)15);
}

// 1: every n >= 1 of this plan runs the fused kernel -- the cores that
// launch_rot_feed sends to rotator_xydir, minus its batch-size threshold, where
// fm_mix_xydir has an instance (13, 16, 19, 20, 24, 27, 29 live stages).
// d_dir / dx: the plan's direction tables.  (The mode is the caller's to check.)
bool	fmx_is_fused(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx);

// Alignment, and no output range (d_acc and the `work_bytes` of d_work
// included) over anything else; nothing is launched.  n > 0.
int	fmx_check_call(size_t n, const uint32_t *d_fcw, const uint32_t *d_pm,
		const uint32_t *d_acc, const int32_t *d_xval, const int32_t *d_yval,
		const int32_t *d_oxval, const int32_t *d_oyval, const void *d_work,
		size_t work_bytes);

// The fused path: two launches on `stream` (fm_reduce, then fm_mix_xydir),
// nothing else.  The caller has checked fmx_is_fused and fmx_check_call.
int	launch_fm_mix(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		size_t n, const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const int32_t *d_xval, const int32_t *d_yval,
		int32_t *d_oxval, int32_t *d_oyval, void *d_work, void *stream);

} // namespace cordic_amd
#endif
