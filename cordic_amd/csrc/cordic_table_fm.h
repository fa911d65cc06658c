// cordic_table_fm.h -- frequency- and phase-modulated oscillator forms of the
// table and quadratic sine cores (cordic_table_fm / cordic_quad_fm and their
// int16 forms), and the phase accumulator they are built on
// (cordic_phase_accumulate): the phase of sample i is a running sum of
// per-sample tuning words, made on the device.  Launchers for
// cordic_abi_table.cpp; the two public functions that need no handle
// (cordic_fm_workspace, cordic_phase_accumulate) are defined in
// cordic_table_fm.hip itself.
//
// The cores' layouts and sample functions are those of cordic_table_nco.h,
// included by the kernel unit: there is one copy of them.  Neither unit holds
// a kernel of the DESIGN section 4.4 sweep.
#ifndef CORDIC_TABLE_FM_H
#define CORDIC_TABLE_FM_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"

namespace cordic_amd {

// The prefix sum is cut into tiles of kFmTile samples; a launch has at most
// kFmMaxBlocks blocks, each with a contiguous span of whole tiles.  The
// workspace is one word for the latched start phase (in a 16-byte slot) and
// one partial sum per block.
constexpr size_t kFmTile = 4096;
constexpr size_t kFmMaxBlocks = 1024;
constexpr size_t kFmWorkBytes = 16 + 4 * kFmMaxBlocks;

// Two launches on `stream` (reduce, then scan + sample + store), nothing else:
//   start = phase0 + (d_acc ? *d_acc : 0)
//   p_i   = start + fcw[0] + .. + fcw[i-1] + (d_pm ? pm[i] : 0)
//   d_sin[i] = core(p_i), d_cos[i] = core(p_i + 2^(PW-2))   (d_cos NULL: none)
//   *d_acc = start + fcw[0] + .. + fcw[n-1]
// io16: the outputs are int16_t (OW <= 16: CORDIC_ERR_CONTAINER otherwise),
// any 2-byte-aligned address; else int32_t, 4-byte aligned.  The launchers
// check alignment and that no output range (d_acc and d_work included)
// overlaps anything else, and choose the layout from (d_lds16, lds_mode,
// lds_entries) as launch_table_nco does.  n == 0: CORDIC_OK, nothing touched.
int	launch_table_fm(const cordic_table_config &t, const int32_t *d_tbl,
		const int16_t *d_lds16, int lds_mode, int lds_entries, size_t n,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, void *d_sin, void *d_cos, bool io16, void *d_work,
		void *stream);
int	launch_quad_fm(const cordic_quad_config &q, const int32_t *d_tables,
		size_t n, const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, void *d_sin, void *d_cos, bool io16, void *d_work,
		void *stream);

} // namespace cordic_amd
#endif
