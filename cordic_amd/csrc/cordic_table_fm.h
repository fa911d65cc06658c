// cordic_table_fm.h -- frequency- and phase-modulated oscillator forms of the
// table and quadratic sine cores (cordic_table_fm / cordic_quad_fm and their
// int16 forms), and the phase accumulator they are built on
// (cordic_phase_accumulate): the phase of sample i is a running sum of
// per-sample tuning words, made on the device.  The launcher for
// cordic_abi_table.cpp; the two public functions that need no handle
// (cordic_fm_workspace, cordic_phase_accumulate) are defined in
// cordic_table_fm.hip itself.
//
// The core comes as a SineCore, and its layouts, their choice and the sample
// functions are those of cordic_table_nco.h: there is one copy of them.
// Neither unit holds a kernel of the DESIGN section 4.4 sweep.
#ifndef CORDIC_TABLE_FM_H
#define CORDIC_TABLE_FM_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_table_nco.h"

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
// any 2-byte-aligned address; else int32_t, 4-byte aligned.  The launcher
// checks alignment and that no output range (d_acc and d_work included)
// overlaps anything else.  The layout is the one launch_sine_nco would choose,
// where its copy fits into LDS beside a tile's phases; else the L2 gather.
// n == 0: CORDIC_OK, nothing touched.
int	launch_sine_fm(const SineCore &c, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, void *d_sin,
		void *d_cos, bool io16, void *d_work, void *stream);

// Launch 1 alone, for the other scan over per-sample tuning words
// (cordic_fm_mix.hip): `grid` blocks, block b sums [b * span, (b + 1) * span)
// of d_fcw cut at n into work[4 + b] (grid <= (n + span - 1) / span), and
// block 0 latches work[0] = phase0 + (d_acc ? *d_acc : 0).
void	launch_fm_reduce(unsigned grid, const uint32_t *d_fcw, size_t n, size_t span,
		uint32_t phase0, const uint32_t *d_acc, uint32_t *work, void *stream);

} // namespace cordic_amd
#endif
