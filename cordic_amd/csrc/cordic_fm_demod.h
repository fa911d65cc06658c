// cordic_fm_demod.h -- FM demodulation on the r2p / sr2p cores (cordic_fm_demod,
// cordic_fm_demod16, cordic_fm_demod_info, cordic_fm_demod_workspace;
// include/cordic_amd.h): the converter's phase differenced sample to sample,
//   freq_i = sext_PW((ph_i - ph_(i-1)) mod 2^PW),
// the inverse of cordic_phase_accumulate.  All four public functions are
// defined in cordic_fm_demod.hip; this header holds what the two paths share.
//
// Neither unit holds a kernel of the DESIGN section 4.4 sweep.
#ifndef CORDIC_FM_DEMOD_H
#define CORDIC_FM_DEMOD_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"

namespace cordic_amd {

// Fused kernel: a block of 256 threads sweeps kFmdPasses passes of 256 vectors
// (4 samples each); the first vector of the sweep is the halo -- the last
// vector of the tile in front, computed again and not stored -- so a tile is
// kFmdTileVecs = 8 * 256 - 1 vectors of output.
constexpr int	 kFmdPasses = 8;
constexpr size_t kFmdTileVecs = (size_t)kFmdPasses * 256 - 1;
constexpr size_t kFmdTile = kFmdTileVecs * 4;		// samples: 8188

// Fallback: the phases are differenced in place in tiles of kFmdDiffTile
// samples, one saved word per tile.
constexpr size_t kFmdDiffTile = 4096;

// d_work, in 32-bit words:
//   [0]       the latched predecessor of sample 0 (fallback)
//   [4, 8)    magnitudes, [8, 12) phases of the fused path's last <= 4 samples
//   [12 + j]  fallback: the phase of the last sample of differencing tile j
constexpr size_t kFmdWorkHead = 12;
constexpr size_t fmd_work_bytes(size_t n)
{
	return n ? ((kFmdWorkHead + (n + kFmdDiffTile - 1) / kFmdDiffTile) * 4 + 15)
			& ~(size_t)15 : 0;
}

// 1: 16-byte-aligned 32-bit arrays of this core run the fused kernel -- the
// cores that launch_topolar sends to topolar_lj.  (The mode is the caller's to
// check.)
bool	fmd_core_is_fused(const cordic_config &cfg);

} // namespace cordic_amd
#endif
