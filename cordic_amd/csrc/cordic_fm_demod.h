// cordic_fm_demod.h -- FM demodulation on the r2p / sr2p cores (cordic_fm_demod,
// cordic_fm_demod16, cordic_fm_demod_info, cordic_fm_demod_workspace;
// include/cordic_amd.h): the converter's phase differenced sample to sample,
//   freq_i = sext_PW((ph_i - ph_(i-1)) mod 2^PW),
// the inverse of cordic_phase_accumulate.  All four public functions are
// defined in cordic_fm_demod.hip; this header holds what the two paths share
// and, for a HIP compiler, the per-vector device code that the fused kernel
// shares with the banks' kernels (cordic_fm_demod_bank.hip).
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

#ifdef __HIPCC__
// ---- device code shared by cordic_fm_demod.hip and cordic_fm_demod_bank.hip
#include "cordic_device.h"

namespace cordic_amd {
namespace fmd {

using namespace dev;

// One vector through the converter: the per-vector body of topolar_lj_sweep
// (cordic_device.h:2287-2360) restated, because the sweep stores what it
// computes.  Built from the same pieces in the same order; rm, rp are the words
// the sweep would store to omag[g], oph[g].
template <int NLIVE, bool DYN, bool UG, bool PLAIN>
__device__ __forceinline__ void pol_lj_vector(const CoreParams &kp, const PolLjRegs &c,
		const uint32_t rbw, const int up, const int down, const i32x4 tx,
		const i32x4 ty, i32x4 &rm, u32x4 &rp)
{
	int64_t x[kVec], y[kVec], p[kVec];
#pragma unroll
	for (int v = 0; v < kVec; v++) {
		// cordic_device.h:2290-2313: the ports, the fold, the quadrant phase
		const int32_t ex = (int32_t)((uint32_t)tx[v] << up) >> down;
		const int32_t ey = (int32_t)((uint32_t)ty[v] << up) >> down;
		const int32_t mx = (int32_t)op_and_or((uint32_t)ex, c.p30, c.sign);
		const int32_t my = (int32_t)op_and_or((uint32_t)ey, c.p30, c.sign);
		const int32_t nmy = (int32_t)((uint32_t)my ^ c.sign);
		x[v] = op_mul(ex, mx);
		op_mad(x[v], ey, my);
		y[v] = op_mul(ey, mx);
		op_mad(y[v], ex, nmy);
		const uint32_t l = ((uint32_t)mx ^ c.sign) >> 1;
		p[v] = op_mul(nmy, (int32_t)l);
	}
	if (PLAIN || down >= 2) {	// :2315-2323, stage 1
#pragma unroll
		for (int v = 0; v < kVec; v++)
			pol_stage1_lj(x[v], y[v], p[v], kp.angle[0], c);
	} else {
#pragma unroll
		for (int v = 0; v < kVec; v++)
			pol_stage1_lj_early(x[v], y[v], p[v], kp.angle[0], c);
	}

	PolTmp m[kVec];
#if CORDIC_STAGE_YIELD
#pragma unroll
	for (int v = 0; v < kVec; v++)
		asm volatile("" : "=v"(m[v].t), "=v"(m[v].nt), "=v"(m[v].sy), "=v"(m[v].sx),
				"=s"(m[v].cc));
#endif
	PolChainLJ<NLIVE, 1, DYN>::run(x, y, p, c, kp, m);

	if (PLAIN || (kp.r >= 2 && kp.r <= 31)) {	// :2336-2353, rounding
#pragma unroll
		for (int v = 0; v < kVec; v++) {
			const uint32_t xh = (uint32_t)((uint64_t)x[v] >> 32);
			uint32_t b;
			asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(b)
				: "v"(xh), "s"(kp.r - 2), "v"(rbw));
			op_mad_s(x[v], 0x40000000u, (int32_t)(b + (uint32_t)kp.round_base));
			rm[v] = (int32_t)((uint64_t)x[v] >> 32) >> (kp.r - 2);
		}
	} else {
#pragma unroll
		for (int v = 0; v < kVec; v++)
			rm[v] = round_to_ow<int64_t>(x[v] >> 30, kp);
	}
#pragma unroll
	for (int v = 0; v < kVec; v++) {		// :2354-2359
		const uint32_t acc = (uint32_t)((uint64_t)p[v] >> 30);
		rp[v] = (acc + 0x80000000u) >> kp.pw_shl;
	}
	apply_unit_gain<UG>(rm, kp);
}

// sext_PW((a - b) mod 2^PW) with sh = 32 - PW
__device__ __forceinline__ int32_t step_of(uint32_t a, uint32_t b, int sh)
{
	return (int32_t)((a - b) << sh) >> sh;
}

} // namespace fmd
} // namespace cordic_amd
#endif // __HIPCC__
#endif
