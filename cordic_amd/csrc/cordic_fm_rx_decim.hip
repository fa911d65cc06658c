// cordic_fm_rx_decim.hip -- the decimating FM receiver's fused path
// (cordic_plan_fm_rx_decim, and cordic_plan_fm_rx_decim16 on int16 arrays;
// include/cordic_amd.h): the tuned receiver (cordic_fm_rx.hip) with the
// decimating mixer's integrate-and-dump by R = 2^k (cordic_fm_mix_decim.hip)
// between the rotator and the converter, 1 <= k <= 8 (k = 0 is the receiver
// itself and never reaches this unit).
//
// Launch 1 is the receiver's fm_rx_reduce, launched by launch_fm_rx
// (cordic_fm_rx.hip), which also owns the grid and the span -- whole passes of
// 1024 input samples LESS the halo's max(4, R), a multiple of R: this unit holds
// launch 2 and nothing of the geometry.
//   fm_rx_decim_xydir<LJ, NLIVE, IO>: fm_rx_xydir's prologue, then
//   fmrxd::pass_loop (cordic_fm_rx_decim.h).  A pass rotates 1024 input samples
//   and sums them in groups of R as the decimating mixer does, but the group's
//   owner writes the floored pair into a ring in LDS, not to memory.  Whenever
//   1024 decimated samples are complete -- every R passes -- the block runs the
//   receiver's back half on the ring: each lane converts 4 consecutive
//   decimated samples, differences their phases and stores one vector.  The
//   converter's chain is paid once per 1024 DECIMATED samples, 1/R of the
//   receiver's cost per input sample, its stores are whole vectors, and the
//   rotator's and the converter's registers are not live together.
// k is a kernel argument, wave-uniform: one instance per <unit, stage count>.
//
// LDS: the tables (dx_lds_layout), 24 exchange words, and the ring: 2 planes of
// 2048 int32, 16 KiB -- 1536 slots would hold the 1535 that can be live; 2048
// make the slot a mask.  The grid is sized by fmrx::blocks_per_cu on the whole:
// 4 blocks per CU while tables + ring stay within 40 KiB, fewer behind larger
// tables.  The barriers that order the ring's writers and readers are listed
// at fmrxd::pass_loop.
//
// CORDIC_FMRXD_MAX_BLOCKS=<n> caps the grid (read at every call; a test and
// A/B knob); the bits do not depend on it.  CORDIC_FMRXD_FALLBACK=1
// (cordic_abi_fm.cpp) sends a fused pair's single call through the fallback.
//
// The unit is compiled four times, as cordic_fm_rx.hip is: once per entry of
// the receiver's unit list (cordic_fm_rx_unit.h), the last on interleaved int16
// I/Q (fmx::IoC16).
// Registers and LDS per instance: profiles/r23/fm_rx_decim.txt; .vgpr_count of
// the 16-bit containers (scratch 0; within 128: 4 waves per SIMD, the grid's 4
// blocks per CU; profiles/r24/fm_rx_c16.txt):
//   live stages                     13   16   19   20   24   27   29
//   fm_rx_decim_xydir<30, N, IoC16> 116  116  117  117  118  121  121
//   ... <30, N, Io16>               115  115  116  116  117  120  120
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_xydir.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_table_nco.h"
#include "cordic_hostargs.h"
#include "cordic_fm_rx_decim.h"
#include "cordic_fm_rx_unit.h"

namespace cordic_amd {

namespace fmrxd {

using namespace dev;

template <int LJ, int NLIVE, typename IO>
__global__ __launch_bounds__(kBlock) void fm_rx_decim_xydir(CoreParams kp, DirArgs da,
		fmrx::RxArgs a, uint32_t log2r)
{
	typedef typename IO::ielem ielem;
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const unsigned tid = threadIdx.x;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	uint32_t bk_base[kDxMaxLevels] = {}, lf_base[kDxMaxLevels] = {};
	dx_lds_layout(da.dx, bk_base, lf_base);
	fmx::block_begin<LJ, NLIVE, IO>(kp, da, lds, bk_base, lf_base, tid);
	uint32_t *ex = lds + a.xw / 4u;
	fmx::front_sum(a.work + 4, blockIdx.x, ex, tid, wave);
	__syncthreads();
	const fmx::RotRegs rr = fmx::block_ready<LJ, NLIVE>(kp, da, lds);

	// the converter's parameters: launch 1 left them in the workspace
	const uint32_t *ckmem = a.work + kFmrxConvAt / 4;
	const fmd::LaneConsts ln(fmrx::conv_params(ckmem, false));
	// (a.span is a multiple of R: output lo >> k is this block's first)
	const size_t lo = (size_t)blockIdx.x * a.span;	// < n by the grid
	const size_t cnt = (a.n - lo < a.span) ? a.n - lo : a.span;
	const size_t olo = lo >> log2r;
	const bool tail = blockIdx.x == gridDim.x - 1;
	// shorts per input sample: IoC16 has both halves in a.x (a.y is not read)
	constexpr size_t kIn = fmx::is_iq<IO>::value ? 2 : 1;
	// the phase of sample lo, without its pm
	uint32_t carry = a.work[0] + ex[8] + ex[9] + ex[10] + ex[11];
	unsigned par = 0, fpar = 0;
	pass_loop<LJ, NLIVE>(kp, da, rr, bk_base, ckmem, ln, a.fcw + lo,
		a.pm ? a.pm + lo : nullptr, static_cast<const ielem *>(a.x) + kIn * lo,
		static_cast<const ielem *>(a.y) + lo, static_cast<ielem *>(a.mag) + olo,
		static_cast<ielem *>(a.freq) + olo, cnt, log2r, blockIdx.x == 0, a.work[1],
		tail ? a.last : nullptr, carry, par, fpar, ex,
		a.xw + (uint32_t)kFmrxdExWords * 4u, tid, wave, IO{});
	if (a.acc && tail && tid == 0)
		*a.acc = carry;
}

} // namespace fmrxd

namespace fmrx {

// this unit's entry point (kUnitLj, UnitIo: cordic_fm_rx_unit.h)
bool FMRX_ENTRY(launch_rxd)(int nlive, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const RxArgs &a, uint32_t log2r)
{
	return fmx::with_stages(nlive, da.dx.n, [&](auto nl) {
		hipLaunchKernelGGL((fmrxd::fm_rx_decim_xydir<kUnitLj, decltype(nl)::value, UnitIo>),
			dim3(grid), dim3(kBlock), lds, st, kp, da, a, log2r);
	});
}

} // namespace fmrx

} // namespace cordic_amd
