// cordic_fm_mix_decim.hip -- the decimating FM mixer's kernels
// (cordic_plan_fm_mix_decim, cordic_plan_fm_mix_decim16; include/cordic_amd.h):
// the FM mixer (cordic_fm_mix.hip) with an integrate-and-dump by R = 2^k behind
// the rotator,
//   (tx_i, ty_i) = what cordic_plan_fm_mix writes for sample i
//   ox[j] = floor((tx_(jR) + .. + tx_(jR+R-1)) / R),   j in [0, n / R)
// and oy likewise.  n is a multiple of R; 1 <= k <= 8 here (k = 0 is the mixer
// itself and never reaches this unit).
//
// Launch 1 is the mixer's fm_reduce, launched by launch_fm_mix
// (cordic_fm_mix.hip), which also owns the grid and the span: this unit holds
// launch 2 and nothing of the geometry.
//   fm_mix_decim_xydir<LJ, NLIVE, IO>: fm_mix_xydir with pass_loop's decimating
//   form (cordic_fm_mix.h, store_decim): behind xydir_vector a lane holds 4
//   consecutive tuned samples.  k = 1: two outputs per lane.  k >= 2: the lane
//   sums its 4; for k > 2 the 2^(k-2) neighbouring lanes of a group are summed
//   as the difference of two values of the inclusive wave scan (the DPP scan of
//   the tuning words, run again on the sums), fetched from the lane a group in
//   front with one ds_bpermute -- the same code for every k -- and the group's
//   last lane stores one element.  R <= 256 samples are 64 lanes at the most,
//   one wave's share of a pass: a group never crosses a wave, a pass or a span
//   (spans are whole passes of 1024), so the data needs no barrier and no LDS.
//   The sum of R OW-bit values needs OW + k bits, 40 for OW 32 and k = 8; it is
//   carried as two 32-bit sums,
//     floor(S / 2^k) = sum(v >> k) + (sum(v & (2^k - 1)) >> k),
//   which is exact: the first is below 2^31 in magnitude, the second below
//   2^16.  The scan wraps modulo 2^32, a difference of two of its values does
//   not.
//   k is a kernel argument, wave-uniform, in a scalar register: one instance
//   per <unit, stage count>, as the mixer has.
// The next pass's loads in flight, the ONE barrier per pass and the exchange
// words are pass_loop's own and unchanged.  A job's last pass may be partial, a
// multiple of R: nothing at or behind n is read (load_pass), nothing at or
// behind n >> k is written (a group lies wholly in front of n or wholly behind).
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps;
// .private_segment_fixed_size is 0 for every instance: nothing spills), next to
// the mixer's (cordic_fm_mix.hip, cordic_fm_mix_bank.hip):
//   live stages                    13   16   19   20   24   27   29
//   fm_mix_xydir<29, N>            98  100   98   98  104  108  108
//   fm_mix_decim_xydir<29, N>      99  102   99   99  103  109  109
//   fm_mix_xydir<30, N>            92   98   95   95  102  103  103
//   fm_mix_decim_xydir<30, N>      97   99   96   96  103  104  104
//   fm_mix_xydir<30, N, Io16>      92   96   92   92   99  100  100
//   fm_mix_decim_xydir<.., Io16>   95   97   94   94  101  102  102
//   fm_mix_xydir<30, N, IoC16io>   90   94   91   91   90   93   93
//   fm_mix_decim_...<.., IoC16io>  91   95   92   92   91   94   94
//   fm_mixbank_xydir<29, N>       114  120  114  114  115  122  122
//   fm_mixbank_decim_xydir<29, N> 119  121  118  118  125  126  126
//   fm_mixbank_xydir<30, N>       115  117  116  116  115  124  124
//   fm_mixbank_decim_xydir<30, N> 117  119  118  118  124  126  126
//   fm_mixbank_xydir<.., Io16>    111  113  112  112  112  120  120
//   fm_mixbank_decim_...<.., Io16> 125 128  126  126  126  128  128
//   fm_mixbank_xydir<.., IoC16io> 111  113  112  112  111  112  112
//   fm_mixbank_decim..<.., IoC16io> 112 114 113  113  112  113  113
//   fmx_decimate<int32 / int16>    18
// The sum costs -1 .. 5 registers in the single call and 1 .. 15 in the bank;
// every instance stays within the 128 that hold 4 waves per SIMD, which the
// grids of both launchers assume, so no occupancy step is crossed.  The IoC16io
// rows (interleaved int16 I/Q in and out, the *_c16 mixers; objects of their
// own, -DCORDIC_FMX_C16, see cordic_fm_mix.hip) store ONE dword (I | Q << 16)
// per decimated sample where Io16 has two 2-byte stores (k = 1: one 8-byte store
// of the lane's two); the decimating bank's instances take 12 .. 15 registers
// fewer than Io16's, which sit at the edge of 128.
//
// Knobs: CORDIC_FMX_MAX_BLOCKS caps the grid as for the mixer
// (cordic_fm_mix.hip).  CORDIC_FMXD_FALLBACK=1 (cordic_abi_fm.cpp; a test and A/B
// knob, read at every single call AND at every workspace query: set it before
// both, the fallback's workspace is the larger one) sends a fused plan's SINGLE
// call through the fallback; banks ignore
// it: their path is chosen at create by the plan alone.
//
// fmx_decimate<T>: the fallback's elementwise launch -- one thread per output,
// R loads, a 64-bit sum, an arithmetic shift.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_xydir.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_hostargs.h"
#include "cordic_fm_mix.h"

namespace cordic_amd {

namespace fmx {

using namespace dev;

// launch 2 of the fused path: fm_mix_xydir (cordic_fm_mix.hip) line for line,
// with the decimating pass loop
template <int LJ, int NLIVE, typename IO>
__global__ __launch_bounds__(kBlock) void fm_mix_decim_xydir(CoreParams kp, DirArgs da,
		FmxArgs a, uint32_t log2r)
{
	typedef typename IO::ielem ielem;
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const unsigned tid = threadIdx.x;
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	uint32_t bk_base[kDxMaxLevels] = {}, lf_base[kDxMaxLevels] = {};
	dx_lds_layout(da.dx, bk_base, lf_base);
	block_begin<LJ, NLIVE, IO>(kp, da, lds, bk_base, lf_base, tid);
	uint32_t *ex = lds + a.xw / 4u;
	front_sum(a.work + 4, blockIdx.x, ex, tid, wave);
	__syncthreads();
	const RotRegs rr = block_ready<LJ, NLIVE>(kp, da, lds);

	// (a.span is whole passes, a multiple of R: output lo >> k is this block's)
	const size_t lo = (size_t)blockIdx.x * a.span;	// < n by the grid
	const size_t hi = (a.n - lo < a.span) ? a.n : lo + a.span;
	uint32_t carry = a.work[0] + ex[8] + ex[9] + ex[10] + ex[11];
	unsigned par = 0;
	pass_loop<LJ, NLIVE>(kp, da, rr, bk_base, a.fcw, a.pm,
		static_cast<const ielem *>(a.x), static_cast<const ielem *>(a.y),
		static_cast<ielem *>(a.ox), static_cast<ielem *>(a.oy), lo, hi, carry, par,
		ex, tid, wave, IO{}, std::true_type{}, log2r);
	if (a.acc && blockIdx.x == gridDim.x - 1 && tid == 0)
		*a.acc = carry;
}

// launch 2 for one <LJ, container>; false: no instance for nlive
template <int LJ, typename IO>
static bool launch_scan(int nlive, int ngroups, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const FmxArgs &a, uint32_t log2r)
{
	return with_stages(nlive, ngroups, [&](auto nl) {
		hipLaunchKernelGGL((fm_mix_decim_xydir<LJ, decltype(nl)::value, IO>), dim3(grid),
			dim3(kBlock), lds, st, kp, da, a, log2r);
	});
}

#ifndef CORDIC_FMX_C16
// the fallback's decimation: out[j] = floor((in[jR] + .. + in[jR + R - 1]) / R)
// for both arrays, j < nout
template <typename T>
__global__ __launch_bounds__(kBlock) void fmx_decimate(size_t nout, uint32_t log2r,
		const T *__restrict__ tx, const T *__restrict__ ty, T *__restrict__ ox,
		T *__restrict__ oy)
{
	const size_t stride = (size_t)gridDim.x * kBlock;
	const size_t r = (size_t)1 << log2r;
	for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < nout; j += stride) {
		int64_t sx = 0, sy = 0;
		for (size_t i = j << log2r; i < (j << log2r) + r; i++) {
			sx += tx[i];
			sy += ty[i];
		}
		ox[j] = (T)(sx >> log2r);
		oy[j] = (T)(sy >> log2r);
	}
}

#endif // CORDIC_FMX_C16

} // namespace fmx

#ifdef CORDIC_FMX_C16
// This object (cordic_fm_mix_decim_c16.o): the kernel's <30, N, IoC16io>
// instances and their launcher, nothing of the host side.
bool launch_fm_mix_decim_scan_c16(int nlive, int ngroups, unsigned grid, size_t lds,
		void *stream, const dev::CoreParams &kp, const dev::DirArgs &da,
		const fmx::FmxArgs &a, uint32_t log2r)
{
	return fmx::launch_scan<30, fmx::IoC16io>(nlive, ngroups, grid, lds,
		static_cast<hipStream_t>(stream), kp, da, a, log2r);
}
#else
bool launch_fm_mix_decim_scan(fmx::Unit unit, int nlive, int ngroups, unsigned grid,
		size_t lds, void *stream, const dev::CoreParams &kp, const dev::DirArgs &da,
		const fmx::FmxArgs &a, uint32_t log2r)
{
	using namespace fmx;
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (unit == kUnitC16)	// (cordic_fm_mix_decim_c16.o)
		return launch_fm_mix_decim_scan_c16(nlive, ngroups, grid, lds, stream, kp, da, a,
			log2r);
	return with_unit(unit, [&](auto lj, auto io) {
		return launch_scan<decltype(lj)::value, decltype(io)>(nlive, ngroups, grid, lds, st,
			kp, da, a, log2r);
	});
}

int launch_fmx_decimate(size_t n, uint32_t log2r, size_t esize, const void *d_tx,
		const void *d_ty, void *d_ox, void *d_oy, void *stream)
{
	using namespace fmx;
	(void)hipGetLastError();
	const size_t nout = n >> log2r;
	// (at most 2^16 blocks, each walking on by the grid)
	const size_t blocks = (nout + kBlock - 1) / kBlock;
	const unsigned grid = (unsigned)(blocks < 65536 ? blocks : 65536);
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (esize == 2)
		hipLaunchKernelGGL(fmx_decimate<int16_t>, dim3(grid), dim3(kBlock), 0, st, nout,
			log2r, static_cast<const int16_t *>(d_tx), static_cast<const int16_t *>(d_ty),
			static_cast<int16_t *>(d_ox), static_cast<int16_t *>(d_oy));
	else
		hipLaunchKernelGGL(fmx_decimate<int32_t>, dim3(grid), dim3(kBlock), 0, st, nout,
			log2r, static_cast<const int32_t *>(d_tx), static_cast<const int32_t *>(d_ty),
			static_cast<int32_t *>(d_ox), static_cast<int32_t *>(d_oy));
	return tnco::finish(true);
}
#endif // CORDIC_FMX_C16

} // namespace cordic_amd
