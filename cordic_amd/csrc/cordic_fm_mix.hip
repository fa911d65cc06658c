// cordic_fm_mix.hip -- the FM mixer's fused path (cordic_plan_fm_mix, and
// cordic_plan_fm_mix16 on int16 I/Q arrays): the rotator with looked-up directions (cordic_xydir.h) behind a prefix sum of
// per-sample tuning words,
//   start = phase0 + *d_acc
//   p_i   = start + fcw[0] + .. + fcw[i-1] + pm[i]      (mod 2^32)
//   (ox_i, oy_i) = what cordic_p2r writes for (x_i, y_i, p_i)
//   *d_acc = start + fcw[0] + .. + fcw[n-1].
//
// Reduce-then-scan in two launches, as cordic_table_fm.hip.  The samples are
// cut into passes of 1024; every block owns a contiguous span of whole passes.
//   1. fm_reduce (cordic_table_fm.hip): each block sums its span of fcw into a
//      workspace word; block 0 latches the start beside them.
//   2. fm_mix_xydir<LJ, NLIVE>: each block stages the direction tables as
//      rotator_xydir does, adds the partials in front of it to the latched
//      start, then walks its span pass by pass.  A lane reads 4 consecutive
//      tuning words (and pm, x, y: one 16-byte access each at whatever 4-byte
//      alignment the array has), sums them, the wave scans the lane sums with
//      DPP moves, the four waves exchange their totals through LDS, and the
//      carry runs from pass to pass in a register.  The lane then rotates its 4
//      samples by the per-vector body of rotator_xydir and stores them.
// No block waits for another: what a block needs of the others is complete
// when launch 2 starts.  *d_acc is read in launch 1 only and written in launch
// 2 only (one thread of the last block).  The price is a second read of fcw:
// 24 bytes per sample (28 with pm) against the 32 (36) of
// cordic_phase_accumulate + cordic_plan_p2r.
//
// The exchange words are double-buffered by pass, so a pass has ONE barrier:
// the four words written in pass i are read by every wave behind barrier i and
// in front of barrier i + 1; they are written again in pass i + 2, which a
// wave reaches only through barrier i + 1, and that opens only when every
// wave has arrived there -- with its reads of pass i behind it.
//
// LDS is the tables' (dx_lds_layout) with 12 words behind them, in the DYNAMIC
// block: the table lookups address LDS by byte offset from 0, which a static
// __shared__ object would displace.
//
// The last, partial vector (n % 4 samples) belongs to one lane of the last
// block, which loads and stores it sample by sample; lanes behind it read and
// write nothing.  There is no extra launch, and nothing outside [0, n) of an
// output is written.
//
// CORDIC_FMX_MAX_BLOCKS=<n> in the environment (read at every call; a test
// and A/B knob like CORDIC_FMD_MAX_BLOCKS) caps the grid at n blocks, so that
// a short call walks many passes per block.  The bits do not depend on it.
//
// xydir_vector, the wave scan, the pass loop and the block's prologue
// (block_begin in front of the barrier: the static_asserts and the staging of
// the tables; block_ready behind it: the trap on the LDS offset and the
// rotator's registers) are device functions in cordic_fm_mix.h, which the
// bank's kernel (cordic_fm_mix_bank.hip) and the receiver's two
// (cordic_fm_rx.hip, cordic_fm_rx_bank.hip) are made of as well.  The host
// side's choice of the instance lives there too: fmx::unit_of (<LJ, container>
// of a core), fmx::with_unit and fmx::with_stages (the one switch over the
// stage counts).  The call check is iq_call_ok and the span of a block
// call_span, both cordic_hostargs.h.  The counts below are the same before and
// after (profiles/r21/fm_fold_isa.txt).
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps;
// .private_segment_fixed_size is 0 for every instance: nothing spills):
//   live stages           13   16   19   20   24   27   29
//   rotator_xydir<29, N>  95   95   96   96   97   98   98
//   fm_mix_xydir<29, N>   98  100   98   98  104  108  108
//   rotator_xydir<30, N>  89   95   90   90   91   94   94
//   fm_mix_xydir<30, N>   92   98   95   95  102  103  103
//   ... <30, N, Io16>     92   96   92   92   99  100  100
//   ... <30, N, IoC16io>  90   94   91   91   90   93   93
// The scan costs 3 .. 11 registers: four more words in flight per lane (fcw and
// pm against the phase) and the carry.  With 512 registers per lane of a SIMD,
// allocated in eights, up to 96 hold 5 waves and up to 128 hold 4: an occupancy
// step IS crossed, from 5 waves to 4, by every instance but <30, 13>, <30, 19>
// and <30, 20> (rotator_xydir's own <29, 24 .. 29> sit at 4 already).  Holding
// the kernel to 96 registers (amdgpu_waves_per_eu) spills 8 .. 72 bytes in all
// but one instance, so the step is taken and the grid is sized for 4 blocks
// per CU.  The tables are 64 KiB at the most, so LDS admits at least two
// blocks, and four wherever the tables stay within 40 KiB.
//
// The container (the third template parameter, Io32 / Io16 of cordic_device.h)
// is what pass_loop loads x and y as and stores ox and oy as, and nothing else:
// fm_reduce, the span geometry, the exchange words and the workspace are the
// same.  The table above was taken again with the parameter in place: every
// 32-bit count is what it was.  The Io16 instances exist for LJ = 30 only -- a
// core with ports of at most 16 bits and WW 35 has 19 or more extra bits and
// takes the 16-bit fallback (fmx_is_fused16) -- and take 0 .. 3 registers FEWER
// than their 32-bit twins: the next pass's x and y wait in two registers each,
// not four.  A lane moves 8 bytes per sample array and pass
// (global_load_dwordx2 / global_store_dwordx2) at any 2-byte alignment: 16
// bytes per sample (20 with pm) against 24 (28).  The 16-bit fallback's two
// elementwise kernels, fmx_widen and fmx_narrow, take 12 registers each.
//
// IoC16io (cordic_fm_mix.h; cordic_plan_fm_mix_c16): interleaved int16 I/Q on
// both sides.  A lane's 4 complex samples are ONE 16-byte load at d_iq + 2 i and
// ONE 16-byte store of four packed dwords (I | Q << 16) at d_oiq + 2 i, at any
// 4-byte alignment; the bytes per sample are Io16's.  The 7 instances live in an
// object of their own -- this source compiled a second time with
// -DCORDIC_FMX_C16 (the Makefile's FMX_C16_SRCS) holds them and
// launch_fm_mix_scan_c16 and nothing of the host side -- so that they build
// beside the others; fmx::with_unit does not know them, launch_fm_mix asks
// fmx::unit_of(ww, esize, iq) and calls that launcher for kUnitC16.  They take 2
// .. 9 registers fewer than the Io16 instances (the next pass's samples wait in
// four registers where Io16 has four in two arrays, and one output address is
// made where Io16 makes two); nothing spills, and the grid's 4 blocks per CU
// hold.  The fallback's interleave kernel, fmx_interleave_c16, is one thread per
// output dword.
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

template <int LJ, int NLIVE, typename IO>
__global__ __launch_bounds__(kBlock) void fm_mix_xydir(CoreParams kp, DirArgs da,
		FmxArgs a)
{
	typedef typename IO::ielem ielem;
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const unsigned tid = threadIdx.x;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	uint32_t bk_base[kDxMaxLevels] = {}, lf_base[kDxMaxLevels] = {};
	dx_lds_layout(da.dx, bk_base, lf_base);
	// ---- prologue (fmx::block_begin / block_ready): the tables, and between
	// the two the waves' shares of the partials in front of this block (ex[8 ..
	// 12); ex[0 .. 8) are pass_loop's exchange words)
	block_begin<LJ, NLIVE, IO>(kp, da, lds, bk_base, lf_base, tid);
	uint32_t *ex = lds + a.xw / 4u;
	front_sum(a.work + 4, blockIdx.x, ex, tid, wave);
	__syncthreads();
	const RotRegs rr = block_ready<LJ, NLIVE>(kp, da, lds);

	const size_t lo = (size_t)blockIdx.x * a.span;	// < n by the grid
	const size_t hi = (a.n - lo < a.span) ? a.n : lo + a.span;
	// the phase of sample lo, without its pm
	uint32_t carry = a.work[0] + ex[8] + ex[9] + ex[10] + ex[11];
	unsigned par = 0;
	pass_loop<LJ, NLIVE>(kp, da, rr, bk_base, a.fcw, a.pm,
		static_cast<const ielem *>(a.x), static_cast<const ielem *>(a.y),
		static_cast<ielem *>(a.ox), static_cast<ielem *>(a.oy), lo, hi, carry, par,
		ex, tid, wave, IO{});
	if (a.acc && blockIdx.x == gridDim.x - 1 && tid == 0)
		*a.acc = carry;
}

// launch 2 for one <LJ, container>; false: no instance for nlive
template <int LJ, typename IO>
static bool launch_scan(int nlive, int ngroups, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const FmxArgs &a)
{
	return with_stages(nlive, ngroups, [&](auto nl) {
		hipLaunchKernelGGL((fm_mix_xydir<LJ, decltype(nl)::value, IO>), dim3(grid),
			dim3(kBlock), lds, st, kp, da, a);
	});
}

#ifndef CORDIC_FMX_C16
// ---------------------------------------------------------------- host side
// the 16-bit fallback's elementwise kernels
__global__ __launch_bounds__(kBlock) void fmx_widen(size_t n,
		const int16_t *__restrict__ x, const int16_t *__restrict__ y,
		int32_t *__restrict__ wx, int32_t *__restrict__ wy)
{
	const size_t stride = (size_t)gridDim.x * kBlock;
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
		wx[i] = x[i];
		wy[i] = y[i];
	}
}

__global__ __launch_bounds__(kBlock) void fmx_narrow(size_t n,
		const int32_t *__restrict__ wox, const int32_t *__restrict__ woy,
		int16_t *__restrict__ ox, int16_t *__restrict__ oy)
{
	const size_t stride = (size_t)gridDim.x * kBlock;
	for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
		ox[i] = (int16_t)wox[i];
		oy[i] = (int16_t)woy[i];
	}
}

// the interleaved forms' fallback: the twin's two output arrays into one
__global__ __launch_bounds__(kBlock) void fmx_interleave_c16(size_t m,
		const int16_t *__restrict__ ox, const int16_t *__restrict__ oy,
		uint32_t *__restrict__ oiq)
{
	const size_t stride = (size_t)gridDim.x * kBlock;
	for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride)
		oiq[j] = pack_iq(ox[j], oy[j]);
}

// (at most 2^16 blocks, each walking on by the grid)
static unsigned elementwise_grid(size_t n)
{
	const size_t blocks = (n + kBlock - 1) / kBlock;
	return (unsigned)(blocks < 65536 ? blocks : 65536);
}

#endif // CORDIC_FMX_C16

} // namespace fmx

#ifdef CORDIC_FMX_C16
// This object (cordic_fm_mix_c16.o): the kernel's <30, N, IoC16io> instances and
// their launcher, nothing of the host side.
bool launch_fm_mix_scan_c16(int nlive, int ngroups, unsigned grid, size_t lds, void *stream,
		const dev::CoreParams &kp, const dev::DirArgs &da, const fmx::FmxArgs &a,
		uint32_t log2r)
{
	(void)log2r;
	return fmx::launch_scan<30, fmx::IoC16io>(nlive, ngroups, grid, lds,
		static_cast<hipStream_t>(stream), kp, da, a);
}
#else
bool fmx_is_fused(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx)
{
	if (!d_dir || dx.n <= 0 || cfg.ww > 35 || cfg.needs_wrap
			|| (cfg.flags & (CORDIC_FLAG_UNIT_GAIN | CORDIC_FLAG_NO_TAILS
				| CORDIC_FLAG_NO_LJ | CORDIC_FLAG_FORCE_GENERIC)))
		return false;
	const dev::CoreParams kp = make_params_jobs(cfg);
	return kp.post_mul == 0 && kp.in_shl >= 1 && kp.in_shl <= 30
		&& fmx::lds_bytes(dx, nullptr) <= 64 * 1024
		&& fmx::with_stages(cfg.nlive, dx.n, [](auto) {});
}

bool fmx_is_fused16(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx)
{
	// (WW 35 is LJ = 29, which has no Io16 instance: with ports of at most 16
	// bits it means 19 or more extra bits)
	return fmx::unit_of(cfg.ww, 2) != fmx::kUnitNone && fmx_is_fused(cfg, d_dir, dx);
}

int fmx_check_call(size_t n, const uint32_t *d_fcw, const uint32_t *d_pm,
		const uint32_t *d_acc, const void *d_xval, const void *d_yval,
		const void *d_oxval, const void *d_oyval, size_t esize, const void *d_work,
		size_t work_bytes, uint32_t log2r, bool iq)
{
	return iq_call_ok(n, d_acc, nullptr, d_fcw, d_pm, d_xval, d_yval, d_oxval, d_oyval,
		esize, d_work, work_bytes, log2r, iq, iq) ? CORDIC_OK : CORDIC_ERR_ARGS;
}

int launch_fm_mix(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		size_t n, const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const void *d_xval, const void *d_yval, void *d_oxval,
		void *d_oyval, size_t esize, void *d_work, void *stream, uint32_t log2r, bool iq)
{
	using namespace fmx;
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (n == 0)
		return CORDIC_OK;
	hipStream_t st = static_cast<hipStream_t>(stream);
	const int cus = jobs_cus_now();
	if (cus < 0) {
		(void)hipGetLastError();
		return CORDIC_ERR_DEVICE;
	}
	uint32_t xw = 0;
	const size_t lds = lds_bytes(dx, &xw);
	// resident blocks: 4 waves of a SIMD by the registers (see the head of
	// this file), fewer where the tables fill the CU's 160 KiB sooner
	size_t cap = (size_t)cus * blocks_per_cu(lds);
	if (cap > kFmxMaxBlocks)
		cap = kFmxMaxBlocks;
	cap = env_block_cap("CORDIC_FMX_MAX_BLOCKS", cap);
	const CallSpan cs = call_span(n, cap, kFmxPass, 0);
	const size_t span = cs.span;
	const unsigned grid = (unsigned)cs.grid;
	uint32_t *work = static_cast<uint32_t *>(d_work);
	launch_fm_reduce(grid, d_fcw, n, span, phase0, d_acc, work, st);
	const FmxArgs a{d_fcw, d_pm, d_acc, work, d_xval, d_yval, d_oxval, d_oyval, n,
		span, xw};
	const DirArgs da{d_dir, dx};
	const CoreParams kp = make_params_jobs(cfg);
	// iq: a.x is d_iq, a.ox is d_oiq, a.y and a.oy are not looked at
	const Unit unit = unit_of(cfg.ww, esize, iq);
	if (log2r)	// the decimating scan (cordic_fm_mix_decim.hip): n is whole groups
		return tnco::finish(launch_fm_mix_decim_scan(unit, cfg.nlive, dx.n, grid, lds,
			stream, kp, da, a, log2r));
	if (unit == kUnitC16)	// (cordic_fm_mix_c16.o)
		return tnco::finish(launch_fm_mix_scan_c16(cfg.nlive, dx.n, grid, lds, stream, kp,
			da, a, 0));
	const bool done = with_unit(unit, [&](auto lj, auto io) {
		return launch_scan<decltype(lj)::value, decltype(io)>(cfg.nlive, dx.n, grid, lds,
			st, kp, da, a);
	});
	return tnco::finish(done);
}

int launch_fmx_widen(size_t n, const int16_t *d_x, const int16_t *d_y, int32_t *d_wx,
		int32_t *d_wy, void *stream)
{
	using namespace fmx;
	(void)hipGetLastError();
	hipLaunchKernelGGL(fmx_widen, dim3(elementwise_grid(n)), dim3(kBlock), 0,
		static_cast<hipStream_t>(stream), n, d_x, d_y, d_wx, d_wy);
	return tnco::finish(true);
}

int launch_fmx_narrow(size_t n, const int32_t *d_wox, const int32_t *d_woy,
		int16_t *d_ox, int16_t *d_oy, void *stream)
{
	using namespace fmx;
	(void)hipGetLastError();
	hipLaunchKernelGGL(fmx_narrow, dim3(elementwise_grid(n)), dim3(kBlock), 0,
		static_cast<hipStream_t>(stream), n, d_wox, d_woy, d_ox, d_oy);
	return tnco::finish(true);
}

int launch_fmx_interleave_c16(size_t m, const int16_t *d_ox, const int16_t *d_oy,
		int16_t *d_oiq, void *stream)
{
	using namespace fmx;
	(void)hipGetLastError();
	hipLaunchKernelGGL(fmx_interleave_c16, dim3(elementwise_grid(m)), dim3(kBlock), 0,
		static_cast<hipStream_t>(stream), m, d_ox, d_oy, reinterpret_cast<uint32_t *>(d_oiq));
	return tnco::finish(true);
}
#endif // CORDIC_FMX_C16

} // namespace cordic_amd
