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
// xydir_vector, the wave scan, the staging of the tables and the pass loop are
// device functions in cordic_fm_mix.h, which the bank's kernel
// (cordic_fm_mix_bank.hip) is made of as well; the counts below are the same
// before and after they moved there.
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps;
// .private_segment_fixed_size is 0 for every instance: nothing spills):
//   live stages           13   16   19   20   24   27   29
//   rotator_xydir<29, N>  95   95   96   96   97   98   98
//   fm_mix_xydir<29, N>   98  100   98   98  104  108  108
//   rotator_xydir<30, N>  89   95   90   90   91   94   94
//   fm_mix_xydir<30, N>   92   98   95   95  102  103  103
//   ... <30, N, Io16>     92   96   92   92   99  100  100
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

struct FmxArgs {
	const uint32_t *fcw, *pm;	// pm may be NULL
	uint32_t *acc;			// may be NULL
	const uint32_t *work;		// fm_reduce's: [0] start, [4 + b] partials
	const void *x, *y;		// int32 or int16, by the kernel's container
	void	*ox, *oy;
	size_t	n, span;		// span: samples per block, whole passes
	uint32_t xw;			// LDS byte offset of the 12 exchange words
};

template <int LJ, int NLIVE, typename IO>
__global__ __launch_bounds__(kBlock) void fm_mix_xydir(CoreParams kp, DirArgs da,
		FmxArgs a)
{
	static_assert(LJ == 29 || LJ == 30, "WW <= 35 cores");
	static_assert(LJ == 30 || sizeof(typename IO::ielem) == 4,
		"16-bit ports and WW 35: the fallback (fmx_is_fused16)");
	typedef typename IO::ielem ielem;
	constexpr int kN = dx_levels(NLIVE);
	static_assert(kN >= 1 && kN <= kDxMaxLevels, "no group to look up");
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const unsigned tid = threadIdx.x;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);

	uint32_t bk_base[kDxMaxLevels] = {}, lf_base[kDxMaxLevels] = {};
	dx_lds_layout(da.dx, bk_base, lf_base);

	// ---- prologue: the fold's rows and the groups' tables, and the waves'
	// shares of the partials in front of this block (ex[8 .. 12); ex[0 .. 8)
	// are pass_loop's exchange words)
	stage_tables<LJ, NLIVE>(kp, da, lds, bk_base, lf_base, tid);
	uint32_t *ex = lds + a.xw / 4u;
	front_sum(a.work + 4, blockIdx.x, ex, tid, wave);
	__syncthreads();

	// LDS is addressed by byte offset from 0: no static LDS in this kernel
	if ((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)lds != 0u)
		__builtin_trap();

	const RotRegs rr = rot_regs<LJ, NLIVE>(kp, da);
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

// ---------------------------------------------------------------- host side
template <int LJ, typename IO>
static bool launch_lj(int nlive, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const FmxArgs &a)
{
	switch (nlive) {
#define X(N) case N: \
	if (da.dx.n != dx_levels(N)) \
		return false; \
	hipLaunchKernelGGL((fm_mix_xydir<LJ, N, IO>), dim3(grid), dim3(kBlock), lds, st, \
		kp, da, a); \
	return true;
	FMX_STAGES(X)
#undef X
	default:
		return false;
	}
}

static bool has_instance(int nlive, int ngroups)
{
	switch (nlive) {
#define X(N) case N: return ngroups == dx_levels(N);
	FMX_STAGES(X)
#undef X
	default:
		return false;
	}
}

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

// (at most 2^16 blocks, each walking on by the grid)
static unsigned elementwise_grid(size_t n)
{
	const size_t blocks = (n + kBlock - 1) / kBlock;
	return (unsigned)(blocks < 65536 ? blocks : 65536);
}

} // namespace fmx

bool fmx_is_fused(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx)
{
	if (!d_dir || dx.n <= 0 || cfg.ww > 35 || cfg.needs_wrap
			|| (cfg.flags & (CORDIC_FLAG_UNIT_GAIN | CORDIC_FLAG_NO_TAILS
				| CORDIC_FLAG_NO_LJ | CORDIC_FLAG_FORCE_GENERIC)))
		return false;
	const dev::CoreParams kp = make_params_jobs(cfg);
	return kp.post_mul == 0 && kp.in_shl >= 1 && kp.in_shl <= 30
		&& fmx::lds_bytes(dx, nullptr) <= 64 * 1024
		&& fmx::has_instance(cfg.nlive, dx.n);
}

bool fmx_is_fused16(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx)
{
	// (WW 35 is LJ = 29, which has no Io16 instance: with ports of at most 16
	// bits it means 19 or more extra bits)
	return cfg.ww < 35 && fmx_is_fused(cfg, d_dir, dx);
}

int fmx_check_call(size_t n, const uint32_t *d_fcw, const uint32_t *d_pm,
		const uint32_t *d_acc, const void *d_xval, const void *d_yval,
		const void *d_oxval, const void *d_oyval, size_t esize, const void *d_work,
		size_t work_bytes)
{
	using namespace fmx;
	if (!d_fcw || !d_xval || !d_yval || !d_oxval || !d_oyval || !d_work
			|| n > (~(size_t)0 >> 4))
		return CORDIC_ERR_ARGS;
	const uintptr_t words = reinterpret_cast<uintptr_t>(d_fcw)
		| reinterpret_cast<uintptr_t>(d_pm) | reinterpret_cast<uintptr_t>(d_acc);
	const uintptr_t samples = reinterpret_cast<uintptr_t>(d_xval)
		| reinterpret_cast<uintptr_t>(d_yval) | reinterpret_cast<uintptr_t>(d_oxval)
		| reinterpret_cast<uintptr_t>(d_oyval);
	if ((words & 3u) || (samples & (esize - 1))
			|| (reinterpret_cast<uintptr_t>(d_work) & 15u))
		return CORDIC_ERR_ARGS;
	const Range out[4] = {range_of(d_oxval, n * esize), range_of(d_oyval, n * esize),
		range_of(d_acc, 4), range_of(d_work, work_bytes)};
	const Range in[4] = {range_of(d_fcw, n * 4), range_of(d_pm, n * 4),
		range_of(d_xval, n * esize), range_of(d_yval, n * esize)};
	return outputs_overlap(out, in) ? CORDIC_ERR_ARGS : CORDIC_OK;
}

int launch_fm_mix(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		size_t n, const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const void *d_xval, const void *d_yval, void *d_oxval,
		void *d_oyval, size_t esize, void *d_work, void *stream)
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
	const size_t npass = (n + kFmxPass - 1) / kFmxPass;
	const size_t per_block = (npass + cap - 1) / cap;
	const size_t span = per_block * kFmxPass;
	const unsigned grid = (unsigned)((npass + per_block - 1) / per_block);
	uint32_t *work = static_cast<uint32_t *>(d_work);
	launch_fm_reduce(grid, d_fcw, n, span, phase0, d_acc, work, st);
	const FmxArgs a{d_fcw, d_pm, d_acc, work, d_xval, d_yval, d_oxval, d_oyval, n,
		span, xw};
	const DirArgs da{d_dir, dx};
	const CoreParams kp = make_params_jobs(cfg);
	const bool done = esize == 2
		? cfg.ww < 35 && launch_lj<30, Io16>(cfg.nlive, grid, lds, st, kp, da, a)
		: cfg.ww == 35
			? launch_lj<29, Io32>(cfg.nlive, grid, lds, st, kp, da, a)
			: launch_lj<30, Io32>(cfg.nlive, grid, lds, st, kp, da, a);
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

} // namespace cordic_amd
