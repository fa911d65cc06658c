// cordic_jobs_io16.hip -- the data-fed job-set kinds on int16 / uint16 sample
// arrays (cordic_jobset_create16): launch_xy_jobs16.  A set runs on the tile
// form of the kernel that the single 16-bit call uses -- rotator_unrolled /
// topolar_unrolled<Narrow32, kDynStages, .., Io16> (cordic_inst_io16.hip) -- so
// it serves exactly the cores that call serves on its vector kernel: WW <= 32,
// wrap at WW 32 only.  Dynamic-exit instances only; no looked-up directions
// (cordic_xydir.h is built on the left-justified 64-bit container).
#include <hip/hip_runtime.h>

#include "cordic_jobs_kernels.h"
#include "cordic_jobs_fused.h"

namespace cordic_amd {

namespace {
using namespace dev;

// ---- the 0..3 samples behind each job's last whole vector: one lane per
// sample, one TileDescXY per sample with addresses of 16-bit values.  The
// literal register semantics in a 64-bit container with the explicit WW-bit
// wrap, like the generic kernels of the single calls (rtl/cordic.v:131-188,
// 231-283, 288-314; rtl/topolar.v:122-152, 217-243, 251-271).
__device__ __forceinline__ int64_t wrap16(int64_t v, const CoreParams &kp)
{
	return kp.wrap ? sext64(v, kp.ww) : v;
}

__device__ __forceinline__ int32_t round16(int64_t v, const CoreParams &kp)
{
	const uint64_t b = ((uint64_t)v >> kp.r) & (uint64_t)kp.round_bit;
	const int64_t w = wrap16((int64_t)((uint64_t)v + (uint64_t)kp.round_base + b), kp);
	int32_t o = (int32_t)(w >> kp.r);
	if (kp.wrap)
		o = sext32(o, kp.ow);
	return kp.post_mul ? unit_gain(o, kp.post_mul) : o;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void xy_job_tails16(CoreParams kp,
		const TileDescXY *__restrict__ t, uint32_t n)
{
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n)
		return;
	const TileDescXY d = t[i];
	const int32_t ix = sext32(*reinterpret_cast<const int16_t *>((uintptr_t)d.in0), kp.iw);
	const int32_t iy = sext32(*reinterpret_cast<const int16_t *>((uintptr_t)d.in1), kp.iw);
	const int64_t ex = (int64_t)((uint64_t)(int64_t)ix << kp.in_shl);
	const int64_t ey = (int64_t)((uint64_t)(int64_t)iy << kp.in_shl);
	int64_t x, y;
	uint32_t p;
	if constexpr (KIND == CORDIC_JOBS_R2P) {
		fold_quadrant<int64_t>(ex, ey, ix < 0, iy < 0, x, y, p);
	} else {
		const uint32_t P = KIND == CORDIC_JOBS_MIX ? (uint32_t)d.in2
			: (uint32_t)*reinterpret_cast<const uint16_t *>((uintptr_t)d.in2)
				<< kp.pw_shl;
		fold_octant<int64_t>(ex, ey, P, x, y, p);
	}
	x = wrap16(x, kp);
	y = wrap16(y, kp);
	for (int s = 0; s < kp.nlive; s++) {
		const int k = s + 1;		// (nlive <= kDynStages: below 64)
		const uint32_t a = kp.angle[s];
		const int64_t sy = y >> k, sx = x >> k;
		// rotator: towards phase 0; converter: towards y = 0
		const bool down = KIND == CORDIC_JOBS_R2P ? y >= 0 : (int32_t)p < 0;
		if (down) {
			x += sy; y -= sx; p += a;
		} else {
			x -= sy; y += sx; p -= a;
		}
		x = wrap16(x, kp);
		y = wrap16(y, kp);
	}
	int16_t *const o0 = reinterpret_cast<int16_t *>((uintptr_t)d.o0);
	if constexpr (KIND == CORDIC_JOBS_R2P) {
		*o0 = (int16_t)round16(x, kp);
		*reinterpret_cast<uint16_t *>((uintptr_t)d.o1) = (uint16_t)(p >> kp.pw_shl);
	} else {
		*o0 = (int16_t)round16(x, kp);
		*reinterpret_cast<int16_t *>((uintptr_t)d.o1) = (int16_t)round16(y, kp);
	}
}

template <int KIND>
void launch_tails(hipStream_t st, const CoreParams &kp, const TileDescXY *t, uint32_t n)
{
	hipLaunchKernelGGL(xy_job_tails16<KIND>, dim3((n + kBlock - 1) / kBlock),
		dim3(kBlock), 0, st, kp, t, n);
}
} // namespace

int launch_xy_jobs16(const cordic_config &cfg, int kind, const JobTables &tabs,
		void *stream)
{
	(void)hipGetLastError();	// (a stale error is not this launch's)
	if (kind != CORDIC_JOBS_R2P && kind != CORDIC_JOBS_P2R_XY && kind != CORDIC_JOBS_MIX)
		return CORDIC_ERR_ARGS;
	const bool pol = kind == CORDIC_JOBS_R2P;
	if (!config_sane(cfg))
		return CORDIC_ERR_ARGS;
	if (pol != (cfg.mode == CORDIC_R2P || cfg.mode == CORDIC_SR2P))
		return CORDIC_ERR_MODE;
	if (cfg.iw > 16 || cfg.ow > 16 || (kind != CORDIC_JOBS_MIX && cfg.pw > 16))
		return CORDIC_ERR_CONTAINER;
	if (tabs.samples == 0)
		return CORDIC_OK;
	// the cores whose single 16-bit call runs the vector kernel (launch_rot_feed,
	// launch_topolar with io16)
	if ((cfg.flags & CORDIC_FLAG_FORCE_GENERIC) || cfg.ww > 32
			|| (cfg.needs_wrap && cfg.ww != 32)
			|| cfg.nlive < 1 || cfg.nlive > kDynStages)
		return CORDIC_ERR_UNSUPPORTED;
	hipStream_t st = static_cast<hipStream_t>(stream);
	CoreParams kp = make_params_jobs(cfg);
	kp.xy_nco = kind == CORDIC_JOBS_MIX ? 1u : 0u;
	if (tabs.ntiles) {
		const TileDescXY *tiles = reinterpret_cast<const TileDescXY *>(tabs.tiles);
		const int blocks = jobs_grid(tabs.ntiles);
		if (blocks < 0) {
			(void)hipGetLastError();
			return CORDIC_ERR_DEVICE;
		}
		const dim3 grid(blocks), block(kBlock);
		if (pol && kp.post_mul != 0)
			hipLaunchKernelGGL((topolar_narrow_tiles<true, Io16>), grid, block, 0, st,
				kp, tiles, tabs.ntiles);
		else if (pol)
			hipLaunchKernelGGL((topolar_narrow_tiles<false, Io16>), grid, block, 0, st,
				kp, tiles, tabs.ntiles);
		else if (kp.post_mul != 0)
			hipLaunchKernelGGL((rotator_xy_tiles<Narrow32, 0, true, Io16>), grid, block,
				0, st, kp, tiles, tabs.ntiles);
		else
			hipLaunchKernelGGL((rotator_xy_tiles<Narrow32, 0, false, Io16>), grid, block,
				0, st, kp, tiles, tabs.ntiles);
		if (hipGetLastError() != hipSuccess)
			return CORDIC_ERR_DEVICE;
		g_last_kernel = CORDIC_KERNEL_UNROLLED;
	}
	if (tabs.ntails) {
		const TileDescXY *t = reinterpret_cast<const TileDescXY *>(tabs.tails);
		if (kind == CORDIC_JOBS_R2P)
			launch_tails<CORDIC_JOBS_R2P>(st, kp, t, tabs.ntails);
		else if (kind == CORDIC_JOBS_MIX)
			launch_tails<CORDIC_JOBS_MIX>(st, kp, t, tabs.ntails);
		else
			launch_tails<CORDIC_JOBS_P2R_XY>(st, kp, t, tabs.ntails);
		if (hipGetLastError() != hipSuccess)
			return CORDIC_ERR_DEVICE;
	}
	return CORDIC_OK;
}

} // namespace cordic_amd
