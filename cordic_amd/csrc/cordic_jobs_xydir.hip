// cordic_jobs_xydir.hip -- tile-reading instances of the looked-up-direction
// rotator (cordic_xydir.h: rotator_xydir<LJ, N, true>) for the stage counts
// that gencordic derives or BASELINE names (13, 16, 19, 20, 24, 27, 29) and
// that cordic_inst_xydir_lj29 / _lj30 do not carry already.  Any other count of
// a core with a direction table runs its set on the dynamic-exit tile kernel
// (rotator_xy_tiles): slower, still one launch.
#include <hip/hip_runtime.h>

#include "cordic_xydir.h"
#include "cordic_jobs_fused.h"

#define CORDIC_XYDIR_MORE_LJ30(X) X(13) X(20) X(24) X(29)
#define CORDIC_XYDIR_MORE_LJ29(X) X(13) X(19) X(20) X(27)

namespace cordic_amd {

bool launch_xydir_tiles(int lj, int nlive, int grid, hipStream_t st,
		const dev::CoreParams &kp, const dev::DirArgs &da, const TileDescXY *tiles,
		uint32_t ntiles, size_t lds)
{
	using namespace dev;
#define X(N) case N: \
	if (da.dx.n != dx_levels(N)) \
		return false; \
	hipLaunchKernelGGL((rotator_xydir<LJ_, N, true>), dim3(grid), dim3(kBlock), lds, \
		st, kp, da, (const i32x4g *)nullptr, (const i32x4g *)nullptr, \
		(const u32x4g *)nullptr, (i32x4g *)nullptr, (i32x4g *)nullptr, (size_t)0, \
		tiles, ntiles); \
	return true;
	if (lj == 30) {
		constexpr int LJ_ = 30;
		switch (nlive) {
		CORDIC_XYDIR_MORE_LJ30(X)
		default: return false;
		}
	}
	if (lj == 29) {
		constexpr int LJ_ = 29;
		switch (nlive) {
		CORDIC_XYDIR_MORE_LJ29(X)
		default: return false;
		}
	}
#undef X
	return false;
}

} // namespace cordic_amd
