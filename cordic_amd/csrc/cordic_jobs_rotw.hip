// cordic_jobs_rotw.hip -- tile-reading rotator for per-sample vectors
// (cordic_jobs_kernels.h: rotator_xy_tiles) at WW 36 .. 40: WideLJ<64 - WW>,
// as cordic_inst_rot_lj28 .. _lj24 serve the single call.
#include <hip/hip_runtime.h>

#include "cordic_jobs_kernels.h"
#include "cordic_jobs_fused.h"

namespace cordic_amd {

namespace {
template <int LJ>
void launch_w(int grid, hipStream_t st, const dev::CoreParams &kp,
		const TileDescXY *tiles, uint32_t ntiles)
{
	using namespace dev;
	// (NGEN is not read by the left-justified chain)
	if (kp.post_mul != 0)
		hipLaunchKernelGGL((rotator_xy_tiles<WideLJ<LJ>, 31 - LJ, true>), dim3(grid),
			dim3(kBlock), 0, st, kp, tiles, ntiles);
	else
		hipLaunchKernelGGL((rotator_xy_tiles<WideLJ<LJ>, 31 - LJ, false>), dim3(grid),
			dim3(kBlock), 0, st, kp, tiles, ntiles);
}
} // namespace

bool launch_rot_xy_tiles_w(int lj, int grid, hipStream_t st, const dev::CoreParams &kp,
		const TileDescXY *tiles, uint32_t ntiles)
{
	switch (lj) {
	case 28: launch_w<28>(grid, st, kp, tiles, ntiles); return true;
	case 27: launch_w<27>(grid, st, kp, tiles, ntiles); return true;
	case 26: launch_w<26>(grid, st, kp, tiles, ntiles); return true;
	case 25: launch_w<25>(grid, st, kp, tiles, ntiles); return true;
	case 24: launch_w<24>(grid, st, kp, tiles, ntiles); return true;
	default: return false;
	}
}

} // namespace cordic_amd
