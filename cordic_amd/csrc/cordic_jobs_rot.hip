// cordic_jobs_rot.hip -- tile-reading rotator for per-sample vectors
// (cordic_jobs_kernels.h: rotator_xy_tiles) in the containers of WW <= 35:
// Narrow32 (wrap at WW 32), WideLJ<30> (WW <= 34), WideLJ<29> (WW 35).
#include <hip/hip_runtime.h>

#include "cordic_jobs_kernels.h"
#include "cordic_jobs_fused.h"

namespace cordic_amd {

namespace {
// NGEN: that of the single call's unit (cordic_inst_rot_narrow / _lj30 / _lj29)
template <typename C, int NGEN>
void launch_c(int grid, hipStream_t st, const dev::CoreParams &kp,
		const TileDescXY *tiles, uint32_t ntiles)
{
	using namespace dev;
	if (kp.post_mul != 0)
		hipLaunchKernelGGL((rotator_xy_tiles<C, NGEN, true>), dim3(grid), dim3(kBlock),
			0, st, kp, tiles, ntiles);
	else
		hipLaunchKernelGGL((rotator_xy_tiles<C, NGEN, false>), dim3(grid), dim3(kBlock),
			0, st, kp, tiles, ntiles);
}
} // namespace

bool launch_rot_xy_tiles(int lj, int grid, hipStream_t st, const dev::CoreParams &kp,
		const TileDescXY *tiles, uint32_t ntiles)
{
	using namespace dev;
	switch (lj) {
	case 0: launch_c<Narrow32, 0>(grid, st, kp, tiles, ntiles); return true;
	case 30: launch_c<WideLJ<30>, 1>(grid, st, kp, tiles, ntiles); return true;
	case 29: launch_c<WideLJ<29>, 2>(grid, st, kp, tiles, ntiles); return true;
	default: return launch_rot_xy_tiles_w(lj, grid, st, kp, tiles, ntiles);
	}
}

} // namespace cordic_amd
