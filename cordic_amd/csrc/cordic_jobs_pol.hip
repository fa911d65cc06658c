// cordic_jobs_pol.hip -- tile-reading converters (cordic_jobs_kernels.h) for
// the r2p / sr2p cores that topolar_lj_jobs does not serve: unit gain at
// WW <= 34, the left-justified wide form at WW 35 .. 40, the 32-bit container
// where the core wraps at WW 32.
#include <hip/hip_runtime.h>

#include "cordic_jobs_kernels.h"
#include "cordic_jobs_fused.h"

namespace cordic_amd {

namespace {
template <int LJ>
void launch_ljw(int grid, hipStream_t st, const dev::CoreParams &kp,
		const TileDescXY *tiles, uint32_t ntiles)
{
	using namespace dev;
	if (kp.post_mul != 0)
		hipLaunchKernelGGL((topolar_ljw_tiles<LJ, true>), dim3(grid), dim3(kBlock),
			0, st, kp, tiles, ntiles);
	else
		hipLaunchKernelGGL((topolar_ljw_tiles<LJ, false>), dim3(grid), dim3(kBlock),
			0, st, kp, tiles, ntiles);
}
} // namespace

bool launch_pol_tiles(int lj, int grid, hipStream_t st, const dev::CoreParams &kp,
		const TileDescXY *tiles, uint32_t ntiles)
{
	using namespace dev;
	switch (lj) {
	case 0:
		if (kp.post_mul != 0)
			hipLaunchKernelGGL((topolar_narrow_tiles<true>), dim3(grid),
				dim3(kBlock), 0, st, kp, tiles, ntiles);
		else
			hipLaunchKernelGGL((topolar_narrow_tiles<false>), dim3(grid),
				dim3(kBlock), 0, st, kp, tiles, ntiles);
		return true;
	case 30:	// (without unit gain: topolar_lj_jobs, cordic_inst_pol_lj.hip)
		if (kp.post_mul == 0)
			return false;
		hipLaunchKernelGGL(topolar_lj_tiles<true>, dim3(grid), dim3(kBlock), 0, st, kp,
			tiles, ntiles);
		return true;
	case 29: launch_ljw<29>(grid, st, kp, tiles, ntiles); return true;
	case 28: launch_ljw<28>(grid, st, kp, tiles, ntiles); return true;
	case 27: launch_ljw<27>(grid, st, kp, tiles, ntiles); return true;
	case 26: launch_ljw<26>(grid, st, kp, tiles, ntiles); return true;
	case 25: launch_ljw<25>(grid, st, kp, tiles, ntiles); return true;
	case 24: launch_ljw<24>(grid, st, kp, tiles, ntiles); return true;
	default: return false;
	}
}

} // namespace cordic_amd
