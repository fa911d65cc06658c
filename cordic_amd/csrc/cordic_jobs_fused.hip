// cordic_jobs_fused.hip -- launch_xy_jobs_fused: the data-fed kinds of a job
// set in one launch on the cores that launch_xy_jobs (cordic_kernels.hip) has
// no tile-reading instance for.  The choice of kernel mirrors the single call
// on the same core (launch_rot_feed for the rotator and the mixer,
// launch_topolar for the converter), so the fused rate tracks the single-call
// rate; the trailing samples go to launch_xy_jobs' own tail launch.
#include <hip/hip_runtime.h>

#include "cordic_device.h"
#include "cordic_launch.h"
#include "cordic_xydir.h"
#include "cordic_hostargs.h"
#include "cordic_jobs_fused.h"

namespace cordic_amd {

using dev::CoreParams;

// Twin of make_params in cordic_kernels.hip (anonymous namespace there); the
// two are to be folded together with the next change to that file.
CoreParams make_params_jobs(const cordic_config &c)
{
	CoreParams kp{};
	const bool rot = (c.mode == CORDIC_P2R || c.mode == CORDIC_SP2R);
	const int lsh = 32 - c.pw;
	for (int i = 0; i < CORDIC_AMD_MAX_STAGES; i++)
		kp.angle[i] = (i < c.nstages) ? (c.angle[i] << lsh) : 0u;
	kp.nlive = c.nlive;
	kp.iw = c.iw;
	kp.in_shl = rot ? (c.ww - c.iw - 1) : (c.ww - c.iw - 2);
	kp.pw_shl = lsh;
	kp.ww = c.ww;
	kp.ow = c.ow;
	kp.r = c.ww - c.ow;
	const bool rounding = c.ww > c.ow + 1;
	kp.round_bit = rounding ? 1u : 0u;
	kp.round_base = rounding ? (((int64_t)1 << (kp.r - 1)) - 1) : 0;
	kp.wrap = c.needs_wrap && c.ww < 64;
	// left-justified wide form: LJ = 64 - WW for WW 35..40, 30 for WW 33, 34
	const int lj = (c.ww >= 35 && c.ww <= 40) ? 64 - c.ww : 30;
	kp.r_lj = kp.r + lj;
	kp.round_base_lj = (int64_t)((uint64_t)kp.round_base << lj);
	kp.post_mul = (c.flags & CORDIC_FLAG_UNIT_GAIN) ? core_gain_annihilator(c) : 0u;
	return kp;
}

int jobs_cus_now()
{
	int dev = 0, cus = 0;
	if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus,
			hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
		return -1;
	return cus;
}

int jobs_grid(uint32_t ntiles)
{
	const int cus = jobs_cus_now();
	if (cus < 0)
		return -1;
	// resident blocks
	const size_t cap = env_block_cap("CORDIC_JOBS_MAX_BLOCKS", (size_t)cus * 8);
	return (int)(ntiles < cap ? ntiles : cap);
}

int launch_xy_jobs_fused(const cordic_config &cfg, int kind, const RotatorJob &j,
		const JobTables &tabs, void *stream)
{
	(void)hipGetLastError();	// (a stale error is not this launch's)
	const bool pol = kind == CORDIC_JOBS_R2P;
	if (!config_sane(cfg))
		return CORDIC_ERR_ARGS;
	if (pol != (cfg.mode == CORDIC_R2P || cfg.mode == CORDIC_SR2P))
		return CORDIC_ERR_MODE;
	if (tabs.samples == 0)
		return CORDIC_OK;
	// the cores whose single call runs the generic kernel (or an A/B form)
	if ((cfg.flags & (CORDIC_FLAG_FORCE_GENERIC | CORDIC_FLAG_NO_LJ))
			|| cfg.ww > 40 || (cfg.needs_wrap && cfg.ww != 32)
			|| cfg.nlive < 1 || cfg.nlive > kDynStages)
		return CORDIC_ERR_UNSUPPORTED;
	hipStream_t st = static_cast<hipStream_t>(stream);
	CoreParams kp = make_params_jobs(cfg);
	kp.xy_nco = kind == CORDIC_JOBS_MIX ? 1u : 0u;
	// (launch_rot_feed: a 64-bit container folds with 32-bit multipliers)
	if (!pol && cfg.ww > 32 && kp.in_shl > 30)
		return CORDIC_ERR_UNSUPPORTED;
	if (tabs.ntiles) {
		const TileDescXY *tiles = reinterpret_cast<const TileDescXY *>(tabs.tiles);
		const int grid = jobs_grid(tabs.ntiles);
		if (grid < 0) {
			(void)hipGetLastError();
			return CORDIC_ERR_DEVICE;
		}
		// container of the single call: 0 = the 32-bit one (wrap at WW 32),
		// else left-justified by 30 (WW <= 34) or 64 - WW (WW 35 .. 40)
		const int lj = cfg.needs_wrap ? 0 : cfg.ww <= 34 ? 30 : 64 - cfg.ww;
		bool done = false;
		int family = CORDIC_KERNEL_UNROLLED;
		if (pol) {
			done = launch_pol_tiles(lj, grid, st, kp, tiles, tabs.ntiles);
			if (lj != 0)
				family = CORDIC_KERNEL_LEFT_JUSTIFIED;
		} else {
			// the direction tables where the single call looks them up
			// (launch_rot_feed), minus the batch-size threshold
			if (j.dir_table && j.dx.n > 0 && kp.post_mul == 0 && kp.in_shl >= 1
					&& kp.in_shl <= 30 && cfg.ww <= 35 && !cfg.needs_wrap
					&& !(cfg.flags & CORDIC_FLAG_NO_TAILS)) {
				dev::DirArgs da{j.dir_table, j.dx};
				const size_t lds = dev::dx_lds_layout(j.dx, nullptr, nullptr);
				if (lds <= 64 * 1024)
					done = launch_xydir_tiles(cfg.ww == 35 ? 29 : 30, cfg.nlive,
						grid, st, kp, da, tiles, tabs.ntiles, lds);
				if (done)
					family = CORDIC_KERNEL_DIRECTIONS;
			}
			if (!done)
				done = launch_rot_xy_tiles(lj, grid, st, kp, tiles, tabs.ntiles);
		}
		if (!done)
			return CORDIC_ERR_UNSUPPORTED;
		if (hipGetLastError() != hipSuccess)
			return CORDIC_ERR_DEVICE;
		g_last_kernel = family;
	}
	if (tabs.ntails) {
		// 0..3 samples behind each job's last whole vector: the generic
		// per-sample kernel of launch_xy_jobs (round_generic applies unit gain
		// and the wrap), which launches nothing else without tiles
		JobTables t = tabs;
		t.ntiles = 0;
		return launch_xy_jobs(cfg, kind, j, t, stream);
	}
	return CORDIC_OK;
}

} // namespace cordic_amd
