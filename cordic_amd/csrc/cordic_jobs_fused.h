// cordic_jobs_fused.h -- tile-reading kernels for the data-fed job-set kinds
// (CORDIC_JOBS_R2P / _P2R_XY / _MIX) on the cores that launch_xy_jobs has no
// instance for.  A set gets the tile form of the kernel family that ONE long
// call on its core uses (launch_rot_feed, launch_topolar); the tile
// descriptors (TileDescXY) are the ones cordic_jobset_create cuts for every
// data-fed set.  Host-visible types only.
//
// Knobs in the environment, for tests and A/B runs like the banks'
// CORDIC_*_PASSES and CORDIC_*_MAX_BLOCKS; the bits depend on neither:
//   CORDIC_JOBS_TILE_PASSES=<1, 2, 4 or 8>, read at create (cordic_abi.cpp:
//     xy_tile_vecs): the tiles of a data-fed set are that many passes of
//     kJobPassVecs vectors instead of what the tile-length rule gives; the
//     seeded kinds keep kJobTileVecs.
//   CORDIC_JOBS_MAX_BLOCKS=<n>, read at every run (jobs_grid below): at most n
//     blocks walk the tiles, in launch_xy_jobs_fused and launch_xy_jobs16.
//     launch_xy_jobs (cordic_kernels.hip: topolar_lj_jobs and the instances of
//     cordic_inst_xydir_*) keeps its own min(tiles, CUs * 8): that unit is one
//     of those the committed sweep is stamped with (tools/build_stamp.py), so
//     its copy is folded into jobs_grid with the next sweep.
//
// None of these units holds a kernel of the DESIGN section 4.4 sweep (no swept
// workload runs a job set), so tools/build_stamp.py does not hash them.
#ifndef CORDIC_JOBS_FUSED_H
#define CORDIC_JOBS_FUSED_H

#include <hip/hip_runtime_api.h>

#include "cordic_internal.h"

namespace cordic_amd {

namespace dev { struct CoreParams; struct DirArgs; }

// The whole set in one launch of a tile kernel (+ the existing trailing-sample
// launch of launch_xy_jobs).  Called after launch_xy_jobs has answered
// CORDIC_ERR_UNSUPPORTED; CORDIC_ERR_UNSUPPORTED again: the single call on
// this core runs the generic kernel (WW > 40, wrap at a width other than 32,
// the A/B flags) -- the caller runs the jobs one by one.
int	launch_xy_jobs_fused(const cordic_config &cfg, int kind, const RotatorJob &job,
		const JobTables &tabs, void *stream);

// The same for a set on int16 / uint16 arrays (cordic_jobset_create16), in
// cordic_jobs_io16.hip: the tile forms of the kernels of cordic_p2r16 /
// cordic_r2p16 (Narrow32 with Io16 loads and stores) and a trailing-sample
// kernel of its own.  CORDIC_ERR_UNSUPPORTED: the single 16-bit call runs the
// generic kernel on this core (WW > 32, wrap below WW 32, more than kDynStages
// live stages, CORDIC_FLAG_FORCE_GENERIC) -- the caller runs the jobs one by one.
int	launch_xy_jobs16(const cordic_config &cfg, int kind, const JobTables &tabs,
		void *stream);

// kernel arguments of a core (as make_params of cordic_kernels.hip) and the
// CUs of the current device (< 0: no device), shared by the two launchers
dev::CoreParams make_params_jobs(const cordic_config &c);
int	jobs_cus_now();
// ... and their grid: one block per tile up to the resident blocks, 8 per CU of
// the current device; a block past that takes every gridDim.x-th tile.  < 0: no
// device.  CORDIC_JOBS_MAX_BLOCKS=<n> caps it further (see the knobs above).
int	jobs_grid(uint32_t ntiles);

// ---- launchers of the tile kernels (cordic_jobs_rot.hip, cordic_jobs_rotw.hip,
// cordic_jobs_pol.hip, cordic_jobs_xydir.hip); false: no instance
//
// rotator with per-sample vectors (a mixer when kp.xy_nco): the dynamic-exit
// form of rotator_unrolled in the container of the single call --
// lj = 0: Narrow32 (wrap at WW 32), 30: WW <= 34, 29: WW 35, 28 .. 24: WW 36 .. 40
bool	launch_rot_xy_tiles(int lj, int grid, hipStream_t st, const dev::CoreParams &kp,
		const TileDescXY *tiles, uint32_t ntiles);
bool	launch_rot_xy_tiles_w(int lj, int grid, hipStream_t st, const dev::CoreParams &kp,
		const TileDescXY *tiles, uint32_t ntiles);
// ... with looked-up directions: rotator_xydir<LJ, N, true> for the counts
// that cordic_inst_xydir_lj29 / _lj30 do not carry (lj = 29: WW 35, 30: WW <= 34)
bool	launch_xydir_tiles(int lj, int nlive, int grid, hipStream_t st,
		const dev::CoreParams &kp, const dev::DirArgs &da, const TileDescXY *tiles,
		uint32_t ntiles, size_t lds);
// converter: lj = 0: Narrow32 (wrap at WW 32), 30: topolar_lj with unit gain
// (WW <= 34), 29 .. 24: topolar_ljw (WW 35 .. 40)
bool	launch_pol_tiles(int lj, int grid, hipStream_t st, const dev::CoreParams &kp,
		const TileDescXY *tiles, uint32_t ntiles);

} // namespace cordic_amd
#endif
