// cordic_abi_plan.h -- the plan handle, for the two C ABI units that take one:
// cordic_abi.cpp (plans, job sets, the int16 calls) and cordic_abi_fm.cpp (the
// plan-side FM layer).  Private to them.
#ifndef CORDIC_ABI_PLAN_H
#define CORDIC_ABI_PLAN_H

#include <atomic>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_internal.h"
#include "cordic_queue_ring.h"

struct cordic_plan {
	cordic_config cfg;
	uint32_t *d_table = nullptr;	// device copy of the seed table
	int m = 0, S = 0, nbuckets = 0, nleaves = 0;
	cordic_amd::DtInfo dt;		// direction tails behind the seeds (dt.n == 0: none)
	uint32_t *d_dir = nullptr;	// direction tables for per-sample vectors
	cordic_amd::DxInfo dx;		// (dx.n == 0: none)
	cordic_amd::QueueRing queues;
	// prologue images of the seeded kernels, per constant vector (round 5;
	// cordic_internal.h: SeedImages -- internally locked, write-once slots)
	cordic_amd::SeedImages *images = nullptr;
	// batch size from which the table-driven kernels serve (< 0: default)
	std::atomic<long long> min_samples{-1};
	// an int16 entry point has been called on this plan: cordic_plan_prepare
	// then also builds the int16 container's image (its own slot)
	mutable std::atomic<bool> io16_used{false};
};

namespace cordic_amd {

// 16-bit containers: do the core's samples (and phase words) fit?
inline int fits16(const cordic_config &c, bool phase_array)
{
	if (c.iw > 16 || c.ow > 16 || (phase_array && c.pw > 16))
		return CORDIC_ERR_CONTAINER;
	return CORDIC_OK;
}

} // namespace cordic_amd
#endif
