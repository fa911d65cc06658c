// cordic_table_fm.hip -- the table and quadratic sine cores as frequency- and
// phase-modulated oscillators (cordic_table_fm / cordic_quad_fm and their
// int16 forms) and the phase accumulator alone (cordic_phase_accumulate):
//   p_i = start + fcw[0] + .. + fcw[i-1] + pm[i]      (mod 2^32)
// with one tuning word and (optionally) one phase word per sample.
//
// The running sum is a prefix sum done as reduce-then-scan in two launches.
// The samples are cut into tiles of 4096; every block owns a contiguous span
// of whole tiles.
//   1. fm_reduce: each block sums its span of fcw into a workspace word;
//      block 0 latches start = phase0 + *d_acc beside them.
//   2. table_fm: each block adds the partials in front of it to the latched
//      start, then walks its span tile by tile: a lane reads 4 consecutive
//      words (one 16-byte access at whatever 4-byte alignment fcw has), sums
//      them, the wave scans the lane sums with __shfl_up, the 16 waves
//      exchange their totals through LDS, and a carry runs from tile to tile.
//      The tile's phases go to LDS; from there the block samples the core and
//      stores on each output's OWN 16-byte grid, as table_nco does.  The last
//      block writes *d_acc.
// No block ever waits for another: what a block needs of the others is
// complete when launch 2 starts.  The price is a second read of fcw.
// The walk over a block's tiles is tile_loop (cordic_table_fm.h), which the
// FM oscillator banks' kernel (cordic_table_fm_bank.hip) runs as well.
//
// *d_acc is read in launch 1 only and written in launch 2 only, so no block
// of a call can see the value the call itself writes.
//
// In place (cordic_phase_accumulate with d_phase == d_fcw): launch 1 has read
// everything before launch 2 writes anything; in launch 2 a block has read a
// whole tile (and issued the next tile's reads, which lie behind this tile's
// last output) before it stores any of it, and spans of different blocks are
// disjoint.
//
// Output grids: a tile [t0, t1) of samples does not end on a 16-byte boundary
// of an output array that sits differently from the tile grid.  A tile stores
// the window [A(t0), A(t1)) of each stream, A(i) = the last index <= i whose
// address is 16-byte aligned, as whole aligned vectors; the up to 7 phases in
// front of t0 that this needs are kept in LDS from the tile before.  The first
// tile of a span starts at the span's first sample and the last one ends at
// its last sample, with scalar stores for the few samples off the grid.
// Nothing outside [0, n) of an output is written.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_table_fm.h"
#include "cordic_table_nco.h"
#include "cordic_jobs_fused.h"
#include "cordic_hostargs.h"

namespace cordic_amd {

namespace tfm {

using namespace tnco;

// the phase as a core of its own: cordic_phase_accumulate's output
struct CoreIdent {
	typedef int32_t entry;
	__device__ __forceinline__ const entry *stage(unsigned char *) const { return nullptr; }
	__device__ __forceinline__ int32_t sample(const entry *, uint32_t ph) const
	{
		return (int32_t)ph;
	}
};

// launch 1: work[4 + b] = the sum of block b's span [b * span, (b + 1) * span)
// of fcw (cut at n), work[0] = phase0 + *d_acc.  The span is read on fcw's own
// 16-byte grid (a sum does not care for the order).
__global__ __launch_bounds__(1024) void fm_reduce(const uint32_t *d_fcw, size_t n,
		size_t span, uint32_t phase0, const uint32_t *d_acc, uint32_t *work)
{
	__shared__ uint32_t wsum[16];
	const size_t lo = (size_t)blockIdx.x * span;	// < n by the grid
	const size_t len = (n - lo < span) ? n - lo : span;
	const uint32_t *f = d_fcw + lo;
	size_t head = head_elems(reinterpret_cast<uintptr_t>(f), 4);
	if (head > len)
		head = len;
	const size_t nv = (len - head) / 4;
	const uint4 *fv = reinterpret_cast<const uint4 *>(f + head);
	uint32_t s = 0;
#pragma unroll 4
	for (size_t g = threadIdx.x; g < nv; g += 1024) {
		const uint4 q = fv[g];
		s += q.x + q.y + q.z + q.w;
	}
	if (threadIdx.x < head)
		s += f[threadIdx.x];
	const size_t t = head + nv * 4 + threadIdx.x;	// fewer than 4 behind the vectors
	if (t < len)
		s += f[t];
	s = block_sum(s, wsum);
	if (threadIdx.x == 0) {
		work[4 + blockIdx.x] = s;
		if (blockIdx.x == 0)
			work[0] = phase0 + (d_acc ? *d_acc : 0u);
	}
}

struct FmArgs {
	const uint32_t *fcw, *pm;	// pm may be NULL
	uint32_t *acc;			// may be NULL
	const uint32_t *work;
	size_t	n, span;		// span: samples per block, whole tiles
	uint32_t quarter;		// 2^(PW-2): the cosine's lead
	uint32_t table_bytes;		// the core's LDS copy, a multiple of 16
};

// launch 2.  Blocks of 1024 threads; dynamic LDS: [the core's table | 8 + 4096
// phases].  d_cos == NULL: sine only (a uniform branch, as a.pm == NULL is).
//
// Registers: every instance stays within 64, so two blocks are resident on a CU
// wherever the LDS admits two, and one block's two barriers per tile hide
// behind the other's loads and stores.
template <typename CORE, typename T>
__global__ __launch_bounds__(1024) void table_fm(CORE core, FmArgs a, T *d_sin,
		T *d_cos)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ uint32_t wsum[16];
	const unsigned tid = threadIdx.x;
	const typename CORE::entry *tab = core.stage(lds_raw);
	// the tile's phases behind the table (tile_loop, cordic_table_fm.h)
	uint32_t *ph = reinterpret_cast<uint32_t *>(lds_raw + a.table_bytes);

	const size_t lo = (size_t)blockIdx.x * a.span;	// < n by the grid
	const size_t hi = (a.n - lo < a.span) ? a.n : lo + a.span;
	// (the grid has at most 1024 blocks: one partial per thread)
	uint32_t carry = a.work[0]
		+ block_sum(tid < blockIdx.x ? a.work[4 + tid] : 0u, wsum);

	tile_loop<CORE, T>(core, tab, ph, wsum, a, d_sin, d_cos, lo, hi, carry);
	if (a.acc && blockIdx.x == gridDim.x - 1 && tid == 0)
		*a.acc = carry;
}

// ---------------------------------------------------------------- host side
// Alignment, and no output range over anything else.  out0 == d_fcw exactly is
// the in-place form where `inplace` allows it.
static int check_call(size_t n, const uint32_t *d_fcw, const uint32_t *d_pm,
		const uint32_t *d_acc, const void *out0, const void *out1, size_t esize,
		const void *d_work, bool inplace)
{
	if (!d_fcw || !out0 || !d_work || n > (~(size_t)0 >> 4))
		return CORDIC_ERR_ARGS;
	const uintptr_t words = reinterpret_cast<uintptr_t>(d_fcw)
		| reinterpret_cast<uintptr_t>(d_pm) | reinterpret_cast<uintptr_t>(d_acc);
	const uintptr_t outs = reinterpret_cast<uintptr_t>(out0)
		| reinterpret_cast<uintptr_t>(out1);
	if ((words & 3u) || (outs & (esize - 1))
			|| (reinterpret_cast<uintptr_t>(d_work) & 15u))
		return CORDIC_ERR_ARGS;
	const Range out[4] = {range_of(out0, n * esize), range_of(out1, n * esize),
		range_of(d_acc, 4), range_of(d_work, kFmWorkBytes)};
	const Range in[2] = {range_of(d_fcw, n * 4), range_of(d_pm, n * 4)};
	return outputs_overlap(out, in, inplace) ? CORDIC_ERR_ARGS : CORDIC_OK;
}

} // namespace tfm

void launch_fm_reduce(unsigned grid, const uint32_t *d_fcw, size_t n, size_t span,
		uint32_t phase0, const uint32_t *d_acc, uint32_t *work, void *stream)
{
	hipLaunchKernelGGL(tfm::fm_reduce, dim3(grid), dim3(1024), 0,
		static_cast<hipStream_t>(stream), d_fcw, n, span, phase0, d_acc, work);
}

namespace tfm {

struct Call {
	size_t	n;
	const uint32_t *d_fcw, *d_pm;
	uint32_t phase0;
	uint32_t *d_acc;
	void	*d_sin, *d_cos, *d_work;
	uint32_t quarter;
	hipStream_t st;
};

// both launches for one layout; false: nothing usable was launched
template <typename CORE, typename T>
bool launch_one(const CORE &core, const Call &c, size_t table_bytes)
{
	const size_t lds = table_bytes + kPhaseBytes;
	// (+ the kernel's static scratch)
	const int per_cu = lds_blocks_per_cu(lds + 128);
	if (per_cu < 1 || !allow_lds((const void *)table_fm<CORE, T>, lds + 128))
		return false;
	const int cus = jobs_cus_now();
	if (cus < 0)
		return false;
	size_t cap = (size_t)cus * per_cu;
	if (cap > kFmMaxBlocks)
		cap = kFmMaxBlocks;
	const size_t ntiles = (c.n + kFmTile - 1) / kFmTile;
	const size_t per_block = (ntiles + cap - 1) / cap;
	const size_t span = per_block * kFmTile;
	const unsigned grid = (unsigned)((ntiles + per_block - 1) / per_block);
	uint32_t *work = static_cast<uint32_t *>(c.d_work);
	launch_fm_reduce(grid, c.d_fcw, c.n, span, c.phase0, c.d_acc, work, c.st);
	const FmArgs a{c.d_fcw, c.d_pm, c.d_acc, work, c.n, span, c.quarter,
		(uint32_t)table_bytes};
	hipLaunchKernelGGL((table_fm<CORE, T>), dim3(grid), dim3(1024), lds, c.st,
		core, a, static_cast<T *>(c.d_sin), static_cast<T *>(c.d_cos));
	return true;
}

} // namespace tfm

int launch_sine_fm(const SineCore &c, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, void *d_sin,
		void *d_cos, bool io16, void *d_work, void *stream)
{
	using namespace tfm;
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (io16 && c.ow() > 16) return CORDIC_ERR_CONTAINER;
	if (n == 0) return CORDIC_OK;
	if (!c.sane()) return CORDIC_ERR_ARGS;
	if (int rc = check_call(n, d_fcw, d_pm, d_acc, d_sin, d_cos, io16 ? 2 : 4,
			d_work, false))
		return rc;
	const Call call{n, d_fcw, d_pm, phase0, d_acc, d_sin, d_cos, d_work,
		c.quarter(), static_cast<hipStream_t>(stream)};
	// (an LDS copy that does not fit beside the phases: the L2 gather)
	return with_layout(c, io16, [&](const auto &core, auto tag, size_t bytes) {
		return launch_one<std::decay_t<decltype(core)>, decltype(tag)>(core, call,
			bytes);
	});
}

} // namespace cordic_amd

// ------------------------------------------------ the two handle-free calls
size_t cordic_fm_workspace(size_t n)
{
	return n ? cordic_amd::kFmWorkBytes : 0;
}

int cordic_phase_accumulate(size_t n, const uint32_t *d_fcw, const uint32_t *d_pm,
		uint32_t phase0, uint32_t *d_acc, uint32_t *d_phase, void *d_work,
		void *stream)
{
	using namespace cordic_amd;
	using namespace cordic_amd::tfm;
	(void)hipGetLastError();
	if (n == 0)
		return CORDIC_OK;
	if (int rc = check_call(n, d_fcw, d_pm, d_acc, d_phase, nullptr, 4, d_work, true))
		return rc;
	const Call c{n, d_fcw, d_pm, phase0, d_acc, d_phase, nullptr, d_work, 0u,
		static_cast<hipStream_t>(stream)};
	return finish(launch_one<CoreIdent, int32_t>(CoreIdent{}, c, 0));
}
