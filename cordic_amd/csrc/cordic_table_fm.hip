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

constexpr int kTile = (int)kFmTile;
// the phases of a tile behind the last 8 of the tile before it
constexpr size_t kPhaseBytes = (size_t)(8 + kTile) * sizeof(uint32_t);

// four consecutive words at any 4-byte-aligned address: one dwordx4 access
struct __attribute__((packed, aligned(4))) Words4 {
	uint32_t v[4];
};

// the phase as a core of its own: cordic_phase_accumulate's output
struct CoreIdent {
	typedef int32_t entry;
	__device__ __forceinline__ const entry *stage(unsigned char *) const { return nullptr; }
	__device__ __forceinline__ int32_t sample(const entry *, uint32_t ph) const
	{
		return (int32_t)ph;
	}
};

// sum of v over the block's 1024 threads, in every thread; wsum: 16 words of
// LDS that are free again when the call returns
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *wsum)
{
#pragma unroll
	for (int d = 32; d; d >>= 1)
		v += __shfl_xor(v, d);
	if ((threadIdx.x & 63u) == 0)
		wsum[threadIdx.x >> 6] = v;
	__syncthreads();
	uint32_t s = 0;
#pragma unroll
	for (int j = 0; j < 16; j++)
		s += wsum[j];
	__syncthreads();
	return s;
}

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
	typedef typename OutVec<T>::type V;
	constexpr int W = 16 / sizeof(T);
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ uint32_t wsum[16];
	const unsigned tid = threadIdx.x, lane = tid & 63u;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const typename CORE::entry *tab = core.stage(lds_raw);
	// ph[8 + j]: the phase of sample t0 + j of the current tile; ph[0 .. 8):
	// the last 8 phases of the tile before it
	uint32_t *ph = reinterpret_cast<uint32_t *>(lds_raw + a.table_bytes);

	const size_t lo = (size_t)blockIdx.x * a.span;	// < n by the grid
	const size_t hi = (a.n - lo < a.span) ? a.n : lo + a.span;
	// (the grid has at most 1024 blocks: one partial per thread)
	uint32_t carry = a.work[0]
		+ block_sum(tid < blockIdx.x ? a.work[4 + tid] : 0u, wsum);

	// this lane's 4 words of the tile at t0; nothing at or behind hi is read
	auto load_tile = [&](size_t t0, uint32_t (&f)[4], uint32_t (&m)[4]) {
		const size_t i = t0 + 4 * (size_t)tid;
		if (i + 4 <= hi) {
			const Words4 q = *reinterpret_cast<const Words4 *>(a.fcw + i);
#pragma unroll
			for (int k = 0; k < 4; k++)
				f[k] = q.v[k];
			if (a.pm) {
				const Words4 r = *reinterpret_cast<const Words4 *>(a.pm + i);
#pragma unroll
				for (int k = 0; k < 4; k++)
					m[k] = r.v[k];
			} else {
#pragma unroll
				for (int k = 0; k < 4; k++)
					m[k] = 0u;
			}
		} else {
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const bool in = i + k < hi;
				f[k] = in ? a.fcw[i + k] : 0u;
				m[k] = (in && a.pm) ? a.pm[i + k] : 0u;
			}
		}
	};

	// one stream's window of the tile [t0, t1): see the head of this file
	auto emit = [&](T *out, uint32_t lead, size_t t0, size_t t1) {
		const size_t w0 = (t0 == lo) ? lo
			: t0 - (size_t)(reinterpret_cast<uintptr_t>(out + t0) & 15u) / sizeof(T);
		const size_t w1 = (t1 == hi) ? hi
			: t1 - (size_t)(reinterpret_cast<uintptr_t>(out + t1) & 15u) / sizeof(T);
		size_t h = head_elems(reinterpret_cast<uintptr_t>(out + w0), sizeof(T));
		if (h > w1 - w0)
			h = w1 - w0;
		// At most 4096 / W vectors, so one per thread covers them.  Behind a
		// span's first tile out + t0 and out + t1 = out + t0 + 4096 sit alike
		// on the 16-byte grid: the window is moved back, not widened, and is
		// 4096 samples (shorter in the last tile).  The first tile has nothing
		// in front of t0: at most 4096 samples again, less its head.
		const size_t nv = (w1 - w0 - h) / W;
		const size_t tail = w0 + h + nv * W;
		// pw[i] for a sample index i in [t0 - 8, t1)
		auto phase_of = [&](size_t i) -> uint32_t {
			return ph[8 + ((ptrdiff_t)i - (ptrdiff_t)t0)];
		};
		if (tid < nv) {
			const size_t e = w0 + h + (size_t)tid * W;
			const uint32_t *pp = ph + (8 + ((ptrdiff_t)e - (ptrdiff_t)t0));
			uint32_t q[W];
			if ((reinterpret_cast<uintptr_t>(pp) & 15u) == 0) {
				// (uniform: the stream sits on the tile grid)
#pragma unroll
				for (int v = 0; v < W; v += 4) {
					const uint4 r = *reinterpret_cast<const uint4 *>(pp + v);
					q[v] = r.x; q[v + 1] = r.y; q[v + 2] = r.z; q[v + 3] = r.w;
				}
			} else {
#pragma unroll
				for (int v = 0; v < W; v++)
					q[v] = pp[v];
			}
			V o;
#pragma unroll
			for (int v = 0; v < W; v++)
				o[v] = (T)core.sample(tab, q[v] + lead);
			__builtin_nontemporal_store(o, reinterpret_cast<V *>(out + e));
		}
		// fewer than W samples each, and only in a span's first / last tile
		if (tid < h)
			out[w0 + tid] = (T)core.sample(tab, phase_of(w0 + tid) + lead);
		if (tid < w1 - tail)
			out[tail + tid] = (T)core.sample(tab, phase_of(tail + tid) + lead);
	};

	uint32_t f[4], m[4];
	load_tile(lo, f, m);
	for (size_t t0 = lo; t0 < hi; t0 += kTile) {
		const size_t t1 = (hi - t0 < (size_t)kTile) ? hi : t0 + kTile;
		// inclusive sums: in the lane, then over the wave's lanes
		const uint32_t s0 = f[0], s1 = s0 + f[1], s2 = s1 + f[2], s3 = s2 + f[3];
		uint32_t incl = s3;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t up = __shfl_up(incl, d);
			if (lane >= (unsigned)d)
				incl += up;
		}
		if (lane == 63)
			wsum[wave] = incl;
		__syncthreads();
		// the waves in front of this one, and the tile's total
		uint32_t front = 0, total = 0;
#pragma unroll
		for (unsigned j = 0; j < 16; j++) {
			const uint32_t w = wsum[j];
			front += (j < wave) ? w : 0u;
			total += w;
		}
		const uint32_t excl = carry + front + incl - s3;
		// Every lane rewrites its own 4 phases only, and the readers of the
		// tile before are past the barrier above: the owners of the last 8
		// move theirs to the front first.  (The first tile of a span never
		// looks in front of itself.)
		uint4 *mine = reinterpret_cast<uint4 *>(ph + 8 + 4 * tid);
		if (tid >= 1022)
			*reinterpret_cast<uint4 *>(ph + 4 * (tid - 1022)) = *mine;
		*mine = make_uint4(excl + m[0], excl + s0 + m[1], excl + s1 + m[2],
			excl + s2 + m[3]);
		carry += total;
		__syncthreads();
		// the next tile's words are on their way while this one is sampled
		load_tile(t0 + kTile, f, m);
		emit(d_sin, 0u, t0, t1);
		if (d_cos)
			emit(d_cos, a.quarter, t0, t1);
	}
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
