// cordic_table_fm.h -- frequency- and phase-modulated oscillator forms of the
// table and quadratic sine cores (cordic_table_fm / cordic_quad_fm and their
// int16 forms), and the phase accumulator they are built on
// (cordic_phase_accumulate): the phase of sample i is a running sum of
// per-sample tuning words, made on the device.  The launcher for
// cordic_abi_table.cpp; the two public functions that need no handle
// (cordic_fm_workspace, cordic_phase_accumulate) are defined in
// cordic_table_fm.hip itself.  Behind them, for HIP units only, the tile loop
// that the single call's kernel and the kernel of the FM oscillator banks
// (cordic_table_fm_bank.hip) share.
//
// The core comes as a SineCore, and its layouts, their choice and the sample
// functions are those of cordic_table_nco.h: there is one copy of them.
// Neither unit holds a kernel of the DESIGN section 4.4 sweep.
#ifndef CORDIC_TABLE_FM_H
#define CORDIC_TABLE_FM_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_table_nco.h"

namespace cordic_amd {

// The prefix sum is cut into tiles of kFmTile samples; a launch has at most
// kFmMaxBlocks blocks, each with a contiguous span of whole tiles.  The
// workspace is one word for the latched start phase (in a 16-byte slot) and
// one partial sum per block.
constexpr size_t kFmTile = 4096;
constexpr size_t kFmMaxBlocks = 1024;
constexpr size_t kFmWorkBytes = 16 + 4 * kFmMaxBlocks;

// Two launches on `stream` (reduce, then scan + sample + store), nothing else:
//   start = phase0 + (d_acc ? *d_acc : 0)
//   p_i   = start + fcw[0] + .. + fcw[i-1] + (d_pm ? pm[i] : 0)
//   d_sin[i] = core(p_i), d_cos[i] = core(p_i + 2^(PW-2))   (d_cos NULL: none)
//   *d_acc = start + fcw[0] + .. + fcw[n-1]
// io16: the outputs are int16_t (OW <= 16: CORDIC_ERR_CONTAINER otherwise),
// any 2-byte-aligned address; else int32_t, 4-byte aligned.  The launcher
// checks alignment and that no output range (d_acc and d_work included)
// overlaps anything else.  The layout is the one launch_sine_nco would choose,
// where its copy fits into LDS beside a tile's phases; else the L2 gather.
// n == 0: CORDIC_OK, nothing touched.
int	launch_sine_fm(const SineCore &c, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, void *d_sin,
		void *d_cos, bool io16, void *d_work, void *stream);

// Launch 1 alone, for the other scan over per-sample tuning words
// (cordic_fm_mix.hip): `grid` blocks, block b sums [b * span, (b + 1) * span)
// of d_fcw cut at n into work[4 + b] (grid <= (n + span - 1) / span), and
// block 0 latches work[0] = phase0 + (d_acc ? *d_acc : 0).
void	launch_fm_reduce(unsigned grid, const uint32_t *d_fcw, size_t n, size_t span,
		uint32_t phase0, const uint32_t *d_acc, uint32_t *work, void *stream);

} // namespace cordic_amd

#ifdef __HIPCC__
// ---- Device side: what table_fm (cordic_table_fm.hip) and the bank's
// table_fmbank (cordic_table_fm_bank.hip) are both made of -- the block sum of
// the prologue and tile_loop, the walk over a span of whole tiles.
//
// Inside a tile everything is counted from the tile's first sample in 32 bits
// (a lane's offset into the tuning words, an output's window [r0, r1), its
// head, vectors and tail): only the tile's own addresses are 64-bit, and they
// are the same in every lane.  With 64-bit sample indices throughout, as the
// loop stood inside table_fm before it became this function, the function
// cost the single call 6 % on an MI355X (the same bits from code objects with
// six more scalar registers spilled into a vector register's lanes); as it
// stands the instances are shorter and spill fewer than before the lift
// (profiles/r19/fm_osc_bank.txt; the register table is in the head of
// cordic_table_fm_bank.hip).
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

// The samples [lo, hi) of one waveform, tile by tile, by a block of 1024
// threads: lane sums, wave scan, the 16 waves' exchange through wsum, the carry
// from tile to tile, the tile's phases to LDS, each output stored on its own
// 16-byte grid with scalar heads and tails (see the head of
// cordic_table_fm.hip), and the next tile's loads in flight meanwhile.
//   carry  in: the phase of sample lo without its pm; out: that of sample hi
//   tab    what core.stage() returned
//   ph     8 + 4096 words of LDS.  ph[8 + j]: the phase of sample t0 + j of the
//          current tile; ph[0 .. 8): the last 8 phases of the tile before it
//   wsum   16 words of LDS
//   a      a.fcw, a.pm (NULL: none): the tuning and phase words, indexed as
//          the outputs are; a.quarter: the cosine's lead
// a.pm == NULL and d_cos == NULL are uniform branches.  Nothing at or behind hi
// is read, nothing outside [lo, hi) of an output is written.  The first thing
// that touches LDS after the call must stand behind a barrier if it writes ph;
// wsum is free (every reader is past the last tile's second barrier).
template <typename CORE, typename T, typename ARGS>
__device__ __forceinline__ void tile_loop(const CORE &core,
		const typename CORE::entry *tab, uint32_t *ph, uint32_t *wsum,
		const ARGS &a, T *d_sin, T *d_cos, size_t lo, size_t hi,
		uint32_t &carry)
{
	typedef typename OutVec<T>::type V;
	constexpr int W = 16 / sizeof(T);
	const unsigned tid = threadIdx.x, lane = tid & 63u;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);

	// this lane's 4 words of the tile at t; nothing at or behind hi is read.
	// What a lane adds to the tile's own address fits 32 bits.
	auto load_tile = [&](size_t t, uint32_t (&f)[4], uint32_t (&m)[4]) {
		const size_t left = (t < hi) ? hi - t : 0;
		const unsigned rem = (left < (size_t)kTile) ? (unsigned)left : (unsigned)kTile;
		const uint32_t *ft = a.fcw + t, *mt = a.pm ? a.pm + t : nullptr;
		const unsigned i = 4u * tid;
		if (i + 4u <= rem) {
			const Words4 q = *reinterpret_cast<const Words4 *>(ft + i);
#pragma unroll
			for (int k = 0; k < 4; k++)
				f[k] = q.v[k];
			if (mt) {
				const Words4 r = *reinterpret_cast<const Words4 *>(mt + i);
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
			for (unsigned k = 0; k < 4; k++) {
				const bool in = i + k < rem;
				f[k] = in ? ft[i + k] : 0u;
				m[k] = (in && mt) ? mt[i + k] : 0u;
			}
		}
	};

	// one stream's window of the tile [t0, t1): see the head of
	// cordic_table_fm.hip.  Everything is counted from the tile's first sample,
	// o = out + t0, in 32 bits: r0 in [-7, 0], r1 in [0, 4096].
	auto emit = [&](T *out, uint32_t lead, size_t t0, size_t t1) {
		T *o = out + t0;
		const int len = (int)(t1 - t0);
		const int r0 = (t0 == lo) ? 0
			: -(int)((reinterpret_cast<uintptr_t>(o) & 15u) / sizeof(T));
		const int r1 = (t1 == hi) ? len
			: len - (int)((reinterpret_cast<uintptr_t>(o + len) & 15u) / sizeof(T));
		int h = (int)head_elems(reinterpret_cast<uintptr_t>(o + r0), sizeof(T));
		if (h > r1 - r0)
			h = r1 - r0;
		// At most 4096 / W vectors, so one per thread covers them.  Behind a
		// span's first tile out + t0 and out + t1 = out + t0 + 4096 sit alike
		// on the 16-byte grid: the window is moved back, not widened, and is
		// 4096 samples (shorter in the last tile).  The first tile has nothing
		// in front of t0: at most 4096 samples again, less its head.
		const int nv = (r1 - r0 - h) / W;
		const int tail = r0 + h + nv * W;
		if ((int)tid < nv) {
			const int e = r0 + h + (int)tid * W;
			const uint32_t *pp = ph + (8 + e);
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
			V ov;
#pragma unroll
			for (int v = 0; v < W; v++)
				ov[v] = (T)core.sample(tab, q[v] + lead);
			__builtin_nontemporal_store(ov, reinterpret_cast<V *>(o + e));
		}
		// fewer than W samples each, and only in a span's first / last tile
		if ((int)tid < h)
			o[r0 + (int)tid] = (T)core.sample(tab, ph[8 + r0 + (int)tid] + lead);
		if ((int)tid < r1 - tail)
			o[tail + (int)tid] = (T)core.sample(tab, ph[8 + tail + (int)tid] + lead);
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
}

} // namespace tfm
} // namespace cordic_amd
#endif // __HIPCC__
#endif
