// cordic_span_reduce.h -- launch 1 of the prefix-sum banks (FM mixer banks,
// cordic_fm_mix_bank.hip; FM oscillator banks, cordic_table_fm_bank.hip), and
// the grids of both launches.  The scheme and the descriptor's common head:
// cordic_span_bank.h.
//
// span_reduce<SPAN, THREADS>: block b sums the tuning words of spans b, b +
// grid, ... of the table, one workspace word per span, part[d.part0 + d.idx];
// a job's first span latches start[d.start] = phase0 + *d_acc.  THREADS is the
// bank's: 16-byte loads at any 4-byte alignment, so that a unit of the bank (a
// pass of 1024 samples at 256 threads, a tile of 4096 at 1024) is one load per
// lane.  The THREADS / 64 words of wsum are double-buffered by span, as the
// exchange words of a pass loop are by pass: ONE barrier per span -- the words
// written for span i are read behind barrier i and written again for span i +
// 2, which a wave reaches only through barrier i + 1.
// Every *d_acc is read here only and written in launch 2 only, which follows in
// stream order; the workspace is written here only.  No block waits for
// another.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_SPAN_REDUCE_H
#define CORDIC_SPAN_REDUCE_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cordic_hostargs.h"
#include "cordic_span_bank.h"

namespace cordic_amd {

// Four consecutive words at any 4-byte-aligned address: one dwordx4 load.  An
// ext-vector and not the packed struct Words4 (cordic_table_fm.h): through the
// struct the instance of 1024 threads takes 60 registers and 324 instructions,
// through this 42 and 223 (profiles/r20/span_bank_isa.txt).
typedef uint32_t span_words4 __attribute__((ext_vector_type(4), aligned(4)));

// What a job's first span latches besides the start word, into the words
// behind the partial sums (SpanRule::words): nothing, unless the bank's
// descriptor has an overload of its own (RxSpan, cordic_fm_rx_bank.h).
template <typename SPAN>
__device__ __forceinline__ void span_latch_more(const SPAN &, uint32_t *)
{
}

template <typename SPAN, int THREADS>
__global__ __launch_bounds__(THREADS) void span_reduce(
		const SPAN *__restrict__ spans, uint32_t nspans,
		uint32_t *__restrict__ start, uint32_t *__restrict__ part)
{
	static_assert(THREADS % 64 == 0, "whole waves");
	__shared__ uint32_t wsum[2][THREADS / 64];
	const unsigned tid = threadIdx.x;
	unsigned par = 0;
	for (uint32_t t = blockIdx.x; t < nspans; t += gridDim.x) {
		const SPAN d = spans[t];
		const uint32_t *f = reinterpret_cast<const uint32_t *>((uintptr_t)d.fcw);
		const span_words4 *fv = reinterpret_cast<const span_words4 *>(f);
		const uint64_t nv = d.n / 4;
		uint32_t s = 0;
#pragma unroll 4
		for (uint64_t g = tid; g < nv; g += THREADS) {
			const span_words4 q = fv[g];
			s += q[0] + q[1] + q[2] + q[3];
		}
		const uint64_t r = nv * 4 + tid;	// fewer than 4 behind the vectors
		if (r < d.n)
			s += f[r];
#pragma unroll
		for (int k = 32; k; k >>= 1)
			s += __shfl_xor(s, k);
		if ((tid & 63u) == 0)
			wsum[par][tid >> 6] = s;
		__syncthreads();
		if (tid == 0) {
			uint32_t sum = 0;
#pragma unroll
			for (int j = 0; j < THREADS / 64; j++)
				sum += wsum[par][j];
			part[d.part0 + d.idx] = sum;
			if (d.flags & kSpanFirst) {
				const uint32_t *acc
					= reinterpret_cast<const uint32_t *>((uintptr_t)d.acc);
				start[d.start] = d.phase0 + (acc ? *acc : 0u);
				span_latch_more(d, part + nspans);
			}
		}
		par ^= 1;
	}
}

// The grids of a run over nspans >= 1 spans on `cus` CUs.  Launch 1 holds
// `reduce_per_cu` blocks a CU (few registers, THREADS / 64 * 8 bytes of LDS).
// Launch 2 has at most the resident blocks, `walk_per_cu` a CU, capped further
// by the environment variable `max_blocks` (read at every run).  Neither has
// more blocks than spans.
struct SpanGrids {
	unsigned reduce, walk;
};
inline SpanGrids span_grids(uint32_t nspans, int cus, int reduce_per_cu,
		const char *max_blocks, size_t walk_per_cu)
{
	const size_t r = (size_t)cus * reduce_per_cu;
	const size_t w = env_block_cap(max_blocks, (size_t)cus * walk_per_cu);
	return SpanGrids{(unsigned)(r < nspans ? r : nspans),
		(unsigned)(w < nspans ? w : nspans)};
}

} // namespace cordic_amd
#endif
