// cordic_table_nco.h -- oscillator (phase-accumulator) forms of the table and
// quadratic sine cores: the phase of sample i is phase0 + (index0 + i) * fcw,
// made in the kernel, so the launch reads no sample array and only stores.
// Launchers for cordic_abi_table.cpp, and (device side) the cores' sample
// functions and table layouts, shared with the oscillator banks
// (cordic_table_bank.hip).
//
// The sample functions RESTATE table_sample, the LDS sample of
// table_lookup_lds, quad_sample and QuadParams of cordic_kernels.hip: that file
// is part of the code state the DESIGN section 4.4 sweep was measured on
// (tools/build_stamp.py hashes it), so nothing can be moved out of it.
// tests/test_table_nco.py pins the two copies to each other on the device, bit
// for bit, on every layout.  None of these units holds a kernel of that sweep.
#ifndef CORDIC_TABLE_NCO_H
#define CORDIC_TABLE_NCO_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"

namespace cordic_amd {

// One launch: out_sin[i] = core(p_i), out_cos[i] = core(p_i + 2^(PW-2)) with
// p_i = phase0 + (index0 + i) * fcw (mod 2^32, the core takes the low PW bits).
// d_cos == NULL: sine only.  io16: the arrays are int16_t (the caller has
// checked OW <= 16), any 2-byte-aligned address; else int32_t, 4-byte aligned.
// The layout is chosen from (d_lds16, lds_mode, lds_entries) exactly as
// launch_table_lookup chooses it.  queue: a tile-queue block, or NULL for the
// static chunk-per-block sweep.
int	launch_table_nco(const cordic_table_config &t, const int32_t *d_tbl,
		const int16_t *d_lds16, int lds_mode, int lds_entries, size_t n,
		uint32_t phase0, uint32_t fcw, uint64_t index0, void *d_sin,
		void *d_cos, bool io16, void *stream, uint32_t *queue);
int	launch_quad_nco(const cordic_quad_config &q, const int32_t *d_tables,
		size_t n, uint32_t phase0, uint32_t fcw, uint64_t index0,
		void *d_sin, void *d_cos, bool io16, void *stream, uint32_t *queue);

} // namespace cordic_amd

#ifdef __HIPCC__
#include "cordic_device.h"

namespace cordic_amd {
namespace tnco {

using dev::i32x4;

// rtl/sintable.v:72-77 / rtl/quarterwav.v:86-108: one gather per sample from
// a table that lives in L2 / Infinity Cache (at most 2^25 entries).
template <bool QUARTER>
__device__ __forceinline__ int32_t table_sample(const int32_t *__restrict__ tbl,
		uint32_t ph, int pw, int ow)
{
	const int sh = 32 - ow;
	if constexpr (!QUARTER) {
		return tbl[ph & ((1u << pw) - 1u)];
	} else {
		const uint32_t qm = (1u << (pw - 2)) - 1u;
		const uint32_t idx = ((ph >> (pw - 2)) & 1u) ? (~ph & qm) : (ph & qm);
		int32_t v = tbl[idx];
		if ((ph >> (pw - 1)) & 1u)
			v = -v;
		return (int32_t)((uint32_t)v << sh) >> sh;	// OW-bit wrap
	}
}

// The same from a copy in LDS (cordic_kernels.hip: table_lookup_lds):
//   MODE 1: -t qtr table as is           (entries = 2^(PW-2))
//   MODE 2: -t tbl folded to a quadrant  (entries = 2^(PW-2) + 1)
//   E = int16_t: packed copy (OW <= 16); int32_t: the table's own entries.
template <int MODE, typename E>
__device__ __forceinline__ int32_t table_sample_lds(const E *lds, uint32_t ph,
		int pw, int ow)
{
	const uint32_t qm = (1u << (pw - 2)) - 1u;
	const int sh = 32 - ow;
	const uint32_t mirror = (ph >> (pw - 2)) & 1u;
	const uint32_t neg = (ph >> (pw - 1)) & 1u;
	int32_t v;
	if constexpr (MODE == 1) {	// rtl/quarterwav.v:86-108
		v = lds[mirror ? (~ph & qm) : (ph & qm)];
		if (neg) v = -v;
		return (int32_t)((uint32_t)v << sh) >> sh;
	} else {			// quadrant fold of rtl/sintable.v:72-77
		const uint32_t j = ph & qm;
		v = lds[mirror ? (qm + 1u - j) : j];
		return neg ? -v : v;
	}
}

// rtl/quadtbl.v on one sample.  Table entries are {C, L, Q, 0} (one 16-byte
// gather).  Every intermediate keeps the width of its RTL register:
//   qprod  QBITS+DXBITS   lsum  LBITS   lprod  LBITS+DXBITS   r_value  CBITS.
struct QuadParams {
	int32_t	pw, ow, xtra, ww, lgtbl, dxbits, cbits, lbits;
};

__device__ __forceinline__ int64_t sext64n(int64_t v, int bits)
{
	const int s = 64 - bits;
	return (int64_t)((uint64_t)v << s) >> s;
}

__device__ __forceinline__ int32_t quad_sample(const i32x4 e, uint32_t ph,
		const QuadParams &qp)
{
	const int sh = qp.dxbits - 1;
	const int32_t dx = (int32_t)(ph & ((1u << sh) - 1u));	// :153 {1'b0, ...}
	const int64_t qprod = (int64_t)e[2] * dx;		// :170
	// :214-221  w_qprod = sign-extended qprod[top : DXBITS-1]; lsum wraps
	const int32_t lsum = (int32_t)sext64n((qprod >> sh) + e[1], qp.lbits);
	const int64_t lprod = (int64_t)lsum * dx;		// :246
	// :270-277  r_value = w_lprod + cv_3 in CBITS bits
	const int64_t r = sext64n((lprod >> sh) + e[0], qp.cbits);
	// :292-300  round to OW bits unless that would overflow
	const uint32_t rw = (uint32_t)r & (uint32_t)((1ull << qp.ww) - 1ull);
	const uint32_t body = (rw >> qp.xtra) & ((1u << (qp.ow - 1)) - 1u);
	const uint32_t top = rw >> (qp.ww - 1);
	uint32_t w = rw;
	const bool pos_max = (top == 0) && body == ((1u << (qp.ow - 1)) - 1u);
	const bool neg_half = (top == 1) && body == (1u << (qp.ow - 2));
	if (!pos_max && !neg_half) {
		const uint32_t b = (rw >> qp.xtra) & 1u;
		w = rw + (1u << (qp.xtra - 1)) - 1u + b;
	}
	const int s = 32 - qp.ow;
	return (int32_t)((w >> qp.xtra) << s) >> s;		// :308
}

typedef int16_t i16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct OutVec;
template <> struct OutVec<int32_t> { typedef i32x4 type; };
template <> struct OutVec<int16_t> { typedef i16x8 type; };

// ---- the layouts: stage() fills the block's LDS copy (if any; blocks of 1024
// threads) and returns what sample() gathers from
template <bool QUARTER> struct CoreL2 {
	typedef int32_t entry;
	const int32_t *tbl;
	int pw, ow;
	__device__ __forceinline__ const entry *stage(unsigned char *) const { return tbl; }
	__device__ __forceinline__ int32_t sample(const entry *t, uint32_t ph) const
	{
		return table_sample<QUARTER>(t, ph, pw, ow);
	}
};

template <int MODE, typename E> struct CoreLds {
	typedef E entry;
	const E *packed;
	int entries, pw, ow;
	__device__ __forceinline__ const entry *stage(unsigned char *raw) const
	{
		E *lds = reinterpret_cast<E *>(raw);
		for (int i = threadIdx.x; i < entries; i += 1024)
			lds[i] = packed[i];
		__syncthreads();
		return lds;
	}
	__device__ __forceinline__ int32_t sample(const entry *lds, uint32_t ph) const
	{
		return table_sample_lds<MODE, E>(lds, ph, pw, ow);
	}
};

struct CoreQuad {
	typedef i32x4 entry;
	const i32x4 *tab;
	QuadParams qp;
	__device__ __forceinline__ const entry *stage(unsigned char *raw) const
	{
		i32x4 *lds = reinterpret_cast<i32x4 *>(raw);
		for (int i = threadIdx.x; i < (1 << qp.lgtbl); i += 1024)
			lds[i] = tab[i];
		__syncthreads();
		return lds;
	}
	__device__ __forceinline__ int32_t sample(const entry *lds, uint32_t ph) const
	{
		const uint32_t imask = (1u << qp.lgtbl) - 1u;
		return quad_sample(lds[(ph >> (qp.dxbits - 1)) & imask], ph, qp);
	}
};

} // namespace tnco
} // namespace cordic_amd
#endif // __HIPCC__
#endif
