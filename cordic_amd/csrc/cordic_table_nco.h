// cordic_table_nco.h -- the table and quadratic sine cores as oscillators.
//
// Host side: SineCore, what a cordic_table or cordic_quad handle knows about
// its device tables, and the launcher of the plain oscillator (the phase of
// sample i is phase0 + (index0 + i) * fcw, made in the kernel, so the launch
// reads no sample array and only stores).  The oscillator banks
// (cordic_table_bank.h) and the modulated oscillators (cordic_table_fm.h) take
// the same descriptor.
//
// Device side: the cores' sample functions and table layouts, and with_layout(),
// the ONE place that decides which layout serves a core.  All three oscillator
// units launch through it.
//
// The sample functions RESTATE table_sample, the LDS sample of
// table_lookup_lds, quad_sample and QuadParams of cordic_kernels.hip: that file
// is part of the code state the DESIGN section 4.4 sweep was measured on
// (tools/build_stamp.py hashes it), so nothing can be moved out of it, and its
// launch_table_lookup keeps a layout ladder of its own.
// tests/test_table_nco.py pins the two copies to each other on the device, bit
// for bit, on every layout.  None of these units holds a kernel of that sweep.
#ifndef CORDIC_TABLE_NCO_H
#define CORDIC_TABLE_NCO_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_internal.h"

namespace cordic_amd {

// elements of `esize` bytes in front of the first 16-byte boundary at or
// behind `addr`
constexpr size_t head_elems(uintptr_t addr, size_t esize)
{
	return ((16u - (size_t)(addr & 15u)) & 15u) / esize;
}

// blocks of one CU that hold `bytes` (> 0) of its 160 KiB of LDS each at the
// same time, two at the most; 0: not even one fits
constexpr int lds_blocks_per_cu(size_t bytes)
{
	const size_t fit = (160 * 1024) / bytes;
	return fit > 2 ? 2 : (int)fit;
}

// A sine core's device tables, as its handle knows them (cordic_table::core,
// cordic_quad::core).  The pointers are held by value and stay the handle's:
// whatever keeps a SineCore (a bank) must not outlive the handle.
struct SineCore {
	bool	quad = false;
	cordic_table_config t{};	// !quad
	cordic_quad_config q{};		// quad
	// the table's 32-bit entries; quad: entries x {C, L, Q, 0}
	const int32_t *d_tbl = nullptr;
	// table cores only, as launch_table_lookup takes them: the packed copy for
	// LDS (modes 1 / 2) or none (modes 3 / 4 fill LDS from d_tbl; 0: no LDS)
	const int16_t *d_lds16 = nullptr;
	int	lds_mode = 0, lds_entries = 0;

	int	pw() const { return quad ? q.pw : t.pw; }
	int	ow() const { return quad ? q.ow : t.ow; }
	uint32_t quarter() const { return 1u << (pw() - 2); }	// the cosine's lead
	// the table is there and its config is one the kernels can index by
	bool	sane() const { return d_tbl && (quad ? quad_sane(q) : table_sane(t)); }
	// a block keeps a copy of the table in LDS (else: gathered from L2)
	bool	in_lds() const { return quad || lds_mode >= 3 || (d_lds16 && lds_mode); }
	// bytes of that copy, a multiple of 16
	size_t	lds_bytes() const
	{
		if (quad)
			return (size_t)q.entries * 16;
		if (!in_lds())
			return 0;
		return ((size_t)lds_entries * (lds_mode >= 3 ? 4 : 2) + 15) & ~(size_t)15;
	}
};

// One launch: out_sin[i] = core(p_i), out_cos[i] = core(p_i + 2^(PW-2)) with
// p_i = phase0 + (index0 + i) * fcw (mod 2^32, the core takes the low PW bits).
// d_cos == NULL: sine only.  io16: the arrays are int16_t (OW <= 16:
// CORDIC_ERR_CONTAINER otherwise), any 2-byte-aligned address; else int32_t,
// 4-byte aligned.  queue: a tile-queue block, or NULL for the static
// chunk-per-block sweep.
int	launch_sine_nco(const SineCore &c, size_t n, uint32_t phase0, uint32_t fcw,
		uint64_t index0, void *d_sin, void *d_cos, bool io16, void *stream,
		uint32_t *queue);

} // namespace cordic_amd

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <type_traits>

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

// ---- the layout choice (host code of the kernel units)

// the status of a launch: false = nothing usable was launched
inline int finish(bool launched)
{
	if (!launched) {
		(void)hipGetLastError();
		return CORDIC_ERR_DEVICE;
	}
	return hipGetLastError() == hipSuccess ? CORDIC_OK : CORDIC_ERR_DEVICE;
}

// A launch of `kern` with `total_bytes` of LDS (dynamic + the kernel's static)
// has to ask for them above 64 KiB.
inline bool allow_lds(const void *kern, size_t total_bytes)
{
	return total_bytes <= 64 * 1024 || hipFuncSetAttribute(kern,
		hipFuncAttributeMaxDynamicSharedMemorySize, (int)total_bytes) == hipSuccess;
}

// Launch on the layout that serves `c`, chosen as launch_table_lookup chooses
// it: the copy in LDS where the handle has one, else (or where `launch` can
// make nothing of it) the gather from L2; the quadratic core's table always
// sits in LDS (CORDIC_ERR_UNSUPPORTED over 64 KiB).
//   launch(const CORE &core, T tag, size_t table_bytes) -> bool
// gets the layout, the store type as a value (int32_t, or int16_t for io16)
// and the bytes of LDS the layout stages into, and returns false when nothing
// usable was launched.  Only the pairs (CORE, T) that exist are handed to it:
// the layouts with 32-bit entries in LDS serve cores of OW > 16 and have no
// int16 instance.  The caller has checked c.sane().
template <typename F>
int with_layout(const SineCore &c, bool io16, F &&launch)
{
	auto typed = [&](const auto &core, auto allow16, size_t bytes) -> bool {
		if constexpr (decltype(allow16)::value) {
			if (io16)
				return launch(core, int16_t{}, bytes);
		}
		if (io16)
			return false;
		return launch(core, int32_t{}, bytes);
	};
	const std::true_type any{};
	const std::false_type wide_only{};
	const size_t bytes = c.lds_bytes();
	if (!c.quad) {
		const cordic_table_config &t = c.t;
		if (c.in_lds()) {
			bool done = false;
			if (!(c.lds_mode >= 3 && io16)) {
				switch (c.lds_mode) {
				case 1:
					done = typed(CoreLds<1, int16_t>{c.d_lds16, c.lds_entries,
						t.pw, t.ow}, any, bytes);
					break;
				case 2:
					done = typed(CoreLds<2, int16_t>{c.d_lds16, c.lds_entries,
						t.pw, t.ow}, any, bytes);
					break;
				case 3:
					done = typed(CoreLds<1, int32_t>{c.d_tbl, c.lds_entries,
						t.pw, t.ow}, wide_only, bytes);
					break;
				default:
					done = typed(CoreLds<2, int32_t>{c.d_tbl, c.lds_entries,
						t.pw, t.ow}, wide_only, bytes);
					break;
				}
			}
			if (done)
				return finish(true);
			(void)hipGetLastError();	// the L2 gather below serves the table
		}
		return finish(t.kind == CORDIC_QTR
			? typed(CoreL2<true>{c.d_tbl, t.pw, t.ow}, any, 0)
			: typed(CoreL2<false>{c.d_tbl, t.pw, t.ow}, any, 0));
	}
	if (bytes > 64 * 1024)
		return CORDIC_ERR_UNSUPPORTED;
	const cordic_quad_config &q = c.q;
	const CoreQuad core{reinterpret_cast<const i32x4 *>(c.d_tbl),
		{q.pw, q.ow, q.xtra, q.ww, q.lgtbl, q.dxbits, q.cbits, q.lbits}};
	return finish(typed(core, any, bytes));
}

} // namespace tnco
} // namespace cordic_amd
#endif // __HIPCC__
#endif
