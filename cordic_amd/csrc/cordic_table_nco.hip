// cordic_table_nco.hip -- the table and quadratic sine cores as oscillators
// (cordic_table_nco / cordic_quad_nco and their int16 forms): a store-only
// stream of 2 .. 8 bytes per sample over an LDS or L2 gather.
//
// One kernel family for every layout the lookups serve (L2 gather full-wave /
// quarter-wave, packed int16 or 32-bit entries in LDS in both folds, the
// quadratic core's {C, L, Q, 0} entries in LDS), x sine-only / quadrature,
// x int32 / int16 outputs.  A lane makes the phases of one 16-byte vector of
// outputs (4 int32 or 8 int16) from the global sample index, gathers once per
// output and stores the vector non-temporally; the quadrature form does both
// gathers from the one staged table and writes two streams.
//
// Alignment: each output stream is cut into [head | 16-byte aligned vectors |
// tail] on its OWN address (d_sin and d_cos may sit differently), so every
// vector store is aligned whatever 4- or 2-byte-aligned address the caller
// passed; block 0 writes the heads and tails with scalar stores.  Nothing
// outside [0, n) of either array is touched.
#include <hip/hip_runtime.h>

#include "cordic_table_nco.h"
#include "cordic_jobs_fused.h"

namespace cordic_amd {

namespace tnco {

using dev::for_each_queued_tile;

struct NcoArgs {
	uint32_t base;		// phase0 + (uint32_t)index0 * fcw
	uint32_t fcw;
	uint32_t quarter;	// 2^(PW-2): the cosine's lead
};

// elements in front of the first 16-byte boundary of `p` (at most n)
template <typename T>
__device__ __forceinline__ size_t head_of(const T *p, size_t n)
{
	const size_t h = ((16u - (size_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u)
		/ sizeof(T);
	return h < n ? h : n;
}

// Persistent 1024-thread blocks (they keep their table in LDS) that pull
// 1024-vector tiles from the per-XCD counters in `queue` in address order --
// the work distribution of the lookups (cordic_kernels.hip: sweep_tiles),
// without the prefetch: there is no input.  queue == NULL: one contiguous
// chunk per block.
template <typename CORE, bool COS, typename T>
__global__ __launch_bounds__(1024) void table_nco(CORE core, NcoArgs na,
		T *__restrict__ d_sin, T *__restrict__ d_cos, size_t n, uint32_t *queue)
{
	typedef typename OutVec<T>::type V;
	constexpr int W = 16 / sizeof(T);
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ uint32_t slot[3];
	const typename CORE::entry *tab = core.stage(lds_raw);

	auto one = [&](size_t i, uint32_t lead) -> T {
		return (T)core.sample(tab, na.base + lead + (uint32_t)i * na.fcw);
	};
	const size_t hs = head_of(d_sin, n);
	const size_t hc = COS ? head_of(d_cos, n) : 0;
	const size_t nvs = (n - hs) / W;
	const size_t nvc = COS ? (n - hc) / W : 0;
	const size_t nvec = nvs > nvc ? nvs : nvc;
	V *vs = reinterpret_cast<V *>(d_sin + hs);
	V *vc = COS ? reinterpret_cast<V *>(d_cos + hc) : nullptr;

	auto one_vector = [&](size_t g) {
		if (g < nvs) {
			uint32_t p = na.base + (uint32_t)(hs + g * W) * na.fcw;
			V o;
#pragma unroll
			for (int v = 0; v < W; v++, p += na.fcw)
				o[v] = (T)core.sample(tab, p);
			__builtin_nontemporal_store(o, &vs[g]);
		}
		if (COS && g < nvc) {
			uint32_t p = na.base + na.quarter + (uint32_t)(hc + g * W) * na.fcw;
			V o;
#pragma unroll
			for (int v = 0; v < W; v++, p += na.fcw)
				o[v] = (T)core.sample(tab, p);
			__builtin_nontemporal_store(o, &vc[g]);
		}
	};
	if (queue) {
		for_each_queued_tile<1024>(queue, slot,
			(uint32_t)((nvec + 1023) / 1024), [&](uint32_t tile) {
				const size_t g = (size_t)tile * 1024 + threadIdx.x;
				if (g < nvec)
					one_vector(g);
			});
	} else {
		size_t chunk = (nvec + gridDim.x - 1) / gridDim.x;
		chunk = (chunk + 1023) / 1024 * 1024;
		const size_t lo = (size_t)blockIdx.x * chunk;
		const size_t hi = (lo + chunk < nvec) ? lo + chunk : nvec;
		for (size_t g = lo + threadIdx.x; g < hi; g += 1024)
			one_vector(g);
	}
	if (blockIdx.x == 0) {
		// heads and tails: fewer than W elements each
		for (size_t i = threadIdx.x; i < hs; i += 1024)
			d_sin[i] = one(i, 0u);
		for (size_t i = hs + nvs * W + threadIdx.x; i < n; i += 1024)
			d_sin[i] = one(i, 0u);
		if (COS) {
			for (size_t i = threadIdx.x; i < hc; i += 1024)
				d_cos[i] = one(i, na.quarter);
			for (size_t i = hc + nvc * W + threadIdx.x; i < n; i += 1024)
				d_cos[i] = one(i, na.quarter);
		}
	}
}

// blocks of 1024 threads: one per 1024 vectors, at most per_cu per CU
static int grid_of(size_t n, int samples_per_lane, int per_cu)
{
	const int cus = jobs_cus_now();
	if (cus < 0)
		return -1;
	const size_t per_block = (size_t)1024 * samples_per_lane;
	const size_t blocks = (n + per_block - 1) / per_block;
	const size_t cap = (size_t)cus * per_cu;
	return (int)(blocks < cap ? (blocks ? blocks : 1) : cap);
}

static bool overlap(const void *a, const void *b, size_t bytes)
{
	const uintptr_t x = reinterpret_cast<uintptr_t>(a);
	const uintptr_t y = reinterpret_cast<uintptr_t>(b);
	return x < y + bytes && y < x + bytes;
}

static int check_outputs(const void *d_sin, const void *d_cos, size_t n, bool io16)
{
	const uintptr_t mask = io16 ? 1u : 3u;
	if (!d_sin || (reinterpret_cast<uintptr_t>(d_sin) & mask)
			|| (reinterpret_cast<uintptr_t>(d_cos) & mask))
		return CORDIC_ERR_ARGS;
	if (d_cos && overlap(d_sin, d_cos, n * (io16 ? 2 : 4)))
		return CORDIC_ERR_ARGS;
	return CORDIC_OK;
}

template <typename CORE, bool COS, typename T>
bool launch_one(const CORE &core, const NcoArgs &na, void *d_sin, void *d_cos,
		size_t n, size_t lds_bytes, int per_cu, hipStream_t st, uint32_t *queue)
{
	const void *kern = (const void *)table_nco<CORE, COS, T>;
	// (+ the kernel's static tile-id slots)
	if (lds_bytes + 64 > 64 * 1024 && hipFuncSetAttribute(kern,
			hipFuncAttributeMaxDynamicSharedMemorySize,
			(int)lds_bytes + 64) != hipSuccess)
		return false;
	const int grid = grid_of(n, 16 / (int)sizeof(T), per_cu);
	if (grid < 0)
		return false;
	hipLaunchKernelGGL((table_nco<CORE, COS, T>), dim3(grid), dim3(1024),
		lds_bytes, st, core, na, static_cast<T *>(d_sin),
		static_cast<T *>(d_cos), n, queue);
	return true;
}

// ALLOW16: instances with int16 outputs exist only for layouts that serve
// cores of OW <= 16
template <typename CORE, bool ALLOW16>
bool launch_core(const CORE &core, const NcoArgs &na, void *d_sin, void *d_cos,
		size_t n, bool io16, size_t lds_bytes, int per_cu, hipStream_t st,
		uint32_t *queue)
{
	if constexpr (ALLOW16) {
		if (io16)
			return d_cos
				? launch_one<CORE, true, int16_t>(core, na, d_sin, d_cos, n,
					lds_bytes, per_cu, st, queue)
				: launch_one<CORE, false, int16_t>(core, na, d_sin, d_cos, n,
					lds_bytes, per_cu, st, queue);
	}
	if (io16)
		return false;
	return d_cos
		? launch_one<CORE, true, int32_t>(core, na, d_sin, d_cos, n, lds_bytes,
			per_cu, st, queue)
		: launch_one<CORE, false, int32_t>(core, na, d_sin, d_cos, n, lds_bytes,
			per_cu, st, queue);
}

static int finish(bool launched)
{
	if (!launched) {
		(void)hipGetLastError();
		return CORDIC_ERR_DEVICE;
	}
	return hipGetLastError() == hipSuccess ? CORDIC_OK : CORDIC_ERR_DEVICE;
}

} // namespace tnco

int launch_table_nco(const cordic_table_config &t, const int32_t *d_tbl,
		const int16_t *d_lds16, int lds_mode, int lds_entries, size_t n,
		uint32_t phase0, uint32_t fcw, uint64_t index0, void *d_sin,
		void *d_cos, bool io16, void *stream, uint32_t *queue)
{
	using namespace tnco;
	(void)hipGetLastError();	// (a stale error is not this launch's)
	if (io16 && t.ow > 16) return CORDIC_ERR_CONTAINER;
	if (n == 0) return CORDIC_OK;
	if (!d_tbl || !table_sane(t)) return CORDIC_ERR_ARGS;
	if (int rc = check_outputs(d_sin, d_cos, n, io16)) return rc;
	hipStream_t st = static_cast<hipStream_t>(stream);
	// (PW <= 32: the low 32 bits of the sample index are all that matters)
	const NcoArgs na{phase0 + (uint32_t)index0 * fcw, fcw, 1u << (t.pw - 2)};
	if (lds_mode >= 3 || (d_lds16 && lds_mode)) {
		// as launch_table_lookup: the LDS copy, two blocks per CU where two fit
		const bool wide = lds_mode >= 3;
		const size_t bytes = ((size_t)lds_entries * (wide ? 4 : 2) + 15) & ~(size_t)15;
		int per_cu = (int)((160 * 1024) / (bytes + 64));
		if (per_cu > 2) per_cu = 2;
		bool done = false;
		if (per_cu >= 1 && !(wide && io16)) {
			switch (lds_mode) {
			case 1:
				done = launch_core<CoreLds<1, int16_t>, true>(
					{d_lds16, lds_entries, t.pw, t.ow}, na, d_sin, d_cos, n,
					io16, bytes, per_cu, st, queue);
				break;
			case 2:
				done = launch_core<CoreLds<2, int16_t>, true>(
					{d_lds16, lds_entries, t.pw, t.ow}, na, d_sin, d_cos, n,
					io16, bytes, per_cu, st, queue);
				break;
			case 3:
				done = launch_core<CoreLds<1, int32_t>, false>(
					{d_tbl, lds_entries, t.pw, t.ow}, na, d_sin, d_cos, n,
					io16, bytes, per_cu, st, queue);
				break;
			default:
				done = launch_core<CoreLds<2, int32_t>, false>(
					{d_tbl, lds_entries, t.pw, t.ow}, na, d_sin, d_cos, n,
					io16, bytes, per_cu, st, queue);
				break;
			}
		}
		if (done)
			return finish(true);
		(void)hipGetLastError();	// the L2 gather kernel below serves the table
	}
	const bool done = t.kind == CORDIC_QTR
		? launch_core<CoreL2<true>, true>({d_tbl, t.pw, t.ow}, na, d_sin, d_cos,
			n, io16, 0, 2, st, queue)
		: launch_core<CoreL2<false>, true>({d_tbl, t.pw, t.ow}, na, d_sin, d_cos,
			n, io16, 0, 2, st, queue);
	return finish(done);
}

int launch_quad_nco(const cordic_quad_config &q, const int32_t *d_tables,
		size_t n, uint32_t phase0, uint32_t fcw, uint64_t index0,
		void *d_sin, void *d_cos, bool io16, void *stream, uint32_t *queue)
{
	using namespace tnco;
	(void)hipGetLastError();
	if (io16 && q.ow > 16) return CORDIC_ERR_CONTAINER;
	if (n == 0) return CORDIC_OK;
	if (!d_tables || !quad_sane(q)) return CORDIC_ERR_ARGS;
	if (int rc = check_outputs(d_sin, d_cos, n, io16)) return rc;
	const size_t bytes = (size_t)q.entries * sizeof(i32x4);
	if (bytes > 64 * 1024)
		return CORDIC_ERR_UNSUPPORTED;
	const NcoArgs na{phase0 + (uint32_t)index0 * fcw, fcw, 1u << (q.pw - 2)};
	const CoreQuad core{reinterpret_cast<const i32x4 *>(d_tables),
		{q.pw, q.ow, q.xtra, q.ww, q.lgtbl, q.dxbits, q.cbits, q.lbits}};
	return finish(launch_core<CoreQuad, true>(core, na, d_sin, d_cos, n, io16,
		bytes, 2, static_cast<hipStream_t>(stream), queue));
}

} // namespace cordic_amd
