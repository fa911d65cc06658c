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
	const size_t h = head_elems(reinterpret_cast<uintptr_t>(p), sizeof(T));
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
		size_t n, size_t lds_bytes, hipStream_t st, uint32_t *queue)
{
	// (+ the kernel's static tile-id slots)
	const int per_cu = lds_blocks_per_cu(lds_bytes + 64);
	if (per_cu < 1 || !allow_lds((const void *)table_nco<CORE, COS, T>, lds_bytes + 64))
		return false;
	const int grid = grid_of(n, 16 / (int)sizeof(T), per_cu);
	if (grid < 0)
		return false;
	hipLaunchKernelGGL((table_nco<CORE, COS, T>), dim3(grid), dim3(1024),
		lds_bytes, st, core, na, static_cast<T *>(d_sin),
		static_cast<T *>(d_cos), n, queue);
	return true;
}

} // namespace tnco

int launch_sine_nco(const SineCore &c, size_t n, uint32_t phase0, uint32_t fcw,
		uint64_t index0, void *d_sin, void *d_cos, bool io16, void *stream,
		uint32_t *queue)
{
	using namespace tnco;
	(void)hipGetLastError();	// (a stale error is not this launch's)
	if (io16 && c.ow() > 16) return CORDIC_ERR_CONTAINER;
	if (n == 0) return CORDIC_OK;
	if (!c.sane()) return CORDIC_ERR_ARGS;
	if (int rc = check_outputs(d_sin, d_cos, n, io16)) return rc;
	hipStream_t st = static_cast<hipStream_t>(stream);
	// (PW <= 32: the low 32 bits of the sample index are all that matters)
	const NcoArgs na{phase0 + (uint32_t)index0 * fcw, fcw, c.quarter()};
	return with_layout(c, io16, [&](const auto &core, auto tag, size_t bytes) {
		typedef std::decay_t<decltype(core)> CORE;
		typedef decltype(tag) T;
		return d_cos
			? launch_one<CORE, true, T>(core, na, d_sin, d_cos, n, bytes, st, queue)
			: launch_one<CORE, false, T>(core, na, d_sin, d_cos, n, bytes, st, queue);
	});
}

} // namespace cordic_amd
