// cordic_fm_demod.hip -- FM demodulation (cordic_fm_demod, cordic_fm_demod16,
// cordic_fm_demod_info, cordic_fm_demod16_info, cordic_fm_demod_workspace): the
// r2p / sr2p converter with its phase differenced from sample to sample,
//   prev   = (phase0 + *d_last) mod 2^PW
//   freq_i = sext_PW((ph_i - ph_(i-1)) mod 2^PW),   ph_(-1) = prev
//   mag_i  = cordic_r2p's,   *d_last = ph_(n-1),
// ph_i being the word cordic_r2p writes to d_ophase[i].
//
// FUSED (fm_demod_lj, fm_demod_tail): the cores that launch_topolar sends to
// topolar_lj (WW <= 34, no wrap) -- 32-bit arrays when all four sit on 16-byte
// boundaries, 16-bit arrays (cordic_fm_demod16; the Io16 instances, 8-byte
// vectors) at any alignment of theirs.  (The 16-byte condition is the 32-bit
// entry point's own, kept as it was: topolar_lj itself takes any
// 4-byte-aligned array, and fm_demod_lj uses the same vector types; displaced
// 32-bit arrays are simply routed to the fallback here.)
// A lane converts the 4 samples of a vector exactly as topolar_lj_sweep does
// and needs one more phase: the last one of the vector in front.  Blocks
// therefore sweep CONTIGUOUS tiles (b, b + gridDim.x, ...) of 8 * 256 - 1 = 2047
// vectors each, by sweep_tile (cordic_fm_demod.h), the sweep of the banks'
// kernel: the halo, the way the predecessor travels and the ONE barrier per pass
// are written there.  2048 vectors are converted for 2047 of output: 1/2048 of
// the work twice, no divergent pass.
// *d_last is read by the halo lane of tile 0 alone; it is written by the tail
// launch that follows in stream order: one lane (tail_of, cordic_fm_demod.h;
// the banks' tail) converts the last <= 4 samples by the same pol_lj_vector
// instance, differences and stores them and writes *d_last.  A call is two
// launches, or one where there is no whole vector or no tail.
//
// CORDIC_FMD_MAX_BLOCKS=<n> in the environment (read at every call; a test
// and A/B knob like CORDIC_FORCE_DYN) caps the fused kernel's grid at n
// blocks, so that a short call runs many tiles per block.  The bits do not
// depend on it.
//
// cordic_last_kernel() is unspecified after these calls: the fallback goes
// through launch_topolar, which records its own kernel, and the fused path
// records none.
//
// Registers (.vgpr_count / scratch bytes of the gfx950 code objects, -O3,
// --save-temps; profiles/r14/fm_refactor_isa.txt, taken again with the
// container parameter in place, profiles/r18/fm_demod16_isa.txt):
//                        topolar_lj  topolar_lj_jobs  fm_demod_lj  fm_demod_tail
//   20 stages, PLAIN         49            57           56 / 0        32 / 0
//   29 stages, PLAIN         49            57           56 / 0        32 / 0
//   dynamic exit             88            97           94 / 0        67 / 0
//   dynamic exit, unit gain  88            97           94 / 0        67 / 0
//   Io16, dynamic exit                                  90 / 0        67 / 0
//   Io16, dyn., unit gain                               90 / 0        67 / 0
// With 512 registers per lane of a SIMD, allocated in eights: 56 -> 8 waves
// (the most a SIMD holds) for the static instances as for topolar_lj's 49,
// and 96 -> 5 waves for the dynamic ones as for its 88.  The differencing
// crosses no occupancy step; no instance spills.  The Io32 counts are what
// they were before the parameter; the Io16 instances (dynamic exit only: a
// core with 16-bit ports has about 13 live stages) hold the prefetched
// vectors in two registers per array where Io32 holds four, 90 -> 96 -> 5
// waves.  32 bytes of LDS per block of fm_demod_lj, none in the tail kernel.
//
// FALLBACK (everything else: WW 35 .. 40 and wider, cores that wrap, the A/B
// flags, 32-bit arrays off the 16-byte grid; T = uint16_t for such cores of
// the 16-bit form): launch_topolar writes
// the raw phases into d_ofreq; fmd_save keeps the last phase of every
// 4096-sample tile (and prev, and writes *d_last -- the same thread reads it
// first); fmd_diff differences in place, a block per tile: every thread has
// read its 4 phases and the one in front before any is overwritten, and the
// word in front of a tile comes from d_work.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_device.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_table_nco.h"
#include "cordic_hostargs.h"
#include "cordic_fm_demod.h"

namespace cordic_amd {

namespace fmd {

using namespace dev;

// Tile t is the vectors [t * kFmdTileVecs, (t + 1) * kFmdTileVecs) cut at nvec,
// t = 0 the one that begins at sample 0 (sweep_tile, cordic_fm_demod.h; the
// element in front of the arrays is the halo of t = 0, which is never loaded).
// The tile's first index goes there in vector registers (vgpr_const), so that
// the addresses are made per lane, as topolar_lj makes them.  Left to itself
// hipcc folds the index into four more scalar pointers per tile, and the
// dynamic-exit instances, whose 40 stage angles live in scalar registers, then
// move about 90 more of them through VGPR lanes inside the chain: 109 against
// 114 Gsample/s on a WW 33 core (profiles/r14/fm_refactor_rates.txt).
//
// IO: the container of the four arrays (Io32 / Io16); nvec, the tiles and the
// index count vectors of 4 samples in either, so the 16-bit form is the same
// kernel on 8-byte vectors.
template <int NLIVE, bool DYN, bool UG, bool PLAIN, typename IO = Io32>
__global__ __launch_bounds__(kBlock) void fm_demod_lj(CoreParams kp,
		const typename IO::ivec *__restrict__ xin,
		const typename IO::ivec *__restrict__ yin,
		typename IO::ivec *__restrict__ omag,
		typename IO::ivec *__restrict__ ofreq, size_t nvec,
		size_t ntiles, uint32_t phase0, const uint32_t *__restrict__ d_last)
{
	__shared__ uint32_t edge[2][kBlock / 64];
	const LaneConsts ln(kp);
	unsigned par = 0;
	for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const size_t base = t * kFmdTileVecs;
		const size_t left = nvec - base;
		const size_t at = (size_t)vgpr_const((uint32_t)(base >> 32)) << 32
			| vgpr_const((uint32_t)base);
		sweep_tile<NLIVE, DYN, UG, PLAIN>(kp, ln, xin - 1, yin - 1, omag - 1, ofreq - 1,
			at, (uint32_t)(left < kFmdTileVecs ? left : kFmdTileVecs), t == 0,
			phase0, d_last, edge, par, IO{});
	}
}

// The tail of the call, one lane (tail_of, cordic_fm_demod.h), behind the sweep
// in stream order
template <int NLIVE, bool DYN, bool UG, bool PLAIN, typename IO = Io32>
__global__ __launch_bounds__(64) void fm_demod_tail(CoreParams kp, DemodTail d)
{
	if (threadIdx.x == 0)
		tail_of<NLIVE, DYN, UG, PLAIN>(kp, d, IO{});
}

// ---- fallback.  T: uint32_t, or uint16_t for the 16-bit form
template <typename T>
struct __attribute__((packed, aligned(sizeof(T)))) Elems4 {
	T v[4];
};

// work[kFmdWorkHead + j] = ph[(j + 1) * 4096 - 1] for every tile with a tile
// behind it; thread 0: work[0] = prev, then *d_last = ph[n - 1]
template <typename T>
__global__ __launch_bounds__(256) void fmd_save(const T *__restrict__ ph, size_t n,
		uint32_t phase0, uint32_t *d_last, uint32_t *__restrict__ work, int sh)
{
	const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
	const size_t stride = (size_t)gridDim.x * 256;
	for (size_t j = id; (j + 1) * kFmdDiffTile < n; j += stride)
		work[kFmdWorkHead + j] = ph[(j + 1) * kFmdDiffTile - 1];
	if (id == 0) {
		work[0] = (phase0 + (d_last ? *d_last : 0u)) & (0xffffffffu >> sh);
		if (d_last)
			*d_last = ph[n - 1];
	}
}

template <typename T>
__global__ __launch_bounds__(1024) void fmd_diff(T *ph, size_t n,
		const uint32_t *__restrict__ work, int sh)
{
	typedef typename std::make_signed<T>::type S;
	const unsigned tid = threadIdx.x;
	const size_t ntiles = (n + kFmdDiffTile - 1) / kFmdDiffTile;
	for (size_t j = blockIdx.x; j < ntiles; j += gridDim.x) {
		const size_t i = j * kFmdDiffTile + 4 * (size_t)tid;
		uint32_t v[4] = {0, 0, 0, 0}, before = 0;
		if (i + 4 <= n) {
			const Elems4<T> q = *reinterpret_cast<const Elems4<T> *>(ph + i);
#pragma unroll
			for (int k = 0; k < 4; k++)
				v[k] = q.v[k];
		} else {
#pragma unroll
			for (int k = 0; k < 4; k++)
				if (i + k < n)
					v[k] = ph[i + k];
		}
		if (i < n)
			before = tid ? (uint32_t)ph[i - 1]
				: j ? work[kFmdWorkHead + j - 1] : work[0];
		// nothing of the tile is overwritten before all of it has been read
		__syncthreads();
		Elems4<T> o;
		o.v[0] = (T)(S)step_of(v[0], before, sh);
#pragma unroll
		for (int k = 1; k < 4; k++)
			o.v[k] = (T)(S)step_of(v[k], v[k - 1], sh);
		if (i + 4 <= n) {
			*reinterpret_cast<Elems4<T> *>(ph + i) = o;
		} else {
#pragma unroll
			for (int k = 0; k < 4; k++)
				if (i + k < n)
					ph[i + k] = o.v[k];
		}
	}
}

// ---------------------------------------------------------------- host side
// Two launches at the most: the sweep over the whole vectors, then the tail.
// IO: the container of the four arrays, which sit on its element's grid.
template <typename IO>
static int run_fused(const cordic_config &cfg, size_t n, const typename IO::ielem *x,
		const typename IO::ielem *y, uint32_t phase0, uint32_t *d_last,
		typename IO::ielem *mag, typename IO::ielem *freq, hipStream_t st)
{
	typedef typename IO::ivec ivec;
	const size_t nvec = n / kVec;
	const CoreParams kp = make_params_jobs(cfg);
	if (nvec) {
		const int cus = jobs_cus_now();
		if (cus < 0) {
			(void)hipGetLastError();
			return CORDIC_ERR_DEVICE;
		}
		const size_t ntiles = (nvec + kFmdTileVecs - 1) / kFmdTileVecs;
		// resident blocks
		const size_t cap = env_block_cap("CORDIC_FMD_MAX_BLOCKS", (size_t)cus * 8);
		const int grid = (int)(ntiles < cap ? ntiles : cap);
		with_instance(cfg, kp, [&](auto inst) {
			typedef decltype(inst) I;
			hipLaunchKernelGGL((fm_demod_lj<I::nlive, I::dyn, I::ug, I::plain, IO>),
				dim3(grid), dim3(kBlock), 0, st, kp, (const ivec *)x,
				(const ivec *)y, (ivec *)mag, (ivec *)freq, nvec, ntiles,
				phase0, (const uint32_t *)d_last);
		}, IO{});
		if (int rc = tnco::finish(true))
			return rc;
	}
	if (nvec * kVec == n && !d_last)
		return CORDIC_OK;
	// the samples behind the last whole vector, and the one in front of them
	const size_t s0 = nvec ? nvec * kVec - 1 : 0;
	const DemodTail tail{reinterpret_cast<uintptr_t>(x + s0),
		reinterpret_cast<uintptr_t>(y + s0), reinterpret_cast<uintptr_t>(mag + s0),
		reinterpret_cast<uintptr_t>(freq + s0), reinterpret_cast<uintptr_t>(d_last),
		(uint32_t)(n - s0), phase0, nvec ? 0u : 1u, 0u};
	with_instance(cfg, kp, [&](auto inst) {
		typedef decltype(inst) I;
		hipLaunchKernelGGL((fm_demod_tail<I::nlive, I::dyn, I::ug, I::plain, IO>), dim3(1),
			dim3(64), 0, st, kp, tail);
	}, IO{});
	return tnco::finish(true);
}

template <typename T>
static int run_fallback(const cordic_config &cfg, size_t n, const void *x,
		const void *y, uint32_t phase0, uint32_t *d_last, void *mag, void *freq,
		uint32_t *work, hipStream_t st)
{
	constexpr bool io16 = sizeof(T) == 2;
	if (int rc = launch_topolar(cfg, n, static_cast<const int32_t *>(x),
			static_cast<const int32_t *>(y), static_cast<int32_t *>(mag),
			static_cast<uint32_t *>(freq), st, io16))
		return rc;
	const int cus = jobs_cus_now();
	if (cus < 0) {
		(void)hipGetLastError();
		return CORDIC_ERR_DEVICE;
	}
	const int sh = 32 - cfg.pw;
	const size_t ntiles = (n + kFmdDiffTile - 1) / kFmdDiffTile;
	const size_t cap = (size_t)cus * 2;
	const size_t sgrid = (ntiles + 255) / 256;
	T *ph = static_cast<T *>(freq);
	hipLaunchKernelGGL(fmd_save<T>, dim3((unsigned)(sgrid < cap ? sgrid : cap)),
		dim3(256), 0, st, (const T *)ph, n, phase0, d_last, work, sh);
	hipLaunchKernelGGL(fmd_diff<T>, dim3((unsigned)(ntiles < cap ? ntiles : cap)),
		dim3(1024), 0, st, ph, n, (const uint32_t *)work, sh);
	return tnco::finish(true);
}

static int demod(const cordic_config *cfg, size_t n, const void *x, const void *y,
		uint32_t phase0, uint32_t *d_last, void *mag, void *freq, void *d_work,
		void *stream, bool io16)
{
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (!cfg)
		return CORDIC_ERR_ARGS;
	if (io16 && (cfg->iw > 16 || cfg->ow > 16 || cfg->pw > 16))
		return CORDIC_ERR_CONTAINER;	// the rule of cordic_r2p16
	if (int rc = fmd_check_core(cfg))
		return rc;
	if (n == 0)
		return CORDIC_OK;
	const size_t es = io16 ? 2 : 4;
	if (!x || !y || !mag || !freq || !d_work || n > (~(size_t)0 >> 4))
		return CORDIC_ERR_ARGS;
	const uintptr_t arrays = reinterpret_cast<uintptr_t>(x)
		| reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(mag)
		| reinterpret_cast<uintptr_t>(freq);
	if ((arrays & (es - 1)) || (reinterpret_cast<uintptr_t>(d_last) & 3u)
			|| (reinterpret_cast<uintptr_t>(d_work) & 15u))
		return CORDIC_ERR_ARGS;
	// (d_work counts as an output on either path, whether or not it is written)
	const Range out[4] = {range_of(mag, n * es), range_of(freq, n * es),
		range_of(d_last, 4), range_of(d_work, fmd_work_bytes(n))};
	const Range in[2] = {range_of(x, n * es), range_of(y, n * es)};
	if (outputs_overlap(out, in))
		return CORDIC_ERR_ARGS;
	hipStream_t st = static_cast<hipStream_t>(stream);
	uint32_t *work = static_cast<uint32_t *>(d_work);
	if (io16) {
		// (any 2-byte alignment: the 16-byte condition below is the 32-bit
		// entry point's own)
		if (fmd_core_is_fused(*cfg))
			return run_fused<Io16>(*cfg, n, static_cast<const int16_t *>(x),
				static_cast<const int16_t *>(y), phase0, d_last,
				static_cast<int16_t *>(mag), static_cast<int16_t *>(freq), st);
		return run_fallback<uint16_t>(*cfg, n, x, y, phase0, d_last, mag, freq,
			work, st);
	}
	if (fmd_core_is_fused(*cfg) && !(arrays & 15u))
		return run_fused<Io32>(*cfg, n, static_cast<const int32_t *>(x),
			static_cast<const int32_t *>(y), phase0, d_last,
			static_cast<int32_t *>(mag), static_cast<int32_t *>(freq), st);
	return run_fallback<uint32_t>(*cfg, n, x, y, phase0, d_last, mag, freq, work,
		st);
}

} // namespace fmd

// launch_topolar's conditions for launch_pol_lj (cordic_kernels.hip)
bool fmd_core_is_fused(const cordic_config &cfg)
{
	return !(cfg.flags & (CORDIC_FLAG_FORCE_GENERIC | CORDIC_FLAG_NO_LJ))
		&& !cfg.needs_wrap && cfg.nlive >= 1 && cfg.nlive <= kDynStages
		&& cfg.ww <= 34;
}

int fmd_check_core(const cordic_config *cfg)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	if (cfg->mode != CORDIC_R2P && cfg->mode != CORDIC_SR2P)
		return CORDIC_ERR_MODE;
	return config_sane(*cfg) ? CORDIC_OK : CORDIC_ERR_ARGS;
}

} // namespace cordic_amd

// ------------------------------------------------------------ the C ABI
size_t cordic_fm_demod_workspace(size_t n)
{
	return cordic_amd::fmd_work_bytes(n);
}

int cordic_fm_demod_info(const cordic_config *cfg, int32_t *fused, int32_t *tile)
{
	using namespace cordic_amd;
	if (int rc = fmd_check_core(cfg))
		return rc;
	const bool f = fmd_core_is_fused(*cfg);
	if (fused)
		*fused = f ? 1 : 0;
	if (tile)
		*tile = f ? (int32_t)kFmdTile : 0;
	return CORDIC_OK;
}

int cordic_fm_demod16_info(const cordic_config *cfg, int32_t *fused, int32_t *tile)
{
	using namespace cordic_amd;
	if (!cfg)
		return CORDIC_ERR_ARGS;
	if (cfg->iw > 16 || cfg->ow > 16 || cfg->pw > 16)
		return CORDIC_ERR_CONTAINER;	// cordic_fm_demod16's order
	return cordic_fm_demod_info(cfg, fused, tile);
}

int cordic_fm_demod(const cordic_config *cfg, size_t n, const int32_t *d_xval,
		const int32_t *d_yval, uint32_t phase0, uint32_t *d_last,
		int32_t *d_omag, int32_t *d_ofreq, void *d_work, void *stream)
{
	return cordic_amd::fmd::demod(cfg, n, d_xval, d_yval, phase0, d_last, d_omag,
		d_ofreq, d_work, stream, false);
}

int cordic_fm_demod16(const cordic_config *cfg, size_t n, const int16_t *d_xval,
		const int16_t *d_yval, uint32_t phase0, uint32_t *d_last,
		int16_t *d_omag, int16_t *d_ofreq, void *d_work, void *stream)
{
	return cordic_amd::fmd::demod(cfg, n, d_xval, d_yval, phase0, d_last, d_omag,
		d_ofreq, d_work, stream, true);
}
