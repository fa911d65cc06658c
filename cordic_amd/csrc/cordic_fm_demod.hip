// cordic_fm_demod.hip -- FM demodulation (cordic_fm_demod, cordic_fm_demod16,
// cordic_fm_demod_info, cordic_fm_demod_workspace): the r2p / sr2p converter
// with its phase differenced from sample to sample,
//   prev   = (phase0 + *d_last) mod 2^PW
//   freq_i = sext_PW((ph_i - ph_(i-1)) mod 2^PW),   ph_(-1) = prev
//   mag_i  = cordic_r2p's,   *d_last = ph_(n-1),
// ph_i being the word cordic_r2p writes to d_ophase[i].
//
// FUSED (fm_demod_lj): the cores that launch_topolar sends to topolar_lj
// (32-bit containers, WW <= 34, no wrap), when all four arrays sit on 16-byte
// boundaries.  (That last condition is this entry point's own: topolar_lj
// itself takes any 4-byte-aligned array, and fm_demod_lj uses the same vector
// types; displaced arrays are simply routed to the fallback here.)  A lane
// converts the 4 samples of a vector exactly as topolar_lj_sweep does and
// needs one more phase: the last one of the vector in front.  Blocks therefore
// sweep CONTIGUOUS tiles (b, b + gridDim.x, ...), 8 passes of 256 vectors each:
//   * inside a wave the predecessor comes from lane - 1 by one DPP move
//     (wave_shr:1), whose lane 0 keeps the value handed in;
//   * that value is the last phase of the wave in front -- wave w - 1 of this
//     pass, or wave 3 of the pass before -- through one LDS word per wave.
//     The words are double-buffered by pass, so a pass has ONE barrier: a
//     word written in pass i was last read in pass i - 2 (waves 1..3, behind
//     that pass's barrier) or at the top of pass i - 1 (wave 0, in front of
//     its barrier), and every wave has passed barrier i - 1 before any writes;
//   * the sweep starts one vector IN FRONT of the tile (the halo): that
//     vector is converted like any other and not stored, so tile t's first
//     vector finds its predecessor where every other one does.  A tile is
//     8 * 256 - 1 = 2047 vectors of output for 2048 converted: 1/2048 of the
//     work twice, no divergent pass.  The halo phase is the same arithmetic on
//     the same inputs as the neighbour's own, so the result does not depend on
//     the grid.  In front of sample 0 the halo lane holds `prev` instead.
// *d_last is read by that one lane; it is written by the tail launch that
// follows in stream order: launch_topolar converts the samples behind the last
// whole vector together with the one in front of them (<= 4 in all) into
// d_work, and a one-thread kernel differences those and writes *d_last.
//
// CORDIC_FMD_MAX_BLOCKS=<n> in the environment (read at every call; a test
// and A/B knob like CORDIC_FORCE_DYN) caps the fused kernel's grid at n
// blocks, so that a short call runs many tiles per block.  The bits do not
// depend on it.
//
// cordic_last_kernel() is unspecified after these calls: the tail and the
// fallback go through launch_topolar, which records its own kernel.
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps):
//                          topolar_lj   topolar_lj_jobs   fm_demod_lj
//   20 and 29 stages, PLAIN    49             57               54
//   dynamic exit (and UG)      88             97               93
// With 512 registers per lane of a SIMD, allocated in eights: 56 -> 8 waves
// (the most a SIMD holds) for the static instances as for topolar_lj's 49,
// and 96 -> 5 waves for the dynamic ones as for its 88.  The differencing
// crosses no occupancy step; no instance spills.  32 bytes of LDS per block.
//
// FALLBACK (everything else: WW 35 .. 40 and wider, cores that wrap, the A/B
// flags, arrays off the 16-byte grid, the 16-bit form): launch_topolar writes
// the raw phases into d_ofreq; fmd_save keeps the last phase of every
// 4096-sample tile (and prev, and writes *d_last -- the same thread reads it
// first); fmd_diff differences in place, a block per tile: every thread has
// read its 4 phases and the one in front before any is overwritten, and the
// word in front of a tile comes from d_work.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "cordic_device.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_fm_demod.h"

namespace cordic_amd {

namespace fmd {

using namespace dev;

// (pol_lj_vector and step_of: cordic_fm_demod.h, shared with the bank's kernels)

// Tile t is the vectors [t * kFmdTileVecs, (t + 1) * kFmdTileVecs) cut at nvec;
// thread tid converts vector t * kFmdTileVecs - 1 + 256 * k + tid in pass k.
// For t = 0 that index wraps in thread 0 of pass 0 (no such vector): it fails
// the `< nvec` tests like any vector behind the end, and 256 later it is 255.
template <int NLIVE, bool DYN, bool UG, bool PLAIN>
__global__ __launch_bounds__(kBlock) void fm_demod_lj(CoreParams kp,
		const i32x4g *__restrict__ xin, const i32x4g *__restrict__ yin,
		i32x4g *__restrict__ omag, i32x4g *__restrict__ ofreq, size_t nvec,
		size_t ntiles, uint32_t phase0, const uint32_t *__restrict__ d_last)
{
	__shared__ uint32_t edge[2][kBlock / 64];
	const unsigned tid = threadIdx.x, lane = tid & 63u;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);

	PolLjRegs c;		// cordic_device.h:2257-2264
	c.sign = vgpr_const(0x80000000u);
	c.p30 = vgpr_const(0x40000000u);
	const uint32_t rbw = vgpr_const(kp.round_bit);
	const int up = 32 - kp.iw;
	const int down = up - kp.in_shl;
	const int sh = kp.pw_shl;

	uint32_t prev = 0;	// the lane in front of sample 0 alone needs it
	if (blockIdx.x == 0 && tid == 0)
		prev = (phase0 + (d_last ? *d_last : 0u)) & (0xffffffffu >> sh);

	unsigned par = 0;
	for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const size_t base = t * kFmdTileVecs;
		size_t g = base + tid - 1;
		i32x4g nx{}, ny{};	// software prefetch, afresh per tile (as
		if (g < nvec) {		// topolar_lj_jobs)
			nx = CORDIC_LOAD_IN(&xin[g]);
			ny = CORDIC_LOAD_IN(&yin[g]);
		}
		for (int k = 0; k < kFmdPasses; k++, g += kBlock) {
			// thread 0's vector is behind the end: so is everyone's
			if (base + (size_t)k * kBlock > nvec)
				break;
			const i32x4 tx = nx, ty = ny;
			const size_t gn = g + kBlock;
			if (k + 1 < kFmdPasses && gn < nvec) {
				nx = CORDIC_LOAD_IN(&xin[gn]);
				ny = CORDIC_LOAD_IN(&yin[gn]);
			}
			i32x4 rm;
			u32x4 rp;
			pol_lj_vector<NLIVE, DYN, UG, PLAIN>(kp, c, rbw, up, down, tx, ty,
				rm, rp);

			uint32_t last = rp[3];
			if (g + 1 == 0)		// in front of sample 0
				last = prev;
			if (lane == 63)
				edge[par][wave] = last;
			uint32_t front = 0;
			if (wave == 0)		// (pass 0: the halo lane's, unused)
				front = edge[par ^ 1][kBlock / 64 - 1];
			__syncthreads();
			if (wave != 0)
				front = edge[par][wave - 1];
			par ^= 1;
			// wave_shr:1 -- lane l gets lane l - 1's `last`, lane 0 keeps
			// `front`
			const uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp(
				(int)front, (int)last, 0x138, 0xf, 0xf, false);
			i32x4 rf;
			rf[0] = step_of(rp[0], before, sh);
#pragma unroll
			for (int v = 1; v < kVec; v++)
				rf[v] = step_of(rp[v], rp[v - 1], sh);
			if ((k | tid) != 0 && g < nvec) {	// (not the halo)
				CORDIC_STORE_OUT(true, &omag[g], rm);
				CORDIC_STORE_OUT(true, &ofreq[g], rf);
			}
		}
	}
}

// The fused path's tail: wmag / wph hold `count` <= 4 converted samples, of
// which the first is only the predecessor when `first` = 1 (a whole vector was
// in front); omag / ofreq point at the sample that wmag[0] belongs to.
__global__ void fmd_finish(const int32_t *__restrict__ wmag,
		const uint32_t *__restrict__ wph, unsigned count, unsigned first,
		uint32_t phase0, uint32_t *d_last, int32_t *__restrict__ omag,
		int32_t *__restrict__ ofreq, int sh)
{
	if (blockIdx.x != 0 || threadIdx.x != 0)
		return;
	uint32_t p = first ? wph[0]
		: (phase0 + (d_last ? *d_last : 0u)) & (0xffffffffu >> sh);
	for (unsigned i = first; i < count; i++) {
		omag[i] = wmag[i];
		ofreq[i] = step_of(wph[i], p, sh);
		p = wph[i];
	}
	if (d_last)
		*d_last = p;
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
struct Range {
	uintptr_t lo;
	size_t	bytes;
};

static bool hits(const Range &a, const Range &b)
{
	return a.bytes && b.bytes && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes;
}

static int check_launch()
{
	return hipGetLastError() == hipSuccess ? CORDIC_OK : CORDIC_ERR_DEVICE;
}

// the instance choice of launch_pol_lj (cordic_inst_pol_lj.hip)
static void launch_lj(const cordic_config &cfg, const CoreParams &kp, int grid,
		hipStream_t st, const int32_t *x, const int32_t *y, int32_t *mag,
		int32_t *freq, size_t nvec, size_t ntiles, uint32_t phase0,
		const uint32_t *d_last)
{
#define FMD_LAUNCH(...) \
	hipLaunchKernelGGL((fm_demod_lj<__VA_ARGS__>), dim3(grid), dim3(kBlock), 0, st, \
		kp, (const i32x4g *)x, (const i32x4g *)y, (i32x4g *)mag, (i32x4g *)freq, \
		nvec, ntiles, phase0, d_last)
	if (kp.post_mul != 0) {		// CORDIC_FLAG_UNIT_GAIN
		FMD_LAUNCH(kDynStages, true, true, false);
		return;
	}
	const bool plain = (32 - kp.iw) - kp.in_shl >= 2 && kp.r >= 2 && kp.r <= 31;
	switch (plain ? cfg.nlive : -1) {
	case 20: FMD_LAUNCH(20, false, false, true); return;
	case 29: FMD_LAUNCH(29, false, false, true); return;
	default: FMD_LAUNCH(kDynStages, true, false, false); return;
	}
#undef FMD_LAUNCH
}

static int run_fused(const cordic_config &cfg, size_t n, const int32_t *x,
		const int32_t *y, uint32_t phase0, uint32_t *d_last, int32_t *mag,
		int32_t *freq, uint32_t *work, hipStream_t st)
{
	const size_t nvec = n / kVec;
	const int sh = 32 - cfg.pw;
	if (nvec) {
		const int cus = jobs_cus_now();
		if (cus < 0) {
			(void)hipGetLastError();
			return CORDIC_ERR_DEVICE;
		}
		const size_t ntiles = (nvec + kFmdTileVecs - 1) / kFmdTileVecs;
		size_t cap = (size_t)cus * 8;	// resident blocks
		if (const char *e = std::getenv("CORDIC_FMD_MAX_BLOCKS")) {
			const long v = std::strtol(e, nullptr, 10);
			if (v >= 1 && (size_t)v < cap)
				cap = (size_t)v;
		}
		const int grid = (int)(ntiles < cap ? ntiles : cap);
		launch_lj(cfg, make_params_jobs(cfg), grid, st, x, y, mag, freq, nvec,
			ntiles, phase0, d_last);
		if (int rc = check_launch())
			return rc;
	}
	if (nvec * kVec == n && !d_last)
		return CORDIC_OK;
	// the samples behind the last whole vector, and the one in front of them
	const size_t s0 = nvec ? nvec * kVec - 1 : 0;
	const unsigned count = (unsigned)(n - s0);
	int32_t *wmag = reinterpret_cast<int32_t *>(work + 4);
	uint32_t *wph = work + 8;
	if (int rc = launch_topolar(cfg, count, x + s0, y + s0, wmag, wph, st))
		return rc;
	hipLaunchKernelGGL(fmd_finish, dim3(1), dim3(64), 0, st, wmag, wph, count,
		nvec ? 1u : 0u, phase0, d_last, mag + s0, freq + s0, sh);
	return check_launch();
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
	return check_launch();
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
	if (cfg->mode != CORDIC_R2P && cfg->mode != CORDIC_SR2P)
		return CORDIC_ERR_MODE;
	if (!config_sane(*cfg))
		return CORDIC_ERR_ARGS;
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
	const Range out[4] = {{reinterpret_cast<uintptr_t>(mag), n * es},
		{reinterpret_cast<uintptr_t>(freq), n * es},
		{reinterpret_cast<uintptr_t>(d_last), d_last ? (size_t)4 : 0},
		{reinterpret_cast<uintptr_t>(d_work), fmd_work_bytes(n)}};
	const Range in[2] = {{reinterpret_cast<uintptr_t>(x), n * es},
		{reinterpret_cast<uintptr_t>(y), n * es}};
	for (int i = 0; i < 4; i++) {
		for (int j = i + 1; j < 4; j++)
			if (hits(out[i], out[j]))
				return CORDIC_ERR_ARGS;
		for (int j = 0; j < 2; j++)
			if (hits(out[i], in[j]))
				return CORDIC_ERR_ARGS;
	}
	hipStream_t st = static_cast<hipStream_t>(stream);
	uint32_t *work = static_cast<uint32_t *>(d_work);
	if (io16)
		return run_fallback<uint16_t>(*cfg, n, x, y, phase0, d_last, mag, freq,
			work, st);
	if (fmd_core_is_fused(*cfg) && !(arrays & 15u))
		return run_fused(*cfg, n, static_cast<const int32_t *>(x),
			static_cast<const int32_t *>(y), phase0, d_last,
			static_cast<int32_t *>(mag), static_cast<int32_t *>(freq), work, st);
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

} // namespace cordic_amd

// ------------------------------------------------------------ the C ABI
size_t cordic_fm_demod_workspace(size_t n)
{
	return cordic_amd::fmd_work_bytes(n);
}

int cordic_fm_demod_info(const cordic_config *cfg, int32_t *fused, int32_t *tile)
{
	using namespace cordic_amd;
	if (!cfg)
		return CORDIC_ERR_ARGS;
	if (cfg->mode != CORDIC_R2P && cfg->mode != CORDIC_SR2P)
		return CORDIC_ERR_MODE;
	if (!config_sane(*cfg))
		return CORDIC_ERR_ARGS;
	const bool f = fmd_core_is_fused(*cfg);
	if (fused)
		*fused = f ? 1 : 0;
	if (tile)
		*tile = f ? (int32_t)kFmdTile : 0;
	return CORDIC_OK;
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
