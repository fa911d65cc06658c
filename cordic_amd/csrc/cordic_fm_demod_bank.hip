// cordic_fm_demod_bank.hip -- FM demodulation banks (cordic_demodbank_create,
// _destroy, _info, _run; include/cordic_amd.h): many cordic_fm_demod jobs of one
// r2p / sr2p core, each with its own arrays, length, phase0 and d_last, in at
// most TWO launches.
//
// FUSED (the cores for which cordic_fm_demod_info answers 1; any 4-byte-aligned
// arrays -- the vector types are aligned(4)):
//   fm_demod_lj_bank   fm_demod_lj (cordic_fm_demod.hip) reading tile
//       descriptors (DemodTile, cordic_fm_demod_bank.h).  The host has cut every
//       job's whole vectors into tiles of at most P * 256 - 1 vectors, never
//       across a job's end; block b sweeps tiles b, b + gridDim.x, ... in the
//       table's order, which is the jobs' own.  Per tile the descriptor arrives
//       as scalar loads; lane j of the sweep (j = 256 * pass + thread) converts
//       vector j - 1 of the tile, so lane 0 converts the halo -- the vector in
//       front of the tile, which belongs to the same job -- and stores nothing.
//       In a job's first tile there is no such vector: lane 0 loads nothing and
//       holds (phase0 + *d_last) mod 2^PW instead.  The predecessor travels as
//       in fm_demod_lj: one DPP move inside a wave, one LDS word per wave
//       between waves and passes, double-buffered by pass, ONE barrier per pass
//       (the argument there holds from tile to tile as well: the parity simply
//       keeps alternating, and pass 0 of a tile uses no word of the pass in
//       front).  A tile of nvec vectors takes nvec / 256 + 1 passes, the same
//       for all threads of the block, so the kernel does not need P.
//   fm_demod_bank_tails   one lane per job whose length is no multiple of 4 or
//       that has a d_last (DemodTail): the samples behind the last whole vector
//       and the one in front of them, at most 4, gathered into one zero-padded
//       vector, converted by the same pol_lj_vector instance, differenced,
//       stored; then *d_last.  A job without a whole vector reads its *d_last
//       here, in the same lane, before writing it.
// Every *d_last is read in the first launch or by the lane that writes it, and
// written only in the second launch, which follows in stream order: no block
// can see a value the same run writes.  Nothing is allocated, copied or
// synchronised at run; no block waits for another; no tile queue.
//
// P (1, 2, 4 or 8) is chosen at create -- fmd_bank_passes: the longest tile that
// still gives every resident block four -- or forced by CORDIC_FMD_BANK_PASSES
// in the environment (read at create; a test and A/B knob).  The grid is
// min(tiles, CUs * 8), capped further by CORDIC_FMD_MAX_BLOCKS (read at every
// run, as cordic_fm_demod does).  The bits depend on neither.
//
// Registers (.vgpr_count / scratch bytes of the gfx950 code objects, -O3,
// --save-temps), next to the table in cordic_fm_demod.hip (fm_demod_lj 54 / 93,
// topolar_lj_jobs 57 / 97):
//                               fm_demod_lj_bank   fm_demod_bank_tails
//   20 stages, PLAIN               46 / 0            40 / 0
//   29 stages, PLAIN               46 / 0            40 / 0
//   dynamic exit                   85 / 0            76 / 0
//   dynamic exit, unit gain        85 / 0            76 / 0
// With 512 registers per lane of a SIMD, allocated in eights: 48 -> 8 waves (the
// most a SIMD holds) for the static instances and 88 -> 5 waves for the dynamic
// ones, the steps fm_demod_lj stands on (56 and 96); the 32-bit indices inside
// a tile cost fewer registers than its 64-bit ones.  No instance spills.  32
// bytes of LDS per block of the main kernel, none in the tail kernel.
//
// ONE BY ONE (every other core: WW >= 35, wrap, CORDIC_FLAG_NO_LJ /
// _FORCE_GENERIC): run loops cordic_fm_demod over the jobs on the stream, with
// a scratch area the bank allocated at create for its longest job.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <new>
#include <vector>

#include "cordic_device.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_devmem.h"
#include "cordic_fm_demod.h"
#include "cordic_fm_demod_bank.h"

namespace cordic_amd {

namespace fmd {

using namespace dev;

template <int NLIVE, bool DYN, bool UG, bool PLAIN>
__global__ __launch_bounds__(kBlock) void fm_demod_lj_bank(CoreParams kp,
		const DemodTile *__restrict__ tiles, uint32_t ntiles)
{
	__shared__ uint32_t edge[2][kBlock / 64];
	const unsigned tid = threadIdx.x, lane = tid & 63u;
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);

	PolLjRegs c;
	c.sign = vgpr_const(0x80000000u);
	c.p30 = vgpr_const(0x40000000u);
	const uint32_t rbw = vgpr_const(kp.round_bit);
	const int up = 32 - kp.iw;
	const int down = up - kp.in_shl;
	const int sh = kp.pw_shl;

	unsigned par = 0;
	for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const DemodTile d = tiles[t];
		// lane j's vector is element j of these: element 0 is the halo
		const i32x4g *xin = reinterpret_cast<const i32x4g *>((uintptr_t)d.x) - 1;
		const i32x4g *yin = reinterpret_cast<const i32x4g *>((uintptr_t)d.y) - 1;
		i32x4g *omag = reinterpret_cast<i32x4g *>((uintptr_t)d.mag) - 1;
		i32x4g *ofreq = reinterpret_cast<i32x4g *>((uintptr_t)d.freq) - 1;
		const uint32_t nvec = d.nvec;
		const bool first = d.first != 0;

		uint32_t prev = 0;	// the lane in front of sample 0 alone needs it
		if (first && tid == 0) {
			const uint32_t *lp = reinterpret_cast<const uint32_t *>((uintptr_t)d.last);
			prev = (d.phase0 + (lp ? *lp : 0u)) & (0xffffffffu >> sh);
		}
		uint32_t j = tid;
		i32x4g nx{}, ny{};	// software prefetch, afresh per tile
		if (j <= nvec && !(first && j == 0)) {
			nx = CORDIC_LOAD_IN(&xin[j]);
			ny = CORDIC_LOAD_IN(&yin[j]);
		}
		// (thread 0's vector is behind the end: so is everyone's)
		for (uint32_t k0 = 0; k0 <= nvec; k0 += kBlock, j += kBlock) {
			const i32x4 tx = nx, ty = ny;
			const uint32_t jn = j + kBlock;
			if (jn <= nvec) {
				nx = CORDIC_LOAD_IN(&xin[jn]);
				ny = CORDIC_LOAD_IN(&yin[jn]);
			}
			i32x4 rm;
			u32x4 rp;
			pol_lj_vector<NLIVE, DYN, UG, PLAIN>(kp, c, rbw, up, down, tx, ty,
				rm, rp);

			uint32_t last = rp[3];
			if (first && j == 0)	// in front of sample 0
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
			if (j != 0 && j <= nvec) {	// (not the halo)
				CORDIC_STORE_OUT(true, &omag[j], rm);
				CORDIC_STORE_OUT(true, &ofreq[j], rf);
			}
		}
	}
}

constexpr int kTailBlock = 64;

template <int NLIVE, bool DYN, bool UG, bool PLAIN>
__global__ __launch_bounds__(kTailBlock) void fm_demod_bank_tails(CoreParams kp,
		const DemodTail *__restrict__ tails, uint32_t ntails)
{
	const uint32_t i = blockIdx.x * kTailBlock + threadIdx.x;
	if (i >= ntails)
		return;
	const DemodTail d = tails[i];
	PolLjRegs c;
	c.sign = vgpr_const(0x80000000u);
	c.p30 = vgpr_const(0x40000000u);
	const uint32_t rbw = vgpr_const(kp.round_bit);
	const int up = 32 - kp.iw;
	const int down = up - kp.in_shl;
	const int sh = kp.pw_shl;

	const int32_t *x = reinterpret_cast<const int32_t *>((uintptr_t)d.x);
	const int32_t *y = reinterpret_cast<const int32_t *>((uintptr_t)d.y);
	int32_t *omag = reinterpret_cast<int32_t *>((uintptr_t)d.mag);
	int32_t *ofreq = reinterpret_cast<int32_t *>((uintptr_t)d.freq);
	uint32_t *lp = reinterpret_cast<uint32_t *>((uintptr_t)d.last);
	i32x4 tx{}, ty{};
#pragma unroll
	for (int v = 0; v < kVec; v++)
		if ((uint32_t)v < d.count) {
			tx[v] = x[v];
			ty[v] = y[v];
		}
	i32x4 rm;
	u32x4 rp;
	pol_lj_vector<NLIVE, DYN, UG, PLAIN>(kp, c, rbw, up, down, tx, ty, rm, rp);
	// element 0 only lends its phase when a whole vector was in front
	uint32_t p = rp[0];
	if (d.first) {
		p = (d.phase0 + (lp ? *lp : 0u)) & (0xffffffffu >> sh);
		omag[0] = rm[0];
		ofreq[0] = step_of(rp[0], p, sh);
		p = rp[0];
	}
#pragma unroll
	for (int v = 1; v < kVec; v++)
		if ((uint32_t)v < d.count) {
			omag[v] = rm[v];
			ofreq[v] = step_of(rp[v], p, sh);
			p = rp[v];
		}
	if (lp)
		*lp = p;
}

static int check_launch()
{
	return hipGetLastError() == hipSuccess ? CORDIC_OK : CORDIC_ERR_DEVICE;
}

} // namespace fmd

// the instance choice of launch_lj (cordic_fm_demod.hip), for both kernels
int launch_fmd_bank(const cordic_config &cfg, const DemodTile *d_tiles,
		uint32_t ntiles, int grid, const DemodTail *d_tails, uint32_t ntails,
		void *stream)
{
	using namespace dev;
	using namespace fmd;
	hipStream_t st = static_cast<hipStream_t>(stream);
	const CoreParams kp = make_params_jobs(cfg);
	const int tgrid = (int)((ntails + kTailBlock - 1) / kTailBlock);
#define FMD_BANK_LAUNCH(...) do { \
	if (ntiles) \
		hipLaunchKernelGGL((fm_demod_lj_bank<__VA_ARGS__>), dim3(grid), \
			dim3(kBlock), 0, st, kp, d_tiles, ntiles); \
	if (ntails) \
		hipLaunchKernelGGL((fm_demod_bank_tails<__VA_ARGS__>), dim3(tgrid), \
			dim3(kTailBlock), 0, st, kp, d_tails, ntails); \
	} while (0)
	const bool plain = (32 - kp.iw) - kp.in_shl >= 2 && kp.r >= 2 && kp.r <= 31;
	if (kp.post_mul != 0) {		// CORDIC_FLAG_UNIT_GAIN
		FMD_BANK_LAUNCH(kDynStages, true, true, false);
	} else if (plain && cfg.nlive == 20) {
		FMD_BANK_LAUNCH(20, false, false, true);
	} else if (plain && cfg.nlive == 29) {
		FMD_BANK_LAUNCH(29, false, false, true);
	} else {
		FMD_BANK_LAUNCH(kDynStages, true, false, false);
	}
#undef FMD_BANK_LAUNCH
	return check_launch();
}

} // namespace cordic_amd

// ------------------------------------------------------------ the C ABI
struct cordic_demodbank {
	cordic_config cfg;
	int	device = -1;
	bool	fused = false;
	int	passes = 0, cus = 0;
	uint64_t samples = 0;
	// fused
	cordic_amd::DemodTile *d_tiles = nullptr;
	cordic_amd::DemodTail *d_tails = nullptr;
	uint32_t ntiles = 0, ntails = 0;
	// one by one: the non-empty jobs and the scratch of the longest
	std::vector<cordic_demod_job> jobs;
	void	*d_work = nullptr;
};

int cordic_demodbank_create(const cordic_config *cfg, size_t njobs,
		const cordic_demod_job *jobs, cordic_demodbank **bank)
{
	using namespace cordic_amd;
	if (!cfg || !bank || (njobs && !jobs))
		return CORDIC_ERR_ARGS;
	if (cfg->mode != CORDIC_R2P && cfg->mode != CORDIC_SR2P)
		return CORDIC_ERR_MODE;
	if (!config_sane(*cfg) || njobs >= ((size_t)1 << 28)
			|| !fmd_bank_jobs_valid(njobs, jobs))
		return CORDIC_ERR_ARGS;
	(void)hipGetLastError();	// (a stale error is not this call's)
	// blocking uploads below: not while the legacy stream is being captured
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	const hipError_t ce = hipStreamIsCapturing(nullptr, &cs);
	(void)hipGetLastError();
	if (ce == hipErrorStreamCaptureImplicit
			|| (ce == hipSuccess && cs != hipStreamCaptureStatusNone))
		return CORDIC_ERR_UNSUPPORTED;

	uint64_t samples = 0, vecs = 0;
	size_t longest = 0;
	for (size_t k = 0; k < njobs; k++) {
		samples += jobs[k].n;
		vecs += jobs[k].n / 4;
		if (jobs[k].n > longest)
			longest = (size_t)jobs[k].n;
	}
	cordic_demodbank *b = new (std::nothrow) cordic_demodbank;
	if (!b)
		return CORDIC_ERR_NOMEM;
	b->cfg = *cfg;
	b->samples = samples;
	b->fused = fmd_core_is_fused(*cfg);
	if (hipGetDevice(&b->device) != hipSuccess) {
		(void)hipGetLastError();
		b->device = -1;
	}
	if (!b->fused) {
		for (size_t k = 0; k < njobs; k++)
			if (jobs[k].n)
				b->jobs.push_back(jobs[k]);
		if (!dev_zalloc(&b->d_work, fmd_work_bytes(longest))) {
			cordic_demodbank_destroy(b);
			return CORDIC_ERR_DEVICE;
		}
		*bank = b;
		return CORDIC_OK;
	}
	b->cus = jobs_cus_now();
	if (b->cus <= 0) {
		(void)hipGetLastError();
		b->cus = 256;
	}
	b->passes = fmd_bank_passes(vecs, b->cus);
	if (const char *e = std::getenv("CORDIC_FMD_BANK_PASSES")) {
		const long v = std::strtol(e, nullptr, 10);
		if (v == 1 || v == 2 || v == 4 || v == 8)
			b->passes = (int)v;
	}
	const uint32_t tile_vecs = fmd_bank_tile_vecs(b->passes);
	if (fmd_bank_count_tiles(njobs, jobs, tile_vecs) > 0xffffffffull) {
		delete b;
		return CORDIC_ERR_ARGS;
	}
	std::vector<DemodTile> tiles;
	std::vector<DemodTail> tails;
	fmd_bank_cut(njobs, jobs, tile_vecs, &tiles, &tails);
	if (!dev_upload(tiles.data(), tiles.size() * sizeof(DemodTile), &b->d_tiles)
			|| !dev_upload(tails.data(), tails.size() * sizeof(DemodTail),
				&b->d_tails)) {
		cordic_demodbank_destroy(b);
		return CORDIC_ERR_DEVICE;
	}
	b->ntiles = (uint32_t)tiles.size();
	b->ntails = (uint32_t)tails.size();
	*bank = b;
	return CORDIC_OK;
}

void cordic_demodbank_destroy(cordic_demodbank *bank)
{
	if (!bank)
		return;
	dev_free(bank->d_tiles, bank->d_tails, bank->d_work);
	delete bank;
}

int cordic_demodbank_info(const cordic_demodbank *bank, uint64_t *samples,
		uint32_t *tiles, uint32_t *tail_jobs, int32_t *fused, int32_t *tile)
{
	if (!bank)
		return CORDIC_ERR_ARGS;
	if (samples) *samples = bank->samples;
	if (tiles) *tiles = bank->ntiles;
	if (tail_jobs) *tail_jobs = bank->ntails;
	if (fused) *fused = bank->fused ? 1 : 0;
	if (tile)
		*tile = bank->fused
			? (int32_t)(cordic_amd::fmd_bank_tile_vecs(bank->passes) * 4) : 0;
	return CORDIC_OK;
}

int cordic_demodbank_run(const cordic_demodbank *bank, void *stream)
{
	using namespace cordic_amd;
	if (!bank)
		return CORDIC_ERR_ARGS;
	(void)hipGetLastError();
	int dev = -1;
	if (hipGetDevice(&dev) != hipSuccess) {
		(void)hipGetLastError();
		return CORDIC_ERR_DEVICE;
	}
	// (the tables hold device addresses)
	if (dev != bank->device)
		return CORDIC_ERR_ARGS;
	if (!bank->fused) {
		for (const cordic_demod_job &jb : bank->jobs)
			if (int rc = cordic_fm_demod(&bank->cfg, (size_t)jb.n, jb.d_xval,
					jb.d_yval, jb.phase0, jb.d_last, jb.d_omag, jb.d_ofreq,
					bank->d_work, stream))
				return rc;
		return CORDIC_OK;
	}
	if (!bank->ntiles && !bank->ntails)
		return CORDIC_OK;
	size_t cap = (size_t)bank->cus * 8;	// resident blocks
	if (const char *e = std::getenv("CORDIC_FMD_MAX_BLOCKS")) {
		const long v = std::strtol(e, nullptr, 10);
		if (v >= 1 && (size_t)v < cap)
			cap = (size_t)v;
	}
	const int grid = (int)(bank->ntiles < cap ? bank->ntiles : cap);
	return launch_fmd_bank(bank->cfg, bank->d_tiles, bank->ntiles, grid,
		bank->d_tails, bank->ntails, stream);
}
