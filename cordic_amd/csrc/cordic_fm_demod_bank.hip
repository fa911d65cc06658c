// cordic_fm_demod_bank.hip -- FM demodulation banks (cordic_demodbank_create,
// _create16, _destroy, _info, _run; include/cordic_amd.h): many cordic_fm_demod
// (cordic_fm_demod16) jobs of one r2p / sr2p core, each with its own arrays,
// length, phase0 and d_last, in at most TWO launches.
//
// FUSED (the cores for which cordic_fm_demod_info answers 1; any 4-byte-aligned
// arrays -- the vector types are aligned(4) -- or, for a bank made by _create16,
// any 2-byte-aligned int16 arrays: the Io16 instances, whose vectors are 8
// bytes and aligned(2)):
//   fm_demod_lj_bank   fm_demod_lj (cordic_fm_demod.hip) reading tile
//       descriptors (DemodTile, cordic_fm_demod_bank.h).  The host has cut every
//       job's whole vectors into tiles of at most P * 256 - 1 vectors, never
//       across a job's end; block b sweeps tiles b, b + gridDim.x, ... in the
//       table's order, which is the jobs' own.  Per tile the descriptor arrives
//       as scalar loads and goes to sweep_tile (cordic_fm_demod.h), which
//       fm_demod_lj runs as well: the halo lane, the way the predecessor travels
//       and the ONE barrier per pass are written there.  A tile of nvec vectors
//       takes nvec / 256 + 1 passes, so the kernel does not need P.
//   fm_demod_bank_tails   one lane per job whose length is no multiple of 4 or
//       that has a d_last (DemodTail), by tail_of (cordic_fm_demod.h), the
//       single call's tail as well: at most 4 samples converted by the same
//       pol_lj_vector instance, differenced, stored; then *d_last.
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
// --save-temps; profiles/r14/fm_refactor_isa.txt), next to the table in
// cordic_fm_demod.hip (fm_demod_lj 56 / 94, topolar_lj_jobs 57 / 97):
//                               fm_demod_lj_bank   fm_demod_bank_tails
//   20 stages, PLAIN               46 / 0            40 / 0
//   29 stages, PLAIN               46 / 0            40 / 0
//   dynamic exit                   85 / 0            76 / 0
//   dynamic exit, unit gain        85 / 0            76 / 0
//   Io16, dynamic exit             81 / 0            76 / 0
//   Io16, dynamic exit, unit gain  81 / 0            76 / 0
// With 512 registers per lane of a SIMD, allocated in eights: 48 -> 8 waves (the
// most a SIMD holds) for the static instances and 88 -> 5 waves for the dynamic
// ones, one step of eight below fm_demod_lj's 56 and 96 at the same numbers of
// waves: it keeps its index inside a tile in 32 bits and one scalar pointer per
// array, where the single call carries a 64-bit index per lane.  Taken again
// with the container parameter in place (profiles/r18/fm_demod16_isa.txt): the
// Io32 counts are what they were; the Io16 instances (dynamic exit only, as in
// cordic_fm_demod.hip) stay in the same step, 81 -> 88 -> 5 waves.  No instance
// spills.  32 bytes of LDS per block of the main kernel, none in the tail kernel.
//
// ONE BY ONE (every other core: WW >= 35, wrap, CORDIC_FLAG_NO_LJ /
// _FORCE_GENERIC): run loops cordic_fm_demod (cordic_fm_demod16) over the jobs
// on the stream, with a scratch area the bank allocated at create for its
// longest job.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "cordic_device.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_devmem.h"
#include "cordic_table_nco.h"
#include "cordic_hostargs.h"
#include "cordic_fm_demod_bank.h"

namespace cordic_amd {

namespace fmd {

using namespace dev;

// IO: the container of the jobs' sample arrays (Io32 / Io16).  The descriptors
// hold byte addresses, so it only decides the vector type behind them.
template <int NLIVE, bool DYN, bool UG, bool PLAIN, typename IO = Io32>
__global__ __launch_bounds__(kBlock) void fm_demod_lj_bank(CoreParams kp,
		const DemodTile *__restrict__ tiles, uint32_t ntiles)
{
	typedef typename IO::ivec ivec;
	__shared__ uint32_t edge[2][kBlock / 64];
	const LaneConsts ln(kp);
	unsigned par = 0;
	for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const DemodTile d = tiles[t];
		// element 0 of these is the halo
		sweep_tile<NLIVE, DYN, UG, PLAIN>(kp, ln,
			reinterpret_cast<const ivec *>((uintptr_t)d.x) - 1,
			reinterpret_cast<const ivec *>((uintptr_t)d.y) - 1,
			reinterpret_cast<ivec *>((uintptr_t)d.mag) - 1,
			reinterpret_cast<ivec *>((uintptr_t)d.freq) - 1, (uint32_t)0, d.nvec,
			d.first != 0, d.phase0,
			reinterpret_cast<const uint32_t *>((uintptr_t)d.last), edge, par, IO{});
	}
}

constexpr int kTailBlock = 64;

template <int NLIVE, bool DYN, bool UG, bool PLAIN, typename IO = Io32>
__global__ __launch_bounds__(kTailBlock) void fm_demod_bank_tails(CoreParams kp,
		const DemodTail *__restrict__ tails, uint32_t ntails)
{
	const uint32_t i = blockIdx.x * kTailBlock + threadIdx.x;
	if (i >= ntails)
		return;
	const DemodTail d = tails[i];
	tail_of<NLIVE, DYN, UG, PLAIN>(kp, d, IO{});
}

// the two launches on the instances of one container
template <typename IO>
static int launch_bank(const cordic_config &cfg, const DemodTile *d_tiles,
		uint32_t ntiles, int grid, const DemodTail *d_tails, uint32_t ntails,
		hipStream_t st)
{
	const CoreParams kp = make_params_jobs(cfg);
	const int tgrid = (int)((ntails + kTailBlock - 1) / kTailBlock);
	with_instance(cfg, kp, [&](auto inst) {
		typedef decltype(inst) I;
		if (ntiles)
			hipLaunchKernelGGL((fm_demod_lj_bank<I::nlive, I::dyn, I::ug, I::plain, IO>),
				dim3(grid), dim3(kBlock), 0, st, kp, d_tiles, ntiles);
		if (ntails)
			hipLaunchKernelGGL((fm_demod_bank_tails<I::nlive, I::dyn, I::ug, I::plain, IO>),
				dim3(tgrid), dim3(kTailBlock), 0, st, kp, d_tails, ntails);
	}, IO{});
	return tnco::finish(true);
}

} // namespace fmd

int launch_fmd_bank(const cordic_config &cfg, const DemodTile *d_tiles,
		uint32_t ntiles, int grid, const DemodTail *d_tails, uint32_t ntails,
		bool io16, void *stream)
{
	hipStream_t st = static_cast<hipStream_t>(stream);
	return io16
		? fmd::launch_bank<dev::Io16>(cfg, d_tiles, ntiles, grid, d_tails, ntails, st)
		: fmd::launch_bank<dev::Io32>(cfg, d_tiles, ntiles, grid, d_tails, ntails, st);
}

} // namespace cordic_amd

// ------------------------------------------------------------ the C ABI
struct cordic_demodbank : BankHandle<cordic_demod_job> {
	cordic_config cfg;
	bool	io16 = false;	// the jobs' sample arrays hold int16
	int	passes = 0;
	// fused
	cordic_amd::DemodTile *d_tiles = nullptr;
	cordic_amd::DemodTail *d_tails = nullptr;
	uint32_t ntiles = 0, ntails = 0;
};

// both creates: `jobs` is either job struct (DemodJobs, cordic_fm_demod_bank.h)
static int demodbank_create(const cordic_config *cfg, size_t njobs,
		cordic_amd::DemodJobs jobs, cordic_demodbank **bank)
{
	using namespace cordic_amd;
	const bool io16 = jobs.esize() == 2;
	if (!bank || (njobs && jobs.none()))
		return CORDIC_ERR_ARGS;
	if (int rc = fmd_check_core(cfg))
		return rc;
	if (io16 && (cfg->iw > 16 || cfg->ow > 16 || cfg->pw > 16))
		return CORDIC_ERR_CONTAINER;	// the rule of cordic_fm_demod16
	if (njobs >= ((size_t)1 << 28) || !fmd_bank_jobs_valid(njobs, jobs))
		return CORDIC_ERR_ARGS;
	(void)hipGetLastError();	// (a stale error is not this call's)
	// the handle keeps its jobs as cordic_demod_job, whatever the container
	std::vector<cordic_demod_job> wide;
	const cordic_demod_job *flat = jobs.j32;
	if (io16) {
		wide.reserve(njobs);
		for (size_t k = 0; k < njobs; k++)
			wide.push_back(jobs[k]);
		flat = wide.data();
	}
	cordic_demodbank *b = nullptr;
	if (int rc = bank_begin(njobs, flat, fmd_core_is_fused(*cfg), fmd_work_bytes, &b))
		return rc;
	b->cfg = *cfg;
	b->io16 = io16;
	if (!b->fused) {
		*bank = b;
		return CORDIC_OK;
	}
	uint64_t vecs = 0;
	for (size_t k = 0; k < njobs; k++)
		vecs += jobs.n(k) / 4;
	b->passes = (int)bank_forced_passes(std::getenv("CORDIC_FMD_BANK_PASSES"), 8,
			(uint32_t)fmd_bank_passes(vecs, b->cus));
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

int cordic_demodbank_create(const cordic_config *cfg, size_t njobs,
		const cordic_demod_job *jobs, cordic_demodbank **bank)
{
	return demodbank_create(cfg, njobs, jobs, bank);
}

int cordic_demodbank_create16(const cordic_config *cfg, size_t njobs,
		const cordic_demod_job16 *jobs, cordic_demodbank **bank)
{
	return demodbank_create(cfg, njobs, jobs, bank);
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
	return bank_run(*bank, [&] {
		if (!bank->ntiles && !bank->ntails)
			return (int)CORDIC_OK;
		// resident blocks
		const size_t cap = env_block_cap("CORDIC_FMD_MAX_BLOCKS", (size_t)bank->cus * 8);
		const int grid = (int)(bank->ntiles < cap ? bank->ntiles : cap);
		return launch_fmd_bank(bank->cfg, bank->d_tiles, bank->ntiles, grid,
			bank->d_tails, bank->ntails, bank->io16, stream);
	}, [&](const cordic_demod_job &jb) {
		if (bank->io16)
			return cordic_fm_demod16(&bank->cfg, (size_t)jb.n,
				reinterpret_cast<const int16_t *>(jb.d_xval),
				reinterpret_cast<const int16_t *>(jb.d_yval), jb.phase0, jb.d_last,
				reinterpret_cast<int16_t *>(jb.d_omag),
				reinterpret_cast<int16_t *>(jb.d_ofreq), bank->d_work, stream);
		return cordic_fm_demod(&bank->cfg, (size_t)jb.n, jb.d_xval, jb.d_yval,
			jb.phase0, jb.d_last, jb.d_omag, jb.d_ofreq, bank->d_work, stream);
	});
}
