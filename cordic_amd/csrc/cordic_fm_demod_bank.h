// cordic_fm_demod_bank.h -- FM demodulation banks: many cordic_fm_demod jobs of
// one r2p / sr2p core in at most TWO launches (include/cordic_amd.h, "FM
// demodulation banks"), on int32 or on int16 I/Q arrays (cordic_demod_job /
// cordic_demod_job16).  The descriptors the host cuts at create, the cutter
// itself -- plain C++ that touches no device, so that a stand-alone program can
// run it under a sanitizer -- and the launchers of the two kernels that walk
// the descriptors (cordic_fm_demod_bank.hip).  Host-visible types only.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_FM_DEMOD_BANK_H
#define CORDIC_FM_DEMOD_BANK_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cordic_amd.h"
#include "cordic_bank_host.h"
#include "cordic_fm_demod.h"
#include "cordic_span_bank.h"

namespace cordic_amd {

// A run of whole vectors (4 samples) of ONE job, never across the job's end:
// at most P * 256 - 1 of them (P = 1, 2, 4, 8 passes of a 256-thread block, one
// lane of which converts the halo -- the vector in front of the run -- again).
struct DemodTile {
	uint64_t x, y;		// byte addresses of the run's first input vector
	uint64_t mag, freq;	// ... and of its first output vector
	uint64_t last;		// first == 1: the job's d_last, or 0
	uint32_t nvec;		// vectors: 1 .. P * 256 - 1
	uint32_t phase0;	// first == 1: the job's
	uint32_t first;		// 1: the run starts at sample 0 of its job, the
	uint32_t pad;		//    halo is (phase0 + *last) mod 2^PW
};				// 56 bytes

// (What the second launch does for a job whose length is no multiple of 4 or
// that has a d_last: DemodTail, cordic_fm_demod.h -- the single call's tail.)

constexpr uint32_t kFmdBankPassVecs = 256;
// vectors of a full tile of P passes
constexpr uint32_t fmd_bank_tile_vecs(int passes)
{
	return (uint32_t)passes * kFmdBankPassVecs - 1;
}
static_assert(kFmdTileVecs == fmd_bank_tile_vecs(kFmdPasses),
	"a tile of the single call is a bank's tile of 8 passes");

// P for a bank of `total_vecs` whole vectors on `cus` CUs: the tile-length rule
// (cordic_bank_host.h) with 8 resident blocks per CU, in the steps 1, 2, 4, 8.
inline int fmd_bank_passes(uint64_t total_vecs, int cus)
{
	return (int)bank_passes(total_vecs, cus, 8, kFmdBankPassVecs, 8);
}

// The jobs of a create, of either struct (JobView, cordic_span_bank.h)
typedef JobView<cordic_demod_job, cordic_demod_job16> DemodJobs;
#define F(f) CORDIC_SAME_FIELD(cordic_demod_job, cordic_demod_job16, f)
static_assert(sizeof(cordic_demod_job) == 56 && F(d_xval) && F(d_yval) && F(d_omag)
	&& F(d_ofreq) && F(d_last) && F(n) && F(phase0) && F(reserved),
	"cordic_demod_job16 is cordic_demod_job with 16-bit sample pointers");
#undef F

// The argument checks of cordic_demodbank_create / _create16 that need no
// device (bank_jobs_valid, cordic_span_bank.h): the four sample arrays
// required, d_last optional; the outputs are d_omag, d_ofreq and the word at
// d_last.
inline bool fmd_bank_jobs_valid(size_t njobs, DemodJobs jobs)
{
	return bank_jobs_valid(njobs, jobs,
		[](const cordic_demod_job &jb, uint64_t es, const void **word) {
			*word = jb.d_last;
			return std::array<JobArray, 4>{{{jb.d_xval, es, true, false},
				{jb.d_yval, es, true, false}, {jb.d_omag, es, true, true},
				{jb.d_ofreq, es, true, true}}};
		});
}

// tiles of `tile_vecs` vectors the jobs cut into (saturating at 2^63)
inline uint64_t fmd_bank_count_tiles(size_t njobs, DemodJobs jobs, uint32_t tile_vecs)
{
	uint64_t t = 0;
	for (size_t k = 0; k < njobs; k++) {
		t += (jobs.n(k) / 4 + tile_vecs - 1) / tile_vecs;
		if (t >> 63)
			break;
	}
	return t;
}

// Cuts valid jobs (fmd_bank_jobs_valid) into tiles, in the jobs' order, and
// tails, one per job that needs the second launch.  The descriptors hold byte
// addresses: a vector is 4 * esize bytes (16 or 8), a sample esize (4 or 2).
inline void fmd_bank_cut(size_t njobs, DemodJobs jobs, uint32_t tile_vecs,
		std::vector<DemodTile> *tiles, std::vector<DemodTail> *tails)
{
	const uint64_t es = jobs.esize();
	for (size_t k = 0; k < njobs; k++) {
		const cordic_demod_job jb = jobs[k];
		if (jb.n == 0)
			continue;
		const uint64_t x = (uintptr_t)jb.d_xval, y = (uintptr_t)jb.d_yval,
			m = (uintptr_t)jb.d_omag, f = (uintptr_t)jb.d_ofreq,
			l = (uintptr_t)jb.d_last;
		const uint64_t nvec = jb.n / 4;
		for (uint64_t v0 = 0; v0 < nvec; v0 += tile_vecs) {
			const uint64_t live = nvec - v0 < tile_vecs ? nvec - v0 : tile_vecs;
			const uint64_t at = v0 * 4 * es;
			tiles->push_back(DemodTile{x + at, y + at, m + at, f + at,
				v0 ? 0 : l, (uint32_t)live, v0 ? 0u : jb.phase0,
				v0 ? 0u : 1u, 0u});
		}
		if (nvec * 4 == jb.n && !l)
			continue;
		const uint64_t s0 = nvec ? nvec * 4 - 1 : 0, at = s0 * es;
		tails->push_back(DemodTail{x + at, y + at, m + at, f + at, l,
			(uint32_t)(jb.n - s0), jb.phase0, nvec ? 0u : 1u, 0u});
	}
}

// The two launches.  grid: blocks of the main kernel (1 .. ntiles).  io16: the
// descriptors were cut from 16-bit jobs.  An empty table launches nothing.
// CORDIC_OK or CORDIC_ERR_DEVICE.
int	launch_fmd_bank(const cordic_config &cfg, const DemodTile *d_tiles,
		uint32_t ntiles, int grid, const DemodTail *d_tails, uint32_t ntails,
		bool io16, void *stream);

} // namespace cordic_amd
#endif
