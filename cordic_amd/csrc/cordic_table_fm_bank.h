// cordic_table_fm_bank.h -- FM oscillator banks: many cordic_table_fm /
// cordic_quad_fm jobs of one sine core in TWO launches (include/cordic_amd.h,
// "FM oscillator banks"), on int32 or on int16 outputs (cordic_fmosc_job /
// cordic_fmosc_job16).  The span descriptors the host cuts at create, the cutter
// itself -- plain C++ that touches no device, so that a stand-alone program can
// run it under a sanitizer (tests/test_fm_osc_bank_host.py) -- and the launcher
// of the two kernels that walk the descriptors (cordic_table_fm_bank.hip).
// Host-visible types only; the handle and its seven entry points live with the
// cores, in cordic_abi_table.cpp.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_TABLE_FM_BANK_H
#define CORDIC_TABLE_FM_BANK_H

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "cordic_amd.h"
#include "cordic_bank_host.h"

namespace cordic_amd {

// A run of whole tiles (4096 samples, kFmTile) of ONE job, never across the
// job's end; only a job's last span may end in a partial tile.
struct FmSpan {
	uint64_t fcw, pm;	// addresses at the span's first sample (pm 0: none)
	uint64_t sin, cos;	// (cos 0: sine only)
	uint64_t acc;		// the job's d_acc, or 0
	uint64_t n;		// samples: >= 1
	uint32_t start;		// index of the job's start word
	uint32_t part0;		// index of the job's first partial sum
	uint32_t idx;		// this span's index within its job
	uint32_t flags;		// kFmSpanFirst | kFmSpanLast
	uint32_t phase0;	// the job's (the first span latches the start)
	uint32_t pad;
};				// 72 bytes
static_assert(sizeof(FmSpan) == 72, "the descriptor is read as scalar words");
constexpr uint32_t kFmSpanFirst = 1, kFmSpanLast = 2;

constexpr uint64_t kFmobTile = 4096;		// = kFmTile
constexpr uint32_t kFmobMaxSpans = 1024;	// per job; = kFmMaxBlocks
constexpr uint32_t kFmobMaxTiles = 1u << 18;	// a base span's: 2^30 samples

inline uint64_t fmob_tiles_of(uint64_t n)
{
	return n / kFmobTile + (n % kFmobTile ? 1 : 0);
}

// T, the tiles of a base span, for a bank of `total_tiles` on `cus` CUs with
// `blocks_per_cu` resident blocks each: the tile-length rule
// (cordic_bank_host.h), steps 1, 2, 4, ...
inline uint32_t fmob_tiles(uint64_t total_tiles, int cus, int blocks_per_cu)
{
	return bank_passes(total_tiles, cus, blocks_per_cu > 0 ? blocks_per_cu : 1, 1,
		kFmobMaxTiles);
}

// CORDIC_FMOB_TILES / CORDIC_FMOB_MAX_SPANS (read at create): a power of two
// within 1 .. 2^18 replaces T; a value within 1 .. 1023 lowers the span cap.
inline uint32_t fmob_forced_tiles(const char *e, uint32_t t)
{
	return bank_forced_passes(e, kFmobMaxTiles, t);
}
inline uint32_t fmob_forced_cap(const char *e)
{
	const long v = e ? std::strtol(e, nullptr, 10) : 0;
	return (v >= 1 && v < (long)kFmobMaxSpans) ? (uint32_t)v : kFmobMaxSpans;
}

// tiles per span of ONE job of n samples: T, doubled until the job has at most
// `cap` spans -- the single call's bound on what a span sums in front of
// itself, one partial per thread
inline uint64_t fmob_job_tiles(uint64_t n, uint32_t tiles, uint32_t cap)
{
	const uint64_t nt = fmob_tiles_of(n);
	uint64_t tj = tiles;
	while ((nt + tj - 1) / tj > cap)
		tj *= 2;
	return tj;
}

// The jobs of a create, of either struct: cordic_fmosc_job16 is
// cordic_fmosc_job field for field but for the element type behind the two
// output pointers, which the host never dereferences.  jobs[k] is job k as a
// cordic_fmosc_job; esize() the bytes of a sample, which is all the checks and
// the cutter know of the container.
struct FmJobs {
	const cordic_fmosc_job *j32 = nullptr;
	const cordic_fmosc_job16 *j16 = nullptr;
	FmJobs(const cordic_fmosc_job *j) : j32(j) {}
	FmJobs(const cordic_fmosc_job16 *j) : j16(j) {}
	FmJobs(std::nullptr_t) {}
	uint64_t esize() const { return j16 ? 2 : 4; }
	uint64_t n(size_t k) const { return j16 ? j16[k].n : j32[k].n; }
	bool	quadrature(size_t k) const
	{
		return j16 ? j16[k].d_cos != nullptr : j32[k].d_cos != nullptr;
	}
	cordic_fmosc_job operator[](size_t k) const
	{
		if (!j16)
			return j32[k];
		const cordic_fmosc_job16 &a = j16[k];
		cordic_fmosc_job b;
		b.d_fcw = a.d_fcw;
		b.d_pm = a.d_pm;
		b.d_sin = reinterpret_cast<int32_t *>(a.d_sin);
		b.d_cos = reinterpret_cast<int32_t *>(a.d_cos);
		b.d_acc = a.d_acc;
		b.n = a.n;
		b.phase0 = a.phase0;
		b.reserved = a.reserved;
		return b;
	}
};

// The argument checks of the four creates that need no device: every job with
// n > 0 has non-NULL d_fcw and d_sin, d_sin and d_cos on the grid of their
// element (4 or 2 bytes), d_fcw, d_pm and d_acc on the 4-byte grid, reserved ==
// 0 and a length within SIZE_MAX >> 4; no output range (d_sin, d_cos, the word
// at d_acc) overlaps another output range or any input range of the bank
// (BankRanges, cordic_bank_host.h), by the true byte ranges: n * esize for an
// output array, n * 4 for d_fcw / d_pm.
inline bool fmob_jobs_valid(size_t njobs, FmJobs jobs)
{
	const uint64_t es = jobs.esize();
	BankRanges r;
	for (size_t k = 0; k < njobs; k++) {
		const cordic_fmosc_job jb = jobs[k];
		if (jb.n == 0)
			continue;
		// inputs, then outputs; pm and cos are optional
		const uintptr_t p[4] = {(uintptr_t)jb.d_fcw, (uintptr_t)jb.d_pm,
			(uintptr_t)jb.d_sin, (uintptr_t)jb.d_cos};
		const uintptr_t a = (uintptr_t)jb.d_acc;
		if (!p[0] || !p[2] || ((p[0] | p[1] | a) & 3u) || ((p[2] | p[3]) & (es - 1))
				|| jb.reserved != 0 || jb.n > (~(size_t)0 >> 4))
			return false;
		for (int i = 0; i < 4; i++)
			if (p[i] && !r.add(p[i], jb.n * (i < 2 ? 4 : es), i >= 2))
				return false;
		if (a && !r.add(a, 4, true))
			return false;
	}
	return r.outputs_clear();
}

// spans the jobs cut into (saturating at 2^63)
inline uint64_t fmob_count_spans(size_t njobs, FmJobs jobs, uint32_t tiles,
		uint32_t cap)
{
	uint64_t t = 0;
	for (size_t k = 0; k < njobs; k++) {
		const uint64_t n = jobs.n(k);
		if (!n)
			continue;
		const uint64_t tj = fmob_job_tiles(n, tiles, cap);
		t += (fmob_tiles_of(n) + tj - 1) / tj;
		if (t >> 63)
			break;
	}
	return t;
}

// Cuts valid jobs (fmob_jobs_valid; fewer than 2^32 spans) into spans, in the
// jobs' order.  Start words are numbered by non-empty job, partial sums by
// span: the workspace of the run has *njobs_live + spans->size() words.  A
// span's addresses are byte addresses: its first sample is esize bytes per
// sample into the outputs and 4 into d_fcw / d_pm.
inline void fmob_cut(size_t njobs, FmJobs jobs, uint32_t tiles, uint32_t cap,
		std::vector<FmSpan> *spans, uint32_t *njobs_live)
{
	const uint64_t es = jobs.esize();
	uint32_t live = 0;
	for (size_t k = 0; k < njobs; k++) {
		const cordic_fmosc_job jb = jobs[k];
		if (jb.n == 0)
			continue;
		const uint64_t len = fmob_job_tiles(jb.n, tiles, cap) * kFmobTile;
		const uint32_t part0 = (uint32_t)spans->size();
		uint32_t idx = 0;
		for (uint64_t s0 = 0; s0 < jb.n; s0 += len, idx++) {
			const uint64_t cnt = jb.n - s0 < len ? jb.n - s0 : len;
			const uint64_t at = s0 * 4, sat = s0 * es;
			spans->push_back(FmSpan{(uintptr_t)jb.d_fcw + at,
				jb.d_pm ? (uintptr_t)jb.d_pm + at : 0,
				(uintptr_t)jb.d_sin + sat,
				jb.d_cos ? (uintptr_t)jb.d_cos + sat : 0,
				(uintptr_t)jb.d_acc, cnt, live, part0, idx,
				(s0 ? 0u : kFmSpanFirst)
					| (s0 + cnt == jb.n ? kFmSpanLast : 0u),
				jb.phase0, 0u});
		}
		live++;
	}
	if (njobs_live)
		*njobs_live = live;
}

// ---- the launcher (cordic_table_fm_bank.hip)
struct SineCore;	// (cordic_table_nco.h)

// What a create asks of the core: the blocks of launch 2 that one CU holds at a
// time on the layout that with_layout (cordic_table_nco.h) chooses for `c` --
// its fall-back to the L2 gather included -- into *blocks_per_cu.  CORDIC_OK;
// CORDIC_ERR_UNSUPPORTED: a quadratic core whose tables exceed 64 KiB;
// CORDIC_ERR_DEVICE: no layout serves the core.  The caller has checked
// c.sane() and the container.
int	fmob_resident(const SineCore &c, bool io16, int *blocks_per_cu);

// The two launches.  d_start / d_part: the bank's workspace (one word per
// non-empty job, one per span).  cus: the device's, at create.  An empty table
// launches nothing.  CORDIC_OK, CORDIC_ERR_DEVICE, or what fmob_resident
// answers.
int	launch_fmosc_bank(const SineCore &c, const FmSpan *d_spans, uint32_t nspans,
		uint32_t *d_start, uint32_t *d_part, int cus, bool io16, void *stream);

} // namespace cordic_amd
#endif
