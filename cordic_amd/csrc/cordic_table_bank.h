// cordic_table_bank.h -- oscillator banks: many cordic_table_nco /
// cordic_quad_nco jobs of one core in ONE launch (include/cordic_amd.h,
// "oscillator banks").  The tables the host cuts at create
// (cordic_abi_table.cpp) and the launcher of the kernel that walks them
// (cordic_table_bank.hip), on the core a SineCore (cordic_table_nco.h) names.
// Host-visible types only.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_TABLE_BANK_H
#define CORDIC_TABLE_BANK_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_table_nco.h"

namespace cordic_amd {

// One run of whole 16-byte vectors of ONE output stream (a job's d_sin or its
// d_cos), never across the stream's end.  Sample v of vector g is sample
// first + g * W + v of job `job` (W = 4 int32 or 8 int16 per vector).
struct OscTile {
	uint64_t base;		// address of vector 0: 16-byte aligned
	uint32_t first;		// low 32 bits of its sample index in the job
	uint32_t nvec;		// vectors: 1 .. tile length
	uint32_t job;		// index into the tunings
	uint32_t lead;		// 0: sine; 2^(PW-2): cosine
};

// What is left of a stream in front of its first 16-byte boundary or behind
// its last whole vector: fewer than W samples, written with scalar stores.
struct OscEdge {
	uint64_t addr;		// of the first sample
	uint32_t first;		// low 32 bits of its sample index in the job
	uint32_t count;		// samples: 1 .. W-1
	uint32_t job;
	uint32_t lead;
};

struct BankTables {
	const OscTile *tiles = nullptr;		// sorted by base
	const OscEdge *edges = nullptr;
	const cordic_osc_tuning *tunings = nullptr;	// per job
	uint32_t ntiles = 0, nedges = 0;
	uint32_t tile_shift = 10;	// tile length = 2^tile_shift vectors (6 .. 10)
};

// Tile length (log2, vectors) for a bank of `total_vecs` whole vectors in
// `streams` non-empty streams on `resident` blocks; the rule is set out in
// cordic_table_bank.hip.
uint32_t bank_tile_shift(uint64_t total_vecs, uint64_t streams, uint64_t resident);
// blocks of the current device that hold the core's table at the same time
// (the single call's per-CU cap x its CUs); < 0: no device
int	sine_bank_resident(const SineCore &c);

// The whole bank in one launch on the layout launch_sine_nco would choose.
// index_offset: low 32 bits of the run-wide addend to every job's index0.
// queue: a tile-queue block, or NULL for one contiguous chunk of tiles per
// block.  An empty bank launches nothing.
int	launch_sine_bank(const SineCore &c, const BankTables &bank,
		uint32_t index_offset, bool io16, void *stream, uint32_t *queue);

} // namespace cordic_amd
#endif
