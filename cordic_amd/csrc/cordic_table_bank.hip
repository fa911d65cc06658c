// cordic_table_bank.hip -- oscillator banks: many oscillator jobs of one table
// or quadratic core (each cordic_table_nco / cordic_quad_nco with a phase0 /
// fcw / index0 / length / output arrays of its own) as ONE store-only launch.
//
// oscbank_create (cordic_abi_table.cpp) cuts every output stream -- a job's
// d_sin is one, its d_cos another -- on its own address into [head | 16-byte
// aligned vectors | tail], the cut cordic_table_nco.hip makes in its kernel.
// The aligned part becomes tiles (OscTile: whole vectors of one stream), sorted
// by destination address so that HBM sees ascending write spans across the
// bank; heads and tails go to an edge list (OscEdge) that the SAME launch
// writes behind its tiles with scalar stores.  Tunings (phase0, fcw, index0)
// stay in a per-job array that tiles name by job index: cordic_oscbank_retune
// rewrites that array and nothing else.
//
// Kernel: persistent 1024-thread blocks stage the core's table ONCE (the
// layouts of cordic_table_nco.h: L2 gather full- / quarter-wave, packed int16
// or 32-bit entries in LDS in both folds, the quadratic core's {C, L, Q, 0}),
// then pull TICKETS from the handle's address-ordered tile queue
// (dev::for_each_queued_tile<1024>); without a queue every block takes one
// contiguous chunk of tickets.  A lane makes one 16-byte vector of outputs (4
// int32 or 8 int16) and stores it non-temporally.  A tile is one stream, so
// there is no sine / quadrature instance: layouts x {int32, int16}, the int16
// ones only for the layouts that serve OW <= 16.
//
// Tile length.  A tile holds up to T = 2^tile_shift vectors, 64 <= T <= 1024,
// and a ticket is 1024 / T consecutive tiles worked side by side by groups of
// T lanes (whole waves: the tile index is wave-uniform, so descriptor and
// tuning come through the scalar cache).  All 1024 lanes therefore have work
// whatever T is, and T decides only how finely ragged streams pack into lanes
// against how long the tile table gets (24 bytes per tile):
//   T = the largest power of two with
//       T <= mean whole vectors per stream, rounded up to a power of two
//                                     (a tile never crosses a stream's end: a
//                                     bank of 64-vector streams gets 64-vector
//                                     tiles, 16 of them per ticket, not 1024-lane
//                                     tickets with 64 lanes at work)
//       T <= total whole vectors / (4 x resident blocks)
//                                     (the job sets' xy_tile_vecs term, kept for
//                                     what it still does here: it does NOT spread
//                                     a small bank over more CUs -- a ticket is
//                                     1024 lanes whatever T is -- but a bank that
//                                     small has few tiles either way, so the short
//                                     tiles cost no table space and pack the ends
//                                     of its ragged streams into fewer idle lanes;
//                                     big banks keep 1024 and a short tile table)
//   clamped to 64 .. 1024.
//
// Grid.  min(tickets, resident blocks), at least one (the edges); resident =
// CUs x the single call's per-CU cap (two blocks where two LDS copies fit, one
// for the 128 KiB tables).  Never more blocks than tickets.  A small bank is
// NOT given fewer blocks than that to save stagings.  The reason is an
// ESTIMATE, not a measurement: every block stages in parallel out of L2 (the
// table is at most 128 KiB and should be L2-resident once the first block has
// read it), so the stagings ought to overlap in wall time, while fewer blocks
// would queue the tickets' stores behind one another on fewer CUs.  The price is
// L2 read traffic of (blocks x table) for a bank that stores little.  Nobody
// has measured either side of this yet; the 16384 x 2^8 shape of
// tools/bench_table_bank.py (256 tickets of int32 sine on up to 256 blocks) is
// the one to judge it by.
//
// Bounds: every address the kernel stores to comes out of the tile and edge
// tables; the host builds them from [d, d + n) of each stream and checks at
// create that no two streams of the bank overlap.
#include <hip/hip_runtime.h>

#include "cordic_table_bank.h"
#include "cordic_table_nco.h"
#include "cordic_jobs_fused.h"

namespace cordic_amd {

namespace tbank {

using namespace tnco;
using dev::for_each_queued_tile;

struct BankArgs {
	const OscTile *tiles;
	const OscEdge *edges;
	const cordic_osc_tuning *tun;
	uint32_t ntiles, nedges, ntickets;
	uint32_t tile_shift;
	uint32_t index_offset;
};

template <typename CORE, typename T>
__global__ __launch_bounds__(1024) void table_bank(CORE core, BankArgs a,
		uint32_t *queue)
{
	typedef typename OutVec<T>::type V;
	constexpr uint32_t W = 16 / sizeof(T);
	// the tables hold addresses of device memory as integers: say so, or the
	// stores become flat ones (which also count as LDS traffic in flight)
	typedef V __attribute__((address_space(1))) GV;
	typedef T __attribute__((address_space(1))) GT;
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ uint32_t slot[3];
	const typename CORE::entry *tab = core.stage(lds_raw);

	// phase of sample `first` of job `job` (PW <= 32: the low 32 bits of the
	// sample index are all that matters)
	auto phase_of = [&](const cordic_osc_tuning &tu, uint32_t first, uint32_t lead) {
		return tu.phase0 + lead
			+ ((uint32_t)tu.index0 + a.index_offset + first) * tu.fcw;
	};
	const uint32_t per = 1024u >> a.tile_shift;		// tiles per ticket
	const uint32_t sub = threadIdx.x >> a.tile_shift;
	const uint32_t g = threadIdx.x & ((1u << a.tile_shift) - 1u);
	auto ticket = [&](uint32_t t) {
		// (tile_shift >= 6: uniform over the wave)
		const uint32_t tile = __builtin_amdgcn_readfirstlane(t * per + sub);
		if (tile >= a.ntiles)
			return;
		const OscTile d = a.tiles[tile];
		if (g >= d.nvec)
			return;
		const cordic_osc_tuning tu = a.tun[d.job];
		uint32_t p = phase_of(tu, d.first + g * W, d.lead);
		V o;
#pragma unroll
		for (uint32_t v = 0; v < W; v++, p += tu.fcw)
			o[v] = (T)core.sample(tab, p);
		__builtin_nontemporal_store(o, reinterpret_cast<GV *>(d.base) + g);
	};
	if (queue) {
		for_each_queued_tile<1024>(queue, slot, a.ntickets, ticket);
	} else {
		const uint32_t chunk = (a.ntickets + gridDim.x - 1) / gridDim.x;
		const uint64_t lo = (uint64_t)blockIdx.x * chunk;
		const uint64_t hi = lo + chunk < a.ntickets ? lo + chunk : a.ntickets;
		for (uint64_t t = lo; t < hi; t++)
			ticket((uint32_t)t);
	}
	// heads and tails of the streams: fewer than W samples each
	for (uint64_t e = (uint64_t)blockIdx.x * 1024u + threadIdx.x; e < a.nedges;
			e += (uint64_t)gridDim.x * 1024u) {
		const OscEdge d = a.edges[e];
		const cordic_osc_tuning tu = a.tun[d.job];
		uint32_t p = phase_of(tu, d.first, d.lead);
		GT *dst = reinterpret_cast<GT *>(d.addr);
		for (uint32_t k = 0; k < d.count; k++, p += tu.fcw)
			dst[k] = (T)core.sample(tab, p);
	}
}

static BankArgs args_of(const BankTables &b, uint32_t index_offset)
{
	const uint32_t per = 1024u >> b.tile_shift;
	return BankArgs{b.tiles, b.edges, b.tunings, b.ntiles, b.nedges,
		(uint32_t)(((uint64_t)b.ntiles + per - 1) / per), b.tile_shift,
		index_offset};
}

// blocks of a CU that hold the core's table at the same time: the single
// call's cap (cordic_table_nco.hip: launch_one); 0: the LDS copy does not fit
static int per_cu_of(size_t lds_bytes)
{
	// (+ the kernel's static tile-id slots)
	return lds_blocks_per_cu(lds_bytes + 64);
}

template <typename CORE, typename T>
bool launch_one(const CORE &core, const BankArgs &a, size_t lds_bytes,
		hipStream_t st, uint32_t *queue)
{
	const int per_cu = per_cu_of(lds_bytes);
	if (per_cu < 1 || !allow_lds((const void *)table_bank<CORE, T>, lds_bytes + 64))
		return false;
	const int cus = jobs_cus_now();
	if (cus < 0)
		return false;
	const uint64_t cap = (uint64_t)cus * (uint64_t)per_cu;
	const uint64_t want = a.ntickets ? a.ntickets : 1;
	const int grid = (int)(want < cap ? want : cap);
	hipLaunchKernelGGL((table_bank<CORE, T>), dim3(grid), dim3(1024), lds_bytes,
		st, core, a, queue);
	return true;
}

} // namespace tbank

uint32_t bank_tile_shift(uint64_t total_vecs, uint64_t streams, uint64_t resident)
{
	if (resident == 0) resident = 1;
	const uint64_t mean = streams ? (total_vecs + streams - 1) / streams : 0;
	uint32_t shift = 10;
	while (shift > 6 && ((total_vecs >> shift) < 4 * resident
			|| mean <= ((uint64_t)1 << (shift - 1))))
		shift--;
	return shift;
}

int sine_bank_resident(const SineCore &c)
{
	// (a copy that does not fit is not staged: the L2 gather, two blocks)
	const int per_cu = tbank::per_cu_of(c.lds_bytes());
	const int cus = jobs_cus_now();
	return cus < 0 ? -1 : cus * (per_cu >= 1 ? per_cu : 2);
}

int launch_sine_bank(const SineCore &c, const BankTables &bank,
		uint32_t index_offset, bool io16, void *stream, uint32_t *queue)
{
	using namespace tbank;
	(void)hipGetLastError();	// (a stale error is not this launch's)
	if (io16 && c.ow() > 16) return CORDIC_ERR_CONTAINER;
	if (bank.ntiles == 0 && bank.nedges == 0) return CORDIC_OK;
	if (!c.sane() || !bank.tunings || (bank.ntiles && !bank.tiles)
			|| (bank.nedges && !bank.edges) || bank.tile_shift < 6
			|| bank.tile_shift > 10)
		return CORDIC_ERR_ARGS;
	hipStream_t st = static_cast<hipStream_t>(stream);
	const BankArgs a = args_of(bank, index_offset);
	return with_layout(c, io16, [&](const auto &core, auto tag, size_t bytes) {
		return launch_one<std::decay_t<decltype(core)>, decltype(tag)>(core, a,
			bytes, st, queue);
	});
}

} // namespace cordic_amd
