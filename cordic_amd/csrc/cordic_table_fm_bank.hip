// cordic_table_fm_bank.hip -- FM oscillator banks (cordic_table_fmbank_create,
// cordic_quad_fmbank_create, their ...16 forms, cordic_fmbank_destroy, _info,
// _run; include/cordic_amd.h): many cordic_table_fm / cordic_quad_fm (or
// ...fm16) jobs of one core, each with its own tuning words, phase words,
// outputs, length, phase0 and d_acc, in TWO launches.  The single call's
// reduce-then-scan (cordic_table_fm.hip) reading span descriptors (FmSpan,
// cordic_table_fm_bank.h): the host has cut every job into spans of whole
// 4096-sample tiles, never across a job's end, a job into at most 1024.
//   1. span_reduce<FmSpan, 1024> (cordic_span_reduce.h, where launch 1 and the
//      descriptor's head are described for both prefix-sum banks): blocks of
//      1024 threads, so that a tile is one 16-byte load per lane.
//   2. table_fmbank<CORE, T>: at most the resident blocks, sized as the single
//      call sizes its grid (lds_blocks_per_cu of table + phases + static, per
//      CU).  A block stages the core's table ONCE, then walks spans b, b +
//      grid, ... in the table's order, which is the jobs' own.  Per span it adds
//      the job's partials in front of the span to the job's start word
//      (block_sum, as the single call's prologue; skipped for a job's first
//      span) and runs tile_loop (cordic_table_fm.h), the loop table_fm runs as
//      well, on [0, n) of the span.  d_cos == NULL and d_pm == NULL are
//      per-span uniform branches.  The job's last span writes *d_acc.
// Every *d_acc is read in launch 1 only and written in launch 2 only, which
// follows in stream order; the workspace is written in launch 1 only.  No block
// waits for another, nothing is allocated, copied or synchronised at run, no
// tile queue.  Nothing outside [0, n) of an output is written: a span's hi is
// its own sample count and tile_loop touches nothing at or behind it.
//
// LDS across spans.  A block's LDS is [the table | 8 + 4096 phases] and the 16
// words wsum, and a block's tiles form one sequence, whatever spans and jobs
// they belong to.
//   - A span's first tile never reads ph[0 .. 8), the phases of the tile
//     before it: emit starts its window at the span's first sample.  (Its
//     lanes 1022 and 1023 still move two stale vectors there; nobody reads
//     them.)
//   - The phases of span k's last tile are read by emit, behind that tile's
//     second barrier.  A lane of span k + 1 overwrites them only behind the
//     first barrier of its first tile (in front of which it writes wsum
//     alone), or behind the barriers of its prologue: either way a barrier
//     that every wave reaches only with its reads of span k behind it.
//   - wsum is free again after each block_sum (its second barrier), and after
//     a tile's second barrier: every reader of a tile's 16 words stands
//     between the tile's two barriers.  So the prologue of span k + 1 and the
//     first tile of a span without a prologue may write it at once.
//   - The carry is set anew per span from the job's start word and partials:
//     nothing of the span before survives in it.
//
// The base span is T tiles, chosen at create -- span_base_units
// (cordic_span_bank.h): the longest span, in the steps 1, 2, 4, ..., that still
// gives every resident block four -- or forced by CORDIC_FMOB_TILES; a job that would have more than 1024 spans
// (CORDIC_FMOB_MAX_SPANS lowers that; both read at create) gets spans twice,
// four times, ... as long, that job alone.  Launch 2's grid is min(spans, CUs *
// resident blocks per CU), capped further by CORDIC_FMOB_MAX_BLOCKS (read at
// every run).  The bits depend on none of the three.
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps;
// .private_segment_fixed_size is 0 for every instance: nothing spills), next to
// the single call's before and after its loop became the shared tile_loop.
// Instances by layout (CORE) and store type (i32 / i16):
//                       CoreLds<1,s16>  CoreLds<2,s16>  CoreLds<1,s32>  CoreLds<2,s32>
//                         i32    i16      i32    i16        i32             i32
//   table_fm before        61     61       61     61         61              61
//   table_fm after         53     55       53     55         53              53
//   table_fmbank           83     85       83     86         83              83
//                       CoreL2<true>    CoreL2<false>   CoreQuad        CoreIdent
//                         i32    i16      i32    i16      i32    i16        i32
//   table_fm before        61     61       61     59       63     63         61
//   table_fm after         53     55       53     55       53     55         53
//   table_fmbank           83     86       83     85       83     87         (none)
//   fm_reduce 48 before and after; span_reduce<FmSpan, 1024> 42 (128 bytes of
//   static LDS)
// table_fm stays within the 64 registers its comment promises.  (The loop lifted
// word for word, with 64-bit sample indices, took 57 .. 61 but spilled six more
// scalar registers into lanes and cost the single call 6 %; tile_loop counts in
// 32 bits inside a tile, see cordic_table_fm.h, and table_fm<CoreLds<2, s16>,
// i32> went from 1221 instructions and 32 lane spills to 1187 and 22.)  The
// bank's kernel takes 83 .. 87: the span's four array addresses, its sample
// count, indices and flags arrive per span where the single call has kernel
// arguments (all instances are at the 106 scalar registers the compiler allows
// itself), and the compiler, free to use 128 at 1024 threads a block,
// schedules more of a tile's loads and samples at once.  Above 64, ONE block of
// 1024 threads is resident on a CU where the single call has two wherever LDS
// admits two: the bank's barriers are not hidden behind a second block.  Asked
// for 64 (amdgpu_waves_per_eu(8, 8)) the instances spilled 52 .. 100 bytes,
// which is refused here.  The grid is still sized as the single call's, by LDS:
// blocks beyond the resident ones start as those end, and a block's share of
// the spans is the same either way.  The rates are in
// profiles/r19/fm_osc_bank.txt.
//
// The layout is with_layout's (cordic_table_nco.h), its fall-back to the L2
// gather where the LDS copy does not fit beside a tile's phases included: every
// core the single call serves is served here, in two launches.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_table_fm.h"
#include "cordic_table_fm_bank.h"
#include "cordic_table_nco.h"
#include "cordic_jobs_fused.h"
#include "cordic_hostargs.h"
#include "cordic_span_reduce.h"

namespace cordic_amd {

static_assert(kFmobRule.unit == kFmTile && kFmobRule.max_spans == kFmMaxBlocks,
	"the single call's geometry");

namespace tfm {

// what tile_loop reads of a span
struct SpanArgs {
	const uint32_t *fcw, *pm;	// pm may be NULL
	uint32_t quarter;		// 2^(PW-2): the cosine's lead
};

// launch 2 (see the head of this file).  Dynamic LDS: [the core's table | 8 +
// 4096 phases], as table_fm.
template <typename CORE, typename T>
__global__ __launch_bounds__(1024) void table_fmbank(CORE core,
		const FmSpan *__restrict__ spans, uint32_t nspans,
		const uint32_t *__restrict__ start, const uint32_t *__restrict__ part,
		uint32_t quarter, uint32_t table_bytes)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ uint32_t wsum[16];
	const unsigned tid = threadIdx.x;
	const typename CORE::entry *tab = core.stage(lds_raw);
	uint32_t *ph = reinterpret_cast<uint32_t *>(lds_raw + table_bytes);

	for (uint32_t t = blockIdx.x; t < nspans; t += gridDim.x) {
		const FmSpan d = spans[t];
		// the phase of the span's first sample, without its pm
		uint32_t carry = start[d.start];
		// (block-uniform; a job has at most 1024 spans: one partial per thread)
		if (d.idx)
			carry += block_sum(tid < d.idx ? part[d.part0 + tid] : 0u, wsum);
		const SpanArgs a{reinterpret_cast<const uint32_t *>((uintptr_t)d.fcw),
			reinterpret_cast<const uint32_t *>((uintptr_t)d.pm), quarter};
		tile_loop<CORE, T>(core, tab, ph, wsum, a,
			reinterpret_cast<T *>((uintptr_t)d.sin),
			reinterpret_cast<T *>((uintptr_t)d.cos), (size_t)0, (size_t)d.n, carry);
		if ((d.flags & kSpanLast) && d.acc && tid == 0)
			*reinterpret_cast<uint32_t *>((uintptr_t)d.acc) = carry;
	}
}

struct BankCall {
	const FmSpan *spans;
	uint32_t nspans;
	uint32_t *start, *part;
	int	cus;
	hipStream_t st;
	int	*per_cu;	// non-NULL: launch nothing, tell the resident blocks
};

// both launches for one layout, or (c.per_cu) what the layout holds per CU;
// false: the layout does not serve
template <typename CORE, typename T>
bool bank_one(const CORE &core, const BankCall &c, uint32_t quarter, size_t table_bytes)
{
	const size_t lds = table_bytes + kPhaseBytes;
	// (+ the kernel's static scratch)
	const int per_cu = lds_blocks_per_cu(lds + 128);
	if (per_cu < 1 || !allow_lds((const void *)table_fmbank<CORE, T>, lds + 128))
		return false;
	if (c.per_cu) {
		*c.per_cu = per_cu;
		return true;
	}
	// launch 1 has two blocks of 16 waves a CU
	const SpanGrids g = span_grids(c.nspans, c.cus, 2, "CORDIC_FMOB_MAX_BLOCKS",
		(size_t)per_cu);
	hipLaunchKernelGGL((span_reduce<FmSpan, 1024>), dim3(g.reduce), dim3(1024), 0, c.st,
		c.spans, c.nspans, c.start, c.part);
	hipLaunchKernelGGL((table_fmbank<CORE, T>), dim3(g.walk), dim3(1024), lds, c.st, core,
		c.spans, c.nspans, (const uint32_t *)c.start, (const uint32_t *)c.part,
		quarter, (uint32_t)table_bytes);
	return true;
}

static int bank_with_layout(const SineCore &c, bool io16, const BankCall &call)
{
	const uint32_t quarter = c.quarter();
	// (an LDS copy that does not fit beside the phases: the L2 gather)
	return with_layout(c, io16, [&](const auto &core, auto tag, size_t bytes) {
		return bank_one<std::decay_t<decltype(core)>, decltype(tag)>(core, call,
			quarter, bytes);
	});
}

} // namespace tfm

int fmob_resident(const SineCore &c, bool io16, int *blocks_per_cu)
{
	(void)hipGetLastError();
	const tfm::BankCall call{nullptr, 0, nullptr, nullptr, 0, nullptr, blocks_per_cu};
	return tfm::bank_with_layout(c, io16, call);
}

int launch_fmosc_bank(const SineCore &c, const FmSpan *d_spans, uint32_t nspans,
		uint32_t *d_start, uint32_t *d_part, int cus, bool io16, void *stream)
{
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (nspans == 0)
		return CORDIC_OK;
	const tfm::BankCall call{d_spans, nspans, d_start, d_part, cus,
		static_cast<hipStream_t>(stream), nullptr};
	return tfm::bank_with_layout(c, io16, call);
}

} // namespace cordic_amd
