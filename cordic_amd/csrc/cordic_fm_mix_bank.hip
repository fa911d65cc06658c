// cordic_fm_mix_bank.hip -- FM mixer banks (cordic_mixbank_create, _create16,
// _destroy, _info, _run; include/cordic_amd.h): many cordic_plan_fm_mix (or
// cordic_plan_fm_mix16) jobs of one plan,
// each with its own arrays, length, phase0 and d_acc, in TWO launches.  The
// single call's reduce-then-scan (cordic_fm_mix.hip) reading span descriptors
// (MixSpan, cordic_fm_mix_bank.h): the host has cut every job into spans of
// whole 1024-sample passes, never across a job's end, a job into at most 4096.
//   1. span_reduce<MixSpan, 256> (cordic_span_reduce.h, where launch 1 and the
//      descriptor's head are described for both prefix-sum banks): a span of
//      one pass is one pass of one block, 256 lanes, one 16-byte load each.
//   2. fm_mixbank_xydir<LJ, NLIVE>: at most the resident blocks.  A block
//      stages the plan's direction tables ONCE (fmx::block_begin / block_ready,
//      the single call's prologue), then walks spans b, b + grid, ... in the
//      table's order, which is the jobs' own.  Per span the descriptor arrives
//      as scalar loads; the block adds the job's partials in
//      front of the span to the job's start word (front_sum, as the single
//      call's prologue; skipped for a job's first span) and runs pass_loop
//      (cordic_fm_mix.h), the loop fm_mix_xydir runs as well: 16-byte accesses
//      at any 4-byte alignment, lane sums / DPP wave scan / four LDS words with
//      ONE barrier per pass, the carry in a register, the next pass's loads in
//      flight, the n % 4 trailing samples by one lane.  The job's last span
//      writes *d_acc.
// Every *d_acc is read in launch 1 only and written in launch 2 only, which
// follows in stream order; the workspace is written in launch 1 only.  No block
// waits for another, nothing is allocated, copied or synchronised at run, no
// tile queue.  Nothing outside [0, n) of an output is written: a span's hi is
// its own sample count and pass_loop touches nothing at or behind it.
//
// LDS words across spans.  The parity `par` of the exchange words ex[0 .. 8)
// is CARRIED ON from span to span, so a block's passes form one sequence,
// whatever jobs they belong to, and the single call's argument holds as it
// stands: the four words written in pass i are read behind barrier i and in
// front of barrier i + 1, and written again in pass i + 2, which a wave reaches
// only through barrier i + 1 -- when every wave has its reads of pass i behind
// it.  (A barrier between spans would do too, but a job's first span has none
// to offer: it skips the prologue.)  The shares ex[8 .. 12) of a span's
// prologue are written in front of the prologue's barrier and read behind it,
// in front of the span's first pass barrier; the next prologue writes them only
// behind that pass barrier (every span has a pass), so no share is overwritten
// while a slower wave still reads it.  The carry is set anew per span from the
// job's start word and partials: nothing of the span before survives in it.
//
// The base span is P passes, chosen at create -- span_base_units
// (cordic_span_bank.h): the longest span, in the steps 1, 2, 4, 8, 16, ..., that
// still gives every resident block four -- or forced by CORDIC_FMXB_PASSES; a job that would have more than 4096 spans
// (CORDIC_FMXB_MAX_SPANS lowers that; both read at create) gets spans twice,
// four times, ... as long, that job alone.  Launch 2's grid is min(spans, CUs *
// resident blocks per CU), capped further by CORDIC_FMXB_MAX_BLOCKS (read at
// every run).  The bits depend on none of the three.
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps;
// .private_segment_fixed_size is 0 for every instance: nothing spills), next to
// the single call's, before and after pass_loop became a shared function:
//   live stages                 13   16   19   20   24   27   29
//   fm_mix_xydir<29, N> before  98  100   98   98  104  108  108
//   fm_mix_xydir<29, N> after   98  100   98   98  104  108  108
//   fm_mixbank_xydir<29, N>    114  120  114  114  115  122  122
//   fm_mix_xydir<30, N> before  92   98   95   95  102  103  103
//   fm_mix_xydir<30, N> after   92   98   95   95  102  103  103
//   fm_mixbank_xydir<30, N>    115  117  116  116  115  124  124
//   ... <30, N, Io16>          111  113  112  112  112  120  120
//   ... <30, N, IoC16io>       111  113  112  112  111  112  112
//   span_reduce<MixSpan, 256>   42 (32 bytes of static LDS)
// The single call's counts did not move.  The bank's kernel takes 12 .. 23
// more: six array addresses, the sample count and the indices arrive per span
// where the single call has them as kernel arguments, and the lane's element
// offsets are made from them anew.  Up to 128 registers hold 4 waves per SIMD,
// the single call's occupancy: no step is crossed, and the grid is sized for 4
// blocks per CU; LDS (the tables, at most 64 KiB, and 12 words) decides where
// it admits fewer, exactly as in launch_fm_mix.
//
// The container of the four sample arrays (Io32 / Io16, the third template
// parameter) reaches pass_loop and nothing else here: MixSpan holds byte
// addresses, which the host's cutter advances by 2 or 4 bytes per sample, and
// span_reduce reads tuning words only.  The table was taken again with
// the parameter in place: the 32-bit rows did not move, and no Io16 instance
// (LJ = 30 only, see fmx_is_fused16) spills.  IoC16io: a bank of interleaved
// jobs (cordic_mixbank_create_c16) -- a span's x is its d_iq, its ox its d_oiq,
// y and oy are 0 (span_place); the instances are in cordic_fm_mix_bank_c16.o,
// this source compiled with -DCORDIC_FMX_C16, behind launch_fmx_bank_walk_c16
// (cordic_fm_mix_bank.h).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_xydir.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_hostargs.h"
#include "cordic_fm_mix.h"
#include "cordic_fm_mix_bank.h"
#include "cordic_span_reduce.h"

namespace cordic_amd {

static_assert(kFmxbRule.unit == kFmxPass && kFmxbRule.max_spans == kFmxMaxBlocks
	&& (size_t)kFmxbBlocksPerCu == kFmxBlocksPerCu, "the single call's geometry");
static_assert(dev::kBlock == 256, "launch 1 is instantiated at the block of launch 2");

namespace fmx {

// launch 2 (see the head of this file)
template <int LJ, int NLIVE, typename IO>
__global__ __launch_bounds__(kBlock) void fm_mixbank_xydir(CoreParams kp, DirArgs da,
		const MixSpan *__restrict__ spans, uint32_t nspans,
		const uint32_t *__restrict__ start, const uint32_t *__restrict__ part,
		uint32_t xw)
{
	typedef typename IO::ielem ielem;
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const unsigned tid = threadIdx.x;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	uint32_t bk_base[kDxMaxLevels] = {}, lf_base[kDxMaxLevels] = {};
	dx_lds_layout(da.dx, bk_base, lf_base);
	block_begin<LJ, NLIVE, IO>(kp, da, lds, bk_base, lf_base, tid);
	uint32_t *ex = lds + xw / 4u;
	__syncthreads();
	const RotRegs rr = block_ready<LJ, NLIVE>(kp, da, lds);
	unsigned par = 0;
	for (uint32_t t = blockIdx.x; t < nspans; t += gridDim.x) {
		const MixSpan d = spans[t];
		// the phase of the span's first sample, without its pm
		uint32_t carry = start[d.start];
		if (d.idx) {		// (block-uniform)
			front_sum(part + d.part0, d.idx, ex, tid, wave);
			__syncthreads();
			carry += ex[8] + ex[9] + ex[10] + ex[11];
		}
		pass_loop<LJ, NLIVE>(kp, da, rr, bk_base,
			reinterpret_cast<const uint32_t *>((uintptr_t)d.fcw),
			reinterpret_cast<const uint32_t *>((uintptr_t)d.pm),
			reinterpret_cast<const ielem *>((uintptr_t)d.x),
			reinterpret_cast<const ielem *>((uintptr_t)d.y),
			reinterpret_cast<ielem *>((uintptr_t)d.ox),
			reinterpret_cast<ielem *>((uintptr_t)d.oy), (size_t)0, (size_t)d.n,
			carry, par, ex, tid, wave, IO{});
		if ((d.flags & kSpanLast) && d.acc && tid == 0)
			*reinterpret_cast<uint32_t *>((uintptr_t)d.acc) = carry;
	}
}

// launch 2 for one <LJ, container>; false: no instance for nlive
template <int LJ, typename IO>
static bool launch_walk(int nlive, int ngroups, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const MixSpan *d_spans, uint32_t nspans,
		const uint32_t *d_start, const uint32_t *d_part, uint32_t xw)
{
	return with_stages(nlive, ngroups, [&](auto nl) {
		hipLaunchKernelGGL((fm_mixbank_xydir<LJ, decltype(nl)::value, IO>), dim3(grid),
			dim3(kBlock), lds, st, kp, da, d_spans, nspans, d_start, d_part, xw);
	});
}

} // namespace fmx

#ifdef CORDIC_FMX_C16
// This object (cordic_fm_mix_bank_c16.o): the kernel's <30, N, IoC16io>
// instances and their launcher, nothing of the host side.
bool launch_fmx_bank_walk_c16(int nlive, int ngroups, unsigned grid, size_t lds,
		void *stream, const dev::CoreParams &kp, const dev::DirArgs &da,
		const MixSpan *d_spans, uint32_t nspans, const uint32_t *d_start,
		const uint32_t *d_part, uint32_t xw, uint32_t log2r)
{
	(void)log2r;
	return fmx::launch_walk<30, fmx::IoC16io>(nlive, ngroups, grid, lds,
		static_cast<hipStream_t>(stream), kp, da, d_spans, nspans, d_start, d_part, xw);
}
#else
int launch_fmx_bank(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		const MixSpan *d_spans, uint32_t nspans, uint32_t *d_start,
		uint32_t *d_part, int cus, bool io16, void *stream, uint32_t log2r, bool iq)
{
	using namespace fmx;
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (nspans == 0)
		return CORDIC_OK;
	hipStream_t st = static_cast<hipStream_t>(stream);
	uint32_t xw = 0;
	const size_t lds = lds_bytes(dx, &xw);
	// launch 1 has 8 waves a SIMD: 8 blocks of 4 waves a CU
	const SpanGrids g = span_grids(nspans, cus, 8, "CORDIC_FMXB_MAX_BLOCKS",
		blocks_per_cu(lds));
	hipLaunchKernelGGL((span_reduce<MixSpan, 256>), dim3(g.reduce), dim3(256), 0, st,
		d_spans, nspans, d_start, d_part);
	const unsigned grid = g.walk;
	const DirArgs da{d_dir, dx};
	const CoreParams kp = make_params_jobs(cfg);
	// iq: the spans' x is d_iq, their ox d_oiq, y and oy are 0 (span_place)
	const Unit unit = unit_of(cfg.ww, io16 ? 2 : 4, iq);
	if (log2r)	// a decimating bank's walk (cordic_fm_mix_bank_decim.hip)
		return tnco::finish(launch_fmx_bank_decim_walk(unit, cfg.nlive, dx.n, grid, lds,
			stream, kp, da, d_spans, nspans, d_start, d_part, xw, log2r));
	if (unit == kUnitC16)	// (cordic_fm_mix_bank_c16.o)
		return tnco::finish(launch_fmx_bank_walk_c16(cfg.nlive, dx.n, grid, lds, stream,
			kp, da, d_spans, nspans, d_start, d_part, xw, 0));
	const bool done = with_unit(unit, [&](auto lj, auto io) {
		return launch_walk<decltype(lj)::value, decltype(io)>(cfg.nlive, dx.n, grid, lds,
			st, kp, da, d_spans, nspans, d_start, d_part, xw);
	});
	return tnco::finish(done);
}
#endif // CORDIC_FMX_C16

} // namespace cordic_amd
