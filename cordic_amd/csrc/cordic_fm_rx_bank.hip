// cordic_fm_rx_bank.hip -- receiver banks (cordic_rxbank_create, _create16,
// _destroy, _info, _run; include/cordic_amd.h): many cordic_plan_fm_rx (or
// cordic_plan_fm_rx16) jobs of one plan and one converter, each with its own
// arrays, length, phase0, dphase0, d_acc and d_last, in TWO launches.  The
// mixer banks' scheme (cordic_fm_mix_bank.hip) around the receiver's pass loop:
// the host has cut every job into spans of whole 1024-sample passes LESS the
// halo's 4 samples, never across a job's end, a job into at most 4096.
//   1. span_reduce<RxSpan, 256> (cordic_span_reduce.h): a span's tuning words
//      into a workspace word; a job's first span latches the start word and,
//      by span_latch_more below, dphase0 + *d_last.
//   2. fm_rxbank_xydir<LJ, NLIVE, IO>: at most the resident blocks.  A block
//      stages the plan's direction tables ONCE (fmx::block_begin / block_ready,
//      cordic_fm_mix.h), then walks spans b, b + grid,
//      ...: the job's partials in front of the span added to its start word
//      (front_sum; skipped for a job's first span), then fmrx::pass_loop
//      (cordic_fm_rx.h), the loop of the single call.  A span that is not its
//      job's first finds the vector in front of it inside the job: lane 0 of
//      its first pass is that halo.  The job's last span writes *d_acc and
//      *d_last.
// Every *d_acc and *d_last is read in launch 1 only and written in launch 2
// only; the workspace is written in launch 1 only.  No block waits for another,
// nothing is allocated, copied or synchronised at run, no tile queue.  Nothing
// outside [0, n) of an output is written.
//
// LDS words across spans: as in the mixer banks, the parity of the exchange
// words -- here the scan's AND the edge words -- runs on from span to span, so
// a block's passes form one sequence whatever jobs they belong to, and the
// shares of a span's prologue are written only behind the pass barriers of the
// span in front.  Wave 0's edge word of "the pass before" is, in a span's first
// pass, the span before's: it reaches lane 0 alone, the halo, which stores
// nothing.
//
// The converter's parameters come from device memory the bank uploaded at
// create (fmrx::conv_params: scalar loads at the head of the converter's chain,
// not 40 angles held in scalar registers across the rotator's).
//
// Knobs: CORDIC_FMRXB_PASSES and CORDIC_FMRXB_MAX_SPANS at create,
// CORDIC_FMRXB_MAX_BLOCKS at every run.  The bits depend on none.
//
// The unit is compiled four times, once per entry of the receiver's unit list
// (cordic_fm_rx_unit.h; unit 0 with launch 1 and the host side; the last on
// interleaved int16 I/Q: a span's x carries d_iq, its y is unused).  Each
// defines ONE entry point, FMRX_ENTRY(launch_rxbank), around fmx::with_stages;
// launch_fmrx_bank indexes the list's table by fmx::unit_of.
//
// Registers: the table in DESIGN.md section 4.8 and profiles/r20/fm_rx.txt;
// .vgpr_count of the 16-bit containers (scratch 0; above 128 both: the banks'
// grid is sized for 3 blocks per CU, kFmrxbBlocksPerCu, which holds up to 168;
// profiles/r24/fm_rx_c16.txt):
//   live stages                   13   16   19   20   24   27   29
//   fm_rxbank_xydir<30, N, IoC16> 132  142  133  133  134  137  137
//   ... <30, N, Io16>             130  132  131  131  132  135  135
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_xydir.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_table_nco.h"
#include "cordic_hostargs.h"
#include "cordic_devmem.h"
#include "cordic_fm_rx.h"
#include "cordic_fm_rx_decim.h"
#include "cordic_fm_rx_bank.h"
#include "cordic_span_reduce.h"
#include "cordic_fm_rx_unit.h"

namespace cordic_amd {

static_assert(kFmrxbRule.unit == kFmrxPass && kFmrxbRule.halo == kFmrxHalo
	&& kFmrxbRule.max_spans == kFmrxMaxBlocks, "the single call's geometry");
static_assert(dev::kBlock == 256, "launch 1 is instantiated at the block of launch 2");

// launch 1, for a job's first span: the phase in front of sample 0, not yet
// taken modulo 2^PW (launch 2 does), into the words behind the partial sums
__device__ __forceinline__ void span_latch_more(const RxSpan &d, uint32_t *more)
{
	const uint32_t *last = reinterpret_cast<const uint32_t *>((uintptr_t)d.last);
	more[d.start] = d.dphase0 + (last ? *last : 0u);
}

namespace fmrx {

using namespace dev;

// launch 2 (see the head of this file)
template <int LJ, int NLIVE, typename IO>
__global__ __launch_bounds__(kBlock) void fm_rxbank_xydir(CoreParams kp, DirArgs da,
		const RxSpan *__restrict__ spans, uint32_t nspans,
		const uint32_t *__restrict__ start, const uint32_t *__restrict__ part,
		const uint32_t *__restrict__ prev, const uint32_t *ckmem, uint32_t xw)
{
	typedef typename IO::ielem ielem;
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const unsigned tid = threadIdx.x;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	uint32_t bk_base[kDxMaxLevels] = {}, lf_base[kDxMaxLevels] = {};
	dx_lds_layout(da.dx, bk_base, lf_base);
	fmx::block_begin<LJ, NLIVE, IO>(kp, da, lds, bk_base, lf_base, tid);
	uint32_t *ex = lds + xw / 4u;
	__syncthreads();
	const fmx::RotRegs rr = fmx::block_ready<LJ, NLIVE>(kp, da, lds);
	const fmd::LaneConsts ln(conv_params(ckmem, false));
	unsigned par = 0;
	for (uint32_t t = blockIdx.x; t < nspans; t += gridDim.x) {
		const RxSpan d = spans[t];
		// the phase of the span's first sample, without its pm
		uint32_t carry = start[d.start];
		if (d.idx) {		// (block-uniform)
			fmx::front_sum(part + d.part0, d.idx, ex, tid, wave);
			__syncthreads();
			carry += ex[8] + ex[9] + ex[10] + ex[11];
		}
		const bool first = d.flags & kSpanFirst, tail = d.flags & kSpanLast;
		const uint32_t before = first ? prev[d.start] & (0xffffffffu >> ln.sh) : 0u;
		pass_loop<LJ, NLIVE>(kp, da, rr, bk_base, ckmem, ln,
			reinterpret_cast<const uint32_t *>((uintptr_t)d.fcw),
			reinterpret_cast<const uint32_t *>((uintptr_t)d.pm),
			reinterpret_cast<const ielem *>((uintptr_t)d.x),
			reinterpret_cast<const ielem *>((uintptr_t)d.y),
			reinterpret_cast<ielem *>((uintptr_t)d.mag),
			reinterpret_cast<ielem *>((uintptr_t)d.freq), (size_t)d.n, first, before,
			tail ? reinterpret_cast<uint32_t *>((uintptr_t)d.last) : nullptr, carry,
			par, ex, tid, wave, IO{});
		if (tail && d.acc && tid == 0)
			*reinterpret_cast<uint32_t *>((uintptr_t)d.acc) = carry;
	}
}

// this unit's entry point (kUnitLj, UnitIo: cordic_fm_rx_unit.h)
bool FMRX_ENTRY(launch_rxbank)(int nlive, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const RxSpan *spans,
		uint32_t nspans, const uint32_t *start, const uint32_t *part,
		const uint32_t *prev, const uint32_t *ckmem, uint32_t xw, uint32_t)
{
	return fmx::with_stages(nlive, da.dx.n, [&](auto nl) {
		hipLaunchKernelGGL((fm_rxbank_xydir<kUnitLj, decltype(nl)::value, UnitIo>),
			dim3(grid), dim3(kBlock), lds, st, kp, da, spans, nspans, start, part, prev,
			ckmem, xw);
	});
}

} // namespace fmrx

#if CORDIC_FMRX_UNIT == 0
int fmrxb_upload_conv(const cordic_config &conv, uint32_t **d_conv)
{
	const dev::CoreParams ck = make_params_jobs(conv);
	return dev_upload(&ck, sizeof ck, d_conv) ? CORDIC_OK : CORDIC_ERR_DEVICE;
}

int launch_fmrx_bank(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		const uint32_t *d_conv, const RxSpan *d_spans, uint32_t nspans,
		uint32_t *d_start, uint32_t *d_part, uint32_t *d_prev, int cus, FmForm form,
		void *stream)
{
	using namespace fmrx;
	const uint32_t log2r = form.log2r;
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (nspans == 0)
		return CORDIC_OK;
	hipStream_t st = static_cast<hipStream_t>(stream);
	// (log2r > 0: the decimating receiver's LDS, with the ring)
	uint32_t xw = 0;
	const size_t lds = log2r ? fmrxd::lds_bytes(dx, &xw) : lds_bytes(dx, &xw);
	size_t per_cu = blocks_per_cu(lds);
	if (per_cu > (size_t)kFmrxbBlocksPerCu)
		per_cu = kFmrxbBlocksPerCu;
	// launch 1 has 8 waves a SIMD: 8 blocks of 4 waves a CU
	const SpanGrids g = span_grids(nspans, cus, 8, "CORDIC_FMRXB_MAX_BLOCKS", per_cu);
	// the instance first: nothing is enqueued for a core without one
#define PLAIN(sfx, lj, io) launch_rxbank_##sfx,
#define DECIM(sfx, lj, io) launch_rxbank_decim_##sfx,
	static BankLaunch *const entry[2][kUnits] = {{CORDIC_FMRX_UNITS(PLAIN)},
		{CORDIC_FMRX_UNITS(DECIM)}};
#undef PLAIN
#undef DECIM
	const fmx::Unit u = fmx::unit_of(cfg.ww, form.esize(), form.iq);
	if (u == fmx::kUnitNone || !fmx_is_fused(cfg, d_dir, dx))
		return tnco::finish(false);
	hipLaunchKernelGGL((span_reduce<RxSpan, 256>), dim3(g.reduce), dim3(256), 0, st,
		d_spans, nspans, d_start, d_part);
	const DirArgs da{d_dir, dx};
	const CoreParams kp = make_params_jobs(cfg);
	return tnco::finish(entry[log2r != 0][u](cfg.nlive, g.walk, lds, st, kp, da, d_spans,
		nspans, d_start, d_part, d_prev, d_conv, xw, log2r));
}
#endif

} // namespace cordic_amd
