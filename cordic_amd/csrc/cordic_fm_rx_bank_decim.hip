// cordic_fm_rx_bank_decim.hip -- launch 2 of the decimating receiver banks
// (cordic_rxbank_create_decim, _create_decim16; include/cordic_amd.h): the
// receiver banks' kernel (cordic_fm_rx_bank.hip) around the decimating
// receiver's pass loop (fmrxd::pass_loop, cordic_fm_rx_decim.h), R = 2^k, 1 <= k
// <= 8.  Launch 1 (span_reduce with the second latch), the grids and the host
// side are cordic_fm_rx_bank.hip's: this unit holds the kernel and nothing of
// the geometry.
//
// The host has cut every job into spans of whole 1024-sample passes LESS the
// halo's max(4, R) input samples (fmrxb_rule, cordic_fm_rx_bank.h): every span
// begins and ends on a multiple of R, its outputs begin at (s0 >> k) elements
// (span_place).  A span that is not its job's first finds the R input samples
// of the decimated sample in front of it inside the job.  A span of fewer than
// R passes flushes once, at its end, with part of the block idle in that flush
// (the bank's default span at k > 4): correct, and not tuned for.
//
// LDS words across spans: the parities of the scan's words (par) and of the
// edge words (fpar) run on from span to span; the ring's stream slots begin
// again at every span, behind the flush that ended the span in front (barriers
// (A) and (B) of fmrxd::pass_loop) and behind the new span's first scan
// barrier.  The shares of a span's prologue (ex[8 .. 12)) are written only
// behind those.
//
// The unit is compiled four times, as cordic_fm_rx_bank.hip is: once per entry
// of the receiver's unit list (cordic_fm_rx_unit.h).
// Registers: profiles/r23/fm_rx_decim.txt; .vgpr_count of the 16-bit containers
// (scratch 0; above 128 both: 3 blocks per CU, kFmrxbBlocksPerCu, which holds up
// to 168; profiles/r24/fm_rx_c16.txt):
//   live stages                         13   16   19   20   24   27   29
//   fm_rxbank_decim_xydir<30, N, IoC16> 134  144  135  135  136  139  139
//   ... <30, N, Io16>                   133  143  134  134  135  138  138
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_xydir.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_hostargs.h"
#include "cordic_fm_rx_decim.h"
#include "cordic_fm_rx_bank.h"
#include "cordic_fm_rx_unit.h"

namespace cordic_amd {

namespace fmrxd {

using namespace dev;

template <int LJ, int NLIVE, typename IO>
__global__ __launch_bounds__(kBlock) void fm_rxbank_decim_xydir(CoreParams kp, DirArgs da,
		const RxSpan *__restrict__ spans, uint32_t nspans,
		const uint32_t *__restrict__ start, const uint32_t *__restrict__ part,
		const uint32_t *__restrict__ prev, const uint32_t *ckmem, uint32_t xw,
		uint32_t log2r)
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
	const fmd::LaneConsts ln(fmrx::conv_params(ckmem, false));
	unsigned par = 0, fpar = 0;
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
			reinterpret_cast<ielem *>((uintptr_t)d.freq), (size_t)d.n, log2r, first,
			before, tail ? reinterpret_cast<uint32_t *>((uintptr_t)d.last) : nullptr,
			carry, par, fpar, ex, xw + (uint32_t)kFmrxdExWords * 4u, tid, wave, IO{});
		if (tail && d.acc && tid == 0)
			*reinterpret_cast<uint32_t *>((uintptr_t)d.acc) = carry;
	}
}

} // namespace fmrxd

namespace fmrx {

// this unit's entry point (kUnitLj, UnitIo: cordic_fm_rx_unit.h)
bool FMRX_ENTRY(launch_rxbank_decim)(int nlive, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const RxSpan *spans,
		uint32_t nspans, const uint32_t *start, const uint32_t *part,
		const uint32_t *prev, const uint32_t *ckmem, uint32_t xw, uint32_t log2r)
{
	return fmx::with_stages(nlive, da.dx.n, [&](auto nl) {
		hipLaunchKernelGGL((fmrxd::fm_rxbank_decim_xydir<kUnitLj, decltype(nl)::value, UnitIo>),
			dim3(grid), dim3(kBlock), lds, st, kp, da, spans, nspans, start, part, prev,
			ckmem, xw, log2r);
	});
}

} // namespace fmrx

} // namespace cordic_amd
