// cordic_fm_mix_bank_decim.hip -- launch 2 of a decimating FM mixer bank
// (cordic_mixbank_create_decim, _create_decim16; include/cordic_amd.h):
// fm_mixbank_xydir (cordic_fm_mix_bank.hip) with pass_loop's decimating form
// (cordic_fm_mix.h; the sum is described in cordic_fm_mix_decim.hip).  The
// host's cutter has put a span's d.ox / d.oy at output (s0 >> k) of the job
// (span_place, cordic_fm_mix_bank.h) -- s0 is whole passes of 1024, a multiple
// of R -- so the loop runs over [0, d.n) and writes [0, d.n >> k) of them.
// Launch 1, the grids and the span table are launch_fmx_bank's, which calls
// this unit for a bank with k > 0.  k is one per bank, a kernel argument.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_xydir.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_hostargs.h"
#include "cordic_fm_mix.h"
#include "cordic_fm_mix_bank.h"

namespace cordic_amd {

namespace fmx {

template <int LJ, int NLIVE, typename IO>
__global__ __launch_bounds__(kBlock) void fm_mixbank_decim_xydir(CoreParams kp, DirArgs da,
		const MixSpan *__restrict__ spans, uint32_t nspans,
		const uint32_t *__restrict__ start, const uint32_t *__restrict__ part,
		uint32_t xw, uint32_t log2r)
{
	typedef typename IO::ielem ielem;
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const unsigned tid = threadIdx.x;
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
			carry, par, ex, tid, wave, IO{}, std::true_type{}, log2r);
		if ((d.flags & kSpanLast) && d.acc && tid == 0)
			*reinterpret_cast<uint32_t *>((uintptr_t)d.acc) = carry;
	}
}

} // namespace fmx

bool launch_fmx_bank_decim_walk(int ww, int nlive, int ngroups, bool io16, unsigned grid,
		size_t lds, void *stream, const dev::CoreParams &kp, const dev::DirArgs &da,
		const MixSpan *d_spans, uint32_t nspans, const uint32_t *d_start,
		const uint32_t *d_part, uint32_t xw, uint32_t log2r)
{
	using namespace fmx;
	hipStream_t st = static_cast<hipStream_t>(stream);
	return with_unit(unit_of(ww, io16 ? 2 : 4), [&](auto lj, auto io) {
		return with_stages(nlive, ngroups, [&](auto nl) {
			hipLaunchKernelGGL((fm_mixbank_decim_xydir<decltype(lj)::value,
				decltype(nl)::value, decltype(io)>), dim3(grid), dim3(kBlock), lds, st,
				kp, da, d_spans, nspans, d_start, d_part, xw, log2r);
		});
	});
}

} // namespace cordic_amd
