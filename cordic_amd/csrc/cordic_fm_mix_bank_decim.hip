// cordic_fm_mix_bank_decim.hip -- launch 2 of a decimating FM mixer bank
// (cordic_mixbank_create_decim, _create_decim16; include/cordic_amd.h):
// fm_mixbank_xydir (cordic_fm_mix_bank.hip) with pass_loop's decimating form
// (cordic_fm_mix.h; the sum is described in cordic_fm_mix_decim.hip).  The
// host's cutter has put a span's d.ox / d.oy at output (s0 >> k) of the job
// (span_place, cordic_fm_mix_bank.h) -- s0 is whole passes of 1024, a multiple
// of R -- so the loop runs over [0, d.n) and writes [0, d.n >> k) of them.
// Launch 1, the grids and the span table are launch_fmx_bank's, which calls
// this unit for a bank with k > 0.  k is one per bank, a kernel argument.
// The <30, N, IoC16io> instances (cordic_mixbank_create_decim_c16) are in
// cordic_fm_mix_bank_decim_c16.o, this source compiled with -DCORDIC_FMX_C16;
// their registers stand in the table of cordic_fm_mix_decim.hip.
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

// launch 2 for one <LJ, container>; false: no instance for nlive
template <int LJ, typename IO>
static bool launch_walk(int nlive, int ngroups, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const MixSpan *d_spans, uint32_t nspans,
		const uint32_t *d_start, const uint32_t *d_part, uint32_t xw, uint32_t log2r)
{
	return with_stages(nlive, ngroups, [&](auto nl) {
		hipLaunchKernelGGL((fm_mixbank_decim_xydir<LJ, decltype(nl)::value, IO>),
			dim3(grid), dim3(kBlock), lds, st, kp, da, d_spans, nspans, d_start, d_part,
			xw, log2r);
	});
}

} // namespace fmx

#ifdef CORDIC_FMX_C16
// This object (cordic_fm_mix_bank_decim_c16.o): the kernel's <30, N, IoC16io>
// instances and their launcher.
bool launch_fmx_bank_decim_walk_c16(int nlive, int ngroups, unsigned grid, size_t lds,
		void *stream, const dev::CoreParams &kp, const dev::DirArgs &da,
		const MixSpan *d_spans, uint32_t nspans, const uint32_t *d_start,
		const uint32_t *d_part, uint32_t xw, uint32_t log2r)
{
	return fmx::launch_walk<30, fmx::IoC16io>(nlive, ngroups, grid, lds,
		static_cast<hipStream_t>(stream), kp, da, d_spans, nspans, d_start, d_part, xw,
		log2r);
}
#else
bool launch_fmx_bank_decim_walk(int unit, int nlive, int ngroups, unsigned grid,
		size_t lds, void *stream, const dev::CoreParams &kp, const dev::DirArgs &da,
		const MixSpan *d_spans, uint32_t nspans, const uint32_t *d_start,
		const uint32_t *d_part, uint32_t xw, uint32_t log2r)
{
	using namespace fmx;
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (unit == kUnitC16)	// (cordic_fm_mix_bank_decim_c16.o)
		return launch_fmx_bank_decim_walk_c16(nlive, ngroups, grid, lds, stream, kp, da,
			d_spans, nspans, d_start, d_part, xw, log2r);
	return with_unit((Unit)unit, [&](auto lj, auto io) {
		return launch_walk<decltype(lj)::value, decltype(io)>(nlive, ngroups, grid, lds, st,
			kp, da, d_spans, nspans, d_start, d_part, xw, log2r);
	});
}
#endif // CORDIC_FMX_C16

} // namespace cordic_amd
