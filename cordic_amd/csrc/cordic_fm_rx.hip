// cordic_fm_rx.hip -- the tuned FM receiver's fused path (cordic_plan_fm_rx, and
// cordic_plan_fm_rx16 on int16 arrays): the FM mixer (cordic_fm_mix.hip) and the
// FM discriminator (cordic_fm_demod.hip) in one kernel, the tuned I/Q in
// registers only,
//   start = phase0 + *d_acc,   prev = (dphase0 + *d_last) mod 2^PW(conv)
//   p_i   = start + fcw[0] + .. + fcw[i-1] + pm[i]      (mod 2^32)
//   (tx_i, ty_i)  = what cordic_p2r writes for (x_i, y_i, p_i) on the plan's core
//   (mag_i, ph_i) = what cordic_r2p writes for (tx_i, ty_i) on conv
//   freq_i = sext_PW((ph_i - ph_(i-1)) mod 2^PW),   ph_(-1) = prev
//   *d_acc = start + fcw[0] + .. + fcw[n-1],   *d_last = ph_(n-1).
//
// Reduce-then-scan in two launches, as the mixer.  The samples are cut into
// spans of P passes of 1024 LESS 4 samples; block b owns span b.
//   1. fm_rx_reduce: each block sums its span of fcw into a workspace word;
//      block 0 latches the start AND prev beside them and copies the
//      converter's kernel parameters behind them.  A job's first and last
//      span run in different blocks of launch 2, and the last one writes
//      *d_last: so launch 2 may not read it.
//   2. fm_rx_xydir<LJ, NLIVE, IO>: the mixer's prologue (fmx::block_begin /
//      block_ready, cordic_fm_mix.h: tables into LDS, the trap; between them the
//      partials in front added to the start), then fmrx::pass_loop
//      (cordic_fm_rx.h): scan, fmx::xydir_vector, fmd::pol_lj_vector on its
//      registers, the differences, two stores.
// No block waits for another.  *d_acc and *d_last are read in launch 1 only and
// written in launch 2 only (one lane of the last block each).  Traffic: fcw
// twice, x, y, mag, freq once: 20 bytes per sample on int32 (24 with pm), 12
// (16) on int16, against 40 (44) and 24 (28) of the two calls.
//
// THE HALO.  A span that is not the call's first needs the phase ph of the
// sample in front of it, which is the MIXER's output there put through the
// converter.  The layout is the discriminator's: lane 0 of a span's first pass
// holds the vector in front of the span (x, y, fcw, pm at lo - 4 .. lo - 1, all
// inside the call's arrays), rotates and converts it with everyone else and
// stores nothing; its phase word is carry - fcw[lo-1] + pm[lo-1], and its tuning
// words are kept out of the scan.  A span of P passes therefore yields 1024 P -
// 4 samples: 1/(256 P) of the arithmetic is done twice, and no pass diverges.
// The alternative -- an extra vector through both chains by wave 0 in front of
// the loop -- would hold the other three waves at the first barrier for a whole
// chain (1/P of the block's time) and would inline both chains a second time.
//
// LDS is the tables' (dx_lds_layout) with 20 words behind them, in the DYNAMIC
// block: the table lookups address LDS by byte offset from 0, which a static
// __shared__ object would displace.  The trap below checks it.
//
// CORDIC_FMRX_MAX_BLOCKS=<n> in the environment (read at every call; a test and
// A/B knob like CORDIC_FMX_MAX_BLOCKS) caps the grid at n blocks.  The bits do
// not depend on it.
//
// The unit is compiled four times, once per entry of the receiver's unit list
// (cordic_fm_rx_unit.h: -DCORDIC_FMRX_UNIT=0 .. 3), so that the four build
// beside each other: <30, Io32> with launch 1 and the host side, <29, Io32>,
// <30, Io16>, and <30, fmx::IoC16> for interleaved int16 I/Q in d_xval
// (cordic_plan_fm_rx_c16).  Each defines ONE entry point, FMRX_ENTRY(launch_rx),
// around fmx::with_stages; launch_fm_rx indexes the list's table by
// fmx::unit_of.  The host side also holds fm_rx_split_c16, the split kernel of
// the *_c16 forms' fallback.
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps;
// .private_segment_fixed_size is 0 for every instance: nothing spills to
// scratch; profiles/r20/fm_rx.txt):
//   live stages              13   16   19   20   24   27   29
//   fm_rx_xydir<29, N>      108  108  108  108  110  114  114
//   fm_rx_xydir<30, N>      108  108  108  108  110  113  113
//   ... <30, N, Io16>       106  106  106  106  108  111  111
//   ... <30, N, IoC16>      106  106  106  106  108  110  111   (profiles/r24/fm_rx_c16.txt)
//   fm_rx_reduce             30 (64 bytes of static LDS)
// against 92 .. 108 of fm_mix_xydir and 90 .. 94 of the dynamic-exit
// discriminator: up to 128 registers hold 4 waves per SIMD, the mixer's own
// occupancy, so no step is crossed and the grid is sized for 4 blocks per CU
// (kFmrxBlocksPerCu), fewer where the tables fill LDS sooner.  Scalars: 105 ..
// 106 of them, 0 parked in VGPR lanes (2 for 27 live stages, 4 for 29; 12 lane
// moves in a whole unit).  With the converter's CoreParams as a kernel argument
// that was 137 .. 160 parked scalars and some 650 v_readlane / v_writelane per
// kernel, about one per multiply-add of the converter's chain, and the call ran
// at 0.86 .. 0.96 of the two calls; hence the parameters in the workspace
// (conv_params, cordic_fm_rx.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "cordic_xydir.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_table_nco.h"
#include "cordic_hostargs.h"
#include "cordic_fm_rx.h"
#include "cordic_fm_rx_decim.h"
#include "cordic_fm_rx_unit.h"

namespace cordic_amd {

namespace fmrx {

using namespace dev;

template <int LJ, int NLIVE, typename IO>
__global__ __launch_bounds__(kBlock) void fm_rx_xydir(CoreParams kp, DirArgs da,
		RxArgs a)
{
	typedef typename IO::ielem ielem;
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const unsigned tid = threadIdx.x;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	uint32_t bk_base[kDxMaxLevels] = {}, lf_base[kDxMaxLevels] = {};
	dx_lds_layout(da.dx, bk_base, lf_base);
	// ---- prologue, the mixer's (fmx::block_begin / block_ready): the tables,
	// and the waves' shares of the partials in front of this block (ex[8 .. 12))
	fmx::block_begin<LJ, NLIVE, IO>(kp, da, lds, bk_base, lf_base, tid);
	uint32_t *ex = lds + a.xw / 4u;
	fmx::front_sum(a.work + 4, blockIdx.x, ex, tid, wave);
	__syncthreads();
	const fmx::RotRegs rr = fmx::block_ready<LJ, NLIVE>(kp, da, lds);

	// the converter's parameters: launch 1 left them in the workspace
	const uint32_t *ckmem = a.work + kFmrxConvAt / 4;
	const fmd::LaneConsts ln(conv_params(ckmem, false));
	const size_t lo = (size_t)blockIdx.x * a.span;	// < n by the grid
	const size_t cnt = (a.n - lo < a.span) ? a.n - lo : a.span;
	const bool tail = blockIdx.x == gridDim.x - 1;
	// shorts per input sample: IoC16 has both halves in a.x (a.y is not read)
	constexpr size_t kIn = fmx::is_iq<IO>::value ? 2 : 1;
	// the phase of sample lo, without its pm
	uint32_t carry = a.work[0] + ex[8] + ex[9] + ex[10] + ex[11];
	unsigned par = 0;
	pass_loop<LJ, NLIVE>(kp, da, rr, bk_base, ckmem, ln, a.fcw + lo,
		a.pm ? a.pm + lo : nullptr, static_cast<const ielem *>(a.x) + kIn * lo,
		static_cast<const ielem *>(a.y) + lo, static_cast<ielem *>(a.mag) + lo,
		static_cast<ielem *>(a.freq) + lo, cnt, blockIdx.x == 0, a.work[1],
		tail ? a.last : nullptr, carry, par, ex, tid, wave, IO{});
	if (a.acc && tail && tid == 0)
		*a.acc = carry;
}

// this unit's entry point (kUnitLj, UnitIo: cordic_fm_rx_unit.h)
bool FMRX_ENTRY(launch_rx)(int nlive, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const RxArgs &a, uint32_t)
{
	return fmx::with_stages(nlive, da.dx.n, [&](auto nl) {
		hipLaunchKernelGGL((fm_rx_xydir<kUnitLj, decltype(nl)::value, UnitIo>),
			dim3(grid), dim3(kBlock), lds, st, kp, da, a);
	});
}

#if CORDIC_FMRX_UNIT == 0
// Four consecutive words at any 4-byte-aligned address: one dwordx4 load
// (span_words4, cordic_span_reduce.h)
typedef uint32_t words4 __attribute__((ext_vector_type(4), aligned(4)));

// launch 1: work[4 + b] = the sum of block b's span [b * span, (b + 1) * span)
// of fcw (cut at n); block 0: work[0] = phase0 + *d_acc, work[1] = (dphase0 +
// *d_last) & pmask, and the converter's parameters at kFmrxConvAt.  fm_reduce
// (cordic_table_fm.hip) with the second latch.
struct ConvWords {
	uint32_t w[sizeof(CoreParams) / 4];
};
static_assert(sizeof(CoreParams) <= kFmrxConvBytes && sizeof(CoreParams) % 4 == 0
	&& kFmrxConvAt % 16 == 0, "the converter's parameters in the workspace");

__global__ __launch_bounds__(1024) void fm_rx_reduce(const uint32_t *d_fcw, size_t n,
		size_t span, uint32_t phase0, const uint32_t *d_acc, uint32_t dphase0,
		const uint32_t *d_last, uint32_t pmask, uint32_t *work, ConvWords ck)
{
	__shared__ uint32_t wsum[16];
	const unsigned tid = threadIdx.x;
	if (blockIdx.x == 0 && tid < sizeof(CoreParams) / 4)
		work[kFmrxConvAt / 4 + tid] = ck.w[tid];
	const size_t lo = (size_t)blockIdx.x * span;	// < n by the grid
	const size_t len = (n - lo < span) ? n - lo : span;
	const uint32_t *f = d_fcw + lo;
	const words4 *fv = reinterpret_cast<const words4 *>(f);
	const size_t nv = len / 4;
	uint32_t s = 0;
#pragma unroll 4
	for (size_t g = tid; g < nv; g += 1024) {
		const words4 q = fv[g];
		s += q[0] + q[1] + q[2] + q[3];
	}
	const size_t r = nv * 4 + tid;	// fewer than 4 behind the vectors
	if (r < len)
		s += f[r];
#pragma unroll
	for (int k = 32; k; k >>= 1)
		s += __shfl_xor(s, k);
	if ((tid & 63u) == 0)
		wsum[tid >> 6] = s;
	__syncthreads();
	if (tid == 0) {
		uint32_t sum = 0;
#pragma unroll
		for (int j = 0; j < 16; j++)
			sum += wsum[j];
		work[4 + blockIdx.x] = sum;
		if (blockIdx.x == 0) {
			work[0] = phase0 + (d_acc ? *d_acc : 0u);
			work[1] = (dphase0 + (d_last ? *d_last : 0u)) & pmask;
		}
	}
}
#endif

} // namespace fmrx

#if CORDIC_FMRX_UNIT == 0
bool fmrx_conv_is_fused(const cordic_config &conv)
{
	return fmd_core_is_fused(conv) && !(conv.flags & CORDIC_FLAG_UNIT_GAIN);
}

int fmrx_check_call(FmForm form, size_t n, const uint32_t *d_fcw, const uint32_t *d_pm,
		const uint32_t *d_acc, const void *d_xval, const void *d_yval,
		const uint32_t *d_last, const void *d_omag, const void *d_ofreq,
		const void *d_work, size_t work_bytes)
{
	return iq_call_ok(n, d_acc, d_last, d_fcw, d_pm, d_xval, d_yval, d_omag, d_ofreq,
		form.esize(), d_work, work_bytes, form.log2r, form.iq) ? CORDIC_OK : CORDIC_ERR_ARGS;
}

// The *_c16 forms' fallback: thread t splits complex samples 4 t .. 4 t + 3, one
// 16-byte load at any 4-byte alignment and two 8-byte stores (x and y lie on the
// 16-byte grid inside the workspace); the last, partial vector goes element by
// element.  Nothing at or behind complex sample n is read or written.
namespace fmrx {
__global__ __launch_bounds__(256) void fm_rx_split_c16(const int16_t *__restrict__ iq,
		int16_t *__restrict__ x, int16_t *__restrict__ y, size_t n)
{
	const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
	if (i + 4 <= n) {
		const u32x4 q = CORDIC_LOAD_IN(reinterpret_cast<const fmx::IoC16::cvec *>(iq + 2 * i));
		u16x4 a, b;
#pragma unroll
		for (int v = 0; v < 4; v++) {
			a[v] = (uint16_t)q[v];
			b[v] = (uint16_t)(q[v] >> 16);
		}
		*reinterpret_cast<u16x4 *>(x + i) = a;
		*reinterpret_cast<u16x4 *>(y + i) = b;
	} else {
		for (size_t j = i; j < n; j++) {
			x[j] = iq[2 * j];
			y[j] = iq[2 * j + 1];
		}
	}
}
} // namespace fmrx

int launch_fmrx_split_c16(size_t n, const int16_t *d_iq, int16_t *d_x, int16_t *d_y,
		void *stream)
{
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (n == 0)
		return CORDIC_OK;
	const size_t blocks = (n + 1023) / 1024;
	if (blocks > 0x7fffffffu)
		return CORDIC_ERR_ARGS;
	hipLaunchKernelGGL(fmrx::fm_rx_split_c16, dim3((unsigned)blocks), dim3(256), 0,
		static_cast<hipStream_t>(stream), d_iq, d_x, d_y, n);
	return tnco::finish(true);
}

int launch_fm_rx(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		const cordic_config &conv, FmForm form, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, const void *d_xval,
		const void *d_yval, uint32_t dphase0, uint32_t *d_last, void *d_omag,
		void *d_ofreq, void *d_work, void *stream)
{
	using namespace fmrx;
	const uint32_t log2r = form.log2r;
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (n == 0)
		return CORDIC_OK;
	hipStream_t st = static_cast<hipStream_t>(stream);
	const int cus = jobs_cus_now();
	if (cus < 0) {
		(void)hipGetLastError();
		return CORDIC_ERR_DEVICE;
	}
	// (log2r > 0: the decimating receiver's LDS, halo and knob)
	uint32_t xw = 0;
	const size_t lds = log2r ? fmrxd::lds_bytes(dx, &xw) : lds_bytes(dx, &xw);
	size_t cap = (size_t)cus * blocks_per_cu(lds);
	if (cap > kFmrxMaxBlocks)
		cap = kFmrxMaxBlocks;
	cap = env_block_cap(log2r ? "CORDIC_FMRXD_MAX_BLOCKS" : "CORDIC_FMRX_MAX_BLOCKS", cap);
	const CallSpan cs = call_span(n, cap, kFmrxPass, log2r ? fmrxd_halo(log2r) : kFmrxHalo);
	const size_t span = cs.span;
	const unsigned grid = (unsigned)cs.grid;
	// the instance first: nothing is enqueued for a core without one
#define PLAIN(sfx, lj, io) launch_rx_##sfx,
#define DECIM(sfx, lj, io) launch_rxd_##sfx,
	static RxLaunch *const entry[2][kUnits] = {{CORDIC_FMRX_UNITS(PLAIN)},
		{CORDIC_FMRX_UNITS(DECIM)}};
#undef PLAIN
#undef DECIM
	const fmx::Unit u = fmx::unit_of(cfg.ww, form.esize(), form.iq);
	if (u == fmx::kUnitNone || !fmx_is_fused(cfg, d_dir, dx))
		return tnco::finish(false);
	uint32_t *work = static_cast<uint32_t *>(d_work);
	const uint32_t pmask = 0xffffffffu >> (32 - conv.pw);
	const CoreParams ck = make_params_jobs(conv);
	ConvWords cw;
	memcpy(&cw, &ck, sizeof cw);
	hipLaunchKernelGGL(fm_rx_reduce, dim3(grid), dim3(1024), 0, st, d_fcw, n, span,
		phase0, (const uint32_t *)d_acc, dphase0, (const uint32_t *)d_last, pmask,
		work, cw);
	const RxArgs a{d_fcw, d_pm, d_acc, d_last, work, d_xval, d_yval, d_omag, d_ofreq,
		n, span, xw};
	const DirArgs da{d_dir, dx};
	const CoreParams kp = make_params_jobs(cfg);
	return tnco::finish(entry[log2r != 0][u](cfg.nlive, grid, lds, st, kp, da, a, log2r));
}
#endif

} // namespace cordic_amd
