// cordic_fm_rx.h -- the tuned FM receiver (cordic_plan_fm_rx, cordic_plan_fm_rx16,
// their _info and _workspace; include/cordic_amd.h): the FM mixer and the FM
// discriminator in ONE kernel, the tuned I/Q never stored,
//   p_i          = start + fcw[0] + .. + fcw[i-1] + pm[i]        (mod 2^32)
//   (tx_i, ty_i) = what cordic_plan_fm_mix writes for (x_i, y_i, p_i)
//   (mag_i, ph_i) = what cordic_r2p writes for (tx_i, ty_i) on conv
//   freq_i       = sext_PW((ph_i - ph_(i-1)) mod 2^PW).
// The launcher and the host checks for cordic_abi_fm.cpp, where the entry
// points live; the fallback (cordic_plan_fm_mix into two arrays
// inside the workspace, then cordic_fm_demod from them) is put together there.
// Behind them, for hipcc only, the pass loop of the call's kernel
// (cordic_fm_rx.hip), written over ONE span with its arrays at the span's first
// sample, which the receiver banks' kernel (cordic_fm_rx_bank.hip) walks
// descriptors with:
// fmx::xydir_vector's registers go straight into fmd::pol_lj_vector.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_FM_RX_H
#define CORDIC_FM_RX_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_internal.h"
#include "cordic_fm_mix.h"
#include "cordic_fm_demod.h"

namespace cordic_amd {

// Fused kernel: a block of 256 threads makes kFmrxPass consecutive samples per
// pass, 4 per lane, and owns a contiguous span of whole passes.  The first
// vector of a span is the HALO -- the vector in front of the span, rotated and
// converted again and not stored, for the phase of the sample in front -- so a
// span of P passes yields P * kFmrxPass - kFmrxHalo samples.  Workspace: [0]
// the latched start, [1] the latched phase in front of sample 0, [4 + b] one
// partial sum per block; behind them, at kFmrxConvAt, the converter's kernel
// parameters (dev::CoreParams), which launch 1 puts there for launch 2 to fetch
// by scalar loads where it uses them (see fmrx::pass_loop).
constexpr size_t kFmrxPass = 1024;
constexpr size_t kFmrxHalo = 4;
constexpr size_t kFmrxMaxBlocks = 4096;
constexpr size_t kFmrxBlocksPerCu = 4;	// by its registers (cordic_fm_rx.hip)
constexpr size_t kFmrxConvAt = 16 + 4 * kFmrxMaxBlocks;
constexpr size_t kFmrxConvBytes = 512;	// >= sizeof(dev::CoreParams)
constexpr size_t kFmrxWorkBytes = kFmrxConvAt + kFmrxConvBytes;

// Fallback: [the mixer call's workspace | tuned x | tuned y | the
// discriminator's workspace], every part on the 16-byte grid; esize is 4 or 2.
// mix_bytes: cordic_plan_fm_mix_workspace / cordic_plan_fm_mix16_workspace.
constexpr size_t fmrx_array_bytes(size_t n, size_t esize)
{
	return (n * esize + 15) & ~(size_t)15;
}
struct FmrxLayout {
	size_t	tx, ty, demod, end;	// byte offsets in d_work
};
// m: the elements of the tuned arrays and of the discriminator's call (the
// decimating receiver: n >> k)
constexpr FmrxLayout fmrx_layout(size_t mix_bytes, size_t m, size_t esize)
{
	const size_t each = fmrx_array_bytes(m, esize);
	return FmrxLayout{mix_bytes, mix_bytes + each, mix_bytes + 2 * each,
		mix_bytes + 2 * each + fmd_work_bytes(m)};
}
constexpr size_t fmrx_work_bytes(bool fused, size_t mix_bytes, size_t n, size_t esize)
{
	return !n ? 0 : fused ? kFmrxWorkBytes : fmrx_layout(mix_bytes, n, esize).end;
}
static_assert(kFmrxWorkBytes % 16 == 0, "a multiple of 16");

// 1: the fused kernel serves this converter behind a fused mixer -- the cores
// of the fused discriminator (fmd_core_is_fused) without CORDIC_FLAG_UNIT_GAIN:
// the one converter instance the receiver carries is the dynamic-exit one.
// (The mode and the container are the caller's to check.)
bool	fmrx_conv_is_fused(const cordic_config &conv);

// Alignment -- the four sample arrays on the grid of the form's container, the
// words on that of 4, d_work on that of 16 -- and no output range (the words at
// d_acc and d_last and the `work_bytes` of d_work included) over anything else,
// by the true byte ranges; nothing is launched.  n > 0.  The two outputs hold
// n >> form.log2r elements.  form.iq: d_xval is the one interleaved input array
// (on the 4-byte grid, 4 n bytes) and d_yval is not looked at.
int	fmrx_check_call(FmForm form, size_t n, const uint32_t *d_fcw, const uint32_t *d_pm,
		const uint32_t *d_acc, const void *d_xval, const void *d_yval,
		const uint32_t *d_last, const void *d_omag, const void *d_ofreq,
		const void *d_work, size_t work_bytes);

// The fused path: two launches on `stream` (fm_rx_reduce, then fm_rx_xydir),
// nothing else.  The sample arrays hold the form's container.
// The caller has checked fmx_is_fused / fmx_is_fused16, fmrx_conv_is_fused and
// fmrx_check_call.
// form.log2r = k in 1 .. 8: launch 2 is fm_rx_decim_xydir
// (cordic_fm_rx_decim.hip), which writes n >> k samples; n is a multiple of 2^k.
// form.iq: d_xval holds interleaved int16 I/Q, 2 n shorts, and d_yval is not
// read -- the <30, IoC16> instances of launch 2 (fmx::IoC16).
int	launch_fm_rx(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		const cordic_config &conv, FmForm form, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, const void *d_xval,
		const void *d_yval, uint32_t dphase0, uint32_t *d_last, void *d_omag,
		void *d_ofreq, void *d_work, void *stream);

// The *_c16 forms' fallback: [the *16 twin's workspace | x | y of n shorts],
// each part on the 16-byte grid; one launch of fm_rx_split_c16 fills x and y
// from d_iq (n > 0 complex samples on the 4-byte grid), then the twin runs.
struct FmrxC16Layout {
	size_t	x, y, end;		// byte offsets in d_work
};
constexpr FmrxC16Layout fmrx_c16_layout(size_t twin_bytes, size_t n)
{
	const size_t at = (twin_bytes + 15) & ~(size_t)15, each = fmrx_array_bytes(n, 2);
	return FmrxC16Layout{at, at + each, at + 2 * each};
}
constexpr size_t fmrx_c16_work_bytes(bool fused, size_t twin_bytes, size_t n)
{
	return !n || fused ? twin_bytes : fmrx_c16_layout(twin_bytes, n).end;
}
int	launch_fmrx_split_c16(size_t n, const int16_t *d_iq, int16_t *d_x, int16_t *d_y,
		void *stream);

} // namespace cordic_amd

#ifdef __HIPCC__
namespace cordic_amd {
namespace fmrx {

using namespace dev;

// the converter instance of every receiver kernel: dynamic exit, no unit gain
constexpr int kConvStages = kDynStages;

// LDS words behind the tables (fmx::lds_bytes has 12): [0, 8) the scan's
// exchange words, [8, 12) the prologue's shares, [12, 20) the edge words
constexpr uint32_t kExWords = 20;

// The converter's parameters where launch 1 left them, as constant memory (a
// wave-uniform address: scalar loads).  opaque: behind an empty asm, so that
// the loads stay where the reference is made.
__device__ __forceinline__ const CoreParams &conv_params(const uint32_t *ckmem, bool opaque)
{
	uint64_t u = (uint64_t)(uintptr_t)ckmem;
	if (opaque)
		asm volatile("" : "+s"(u));
	return *(const CoreParams *)(const __attribute__((address_space(4))) CoreParams *)u;
}

// The pass loop: samples [0, n) of ONE span, whose six arrays begin at the
// span's first sample, 1024 vectors-of-4 per pass.  Lane j of the span (j = 256
// * pass + thread) has the samples 4 j - 4 .. 4 j - 1: lane 0 is the halo, the
// vector in front of the span, which is rotated and converted like any other
// and not stored -- the same arithmetic on the same inputs as its own span's,
// so the bits do not depend on how a job was cut.  first: the span begins at
// sample 0 of its job; there is no such vector, lane 0 loads nothing and lends
// `prev` = (dphase0 + *d_last) mod 2^PW, which launch 1 latched.
// carry: in, the phase of sample 0 without its pm; out, that of sample n.  The
// halo's own phase is carry - fcw[-1] + pm[-1]: its tuning words are kept out
// of the scan.
// par: the parity of the exchange words (ex[0 .. 8): the scan's, as
// fmx::pass_loop; ex[12 .. 20): the edge words, as fmd::sweep_tile), which are
// double-buffered by pass; it runs on from span to span (a bank's block walks
// many).  A pass has TWO barriers, the scan's and the edges': the phase that
// crosses a wave edge exists only behind the converter's chain.  The parity is
// still needed, for the edge words: wave 0 reads wave 3's word of the pass
// BEFORE behind its own chain, in front of the edges' barrier, where wave 3 of
// this pass may already be writing its new one -- the two have only the scan's
// barrier between them and both lie behind it.  (The scan's words alone could
// share one buffer now; they follow the same parity rather than a rule of
// their own.)
// ckmem: the converter's CoreParams in the workspace.  As a kernel argument
// its 40 stage angles stay in scalar registers from the prologue on, next to
// everything the rotator keeps there, and hipcc then parks about 150 scalars in
// VGPR lanes and fetches an angle per stage by v_readlane inside the
// converter's chain (one lane move per multiply-add; 0.86 .. 0.96 of the two
// calls' rate).  Read from constant memory behind an address the compiler
// cannot see through, they are loaded (s_load) where the chain begins, every
// pass, and are dead again behind it.
// d_last: where the lane with sample n - 1 writes its phase; NULL in every
// span but a job's last, and where the job has none.  pm may be NULL
// (wave-uniform).  IO = fmx::IoC16: ax is the span's interleaved I/Q (complex
// sample i at ax + 2 i, one 16-byte load per lane), ay is not read.  Nothing at or behind n is read or written, and in front of
// sample 0 only the halo vector is read.
template <int LJ, int NLIVE, typename IO>
__device__ __forceinline__ void pass_loop(const CoreParams &kp, const DirArgs &da,
		const fmx::RotRegs &rr, const uint32_t (&bk_base)[kDxMaxLevels],
		const uint32_t *ckmem, const fmd::LaneConsts &ln, const uint32_t *fcw,
		const uint32_t *pm, const typename IO::ielem *ax,
		const typename IO::ielem *ay, typename IO::ielem *amag,
		typename IO::ielem *afreq, const size_t n, const bool first,
		const uint32_t prev, uint32_t *d_last, uint32_t &carry, unsigned &par,
		uint32_t *ex, const unsigned tid, const unsigned wave, IO)
{
	typedef typename IO::ivec ivec;
	typedef typename IO::ielem ielem;
	// 4 samples as they lie in memory (IoC16: 4 complex ones, in x; ay unused)
	typedef typename fmx::raw_in<IO>::type raw4;
	const ptrdiff_t sn = (ptrdiff_t)n;
	const unsigned lane = tid & 63u;
	// this lane's 4 samples of the pass at t0
	auto load_pass = [&](size_t t0, u32x4 &f, u32x4 &m, raw4 &x, raw4 &y) {
		const ptrdiff_t i = (ptrdiff_t)t0 + (ptrdiff_t)(kVec * tid) - (ptrdiff_t)kFmrxHalo;
		f = u32x4{};
		m = u32x4{};
		x = raw4{};
		y = raw4{};
		if (i < 0 ? !first : i + kVec <= sn) {
			f = CORDIC_LOAD_IN(reinterpret_cast<const u32x4g *>(fcw + i));
			if (pm)	// (wave-uniform)
				m = CORDIC_LOAD_IN(reinterpret_cast<const u32x4g *>(pm + i));
			if constexpr (fmx::is_iq<IO>::value) {
				x = CORDIC_LOAD_IN(reinterpret_cast<const typename IO::cvec *>(ax + 2 * i));
			} else {
				x = CORDIC_LOAD_IN(reinterpret_cast<const ivec *>(ax + i));
				y = CORDIC_LOAD_IN(reinterpret_cast<const ivec *>(ay + i));
			}
		} else if (i >= 0 && i < sn) {	// the last, partial vector: one lane
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				if (i + v < sn) {
					f[v] = fcw[i + v];
					if (pm)
						m[v] = pm[i + v];
					if constexpr (fmx::is_iq<IO>::value) {
						x[v] = reinterpret_cast<const uint32_t *>(ax)[i + v];
					} else {
						x[v] = ax[i + v];
						y[v] = ay[i + v];
					}
				}
			}
		}
	};

	u32x4 nf, nm;
	raw4 nx, ny;
	load_pass(0, nf, nm, nx, ny);
	for (size_t t0 = 0; t0 < n + kFmrxHalo; t0 += kFmrxPass) {
		const bool halo = t0 == 0 && tid == 0;
		u32x4 f = nf;
		const u32x4 m = nm;
		i32x4 tx, ty;
		fmx::widen_iq(IO{}, nx, ny, tx, ty);
		if (t0 + kFmrxPass < n + kFmrxHalo)
			load_pass(t0 + kFmrxPass, nf, nm, nx, ny);

		// the halo's tuning words lie in front of the span: not in the scan
		const uint32_t hf = halo ? f[3] : 0u;
		if (halo)
			f = u32x4{};
		const uint32_t s0 = f[0], s1 = s0 + f[1], s2 = s1 + f[2], s3 = s2 + f[3];
		const uint32_t incl = fmx::wave_scan(s3);
		if (lane == 63u)
			ex[par * 4 + wave] = incl;
		__syncthreads();
		const u32x4 w = *reinterpret_cast<const u32x4 *>(ex + par * 4);
		const uint32_t front = (wave > 0 ? w[0] : 0u) + (wave > 1 ? w[1] : 0u)
			+ (wave > 2 ? w[2] : 0u);
		const uint32_t excl = carry + front + incl - s3;
		carry += w[0] + w[1] + w[2] + w[3];

		const uint32_t ph[kVec] = {excl + m[0], excl + s0 + m[1], excl + s1 + m[2],
			excl + s2 + m[3] - hf};
		uint32_t pb[kVec];
#pragma unroll
		for (int v = 0; v < kVec; v++)	// cordic_xydir.h:202-205
			asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(pb[v])
				: "v"(ph[v]), "s"(kp.pw_shl), "v"(rr.k45));

		i32x4 rx, ry;
		fmx::xydir_vector<LJ, NLIVE>(kp, da, rr.ljc, rr.maskv, bk_base, rr.full_ports,
			tx, ty, pb, rx, ry);
		i32x4 rm;
		u32x4 rp;
		fmd::pol_lj_vector<kConvStages, true, false, false>(conv_params(ckmem, true), ln,
			rx, ry, rm, rp);

		// the phase in front of this lane's first sample (fmd::sweep_tile)
		uint32_t last = rp[3];
		if (halo && first)
			last = prev;
		uint32_t *edge = ex + 12 + par * 4;
		if (lane == 63u)
			edge[wave] = last;
		uint32_t before0 = 0;
		if (wave == 0)		// (pass 0: the halo lane's, unused)
			before0 = ex[12 + (par ^ 1u) * 4 + 3];
		__syncthreads();
		if (wave != 0)
			before0 = edge[wave - 1];
		par ^= 1;
		// wave_shr:1 -- lane l gets lane l - 1's `last`, lane 0 keeps before0
		const uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp(
			(int)before0, (int)last, 0x138, 0xf, 0xf, false);
		const int sh = ln.sh;
		i32x4 rf;
		rf[0] = fmd::step_of(rp[0], before, sh);
#pragma unroll
		for (int v = 1; v < kVec; v++)
			rf[v] = fmd::step_of(rp[v], rp[v - 1], sh);

		const ptrdiff_t i = (ptrdiff_t)t0 + (ptrdiff_t)(kVec * tid) - (ptrdiff_t)kFmrxHalo;
		if (i >= 0 && i + kVec <= sn) {
			CORDIC_STORE_OUT(true, reinterpret_cast<ivec *>(amag + i), IO::narrow(rm));
			CORDIC_STORE_OUT(true, reinterpret_cast<ivec *>(afreq + i), IO::narrow(rf));
		} else if (i >= 0 && i < sn) {
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				if (i + v < sn) {
					amag[i + v] = (ielem)rm[v];
					afreq[i + v] = (ielem)rf[v];
				}
			}
		}
		// the lane with sample n - 1
		if (d_last && i >= 0 && i < sn && sn - i <= kVec) {
			const int k = (int)(sn - i);
			*d_last = k == 1 ? rp[0] : k == 2 ? rp[1] : k == 3 ? rp[2] : rp[3];
		}
	}
}

// ---- the single call's kernel arguments (its launchers: cordic_fm_rx_unit.h)
struct RxArgs {
	const uint32_t *fcw, *pm;	// pm may be NULL
	uint32_t *acc, *last;		// either may be NULL
	const uint32_t *work;		// [0] start, [1] prev, [4 + b] partials, conv
	const void *x, *y;		// int32 or int16, by the kernel's container
					// (IoC16: x interleaved, y not read)
	void	*mag, *freq;
	size_t	n, span;		// span: samples per block, whole passes less the halo
	uint32_t xw;			// LDS byte offset of the exchange words
};
// ---- host side of both units
// the tables and the exchange words behind them
inline size_t lds_bytes(const DxInfo &dx, uint32_t *xw)
{
	const uint32_t at = (dx_lds_layout(dx, nullptr, nullptr) + 15u) & ~15u;
	if (xw)
		*xw = at;
	return (size_t)at + kExWords * 4;
}

// resident blocks per CU: by the registers (see the head of cordic_fm_rx.hip),
// fewer where the tables fill the CU's 160 KiB sooner
inline size_t blocks_per_cu(size_t lds)
{
	const size_t per_cu = (160 * 1024) / lds;
	return per_cu > kFmrxBlocksPerCu ? kFmrxBlocksPerCu : per_cu;
}

} // namespace fmrx
} // namespace cordic_amd
#endif // __HIPCC__
#endif
