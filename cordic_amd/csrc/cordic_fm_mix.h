// cordic_fm_mix.h -- the FM mixer (cordic_plan_fm_mix, cordic_plan_fm_mix_info,
// cordic_plan_fm_mix_workspace, and cordic_plan_fm_mix16 / _workspace on int16
// I/Q arrays; include/cordic_amd.h): the rotator with
// looked-up directions whose phase is the running sum of per-sample tuning
// words, made in the kernel,
//   p_i = start + fcw[0] + .. + fcw[i-1] + pm[i]      (mod 2^32)
//   (ox_i, oy_i) = cordic_p2r(x_i, y_i, p_i).
// The launcher and the host checks for cordic_abi_fm.cpp, where the entry
// points live; the fallback (cordic_phase_accumulate into
// the workspace, then cordic_plan_p2r) is put together there, and so is the
// 16-bit fallback (widen, the 32-bit call, narrow).  The decimating mixer
// (cordic_plan_fm_mix_decim, _decim16: R = 2^k tuned samples summed, one kept)
// is the same launcher with k, its workspace and its fallback's launch.  Behind
// them, for hipcc only, the device functions that the kernel of this call and the kernel
// of the FM mixer banks (cordic_fm_mix_bank.hip) share.
//
// Neither unit holds a kernel of the DESIGN section 4.4 sweep (no swept
// workload has per-sample tuning words), so tools/build_stamp.py does not hash
// them.
#ifndef CORDIC_FM_MIX_H
#define CORDIC_FM_MIX_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"
#include "cordic_internal.h"
#include "cordic_table_fm.h"

namespace cordic_amd {

// Fused kernel: a block of 256 threads makes kFmxPass consecutive samples per
// pass, 4 per lane, and owns a contiguous span of whole passes; a launch has
// at most kFmxMaxBlocks blocks.  Its workspace is fm_reduce's: one word for
// the latched start (in a 16-byte slot) and one partial sum per block.
constexpr size_t kFmxPass = 1024;
constexpr size_t kFmxMaxBlocks = 4096;
constexpr size_t kFmxBlocksPerCu = 4;	// by its registers (cordic_fm_mix.hip)
constexpr size_t kFmxWorkBytes = 16 + 4 * kFmxMaxBlocks;

// Fallback: [cordic_phase_accumulate's own scratch | n phases]
constexpr size_t kFmxPhaseAt = kFmWorkBytes;
static_assert(kFmxPhaseAt % 16 == 0, "the phases sit on the 16-byte grid");

constexpr size_t fmx_work_bytes(bool fused, size_t n)
{
	return !n ? 0 : fused ? kFmxWorkBytes
		: kFmxPhaseAt + ((n * 4 + 15) & ~(size_t)15);
}

// 1: every n >= 1 of this plan runs the fused kernel -- the cores that
// launch_rot_feed sends to rotator_xydir, minus its batch-size threshold, where
// fm_mix_xydir has an instance (13, 16, 19, 20, 24, 27, 29 live stages).
// d_dir / dx: the plan's direction tables.  (The mode is the caller's to check.)
bool	fmx_is_fused(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx);

// The same question for the int16 container (cordic_plan_fm_mix16, a 16-bit
// bank): the fused plans of the 32-bit form with WW < 35.  The Io16 kernels are
// instantiated for LJ = 30 only; a core with 16-bit ports and WW 35 has 19 or
// more extra bits and takes the 16-bit fallback.
bool	fmx_is_fused16(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx);

// A call's form, for the plan-side FM layer (cordic_abi_fm.cpp) and the
// receiver's launchers: the sample arrays' container in bytes (4: int32, 2:
// int16), whether the input is ONE array of interleaved I/Q (the *_c16 forms,
// container 2), and k = log2r (0: not decimating).
struct FmForm {
	uint32_t container = 4;
	bool	iq = false;
	uint32_t log2r = 0;
	constexpr size_t esize() const { return container; }
	constexpr bool io16() const { return container == 2; }
	// the same call at k = 0; on split arrays
	constexpr FmForm plain() const { return FmForm{container, iq, 0}; }
	constexpr FmForm split() const { return FmForm{container, false, log2r}; }
};

// The 16-bit fallback widens into d_work, runs the 32-bit call there and
// narrows: [the 32-bit call's workspace | x | y | ox | oy], the four as int32,
// every part on the 16-byte grid.  fused32: fmx_is_fused of the plan.
constexpr size_t fmx16_array_bytes(size_t n)
{
	return (n * 4 + 15) & ~(size_t)15;
}
struct Fmx16Layout {
	size_t	x, y, ox, oy, end;	// byte offsets in d_work
};
// mix_bytes: the 32-bit call's own workspace
constexpr Fmx16Layout fmx16_layout(size_t mix_bytes, size_t n)
{
	const size_t each = fmx16_array_bytes(n);
	return Fmx16Layout{mix_bytes, mix_bytes + each, mix_bytes + 2 * each,
		mix_bytes + 3 * each, mix_bytes + 4 * each};
}
constexpr size_t fmx16_work_bytes(bool fused16, bool fused32, size_t n)
{
	return !n ? 0 : fused16 ? kFmxWorkBytes
		: fmx16_layout(fmx_work_bytes(fused32, n), n).end;
}
static_assert(kFmxWorkBytes % 16 == 0, "the widened arrays sit on the 16-byte grid");

// Alignment -- the four sample arrays on the grid of `esize`, their element
// size in bytes (4 or 2), the words on that of 4, d_work on that of 16 -- and
// no output range (d_acc and the `work_bytes` of d_work included) over
// anything else, by the true byte ranges; nothing is launched.  n > 0.  log2r:
// the two outputs hold n >> log2r elements (the decimating mixer).
// iq (the *_c16 mixers): d_xval is the one interleaved input (4 n bytes) and
// d_oxval the one interleaved output (4 (n >> log2r) bytes), both on the grid of
// a complex sample; d_yval and d_oyval are not looked at.
int	fmx_check_call(size_t n, const uint32_t *d_fcw, const uint32_t *d_pm,
		const uint32_t *d_acc, const void *d_xval, const void *d_yval,
		const void *d_oxval, const void *d_oyval, size_t esize, const void *d_work,
		size_t work_bytes, uint32_t log2r = 0, bool iq = false);

// The fused path: two launches on `stream` (fm_reduce, then fm_mix_xydir),
// nothing else.  The sample arrays hold int32 (esize 4) or int16 (esize 2).
// The caller has checked fmx_is_fused / fmx_is_fused16 and fmx_check_call.
// log2r = k in 1 .. 8: launch 2 is fm_mix_decim_xydir (cordic_fm_mix_decim.hip),
// which writes n >> k sums; n is a multiple of 2^k.
int	launch_fm_mix(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		size_t n, const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const void *d_xval, const void *d_yval, void *d_oxval,
		void *d_oyval, size_t esize, void *d_work, void *stream, uint32_t log2r = 0,
		bool iq = false);

// ---- the decimating mixer (cordic_plan_fm_mix_decim, _decim16), k = log2r in
// 1 .. 8 and n a multiple of 2^k.  Fused where the mixer is, with the mixer's
// workspace.  Its fallback is the mixer's call -- whatever path that takes --
// into two full-rate arrays inside d_work and one elementwise launch behind
// it: [the mixer call's workspace | tx | ty], each part on the 16-byte grid.
constexpr size_t fmxd_array_bytes(size_t n, size_t esize)
{
	return (n * esize + 15) & ~(size_t)15;
}
struct FmxdLayout {
	size_t	tx, ty, end;		// byte offsets in d_work
};
// mix_bytes: the mixer call's own workspace for n samples of that container
constexpr FmxdLayout fmxd_layout(size_t mix_bytes, size_t n, size_t esize)
{
	const size_t each = fmxd_array_bytes(n, esize);
	return FmxdLayout{mix_bytes, mix_bytes + each, mix_bytes + 2 * each};
}
constexpr size_t fmxd_work_bytes(bool fused, size_t mix_bytes, size_t n, size_t esize)
{
	return !n ? 0 : fused ? kFmxWorkBytes : fmxd_layout(mix_bytes, n, esize).end;
}

// log2r <= 8 and n a multiple of 2^log2r
constexpr bool fmxd_shape_ok(uint64_t n, uint32_t log2r)
{
	return log2r <= 8 && !(n & (((uint64_t)1 << log2r) - 1));
}

// The fallback's launch, on `stream`: d_ox[j], d_oy[j] = floor(the sum of 2^k
// consecutive elements of d_tx, d_ty / 2^k), j < n >> k; arrays of int32
// (esize 4) or int16 (2) at any element alignment.
int	launch_fmx_decimate(size_t n, uint32_t log2r, size_t esize, const void *d_tx,
		const void *d_ty, void *d_ox, void *d_oy, void *stream);

// The two elementwise launches of the 16-bit fallback, on `stream`: x and y
// into int32 arrays, ox and oy back into shorts (the low 16 bits: the 32-bit
// outputs are sign-extended OW-bit values, OW <= 16).  Any 2-byte alignment.
int	launch_fmx_widen(size_t n, const int16_t *d_x, const int16_t *d_y,
		int32_t *d_wx, int32_t *d_wy, void *stream);
int	launch_fmx_narrow(size_t n, const int32_t *d_wox, const int32_t *d_woy,
		int16_t *d_ox, int16_t *d_oy, void *stream);

// ---- the mixers on INTERLEAVED int16 I/Q, in and out (cordic_plan_fm_mix_c16,
// _decim_c16, cordic_mixbank_create_c16 / _create_decim_c16): the *16 twins with
// d_iq (complex sample i is the dword at d_iq + 2 i, I in its low half) in the
// place of d_xval / d_yval and d_oiq in that of d_oxval / d_oyval.  Fused where
// the twin is, with the twin's launches and workspace: launch_fm_mix with iq,
// whose launch 2 is a <30, N, IoC16io> instance (below).  The fallback is [the
// twin's workspace | x | y of n shorts | ox | oy of n >> k shorts], each part on
// the 16-byte grid: one split launch (launch_fmrx_split_c16, cordic_fm_rx.h),
// the twin, one interleave launch.
struct FmxC16Layout {
	size_t	x, y, ox, oy, end;	// byte offsets in d_work
};
constexpr FmxC16Layout fmx_c16_layout(size_t twin_bytes, size_t n, uint32_t log2r)
{
	const size_t at = (twin_bytes + 15) & ~(size_t)15;
	const size_t in = fmxd_array_bytes(n, 2), out = fmxd_array_bytes(n >> log2r, 2);
	return FmxC16Layout{at, at + in, at + 2 * in, at + 2 * in + out,
		at + 2 * in + 2 * out};
}
constexpr size_t fmx_c16_work_bytes(bool fused, size_t twin_bytes, size_t n, uint32_t log2r)
{
	return !n || fused ? twin_bytes : fmx_c16_layout(twin_bytes, n, log2r).end;
}
// d_oiq[2 j], d_oiq[2 j + 1] = d_ox[j], d_oy[j], j < m; d_oiq on the 4-byte grid
int	launch_fmx_interleave_c16(size_t m, const int16_t *d_ox, const int16_t *d_oy,
		int16_t *d_oiq, void *stream);

} // namespace cordic_amd

#ifdef __HIPCC__
// ---- device side: what fm_mix_xydir (cordic_fm_mix.hip) and the bank's
// fm_mixbank_xydir (cordic_fm_mix_bank.hip) are both made of -- the staging of
// the direction tables, the per-vector body of the rotator, the wave scan and
// the pass loop over a contiguous run of samples -- and what they share with
// the receiver's kernels (cordic_fm_rx.hip, cordic_fm_rx_bank.hip): the block's
// prologue and, on the host, the choice of the instance.
#include "cordic_xydir.h"

namespace cordic_amd {
namespace fmx {

using namespace dev;

// the arguments of launch 2 of a single call (fm_mix_xydir, and
// fm_mix_decim_xydir of cordic_fm_mix_decim.hip)
struct FmxArgs {
	const uint32_t *fcw, *pm;	// pm may be NULL
	uint32_t *acc;			// may be NULL
	const uint32_t *work;		// fm_reduce's: [0] start, [4 + b] partials
	const void *x, *y;		// int32 or int16, by the kernel's container
	void	*ox, *oy;
	size_t	n, span;		// span: samples per block, whole passes
	uint32_t xw;			// LDS byte offset of the 12 exchange words
};

typedef const __attribute__((address_space(3))) u32x4 lds_entry;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(3))) u32x2 lds_bucket;

// One vector through the rotator: the per-vector body of rotator_xydir's sweep
// (cordic_xydir.h:188-194 and 208-355) restated, because the sweep reads the
// phases it rotates by and stores what it computes.  Built from the same
// pieces in the same order; pb is the biased, left-justified phase of
// :204-205, rx / ry are the words the sweep would store to ox[g], oy[g]; ljc,
// maskv, bk_base and full_ports are the kernel's constants of :93-94 and
// :149-158.
template <int LJ, int NLIVE>
__device__ __forceinline__ void xydir_vector(const CoreParams &kp, const DirArgs &da,
		const LjRegs &ljc, const uint32_t (&maskv)[kDxMaxLevels],
		const uint32_t (&bk_base)[kDxMaxLevels], const bool full_ports, i32x4 tx,
		i32x4 ty, const uint32_t (&pb)[kVec], i32x4 &rx, i32x4 &ry)
{
	constexpr int kN = dx_levels(NLIVE);
	if (!full_ports) {		// :188-194, the ports
#pragma unroll
		for (int v = 0; v < kVec; v++) {
			tx[v] = sext32(tx[v], kp.iw);
			ty[v] = sext32(ty[v], kp.iw);
		}
	}
	int64_t x[kVec], y[kVec];
	uint32_t u[kVec];
	u32x4 m[kVec];
#pragma unroll
	for (int v = 0; v < kVec; v++)		// :211-215, the fold's row
		m[v] = *(lds_entry *)(uintptr_t)((pb[v] >> 25) & 0x70u);
#pragma unroll
	for (int v = 0; v < kVec; v++) {	// :216-225, fold and stage 1
		int64_t fx = op_mul(ty[v], (int32_t)m[v][2]);	// -B * i_y
		op_mad(fx, tx[v], (int32_t)m[v][0]);		// + A * i_x
		int64_t fy = op_mul(ty[v], (int32_t)m[v][0]);	//  A * i_y
		op_mad(fy, tx[v], (int32_t)m[v][1]);		// + B * i_x
		x[v] = (int64_t)((uint64_t)fx << LJ);
		y[v] = (int64_t)((uint64_t)fy << LJ);
		u[v] = (pb[v] & 0x3fffffffu) + m[v][3];
	}

	auto group = [&](auto G_) {		// :227-316, a group of looked-up stages
		constexpr int G = decltype(G_)::value;
		constexpr int T = dx_size(NLIVE, G);
		constexpr int K0 = dx_first(NLIVE, G);		// stages done
		constexpr bool more = (G + 1 < kN) || dx_rest(NLIVE) > 0;
		const uint32_t sh3 = (uint32_t)da.dx.lv[G].shift - 3u;
		u32x2 b2[kVec];
#pragma unroll
		for (int v = 0; v < kVec; v++) {
			uint32_t a;
			asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(a)
				: "v"(u[v] >> sh3), "v"(maskv[G]), "s"(bk_base[G]));
			b2[v] = *(lds_bucket *)(uintptr_t)a;
		}
		constexpr int W = 2 * T + (more ? 1 : 0);	// dwords used
		constexpr int kStride = dt_entry_dwords(T) * 4;
		static_assert(dt_entry_dwords(T) >= 2 * T + 1, "entry stride");
		uint32_t ea[kVec];
#pragma unroll
		for (int v = 0; v < kVec; v++) {
			const uint32_t cc = (b2[v][0] - u[v]) >> 31;	// u >= bound
			if constexpr ((kStride & (kStride - 1)) == 0)
				asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(ea[v])
					: "v"(cc), "n"(__builtin_ctz(kStride)), "v"(b2[v][1]));
			else if constexpr (kStride <= 64)
				asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(ea[v])
					: "v"(cc), "n"(kStride), "v"(b2[v][1]));
			else
				asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(ea[v])
					: "v"(cc), "s"(kStride), "v"(b2[v][1]));
		}
		uint32_t en[kVec][12];
#pragma unroll
		for (int v = 0; v < kVec; v++) {
#pragma unroll
			for (int at = 0; at < W; at += 4) {
				if (W - at >= 4) {
					const u32x4 t4 = *(lds_entry *)(uintptr_t)(ea[v] + 4u * at);
					en[v][at] = t4[0]; en[v][at + 1] = t4[1];
					en[v][at + 2] = t4[2]; en[v][at + 3] = t4[3];
				} else if (W - at == 3) {
					// (ds_read_b96, as the sweep reads them)
					typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
					const u32x3 t4 = *(const __attribute__((address_space(3)))
						u32x3 *)(uintptr_t)(ea[v] + 4u * at);
					en[v][at] = t4[0]; en[v][at + 1] = t4[1];
					en[v][at + 2] = t4[2];
				} else if (W - at == 2) {
					const u32x2 t2 = *(lds_bucket *)(uintptr_t)(ea[v] + 4u * at);
					en[v][at] = t2[0]; en[v][at + 1] = t2[1];
				} else {
					en[v][at] = *(const __attribute__((address_space(3)))
						uint32_t *)(uintptr_t)(ea[v] + 4u * at);
				}
			}
		}
		auto stage = [&](auto J_) {
			constexpr int J = decltype(J_)::value;
			if constexpr (J < T) {
				constexpr int K = K0 + J + 1;	// this stage's shift
#pragma unroll
				for (int v = 0; v < kVec; v++) {
					const int32_t ns_ = (int32_t)en[v][2 * J];
					const int32_t s_ = (int32_t)en[v][2 * J + 1];
					if constexpr (K < LjConst<LJ>::first)
						rot_stage_lj_early_dir<LJ, K>(x[v], y[v], ns_, s_);
					else
						rot_stage_lj_dir<LJ, K>(x[v], y[v], ns_, s_);
				}
			}
		};
		stage(std::integral_constant<int, 0>{});
		stage(std::integral_constant<int, 1>{});
		stage(std::integral_constant<int, 2>{});
		stage(std::integral_constant<int, 3>{});
		stage(std::integral_constant<int, 4>{});
		if constexpr (more) {
#pragma unroll
			for (int v = 0; v < kVec; v++)
				u[v] -= en[v][2 * T];
		}
	};
	if constexpr (kN > 0) group(std::integral_constant<int, 0>{});
	if constexpr (kN > 1) group(std::integral_constant<int, 1>{});
	if constexpr (kN > 2) group(std::integral_constant<int, 2>{});
	if constexpr (kN > 3) group(std::integral_constant<int, 3>{});
	if constexpr (kN > 4) group(std::integral_constant<int, 4>{});
	constexpr int kRest = dx_rest(NLIVE);
	if constexpr (kRest > 0) {		// :322-333, the residual stages
		int64_t p[kVec];
#pragma unroll
		for (int v = 0; v < kVec; v++) {
			const int32_t r = (int32_t)(u[v] - da.dx.bias_last);
			p[v] = (int64_t)(((uint64_t)(uint32_t)(r >> 1) << 32)
					| ((uint32_t)r << 31));
		}
		RotChainLJ<LJ, NLIVE, NLIVE - kRest, false>::run(x, y, p, kp, ljc);
	}

	if (kp.r_lj == 32) {			// :335-355, rounding
#pragma unroll
		for (int v = 0; v < kVec; v++) {
			rx[v] = round_to_ow_lj32<LJ>(x[v], kp);
			ry[v] = round_to_ow_lj32<LJ>(y[v], kp);
		}
	} else if (kp.r_lj > 32 && kp.r < 31) {
		const uint32_t sh = (uint32_t)kp.r_lj - 32u;
#pragma unroll
		for (int v = 0; v < kVec; v++) {
			rx[v] = round_to_ow_lj_hi<LJ>(x[v], kp, sh);
			ry[v] = round_to_ow_lj_hi<LJ>(y[v], kp, sh);
		}
	} else {
#pragma unroll
		for (int v = 0; v < kVec; v++) {
			rx[v] = round_to_ow_lj<LJ>(x[v], kp);
			ry[v] = round_to_ow_lj<LJ>(y[v], kp);
		}
	}
}

// v + the v of every lane in front, over the wave's 64 lanes: four shifts
// inside the rows of 16, then row 0's and 2's last lane to the row behind, then
// lane 31 to the upper half.  A lane without a source adds 0.
__device__ __forceinline__ uint32_t wave_scan(uint32_t v)
{
#define FMX_DPP(ctrl, rows) \
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xf, false)
	FMX_DPP(0x111, 0xf);	// row_shr:1
	FMX_DPP(0x112, 0xf);	// row_shr:2
	FMX_DPP(0x114, 0xf);	// row_shr:4
	FMX_DPP(0x118, 0xf);	// row_shr:8
	FMX_DPP(0x142, 0xa);	// row_bcast:15 into rows 1 and 3
	FMX_DPP(0x143, 0xc);	// row_bcast:31 into rows 2 and 3
#undef FMX_DPP
	return v;
}

// ---- the decimating mixer's integrate-and-dump (pass_loop with DECIM), by R =
// 2^k, 1 <= k <= 8 (wave-uniform).
//
// The sum of v over this lane and the g - 1 lanes in front of it, g = 1, 2, 4,
// .. 64 (wave-uniform), for the LAST lane of every aligned group of g: the
// inclusive wave scan less its value a group in front, which one ds_bpermute
// fetches (no LDS is addressed); the wave's first group has nothing in front.
// The scan wraps modulo 2^32 and the difference undoes it.  Every lane of the
// wave runs this (DPP and the permute read inactive lanes as garbage).
__device__ __forceinline__ uint32_t group_sum(uint32_t v, const uint32_t g,
		const unsigned lane)
{
	const uint32_t s = wave_scan(v);
	const uint32_t p = (uint32_t)__builtin_amdgcn_ds_bpermute(
		(int)(((lane - g) & 63u) << 2), (int)s);
	return s - (lane >= g ? p : 0u);
}

// rx / ry: this lane's 4 tuned samples, numbers i .. i + 3 of the job (i a
// multiple of 4); hi: the job's or span's end, a multiple of R.  Writes
// ox[i >> k], oy[i >> k] = floor(sum of the group / R) for every group in front
// of hi, from the lane that holds the group's last sample, and nothing else.  A
// group is 2^(k-2) neighbouring lanes (k = 1: half a lane), never more than a
// wave, and lies wholly in front of hi or wholly behind.  The exact sum has OW
// + k bits; it travels as sum(v >> k), below 2^31 in magnitude, and sum(v & (R
// - 1)), below 2^16: floor(S / R) = the first + (the second >> k).  Plain
// stores: non-temporal ones measured the same (profiles/r22/ab_nt_stores.txt).
//
// OIQ (the interleaved output of IoC16io, below): ox is d_oiq, output j is the
// dword at ox + 2 j, packed (I | Q << 16), and oy is not looked at.  k = 1: the
// lane's two outputs are one 8-byte store (hi is a multiple of 2 only: where i +
// 2 == hi the one dword); k >= 2: one dword where the split form has two 2-byte
// stores.
__device__ __forceinline__ uint32_t pack_iq(int32_t re, int32_t im)
{
	return ((uint32_t)re & 0xffffu) | ((uint32_t)im << 16);
}

template <bool OIQ = false, typename T>
__device__ __forceinline__ void store_decim(const i32x4 &rx, const i32x4 &ry, T *ox,
		T *oy, const size_t i, const size_t hi, const uint32_t k, const unsigned tid)
{
	if (k == 1) {		// two outputs per lane
		const size_t o = i >> 1;
		if constexpr (OIQ) {
			typedef u32x2 u32x2g __attribute__((aligned(4)));
			u32x2 d;
#pragma unroll
			for (int h = 0; h < 2; h++) {
				const int32_t a = rx[2 * h], b = rx[2 * h + 1];
				const int32_t c = ry[2 * h], e = ry[2 * h + 1];
				d[h] = pack_iq((a >> 1) + (b >> 1) + (((a & 1) + (b & 1)) >> 1),
					(c >> 1) + (e >> 1) + (((c & 1) + (e & 1)) >> 1));
			}
			uint32_t *o2 = reinterpret_cast<uint32_t *>(ox) + o;
			if (i + kVec <= hi)
				*reinterpret_cast<u32x2g *>(o2) = d;
			else if (i < hi)
				o2[0] = d[0];
			return;
		}
#pragma unroll
		for (int h = 0; h < 2; h++) {
			if (i + 2 * h < hi) {
				const int32_t a = rx[2 * h], b = rx[2 * h + 1];
				const int32_t c = ry[2 * h], d = ry[2 * h + 1];
				ox[o + h] = (T)((a >> 1) + (b >> 1) + (((a & 1) + (b & 1)) >> 1));
				oy[o + h] = (T)((c >> 1) + (d >> 1) + (((c & 1) + (d & 1)) >> 1));
			}
		}
		return;
	}
	const uint32_t low = (1u << k) - 1u;
	uint32_t hx = 0, lx = 0, hy = 0, ly = 0;
#pragma unroll
	for (int v = 0; v < kVec; v++) {
		hx += (uint32_t)(rx[v] >> k);
		lx += (uint32_t)rx[v] & low;
		hy += (uint32_t)(ry[v] >> k);
		ly += (uint32_t)ry[v] & low;
	}
	const uint32_t g = 1u << (k - 2);	// lanes of a group
	const unsigned lane = tid & 63u;
	if (k > 2) {
		hx = group_sum(hx, g, lane);
		lx = group_sum(lx, g, lane);
		hy = group_sum(hy, g, lane);
		ly = group_sum(ly, g, lane);
	}
	if ((lane & (g - 1u)) == g - 1u && i < hi) {
		if constexpr (OIQ) {
			reinterpret_cast<uint32_t *>(ox)[i >> k] = pack_iq(
				(int32_t)(hx + (lx >> k)), (int32_t)(hy + (ly >> k)));
		} else {
			ox[i >> k] = (T)(int32_t)(hx + (lx >> k));
			oy[i >> k] = (T)(int32_t)(hy + (ly >> k));
		}
	}
}

// The block's prologue: the fold's rows and the groups' tables into LDS
// (cordic_xydir.h:97-139).  The caller's barrier follows.
template <int LJ, int NLIVE>
__device__ __forceinline__ void stage_tables(const CoreParams &kp, const DirArgs &da,
		uint32_t *lds, const uint32_t (&bk_base)[kDxMaxLevels],
		const uint32_t (&lf_base)[kDxMaxLevels], const unsigned tid)
{
	constexpr int kN = dx_levels(NLIVE);
	if (tid < 8) {
		const int q = tid >> 1;
		const int32_t dir = (tid & 1) ? 1 : -1;	// phase >= 0 : < 0
		const int32_t k = (int32_t)(1u << (kp.in_shl & 31));
		const int32_t cs = (q == 0) ? k : (q == 2) ? -k : 0;
		const int32_t sn = (q == 1) ? k : (q == 3) ? -k : 0;
		int32_t *row = reinterpret_cast<int32_t *>(lds) + tid * 4;
		const int32_t ra = cs - dir * (sn / 2), rb = sn + dir * (cs / 2);
		row[0] = ra;
		row[1] = rb;
		row[2] = -rb;
		row[3] = (int32_t)(da.dx.bias0 - 0x20000000u
				- (uint32_t)(dir * (int32_t)kp.angle[0]));
	}
#pragma unroll
	for (int g = 0; g < kN; g++) {
		const DtLevel lv = da.dx.lv[g];
		const uint32_t *src = da.table + lv.word;
		uint32_t *bk = lds + bk_base[g] / 4u;
		const uint32_t stride = (uint32_t)dt_entry_dwords(lv.t) * 4u;
		for (int i = tid; i < lv.nb * 2; i += kBlock) {
			const uint32_t w = src[i];
			bk[i] = (i & 1) ? lf_base[g] + w * stride : w;
		}
		const uint32_t *lsrc = src + (size_t)lv.nb * 2;
		uint32_t *lf = lds + lf_base[g] / 4u;
		for (int e = tid; e < lv.nl; e += kBlock) {
			const uint32_t pat = lsrc[2 * e];
			uint32_t *d = lf + (size_t)e * dt_entry_dwords(lv.t);
			for (int jj = 0; jj < lv.t; jj++) {
				// bit set: residual >= 0 at that stage, s = +1
				const bool pos = (pat >> (lv.t - 1 - jj)) & 1u;
				const uint32_t plus = LjConst<LJ>::bit;
				const uint32_t minus = LjConst<LJ>::mask | LjConst<LJ>::bit;
				d[2 * jj + 0] = pos ? minus : plus;	// -s 2^LJ (x)
				d[2 * jj + 1] = pos ? plus : minus;	//  s 2^LJ (y)
			}
			d[2 * lv.t] = lsrc[2 * e + 1];		// u_next = u - this
		}
	}
}

// the sum of work[0 .. count) over the block, in four shares: ex[8 + wave].
// The caller's barrier follows; ex[8] + .. + ex[11] is the sum.
__device__ __forceinline__ void front_sum(const uint32_t *work, unsigned count,
		uint32_t *ex, const unsigned tid, const unsigned wave)
{
	uint32_t s = 0;
	for (unsigned j = tid; j < count; j += kBlock)
		s += work[j];
#pragma unroll
	for (int d = 32; d; d >>= 1)
		s += __shfl_xor(s, d);
	if ((tid & 63u) == 0)
		ex[8 + wave] = s;
}

// the rotator's constants that live in registers for the whole kernel
struct RotRegs {
	LjRegs	ljc;
	uint32_t maskv[kDxMaxLevels];
	uint32_t k45;
	bool	full_ports;	// wave-uniform: no sign extension
};

template <int LJ, int NLIVE>
__device__ __forceinline__ RotRegs rot_regs(const CoreParams &kp, const DirArgs &da)
{
	RotRegs r{};
	r.ljc.mask = vgpr_const(LjConst<LJ>::mask);
	r.ljc.bit = vgpr_const(LjConst<LJ>::bit);
	r.ljc.maskbit = vgpr_const(LjConst<LJ>::mask | LjConst<LJ>::bit);
#pragma unroll
	for (int g = 0; g < dx_levels(NLIVE); g++)
		r.maskv[g] = vgpr_const(((uint32_t)da.dx.lv[g].nb - 1u) << 3);
	r.k45 = vgpr_const(0x20000000u);
	r.full_ports = kp.iw == 32;
	return r;
}

// ---- IoC16: the container of INTERLEAVED int16 I/Q on the input side (the
// *_c16 receivers, include/cordic_amd.h): complex sample i is the dword at iq +
// 2 i, I in its low half and Q in its high half.  The outputs are Io16's (two
// separate int16 arrays), so everything the kernels ask a container for on the
// store side is inherited.  A lane's 4 complex samples are ONE 16-byte load at
// any 4-byte-aligned address (the element alignment of `cvec`, as u32x4g's);
// they wait for their pass as the 4 dwords they are and are separated in
// registers: v_bfe_i32 for I, v_ashrrev_i32 for Q, the two instructions per
// sample that the widening of two packed shorts costs Io16.  The loops take the
// new path behind is_iq<IO> (if constexpr) and an overload of widen_iq; for
// Io32 / Io16 they are the code they were.  The receiver kernels use it; if the
// mixer family wants the format, fmx::pass_loop takes the same policy.
struct IoC16 : Io16 {
	typedef u32x4 cvec __attribute__((aligned(4)));
};
// IoC16io: interleaved on BOTH sides (the *_c16 mixers): the input is IoC16's,
// and the two outputs are one array, complex sample j the dword (I | Q << 16) at
// oiq + 2 j -- a lane's 4 are ONE 16-byte store at any 4-byte-aligned address,
// packed in registers (v_and_or / v_lshl_or per sample, the two that narrowing
// two values to shorts costs Io16); fmx::pass_loop stores them behind
// is_oiq<IO>, and store_decim one dword per decimated sample.
struct IoC16io : IoC16 {};
template <typename IO> struct is_iq : std::false_type {};
template <> struct is_iq<IoC16> : std::true_type {};
template <> struct is_iq<IoC16io> : std::true_type {};
template <typename IO> struct is_oiq : std::false_type {};
template <> struct is_oiq<IoC16io> : std::true_type {};
// 4 input samples of one array as they wait in registers (IoC16: of both)
template <typename IO> struct raw_in {
	typedef decltype(IO::narrow(i32x4{})) type;
};
template <> struct raw_in<IoC16> {
	typedef u32x4 type;
};
template <> struct raw_in<IoC16io> : raw_in<IoC16> {};
// a lane's (x, y) from what it loaded
template <typename IO, typename RAW>
__device__ __forceinline__ void widen_iq(IO, const RAW &nx, const RAW &ny, i32x4 &tx,
		i32x4 &ty)
{
	tx = IO::widen(nx);
	ty = IO::widen(ny);
}
__device__ __forceinline__ void widen_iq(IoC16, const u32x4 &q, const u32x4 &, i32x4 &tx,
		i32x4 &ty)
{
#pragma unroll
	for (int v = 0; v < kVec; v++) {
		tx[v] = (int32_t)(q[v] << 16) >> 16;
		ty[v] = (int32_t)q[v] >> 16;
	}
}
__device__ __forceinline__ void widen_iq(IoC16io, const u32x4 &q, const u32x4 &n, i32x4 &tx,
		i32x4 &ty)
{
	widen_iq(IoC16{}, q, n, tx, ty);
}

// ---- the block's prologue, of all four launch-2 kernels (fm_mix_xydir,
// fm_mixbank_xydir, fm_rx_xydir, fm_rxbank_xydir): one piece for each side of
// the barrier, which is the caller's -- a single call puts its front_sum
// between the two, a bank has its own per span.  The kernels keep five lines
// of their own in front: the DYNAMIC block `lds` (the table lookups address LDS
// by byte offset from 0, which a static __shared__ object would displace), tid,
// wave, the two arrays that dx_lds_layout fills, and ex behind the tables.
// Held in a struct that block_begin returns, or filled through a reference by a
// dx_lds_layout called from here, hipcc makes other code of them
// (profiles/r21/fm_fold_isa.txt).
//
// In front of the barrier: the fold's rows and the groups' tables into LDS.
template <int LJ, int NLIVE, typename IO>
__device__ __forceinline__ void block_begin(const CoreParams &kp, const DirArgs &da,
		uint32_t *lds, const uint32_t (&bk_base)[kDxMaxLevels],
		const uint32_t (&lf_base)[kDxMaxLevels], const unsigned tid)
{
	static_assert(LJ == 29 || LJ == 30, "WW <= 35 cores");
	static_assert(LJ == 30 || sizeof(typename IO::ielem) == 4,
		"16-bit ports and WW 35: the fallback, or one by one (fmx_is_fused16)");
	constexpr int kN = dx_levels(NLIVE);
	static_assert(kN >= 1 && kN <= kDxMaxLevels, "no group to look up");
	stage_tables<LJ, NLIVE>(kp, da, lds, bk_base, lf_base, tid);
}

// Behind it: the trap on an LDS block that does not begin at 0, and the
// rotator's registers.
template <int LJ, int NLIVE>
__device__ __forceinline__ RotRegs block_ready(const CoreParams &kp, const DirArgs &da,
		const uint32_t *lds)
{
	if ((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)lds != 0u)
		__builtin_trap();
	return rot_regs<LJ, NLIVE>(kp, da);
}

// The pass loop: samples [lo, hi) of the six arrays, 1024 per pass, 4 per lane.
// carry: in, the phase of sample lo without its pm; out, that of sample hi.
// par: the parity of the exchange words ex[0 .. 8), which are double-buffered
// by pass, so that a pass has ONE barrier; it runs on from call to call.
// pm may be NULL (wave-uniform).  Nothing at or behind hi is read or written.
//
// IO (Io32 / Io16, cordic_device.h, or IoC16io above; deduced from the tag
// behind `wave`) is the container of the four sample arrays and of nothing else
// (IoC16io: ax is d_iq, aox is d_oiq, complex sample i at + 2 i shorts, ay and
// aoy are not looked at; the load and the store take the paths behind is_iq<IO>
// and is_oiq<IO>, and for the other two the loop is the code it was): a lane's 4 samples
// are one 16-byte or one 8-byte access per array, at any element alignment,
// widened behind the load and narrowed in front of the store; the tuning words
// and pm are 32-bit words in either, and so is everything in between.  The
// next pass's samples wait in the container's own vector (two registers per
// array for Io16), so Io32 is the loop it was.
//
// DECIM (deduced from a std::true_type behind the container's tag; the
// decimating mixer, cordic_fm_mix_decim.hip and cordic_fm_mix_bank_decim.hip):
// the tuned samples are not stored but summed in groups of 2^log2r and one
// value per group is (store_decim, above); hi - lo and lo are multiples of
// 2^log2r, aox / aoy are indexed by sample >> log2r.  Everything in front of
// the stores is the same text, and without the tag the loop is the code it was.
template <int LJ, int NLIVE, typename IO, bool DECIM = false>
__device__ __forceinline__ void pass_loop(const CoreParams &kp, const DirArgs &da,
		const RotRegs &rr, const uint32_t (&bk_base)[kDxMaxLevels],
		const uint32_t *fcw, const uint32_t *pm, const typename IO::ielem *ax,
		const typename IO::ielem *ay, typename IO::ielem *aox,
		typename IO::ielem *aoy, const size_t lo, const size_t hi, uint32_t &carry,
		unsigned &par, uint32_t *ex, const unsigned tid, const unsigned wave, IO,
		std::integral_constant<bool, DECIM> = {},
		[[maybe_unused]] const uint32_t log2r = 0)
{
	typedef typename IO::ivec ivec;
	typedef typename IO::ielem ielem;
	// 4 samples as they lie in memory (interleaved: 4 complex ones, in x)
	typedef typename raw_in<IO>::type raw4;
	// this lane's 4 samples of the pass at t0; nothing at or behind hi is read,
	// and a tuning word that is not there counts 0
	auto load_pass = [&](size_t t0, u32x4 &f, u32x4 &m, raw4 &x, raw4 &y) {
		const size_t i = t0 + (size_t)kVec * tid;
		f = u32x4{};
		m = u32x4{};
		x = raw4{};
		y = raw4{};
		if (i + kVec <= hi) {
			f = CORDIC_LOAD_IN(reinterpret_cast<const u32x4g *>(fcw + i));
			if (pm)	// (wave-uniform)
				m = CORDIC_LOAD_IN(reinterpret_cast<const u32x4g *>(pm + i));
			if constexpr (is_iq<IO>::value) {
				x = CORDIC_LOAD_IN(reinterpret_cast<const typename IO::cvec *>(ax + 2 * i));
			} else {
				x = CORDIC_LOAD_IN(reinterpret_cast<const ivec *>(ax + i));
				y = CORDIC_LOAD_IN(reinterpret_cast<const ivec *>(ay + i));
			}
		} else if (i < hi) {	// the last, partial vector: one lane of the job
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				if (i + v < hi) {
					f[v] = fcw[i + v];
					if (pm)
						m[v] = pm[i + v];
					if constexpr (is_iq<IO>::value) {
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
	load_pass(lo, nf, nm, nx, ny);
	for (size_t t0 = lo; t0 < hi; t0 += kFmxPass) {
		const u32x4 f = nf, m = nm;
		i32x4 tx, ty;
		widen_iq(IO{}, nx, ny, tx, ty);
		// the next pass's words are on their way while this one is rotated
		if (t0 + kFmxPass < hi)
			load_pass(t0 + kFmxPass, nf, nm, nx, ny);

		// inclusive sums: in the lane, then over the wave's lanes
		const uint32_t s0 = f[0], s1 = s0 + f[1], s2 = s1 + f[2], s3 = s2 + f[3];
		const uint32_t incl = wave_scan(s3);
		if ((tid & 63u) == 63u)
			ex[par * 4 + wave] = incl;
		__syncthreads();
		const u32x4 w = *reinterpret_cast<const u32x4 *>(ex + par * 4);
		par ^= 1;
		// the waves in front of this one, and the pass's total
		const uint32_t front = (wave > 0 ? w[0] : 0u) + (wave > 1 ? w[1] : 0u)
			+ (wave > 2 ? w[2] : 0u);
		const uint32_t excl = carry + front + incl - s3;
		carry += w[0] + w[1] + w[2] + w[3];

		const uint32_t ph[kVec] = {excl + m[0], excl + s0 + m[1], excl + s1 + m[2],
			excl + s2 + m[3]};
		uint32_t pb[kVec];
#pragma unroll
		for (int v = 0; v < kVec; v++)	// cordic_xydir.h:202-205
			asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(pb[v])
				: "v"(ph[v]), "s"(kp.pw_shl), "v"(rr.k45));

		i32x4 rx, ry;
		xydir_vector<LJ, NLIVE>(kp, da, rr.ljc, rr.maskv, bk_base, rr.full_ports, tx,
			ty, pb, rx, ry);

		const size_t i = t0 + (size_t)kVec * tid;
		if constexpr (DECIM) {
			store_decim<is_oiq<IO>::value>(rx, ry, aox, aoy, i, hi, log2r, tid);
		} else if constexpr (is_oiq<IO>::value) {
			// four packed dwords at aox + 2 i; the last, partial vector dword
			// by dword
			u32x4 d;
#pragma unroll
			for (int v = 0; v < kVec; v++)
				d[v] = pack_iq(rx[v], ry[v]);
			uint32_t *o = reinterpret_cast<uint32_t *>(aox) + i;
			if (i + kVec <= hi) {
				CORDIC_STORE_OUT(true, reinterpret_cast<typename IO::cvec *>(o), d);
			} else if (i < hi) {
#pragma unroll
				for (int v = 0; v < kVec; v++)
					if (i + v < hi)
						o[v] = d[v];
			}
		} else if (i + kVec <= hi) {
			CORDIC_STORE_OUT(true, reinterpret_cast<ivec *>(aox + i), IO::narrow(rx));
			CORDIC_STORE_OUT(true, reinterpret_cast<ivec *>(aoy + i), IO::narrow(ry));
		} else if (i < hi) {
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				if (i + v < hi) {
					aox[i + v] = (ielem)rx[v];
					aoy[i + v] = (ielem)ry[v];
				}
			}
		}
	}
}

// ---- host side of both units
// the tables and the 12 exchange words behind them
inline size_t lds_bytes(const DxInfo &dx, uint32_t *xw)
{
	const uint32_t at = (dx_lds_layout(dx, nullptr, nullptr) + 15u) & ~15u;
	if (xw)
		*xw = at;
	return (size_t)at + 12 * 4;
}

// resident blocks per CU: 4 waves of a SIMD by the registers (see the heads of
// the two units), fewer where the tables fill the CU's 160 KiB sooner
inline size_t blocks_per_cu(size_t lds)
{
	const size_t per_cu = (160 * 1024) / lds;
	return per_cu > kFmxBlocksPerCu ? kFmxBlocksPerCu : per_cu;
}

// ---- which instance serves a plan, for all four launch-2 kernels
// <LJ, container> of a core of working width ww on samples of esize bytes: the
// one home of "WW 35 is LJ 29" and "no Io16 at WW 35" (fmx_is_fused16).  The
// receiver's units, compiled once per value, index their entry points by it
// (their list, in this order: cordic_fm_rx_unit.h).
// kUnitC16: the receivers' <30, IoC16> units, for interleaved 16-bit input --
// where Io16 serves, and nowhere else.
enum Unit { kUnitNone = -1, kUnitLj30 = 0, kUnitLj29 = 1, kUnitIo16 = 2, kUnitC16 = 3 };
constexpr Unit unit_of(int ww, size_t esize)
{
	return esize == 2 ? (ww < 35 ? kUnitIo16 : kUnitNone)
		: ww == 35 ? kUnitLj29 : kUnitLj30;
}
constexpr Unit unit_of(int ww, size_t esize, bool iq)
{
	const Unit u = unit_of(ww, esize);
	return !iq ? u : u == kUnitIo16 ? kUnitC16 : kUnitNone;
}

// Calls f(integral_constant<int, LJ>, IO) for the unit; false: none, or f's.
// kUnitC16 is NOT served here and answers false: its instances live in objects
// of their own, behind launchers of their own -- the receivers' in
// cordic_fm_rx_unit.h, the mixers' launch_fm_mix_scan_c16 and its three kin
// (below, and cordic_fm_mix_bank.h) -- so that a unit that calls with_unit does
// not instantiate them.  A launcher that can meet kUnitC16 asks for it by name
// in front of this call (launch_fm_mix, launch_fm_mix_decim_scan,
// launch_fmx_bank, launch_fmx_bank_decim_walk); one that forgets launches
// nothing and reports CORDIC_ERR_DEVICE through tnco::finish(false), which the
// per-instance tests of tests/test_fm_mix_c16.py and _bank.py would show.
template <typename F>
bool with_unit(Unit u, F &&f)
{
	switch (u) {
	case kUnitLj30: return f(std::integral_constant<int, 30>{}, Io32{});
	case kUnitLj29: return f(std::integral_constant<int, 29>{}, Io32{});
	case kUnitIo16: return f(std::integral_constant<int, 30>{}, Io16{});
	default: return false;
	}
}

// the stage counts the job-set instances of rotator_xydir carry
// (cordic_jobs_xydir.hip)
#define FMX_STAGES(X) X(13) X(16) X(19) X(20) X(24) X(27) X(29)

// Calls f(integral_constant<int, N>) for N = nlive; false, and no call, where
// no kernel is instantiated for nlive or the tables have another number of
// groups than the instance looks up (the shape of fmd::with_instance).
template <typename F>
bool with_stages(int nlive, int ngroups, F &&f)
{
	switch (nlive) {
#define X(N) case N: \
	if (ngroups != dx_levels(N)) \
		return false; \
	f(std::integral_constant<int, N>{}); \
	return true;
	FMX_STAGES(X)
#undef X
	default:
		return false;
	}
}

} // namespace fmx

// Launch 2 of a decimating single call, for launch_fm_mix
// (cordic_fm_mix_decim.hip); false: no instance.
bool	launch_fm_mix_decim_scan(fmx::Unit unit, int nlive, int ngroups, unsigned grid,
		size_t lds, void *stream, const dev::CoreParams &kp, const dev::DirArgs &da,
		const fmx::FmxArgs &a, uint32_t log2r);

// Launch 2 on interleaved int16 I/Q, in and out (fmx::kUnitC16; a.x is d_iq,
// a.ox is d_oiq): the <30, N, IoC16io> instances.  fmx::with_unit does not know
// them: each of the four mixer sources (cordic_fm_mix.hip, .._decim.hip,
// .._bank.hip, .._bank_decim.hip) is compiled a second time with
// -DCORDIC_FMX_C16 into an object of its own, which holds the kernel's 7
// instances and one launcher -- these two, and the banks' two in
// cordic_fm_mix_bank.h -- so that they build beside the others.  The plain form
// ignores log2r.  false: no instance.
typedef bool FmxScanC16(int nlive, int ngroups, unsigned grid, size_t lds, void *stream,
		const dev::CoreParams &kp, const dev::DirArgs &da, const fmx::FmxArgs &a,
		uint32_t log2r);
FmxScanC16 launch_fm_mix_scan_c16, launch_fm_mix_decim_scan_c16;

} // namespace cordic_amd
#endif // __HIPCC__
#endif
