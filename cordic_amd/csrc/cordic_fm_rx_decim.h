// cordic_fm_rx_decim.h -- the decimating FM receiver (cordic_plan_fm_rx_decim,
// cordic_plan_fm_rx_decim16 and their _workspace; include/cordic_amd.h): the FM
// mixer, the integrate-and-dump by R = 2^k and the FM discriminator in ONE
// kernel,
//   (tx_i, ty_i) = what cordic_plan_fm_mix writes for sample i
//   (dx_j, dy_j) = floor((tx_(jR) + .. + tx_(jR+R-1)) / R), likewise y
//   (mag_j, ph_j) = what cordic_r2p writes for (dx_j, dy_j) on conv
//   freq_j       = sext_PW((ph_j - ph_(j-1)) mod 2^PW),
// neither the tuned nor the decimated I/Q stored.  The geometry's constants and
// the workspace rule for cordic_abi_fm.cpp, where the fallback (the decimating
// mixer into two arrays inside the workspace, then cordic_fm_demod from them)
// is put together; the launcher is launch_fm_rx (cordic_fm_rx.h) with log2r.
// Behind them, for hipcc only, the pass loop of the call's kernel
// (cordic_fm_rx_decim.hip), written over ONE span as fmrx::pass_loop is.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_FM_RX_DECIM_H
#define CORDIC_FM_RX_DECIM_H

#include <cstddef>
#include <cstdint>

#include "cordic_fm_rx.h"

namespace cordic_amd {

// The staging ring of decimated samples in the block's LDS, behind the tables
// and the exchange words: kFmrxdRing slots of one int32 in each of two planes
// (x, then y), 16 KiB.  A flush converts 1024 of them; a pass adds at most 512
// (k = 1) behind what a flush left, fewer than 1024: at most 1535 are live, so
// 1536 slots would do; 2048 make the slot's index a mask, for 4 KiB more.
constexpr size_t kFmrxdRing = 2048;
constexpr size_t kFmrxdFlush = 1024;		// decimated samples per flush
constexpr size_t kFmrxdExWords = 24;		// fmrx's 20, [20] the halo's total
constexpr size_t kFmrxdLdsExtra = kFmrxdExWords * 4 + 2 * kFmrxdRing * 4;

// the input samples in front of a span that are rotated and summed again for
// the phase of the decimated sample in front: max(4, R)
constexpr size_t fmrxd_halo(uint32_t log2r)
{
	return log2r > 2 ? (size_t)1 << log2r : 4;
}

// Fallback: [the decimating mixer call's workspace | T_x | T_y of n >> k
// elements | the discriminator's workspace for n >> k], each part on the
// 16-byte grid: fmrx_layout (cordic_fm_rx.h) with m = n >> k.  mixd_bytes: cordic_plan_fm_mix_decim_workspace(n, k) (_decim16).
constexpr size_t fmrxd_work_bytes(bool fused, size_t mixd_bytes, size_t n, uint32_t log2r,
		size_t esize)
{
	return !n ? 0 : fused ? kFmrxWorkBytes
		: fmrx_layout(mixd_bytes, n >> log2r, esize).end;
}

} // namespace cordic_amd

#ifdef __HIPCC__
namespace cordic_amd {
namespace fmrxd {

using namespace dev;

typedef __attribute__((address_space(3))) int32_t lds_i32;
typedef const __attribute__((address_space(3))) i32x4 lds_i32x4;

// The pass loop: input samples [0, n) of ONE span, n a multiple of R = 2^k (k
// in 1 .. 8, wave-uniform), whose four input arrays begin at the span's first
// sample and whose two outputs begin at its first DECIMATED sample; m = n >> k
// of those are written.
//
// FRONT HALF of a pass, fmx::pass_loop's decimating form up to the group sum:
// lane j of the span (j = 256 * pass + thread) has the input samples 4 j - H ..
// 4 j - H + 3, H = max(4, R): the first H / 4 <= 64 lanes, all in wave 0 of the
// first pass, are the HALO, the R samples of the decimated sample in front of
// the span (k = 1: the two in front), rotated and summed like any others.
// first: the span begins at sample 0 of its job; the halo lanes load nothing,
// stage nothing and `prev` is lent instead.  The halo's tuning words take part
// in the scan; their total -- the inclusive scan at lane H / 4 - 1 of wave 0,
// through ex[20], written in front of the scan's barrier -- is taken off
// `carry`, so that the halo's phases are carry - fcw[-1] - .. : the bits of its
// own span.  The owner of a group (its last lane for k >= 2, both halves of a
// lane for k = 1) writes the floored sums to the ring: decimated sample d of the
// span to STREAM slot d + 4 (the halo's to slot 3), ring slot = stream slot &
// (kFmrxdRing - 1).  Groups are aligned in the lanes because 1024 and H are
// multiples of R.
//
// FLUSH, whenever kFmrxdFlush stream slots are complete behind the last flush,
// and at the span's end for the rest: fmrx::pass_loop's back half on the ring.
// Lane t of flush f reads stream slots 1024 f + 4 t .. + 3, converts them, gets
// the phase in front from lane t - 1 (wave_shr:1), from the wave in front (edge
// words) or from the flush before (wave 3's edge word of the other parity) and
// stores one vector at decimated sample 1024 f + 4 t - 4: lane 0 of flush 0 has
// slots 0 .. 3 and stores nothing.  Slots 0 .. 2 (and 3 of a first span) hold
// whatever LDS held: their results reach no store.
//
// BARRIERS.  (A) at the head of a flush orders the ring writes of this pass and
// of those before it in front of the flush's reads.  The ring reads of a flush
// in pass p are ordered in front of the overwrite of their slots by the scan's
// barrier of pass p + 1: a slot is written again 2048 stream slots later, which
// is at least two passes on (a pass completes at most 512), and a pass writes
// the ring behind its scan's barrier.  (B), the edges' barrier of
// fmrx::pass_loop, stands between a wave's edge word and its reader; the edge
// words are double-buffered by flush (fpar) as the receiver's are by pass.
// ex[20] is written in a span's first pass in front of the scan's barrier and
// read behind it; every span ends in a flush, whose (A) and (B) lie between
// that read and the next span's write.
// carry, par, ckmem, d_last, pm: as fmrx::pass_loop.  fpar: the parity of the
// edge words, which runs on from span to span like par.
template <int LJ, int NLIVE, typename IO>
__device__ __forceinline__ void pass_loop(const CoreParams &kp, const DirArgs &da,
		const fmx::RotRegs &rr, const uint32_t (&bk_base)[kDxMaxLevels],
		const uint32_t *ckmem, const fmd::LaneConsts &ln, const uint32_t *fcw,
		const uint32_t *pm, const typename IO::ielem *ax,
		const typename IO::ielem *ay, typename IO::ielem *amag,
		typename IO::ielem *afreq, const size_t n, const uint32_t k, const bool first,
		const uint32_t prev, uint32_t *d_last, uint32_t &carry, unsigned &par,
		unsigned &fpar, uint32_t *ex, const uint32_t ring_at, const unsigned tid,
		const unsigned wave, IO)
{
	typedef typename IO::ivec ivec;
	typedef typename IO::ielem ielem;
	// 4 samples as they lie in memory (IoC16: 4 complex ones, in x; ay unused)
	typedef typename fmx::raw_in<IO>::type raw4;
	const ptrdiff_t sn = (ptrdiff_t)n;
	const ptrdiff_t halo_n = k > 2 ? (ptrdiff_t)1 << k : 4;
	const ptrdiff_t sm = sn >> k;			// decimated samples of the span
	const unsigned lane = tid & 63u;
	// the ring's planes, by LDS byte offset (the block's LDS begins at 0)
	const uint32_t ringx = ring_at, ringy = ring_at + (uint32_t)kFmrxdRing * 4u;
	// this lane's 4 samples of the pass at t0
	auto load_pass = [&](size_t t0, u32x4 &f, u32x4 &m, raw4 &x, raw4 &y) {
		const ptrdiff_t i = (ptrdiff_t)t0 + (ptrdiff_t)(kVec * tid) - halo_n;
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
		} else if (i >= 0 && i < sn) {	// k = 1: the last, partial vector
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

	size_t flushed = 0;		// stream slots behind the flushes
	u32x4 nf, nm;
	raw4 nx, ny;
	load_pass(0, nf, nm, nx, ny);
	for (size_t t0 = 0; t0 < n + (size_t)halo_n; t0 += kFmrxPass) {
		const u32x4 f = nf, m = nm;
		i32x4 tx, ty;
		fmx::widen_iq(IO{}, nx, ny, tx, ty);
		const bool last_pass = t0 + kFmrxPass >= n + (size_t)halo_n;
		if (!last_pass)
			load_pass(t0 + kFmrxPass, nf, nm, nx, ny);

		const uint32_t s0 = f[0], s1 = s0 + f[1], s2 = s1 + f[2], s3 = s2 + f[3];
		const uint32_t incl = fmx::wave_scan(s3);
		if (lane == 63u)
			ex[par * 4 + wave] = incl;
		// the halo's total (a first span's halo loaded zeros)
		if (t0 == 0 && tid == (unsigned)(halo_n / kVec) - 1u)
			ex[20] = incl;
		__syncthreads();
		const u32x4 w = *reinterpret_cast<const u32x4 *>(ex + par * 4);
		par ^= 1;
		const uint32_t front = (wave > 0 ? w[0] : 0u) + (wave > 1 ? w[1] : 0u)
			+ (wave > 2 ? w[2] : 0u);
		if (t0 == 0)
			carry -= ex[20];
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
		fmx::xydir_vector<LJ, NLIVE>(kp, da, rr.ljc, rr.maskv, bk_base, rr.full_ports,
			tx, ty, pb, rx, ry);

		// ---- the sums (fmx::store_decim), the owner's into the ring
		const ptrdiff_t i = (ptrdiff_t)t0 + (ptrdiff_t)(kVec * tid) - halo_n;
		const bool mine = (i >= 0 || !first) && i < sn;
		if (k == 1) {		// two decimated samples per lane
#pragma unroll
			for (int h = 0; h < 2; h++) {
				if (mine && i + 2 * h < sn) {
					const int32_t a = rx[2 * h], b = rx[2 * h + 1];
					const int32_t c = ry[2 * h], d = ry[2 * h + 1];
					const uint32_t q = ((uint32_t)((i >> 1) + 4 + h)
						& (uint32_t)(kFmrxdRing - 1)) * 4u;
					*(lds_i32 *)(uintptr_t)(ringx + q)
						= (a >> 1) + (b >> 1) + (((a & 1) + (b & 1)) >> 1);
					*(lds_i32 *)(uintptr_t)(ringy + q)
						= (c >> 1) + (d >> 1) + (((c & 1) + (d & 1)) >> 1);
				}
			}
		} else {
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
			if (k > 2) {
				hx = fmx::group_sum(hx, g, lane);
				lx = fmx::group_sum(lx, g, lane);
				hy = fmx::group_sum(hy, g, lane);
				ly = fmx::group_sum(ly, g, lane);
			}
			if ((lane & (g - 1u)) == g - 1u && mine) {
				const uint32_t q = ((uint32_t)((i >> k) + 4)
					& (uint32_t)(kFmrxdRing - 1)) * 4u;
				*(lds_i32 *)(uintptr_t)(ringx + q) = (int32_t)(hx + (lx >> k));
				*(lds_i32 *)(uintptr_t)(ringy + q) = (int32_t)(hy + (ly >> k));
			}
		}

		// ---- the flushes this pass completes (block-uniform)
		const size_t endi = t0 + kFmrxPass - (size_t)halo_n < n
			? t0 + kFmrxPass - (size_t)halo_n : n;
		const size_t done = (endi >> k) + 4;	// stream slots complete
		while (flushed + kFmrxdFlush <= done || (last_pass && flushed < done)) {
			__syncthreads();	// (A)
			const uint32_t q = ((uint32_t)(flushed + kVec * tid)
				& (uint32_t)(kFmrxdRing - 1)) * 4u;
			const i32x4 dx = *(lds_i32x4 *)(uintptr_t)(ringx + q);
			const i32x4 dy = *(lds_i32x4 *)(uintptr_t)(ringy + q);
			i32x4 rm;
			u32x4 rp;
			fmd::pol_lj_vector<fmrx::kConvStages, true, false, false>(
				fmrx::conv_params(ckmem, true), ln, dx, dy, rm, rp);

			// the phase in front of this lane's first sample (fmrx::pass_loop)
			const bool head = flushed == 0 && tid == 0;
			uint32_t last = rp[3];
			if (head && first)
				last = prev;
			uint32_t *edge = ex + 12 + fpar * 4;
			if (lane == 63u)
				edge[wave] = last;
			uint32_t before0 = 0;
			if (wave == 0)		// (flush 0: the head lane's, unused)
				before0 = ex[12 + (fpar ^ 1u) * 4 + 3];
			__syncthreads();	// (B)
			if (wave != 0)
				before0 = edge[wave - 1];
			fpar ^= 1;
			const uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp(
				(int)before0, (int)last, 0x138, 0xf, 0xf, false);
			const int sh = ln.sh;
			i32x4 rf;
			rf[0] = fmd::step_of(rp[0], before, sh);
#pragma unroll
			for (int v = 1; v < kVec; v++)
				rf[v] = fmd::step_of(rp[v], rp[v - 1], sh);

			// decimated sample of this lane's first slot
			const ptrdiff_t j = (ptrdiff_t)flushed + (ptrdiff_t)(kVec * tid) - 4;
			if (j >= 0 && j + kVec <= sm) {
				CORDIC_STORE_OUT(true, reinterpret_cast<ivec *>(amag + j), IO::narrow(rm));
				CORDIC_STORE_OUT(true, reinterpret_cast<ivec *>(afreq + j), IO::narrow(rf));
			} else if (j >= 0 && j < sm) {
#pragma unroll
				for (int v = 0; v < kVec; v++) {
					if (j + v < sm) {
						amag[j + v] = (ielem)rm[v];
						afreq[j + v] = (ielem)rf[v];
					}
				}
			}
			// the lane with decimated sample m - 1
			if (d_last && j >= 0 && j < sm && sm - j <= kVec) {
				const int e = (int)(sm - j);
				*d_last = e == 1 ? rp[0] : e == 2 ? rp[1] : e == 3 ? rp[2] : rp[3];
			}
			flushed += kFmrxdFlush;
		}
	}
}

// the tables, the exchange words and the ring behind them
inline size_t lds_bytes(const DxInfo &dx, uint32_t *xw)
{
	const uint32_t at = (dx_lds_layout(dx, nullptr, nullptr) + 15u) & ~15u;
	if (xw)
		*xw = at;
	return (size_t)at + kFmrxdLdsExtra;
}

} // namespace fmrxd
} // namespace cordic_amd
#endif // __HIPCC__
#endif
