// cordic_fm_mix.hip -- the FM mixer's fused path (cordic_plan_fm_mix): the
// rotator with looked-up directions (cordic_xydir.h) behind a prefix sum of
// per-sample tuning words,
//   start = phase0 + *d_acc
//   p_i   = start + fcw[0] + .. + fcw[i-1] + pm[i]      (mod 2^32)
//   (ox_i, oy_i) = what cordic_p2r writes for (x_i, y_i, p_i)
//   *d_acc = start + fcw[0] + .. + fcw[n-1].
//
// Reduce-then-scan in two launches, as cordic_table_fm.hip.  The samples are
// cut into passes of 1024; every block owns a contiguous span of whole passes.
//   1. fm_reduce (cordic_table_fm.hip): each block sums its span of fcw into a
//      workspace word; block 0 latches the start beside them.
//   2. fm_mix_xydir<LJ, NLIVE>: each block stages the direction tables as
//      rotator_xydir does, adds the partials in front of it to the latched
//      start, then walks its span pass by pass.  A lane reads 4 consecutive
//      tuning words (and pm, x, y: one 16-byte access each at whatever 4-byte
//      alignment the array has), sums them, the wave scans the lane sums with
//      DPP moves, the four waves exchange their totals through LDS, and the
//      carry runs from pass to pass in a register.  The lane then rotates its 4
//      samples by the per-vector body of rotator_xydir and stores them.
// No block waits for another: what a block needs of the others is complete
// when launch 2 starts.  *d_acc is read in launch 1 only and written in launch
// 2 only (one thread of the last block).  The price is a second read of fcw:
// 24 bytes per sample (28 with pm) against the 32 (36) of
// cordic_phase_accumulate + cordic_plan_p2r.
//
// The exchange words are double-buffered by pass, so a pass has ONE barrier:
// the four words written in pass i are read by every wave behind barrier i and
// in front of barrier i + 1; they are written again in pass i + 2, which a
// wave reaches only through barrier i + 1, and that opens only when every
// wave has arrived there -- with its reads of pass i behind it.
//
// LDS is the tables' (dx_lds_layout) with 12 words behind them, in the DYNAMIC
// block: the table lookups address LDS by byte offset from 0, which a static
// __shared__ object would displace.
//
// The last, partial vector (n % 4 samples) belongs to one lane of the last
// block, which loads and stores it sample by sample; lanes behind it read and
// write nothing.  There is no extra launch, and nothing outside [0, n) of an
// output is written.
//
// CORDIC_FMX_MAX_BLOCKS=<n> in the environment (read at every call; a test
// and A/B knob like CORDIC_FMD_MAX_BLOCKS) caps the grid at n blocks, so that
// a short call walks many passes per block.  The bits do not depend on it.
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps;
// .private_segment_fixed_size is 0 for every instance: nothing spills):
//   live stages           13   16   19   20   24   27   29
//   rotator_xydir<29, N>  95   95   96   96   97   98   98
//   fm_mix_xydir<29, N>   98  100   98   98  104  108  108
//   rotator_xydir<30, N>  89   95   90   90   91   94   94
//   fm_mix_xydir<30, N>   92   98   95   95  102  103  103
// The scan costs 3 .. 11 registers: four more words in flight per lane (fcw and
// pm against the phase) and the carry.  With 512 registers per lane of a SIMD,
// allocated in eights, up to 96 hold 5 waves and up to 128 hold 4: an occupancy
// step IS crossed, from 5 waves to 4, by every instance but <30, 13>, <30, 19>
// and <30, 20> (rotator_xydir's own <29, 24 .. 29> sit at 4 already).  Holding
// the kernel to 96 registers (amdgpu_waves_per_eu) spills 8 .. 72 bytes in all
// but one instance, so the step is taken and the grid is sized for 4 blocks
// per CU.  The tables are 64 KiB at the most, so LDS admits at least two
// blocks, and four wherever the tables stay within 40 KiB.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cordic_xydir.h"
#include "cordic_launch.h"
#include "cordic_jobs_fused.h"
#include "cordic_hostargs.h"
#include "cordic_fm_mix.h"

namespace cordic_amd {

namespace fmx {

using namespace dev;

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

struct FmxArgs {
	const uint32_t *fcw, *pm;	// pm may be NULL
	uint32_t *acc;			// may be NULL
	const uint32_t *work;		// fm_reduce's: [0] start, [4 + b] partials
	const int32_t *x, *y;
	int32_t	*ox, *oy;
	size_t	n, span;		// span: samples per block, whole passes
	uint32_t xw;			// LDS byte offset of the 12 exchange words
};

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

template <int LJ, int NLIVE>
__global__ __launch_bounds__(kBlock) void fm_mix_xydir(CoreParams kp, DirArgs da,
		FmxArgs a)
{
	static_assert(LJ == 29 || LJ == 30, "WW <= 35 cores");
	constexpr int kN = dx_levels(NLIVE);
	static_assert(kN >= 1 && kN <= kDxMaxLevels, "no group to look up");
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const unsigned tid = threadIdx.x;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);

	uint32_t bk_base[kDxMaxLevels] = {}, lf_base[kDxMaxLevels] = {};
	dx_lds_layout(da.dx, bk_base, lf_base);

	// ---- prologue: the fold's rows and the groups' tables
	// (cordic_xydir.h:97-139)
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
	// ex[0 .. 8): the waves' totals, double-buffered by pass; ex[8 .. 12): the
	// waves' shares of the partials in front of this block
	uint32_t *ex = lds + a.xw / 4u;
	{
		uint32_t s = 0;
		for (unsigned j = tid; j < blockIdx.x; j += kBlock)
			s += a.work[4 + j];
#pragma unroll
		for (int d = 32; d; d >>= 1)
			s += __shfl_xor(s, d);
		if ((tid & 63u) == 0)
			ex[8 + wave] = s;
	}
	__syncthreads();

	// LDS is addressed by byte offset from 0: no static LDS in this kernel
	if ((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)lds != 0u)
		__builtin_trap();

	LjRegs ljc{};
	ljc.mask = vgpr_const(LjConst<LJ>::mask);
	ljc.bit = vgpr_const(LjConst<LJ>::bit);
	ljc.maskbit = vgpr_const(LjConst<LJ>::mask | LjConst<LJ>::bit);
	uint32_t maskv[kDxMaxLevels] = {};
#pragma unroll
	for (int g = 0; g < kN; g++)
		maskv[g] = vgpr_const(((uint32_t)da.dx.lv[g].nb - 1u) << 3);
	const uint32_t k45 = vgpr_const(0x20000000u);
	const bool full_ports = kp.iw == 32;	// wave-uniform: no sign extension

	const size_t lo = (size_t)blockIdx.x * a.span;	// < n by the grid
	const size_t hi = (a.n - lo < a.span) ? a.n : lo + a.span;
	// the phase of sample lo, without its pm
	uint32_t carry = a.work[0] + ex[8] + ex[9] + ex[10] + ex[11];

	// this lane's 4 samples of the pass at t0; nothing at or behind hi is read,
	// and a tuning word that is not there counts 0
	auto load_pass = [&](size_t t0, u32x4 &f, u32x4 &m, i32x4 &x, i32x4 &y) {
		const size_t i = t0 + (size_t)kVec * tid;
		f = u32x4{};
		m = u32x4{};
		x = i32x4{};
		y = i32x4{};
		if (i + kVec <= hi) {
			f = CORDIC_LOAD_IN(reinterpret_cast<const u32x4g *>(a.fcw + i));
			if (a.pm)	// (wave-uniform)
				m = CORDIC_LOAD_IN(reinterpret_cast<const u32x4g *>(a.pm + i));
			x = CORDIC_LOAD_IN(reinterpret_cast<const i32x4g *>(a.x + i));
			y = CORDIC_LOAD_IN(reinterpret_cast<const i32x4g *>(a.y + i));
		} else if (i < hi) {	// the last, partial vector: one lane of the call
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				if (i + v < hi) {
					f[v] = a.fcw[i + v];
					if (a.pm)
						m[v] = a.pm[i + v];
					x[v] = a.x[i + v];
					y[v] = a.y[i + v];
				}
			}
		}
	};

	u32x4 nf, nm;
	i32x4 nx, ny;
	load_pass(lo, nf, nm, nx, ny);
	unsigned par = 0;
	for (size_t t0 = lo; t0 < hi; t0 += kFmxPass) {
		const u32x4 f = nf, m = nm;
		const i32x4 tx = nx, ty = ny;
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
				: "v"(ph[v]), "s"(kp.pw_shl), "v"(k45));

		i32x4 rx, ry;
		xydir_vector<LJ, NLIVE>(kp, da, ljc, maskv, bk_base, full_ports, tx, ty, pb,
			rx, ry);

		const size_t i = t0 + (size_t)kVec * tid;
		if (i + kVec <= hi) {
			CORDIC_STORE_OUT(true, reinterpret_cast<i32x4g *>(a.ox + i), rx);
			CORDIC_STORE_OUT(true, reinterpret_cast<i32x4g *>(a.oy + i), ry);
		} else if (i < hi) {
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				if (i + v < hi) {
					a.ox[i + v] = rx[v];
					a.oy[i + v] = ry[v];
				}
			}
		}
	}
	if (a.acc && blockIdx.x == gridDim.x - 1 && tid == 0)
		*a.acc = carry;
}

// ---------------------------------------------------------------- host side
// the tables and the exchange words behind them
static size_t lds_bytes(const DxInfo &dx, uint32_t *xw)
{
	const uint32_t at = (dx_lds_layout(dx, nullptr, nullptr) + 15u) & ~15u;
	if (xw)
		*xw = at;
	return (size_t)at + 12 * 4;
}

// the stage counts the job-set instances of rotator_xydir carry
// (cordic_jobs_xydir.hip)
#define FMX_STAGES(X) X(13) X(16) X(19) X(20) X(24) X(27) X(29)

template <int LJ>
static bool launch_lj(int nlive, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const FmxArgs &a)
{
	switch (nlive) {
#define X(N) case N: \
	if (da.dx.n != dx_levels(N)) \
		return false; \
	hipLaunchKernelGGL((fm_mix_xydir<LJ, N>), dim3(grid), dim3(kBlock), lds, st, \
		kp, da, a); \
	return true;
	FMX_STAGES(X)
#undef X
	default:
		return false;
	}
}

static bool has_instance(int nlive, int ngroups)
{
	switch (nlive) {
#define X(N) case N: return ngroups == dx_levels(N);
	FMX_STAGES(X)
#undef X
	default:
		return false;
	}
}

} // namespace fmx

bool fmx_is_fused(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx)
{
	if (!d_dir || dx.n <= 0 || cfg.ww > 35 || cfg.needs_wrap
			|| (cfg.flags & (CORDIC_FLAG_UNIT_GAIN | CORDIC_FLAG_NO_TAILS
				| CORDIC_FLAG_NO_LJ | CORDIC_FLAG_FORCE_GENERIC)))
		return false;
	const dev::CoreParams kp = make_params_jobs(cfg);
	return kp.post_mul == 0 && kp.in_shl >= 1 && kp.in_shl <= 30
		&& fmx::lds_bytes(dx, nullptr) <= 64 * 1024
		&& fmx::has_instance(cfg.nlive, dx.n);
}

int fmx_check_call(size_t n, const uint32_t *d_fcw, const uint32_t *d_pm,
		const uint32_t *d_acc, const int32_t *d_xval, const int32_t *d_yval,
		const int32_t *d_oxval, const int32_t *d_oyval, const void *d_work,
		size_t work_bytes)
{
	using namespace fmx;
	if (!d_fcw || !d_xval || !d_yval || !d_oxval || !d_oyval || !d_work
			|| n > (~(size_t)0 >> 4))
		return CORDIC_ERR_ARGS;
	const uintptr_t words = reinterpret_cast<uintptr_t>(d_fcw)
		| reinterpret_cast<uintptr_t>(d_pm) | reinterpret_cast<uintptr_t>(d_acc)
		| reinterpret_cast<uintptr_t>(d_xval) | reinterpret_cast<uintptr_t>(d_yval)
		| reinterpret_cast<uintptr_t>(d_oxval) | reinterpret_cast<uintptr_t>(d_oyval);
	if ((words & 3u) || (reinterpret_cast<uintptr_t>(d_work) & 15u))
		return CORDIC_ERR_ARGS;
	const Range out[4] = {range_of(d_oxval, n * 4), range_of(d_oyval, n * 4),
		range_of(d_acc, 4), range_of(d_work, work_bytes)};
	const Range in[4] = {range_of(d_fcw, n * 4), range_of(d_pm, n * 4),
		range_of(d_xval, n * 4), range_of(d_yval, n * 4)};
	return outputs_overlap(out, in) ? CORDIC_ERR_ARGS : CORDIC_OK;
}

int launch_fm_mix(const cordic_config &cfg, const uint32_t *d_dir, const DxInfo &dx,
		size_t n, const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const int32_t *d_xval, const int32_t *d_yval,
		int32_t *d_oxval, int32_t *d_oyval, void *d_work, void *stream)
{
	using namespace fmx;
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (n == 0)
		return CORDIC_OK;
	hipStream_t st = static_cast<hipStream_t>(stream);
	const int cus = jobs_cus_now();
	if (cus < 0) {
		(void)hipGetLastError();
		return CORDIC_ERR_DEVICE;
	}
	uint32_t xw = 0;
	const size_t lds = lds_bytes(dx, &xw);
	// resident blocks: 4 waves of a SIMD by the registers (see the head of
	// this file), fewer where the tables fill the CU's 160 KiB sooner
	size_t per_cu = (160 * 1024) / lds;
	if (per_cu > kFmxBlocksPerCu)
		per_cu = kFmxBlocksPerCu;
	size_t cap = (size_t)cus * per_cu;
	if (cap > kFmxMaxBlocks)
		cap = kFmxMaxBlocks;
	cap = env_block_cap("CORDIC_FMX_MAX_BLOCKS", cap);
	const size_t npass = (n + kFmxPass - 1) / kFmxPass;
	const size_t per_block = (npass + cap - 1) / cap;
	const size_t span = per_block * kFmxPass;
	const unsigned grid = (unsigned)((npass + per_block - 1) / per_block);
	uint32_t *work = static_cast<uint32_t *>(d_work);
	launch_fm_reduce(grid, d_fcw, n, span, phase0, d_acc, work, st);
	const FmxArgs a{d_fcw, d_pm, d_acc, work, d_xval, d_yval, d_oxval, d_oyval, n,
		span, xw};
	const DirArgs da{d_dir, dx};
	const CoreParams kp = make_params_jobs(cfg);
	const bool done = cfg.ww == 35
		? launch_lj<29>(cfg.nlive, grid, lds, st, kp, da, a)
		: launch_lj<30>(cfg.nlive, grid, lds, st, kp, da, a);
	return tnco::finish(done);
}

} // namespace cordic_amd
