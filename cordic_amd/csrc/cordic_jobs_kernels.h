// cordic_jobs_kernels.h -- device side of the tile-reading job-set kernels
// (cordic_jobs_fused.h).  Each kernel is the body of the single-call kernel it
// mirrors, built from the same stage primitives of cordic_device.h, around a
// loop over tile descriptors: block b sweeps tiles b, b + gridDim.x, ... in the
// table's order, the block's 256 lanes over the tile's `live` vectors (as
// topolar_lj_jobs and rotator_xydir<.., true> do).  Whole vectors only; the
// 0..3 samples behind a job's last vector go to xy_job_tails.
#ifndef CORDIC_JOBS_KERNELS_H
#define CORDIC_JOBS_KERNELS_H

#include <hip/hip_runtime.h>

#include "cordic_device.h"
#include "cordic_launch.h"

namespace cordic_amd {
namespace dev {

// ---- rotator, per-sample vectors (CORDIC_JOBS_P2R_XY; CORDIC_JOBS_MIX when
// kp.xy_nco): rotator_unrolled<C, kDynStages, NGEN, Feed::PhaseArray_XYArray,
// true, IO, UG> per tile.  A mixer tile's phases start from the descriptor's
// {fcw, phase} pair (TileDescXY::in2), as in rotator_xydir<.., true>.  IO = Io16
// (Narrow32 only, cordic_jobs_io16.hip): the descriptor's addresses are those
// of int16 / uint16 arrays, a lane moves 8 bytes per array per pass.
template <typename C, int NGEN, bool UG, typename IO = Io32>
__global__ __launch_bounds__(kBlock) void rotator_xy_tiles(CoreParams kp,
		const TileDescXY *__restrict__ tiles, uint32_t ntiles)
{
	using T = typename std::conditional<C::wide, int64_t, int32_t>::type;
	using U = typename std::make_unsigned<T>::type;
	using Z = typename std::conditional<C::wide, int64_t, uint32_t>::type;
	using IVec = typename IO::ivec;
	using UVec = typename IO::uvec;
	constexpr int NLIVE = kDynStages;
	// the fold as four multiply-adds in a 64-bit container, stage 1 folded in
	// on the left-justified ones (rotator_unrolled: kMadFold, fold1)
	constexpr bool kMadFold = C::wide;
	const bool fold1 = kMadFold && C::lj != 0 && kp.in_shl >= 1 && kp.nlive >= 1;
	__shared__ int32_t rot_tab[8][4];
	if constexpr (kMadFold) {
		if (threadIdx.x < 8) {
			// q = 0: (x, y); 1: (-y, x); 2: (-x, -y); 3: (y, -x)
			const int q = threadIdx.x >> 1;
			const int32_t dir = (threadIdx.x & 1) ? 1 : -1;	// phase >= 0 : < 0
			const int32_t k = (int32_t)(1u << (kp.in_shl & 31));
			const int32_t c = (q == 0) ? k : (q == 2) ? -k : 0;
			const int32_t sn = (q == 1) ? k : (q == 3) ? -k : 0;
			int32_t a = c, b = sn, dp = 0;
			if (fold1) {
				a = c - dir * (sn / 2);
				b = sn + dir * (c / 2);
				dp = -dir * (int32_t)kp.angle[0];
			}
			rot_tab[threadIdx.x][0] = a;
			rot_tab[threadIdx.x][1] = b;
			rot_tab[threadIdx.x][2] = -b;
			rot_tab[threadIdx.x][3] = dp;
		}
		__syncthreads();
	}
	LjRegs ljc{};
	if constexpr (C::lj != 0) {
		ljc.mask = vgpr_const(LjConst<C::lj>::mask);
		ljc.bit = vgpr_const(LjConst<C::lj>::bit);
		ljc.maskbit = vgpr_const(LjConst<C::lj>::mask | LjConst<C::lj>::bit);
	}
	const bool gen_phase = kp.xy_nco != 0;

	for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const TileDescXY d = tiles[t];
		const IVec *__restrict__ xin = reinterpret_cast<const IVec *>((uintptr_t)d.in0);
		const IVec *__restrict__ yin = reinterpret_cast<const IVec *>((uintptr_t)d.in1);
		const UVec *__restrict__ phin = reinterpret_cast<const UVec *>((uintptr_t)d.in2);
		IVec *__restrict__ ox = reinterpret_cast<IVec *>((uintptr_t)d.o0);
		IVec *__restrict__ oy = reinterpret_cast<IVec *>((uintptr_t)d.o1);
		const uint32_t acc0 = (uint32_t)d.in2, fcw = (uint32_t)(d.in2 >> 32);
		const size_t nvec = d.live;
		size_t g = threadIdx.x;
		// software prefetch (see rotator_unrolled)
		UVec nph{};
		IVec nx{}, ny{};
		if (g < nvec) {
			if (!gen_phase)
				nph = CORDIC_LOAD_IN(&phin[g]);
			nx = CORDIC_LOAD_IN(&xin[g]);
			ny = CORDIC_LOAD_IN(&yin[g]);
		}
		for (; g < nvec; g += kBlock) {
			const u32x4 tph = IO::widen(nph);
			const i32x4 tx = IO::widen(nx), ty = IO::widen(ny);
			const size_t gn = g + kBlock;
			if (gn < nvec) {
				if (!gen_phase)
					nph = CORDIC_LOAD_IN(&phin[gn]);
				nx = CORDIC_LOAD_IN(&xin[gn]);
				ny = CORDIC_LOAD_IN(&yin[gn]);
			}

			uint32_t P[kVec];
			if (gen_phase) {
				P[0] = acc0 + (uint32_t)(g * kVec) * fcw;
#pragma unroll
				for (int v = 1; v < kVec; v++)
					P[v] = P[v - 1] + fcw;
			} else {
				left_justify(tph, P, kp.pw_shl);
			}

			int64_t x[kVec], y[kVec], p[kVec];
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				const int32_t ix = sext32(tx[v], kp.iw);
				const int32_t iy = sext32(ty[v], kp.iw);
				if constexpr (kMadFold) {	// launcher: in_shl <= 30
					const uint32_t pb = P[v] + 0x20000000u;
					// row = quadrant x direction, 16 bytes each
					const uint32_t row = (pb >> 25) & 0x70u;
					const i32x4 m = *reinterpret_cast<const i32x4 *>(
						reinterpret_cast<const char *>(&rot_tab[0][0]) + row);
					int64_t fx = op_mul(iy, m[2]);	// -B * i_y
					op_mad(fx, ix, m[0]);		// + A * i_x
					int64_t fy = op_mul(iy, m[0]);	//  A * i_y
					op_mad(fy, ix, m[1]);		// + B * i_x
					x[v] = fx;
					y[v] = fy;
					p[v] = (int64_t)((pb & 0x3fffffffu) - 0x20000000u
							+ (uint32_t)m[3]);
				} else {
					const T ex = (T)((U)(T)ix << kp.in_shl);
					const T ey = (T)((U)(T)iy << kp.in_shl);
					T fx, fy;
					uint32_t fp;
					fold_octant<T>(ex, ey, P[v], fx, fy, fp);
					x[v] = (int64_t)(Z)fx;
					y[v] = (int64_t)(Z)fy;
					p[v] = (int64_t)fp;
				}
			}

			i32x4 rx, ry;
			if constexpr (C::lj == 0) {
				RotChain<C, NLIVE, NGEN, 0, true>::run(x, y, p, kp);
#pragma unroll
				for (int v = 0; v < kVec; v++) {
					rx[v] = round_to_ow<T>((T)x[v], kp);
					ry[v] = round_to_ow<T>((T)y[v], kp);
				}
			} else {
				constexpr int LJ = C::lj;
#pragma unroll
				for (int v = 0; v < kVec; v++) {
					x[v] = (int64_t)((uint64_t)x[v] << LJ);
					y[v] = (int64_t)((uint64_t)y[v] << LJ);
					p[v] = (int64_t)((uint64_t)(int64_t)(int32_t)(uint32_t)p[v]
							<< LjPhase<LJ>::ps);
				}
				if (!fold1)	// else stage 1 came out of the fold's multiply-adds
					RotChainLJ<LJ, 1, 0, true>::run(x, y, p, kp, ljc);
				RotChainLJ<LJ, NLIVE, 1, true>::run(x, y, p, kp, ljc);
				if (kp.r_lj == 32) {
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
			apply_unit_gain<UG>(rx, kp);
			apply_unit_gain<UG>(ry, kp);
			CORDIC_STORE_OUT(true, &ox[g], IO::narrow(rx));
			CORDIC_STORE_OUT(true, &oy[g], IO::narrow(ry));
		}
	}
}

// ---- converter, left-justified, WW <= 34: topolar_lj's sweep per tile (the
// same way topolar_lj_jobs wraps it; instantiated for unit gain only)
template <bool UG>
__global__ __launch_bounds__(kBlock) void topolar_lj_tiles(CoreParams kp,
		const TileDescXY *__restrict__ tiles, uint32_t ntiles)
{
	for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const TileDescXY d = tiles[t];
		topolar_lj_sweep<kDynStages, true, Io32, UG, false>(kp,
			reinterpret_cast<const i32x4g *>((uintptr_t)d.in0),
			reinterpret_cast<const i32x4g *>((uintptr_t)d.in1),
			reinterpret_cast<i32x4g *>((uintptr_t)d.o0),
			reinterpret_cast<u32x4g *>((uintptr_t)d.o1),
			(size_t)d.live, (size_t)threadIdx.x, (size_t)kBlock);
	}
}

// ---- converter, left-justified, WW 35 .. 40: topolar_ljw<LJ, kDynStages, Io32,
// UG> per tile (LJ = 64 - WW)
template <int LJ, bool UG>
__global__ __launch_bounds__(kBlock) void topolar_ljw_tiles(CoreParams kp,
		const TileDescXY *__restrict__ tiles, uint32_t ntiles)
{
	PolWideRegs c;
	c.bit = vgpr_const(1u << LJ);
	c.mask = vgpr_const(~((2u << LJ) - 1u));
	const uint32_t sign = vgpr_const(0x80000000u), p30 = vgpr_const(0x40000000u);
	const int up = 32 - kp.iw;
	// the rounded magnitude is bits r+LJ .. of x~: in the high word if
	// r + LJ >= 32, with the increment (base + tie) a signed multiplicand
	const bool round_hi = kp.r + LJ >= 32 && kp.r <= 31;

	for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const TileDescXY d = tiles[t];
		const i32x4g *__restrict__ xin = reinterpret_cast<const i32x4g *>((uintptr_t)d.in0);
		const i32x4g *__restrict__ yin = reinterpret_cast<const i32x4g *>((uintptr_t)d.in1);
		i32x4g *__restrict__ omag = reinterpret_cast<i32x4g *>((uintptr_t)d.o0);
		u32x4g *__restrict__ oph = reinterpret_cast<u32x4g *>((uintptr_t)d.o1);
		const size_t nvec = d.live;
		size_t g = threadIdx.x;
		i32x4g nx{}, ny{};		// software prefetch
		if (g < nvec) {
			nx = CORDIC_LOAD_IN(&xin[g]);
			ny = CORDIC_LOAD_IN(&yin[g]);
		}
		for (; g < nvec; g += kBlock) {
			const i32x4 tx = nx, ty = ny;
			const size_t gn = g + kBlock;
			if (gn < nvec) {
				nx = CORDIC_LOAD_IN(&xin[gn]);
				ny = CORDIC_LOAD_IN(&yin[gn]);
			}
			int64_t x[kVec], y[kVec], p[kVec];
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				const int32_t ex = (int32_t)((uint32_t)tx[v] << up);
				const int32_t ey = (int32_t)((uint32_t)ty[v] << up);
				// fold and quadrant phase as in topolar_ljw
				const int32_t mx = (int32_t)op_and_or((uint32_t)ex, p30, sign);
				const int32_t my = (int32_t)op_and_or((uint32_t)ey, p30, sign);
				const int32_t nmy = (int32_t)((uint32_t)my ^ sign);
				x[v] = op_mul(ex, mx);
				op_mad(x[v], ey, my);
				y[v] = op_mul(ey, mx);
				op_mad(y[v], ex, nmy);
				const uint32_t l = ((uint32_t)mx ^ sign) >> 1;	// 2^29 (2 + sx)
				p[v] = op_mul(nmy >> (30 - LJ), (int32_t)l);	// -sy 2^LJ
			}

			PolChainW<LJ, kDynStages, 0>::run(x, y, p, c, kp);

			i32x4 rm;
			u32x4 rp;
			if (round_hi) {
				const int sh = kp.r + LJ - 32;
#pragma unroll
				for (int v = 0; v < kVec; v++) {
					// tie bit r of x: bit sh of the high word (0 .. 28)
					const uint32_t xh = (uint32_t)((uint64_t)x[v] >> 32);
					const uint32_t b = (xh >> sh) & kp.round_bit;
					op_mad_s(x[v], 1u << LJ, (int32_t)(b + (uint32_t)kp.round_base));
					rm[v] = (int32_t)((uint64_t)x[v] >> 32) >> sh;
				}
			} else {
#pragma unroll
				for (int v = 0; v < kVec; v++)
					rm[v] = round_to_ow<int64_t>(x[v] >> LJ, kp);
			}
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				const uint32_t acc = (uint32_t)((uint64_t)p[v] >> LJ);
				rp[v] = (acc + 0x80000000u) >> kp.pw_shl;	// rtl/topolar.v:269
			}
			apply_unit_gain<UG>(rm, kp);
			CORDIC_STORE_OUT(true, &omag[g], rm);
			CORDIC_STORE_OUT(true, &oph[g], rp);
		}
	}
}

// ---- converter in the 32-bit container (wrap at WW 32): topolar_unrolled<
// Narrow32, kDynStages, 0, true, IO, UG> per tile
template <bool UG, typename IO = Io32>
__global__ __launch_bounds__(kBlock) void topolar_narrow_tiles(CoreParams kp,
		const TileDescXY *__restrict__ tiles, uint32_t ntiles)
{
	using IVec = typename IO::ivec;
	using UVec = typename IO::uvec;
	for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const TileDescXY d = tiles[t];
		const IVec *__restrict__ xin = reinterpret_cast<const IVec *>((uintptr_t)d.in0);
		const IVec *__restrict__ yin = reinterpret_cast<const IVec *>((uintptr_t)d.in1);
		IVec *__restrict__ omag = reinterpret_cast<IVec *>((uintptr_t)d.o0);
		UVec *__restrict__ oph = reinterpret_cast<UVec *>((uintptr_t)d.o1);
		const size_t nvec = d.live;
		size_t g = threadIdx.x;
		IVec nx{}, ny{};		// software prefetch
		if (g < nvec) {
			nx = CORDIC_LOAD_IN(&xin[g]);
			ny = CORDIC_LOAD_IN(&yin[g]);
		}
		for (; g < nvec; g += kBlock) {
			const i32x4 tx = IO::widen(nx), ty = IO::widen(ny);
			const size_t gn = g + kBlock;
			if (gn < nvec) {
				nx = CORDIC_LOAD_IN(&xin[gn]);
				ny = CORDIC_LOAD_IN(&yin[gn]);
			}
			int64_t x[kVec], y[kVec], p[kVec];
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				const int32_t ix = sext32(tx[v], kp.iw);
				const int32_t iy = sext32(ty[v], kp.iw);
				const int32_t ex = (int32_t)((uint32_t)ix << kp.in_shl);
				const int32_t ey = (int32_t)((uint32_t)iy << kp.in_shl);
				int32_t fx, fy;
				uint32_t fp;
				fold_quadrant_masks<int32_t>(ex, ey, ix, iy, fx, fy, fp);
				x[v] = (int64_t)(uint32_t)fx;
				y[v] = (int64_t)(uint32_t)fy;
				p[v] = (int64_t)fp;
			}

			PolChain<Narrow32, kDynStages, 0, 0, true>::run(x, y, p, kp);

			i32x4 rm;
			u32x4 rp;
#pragma unroll
			for (int v = 0; v < kVec; v++) {
				rm[v] = round_to_ow<int32_t>((int32_t)x[v], kp);
				rp[v] = (uint32_t)p[v] >> kp.pw_shl;	// rtl/topolar.v:269
			}
			apply_unit_gain<UG>(rm, kp);
			CORDIC_STORE_OUT(true, &omag[g], IO::narrow(rm));
			CORDIC_STORE_OUT(true, &oph[g], IO::narrow(rp));
		}
	}
}

} // namespace dev
} // namespace cordic_amd
#endif
