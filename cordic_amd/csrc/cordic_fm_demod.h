// cordic_fm_demod.h -- FM demodulation on the r2p / sr2p cores (cordic_fm_demod,
// cordic_fm_demod16, cordic_fm_demod_info, cordic_fm_demod_workspace;
// include/cordic_amd.h): the converter's phase differenced sample to sample,
//   freq_i = sext_PW((ph_i - ph_(i-1)) mod 2^PW),
// the inverse of cordic_phase_accumulate.  All four public functions are
// defined in cordic_fm_demod.hip; this header holds what the two paths share
// and, for a HIP compiler, everything the fused kernels have in common with the
// banks' kernels (cordic_fm_demod_bank.hip): the converter's per-vector body,
// the sweep of one tile, the tail of one job, the lane constants and the choice
// of the instance.
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_FM_DEMOD_H
#define CORDIC_FM_DEMOD_H

#include <cstddef>
#include <cstdint>

#include "cordic_amd.h"

namespace cordic_amd {

// Fused kernel: a block of 256 threads sweeps kFmdPasses passes of 256 vectors
// (4 samples each); the first vector of the sweep is the halo -- the last
// vector of the tile in front, computed again and not stored -- so a tile is
// kFmdTileVecs = 8 * 256 - 1 vectors of output.
constexpr int	 kFmdPasses = 8;
constexpr size_t kFmdTileVecs = (size_t)kFmdPasses * 256 - 1;
constexpr size_t kFmdTile = kFmdTileVecs * 4;		// samples: 8188

// Fallback: the phases are differenced in place in tiles of kFmdDiffTile
// samples, one saved word per tile.
constexpr size_t kFmdDiffTile = 4096;

// d_work, in 32-bit words:
//   [0]       the latched predecessor of sample 0 (fallback)
//   [4, 12)   kept for the size's sake (cordic_fm_demod_workspace is public):
//             the fused path parked its last <= 4 samples here once; its tail
//             converts them in registers now and writes no word of d_work
//   [12 + j]  fallback: the phase of the last sample of differencing tile j
constexpr size_t kFmdWorkHead = 12;
constexpr size_t fmd_work_bytes(size_t n)
{
	return n ? ((kFmdWorkHead + (n + kFmdDiffTile - 1) / kFmdDiffTile) * 4 + 15)
			& ~(size_t)15 : 0;
}

// 1: 16-byte-aligned 32-bit arrays of this core, and 16-bit arrays at any
// alignment of theirs, run the fused kernel -- the cores that launch_topolar
// sends to topolar_lj.  (The mode, and the 16-bit container's limit on the
// ports, are the caller's to check.)
bool	fmd_core_is_fused(const cordic_config &cfg);

// What cordic_fm_demod_info, cordic_fm_demod and cordic_demodbank_create ask of
// a core, in this order: CORDIC_ERR_ARGS (no configuration), CORDIC_ERR_MODE
// (neither r2p nor sr2p), CORDIC_ERR_ARGS (not sane), or CORDIC_OK.
int	fmd_check_core(const cordic_config *cfg);

// The tail of a job whose length is no multiple of 4 or that has a d_last:
// `count` samples from sample s0 = (n / 4 ? n / 4 * 4 - 1 : 0) on -- the ones
// behind the last whole vector and, when first == 0, the one in front of them,
// which only lends its phase (fmd::tail_of).
struct DemodTail {
	uint64_t x, y, mag, freq;	// addresses of sample s0 in the four arrays
	uint64_t last;			// the job's d_last, or 0
	uint32_t count;			// 1 .. 4
	uint32_t phase0;
	uint32_t first;			// 1: s0 is sample 0 of the job (no whole
	uint32_t pad;			//    vector): the lane reads *last itself
};					// 56 bytes

} // namespace cordic_amd

#ifdef __HIPCC__
// ---- code shared by cordic_fm_demod.hip and cordic_fm_demod_bank.hip
#include "cordic_device.h"

namespace cordic_amd {
namespace fmd {

using namespace dev;

// A lane's constants: those topolar_lj_sweep sets up in front of its loop, and
// sh = 32 - PW for step_of.
struct LaneConsts {
	PolLjRegs c;
	uint32_t rbw;		// width of the rounding's tie bit (0 or 1), in a VGPR
	int	up, down;	// port -> sign bit of the word, and back to i << in_shl
	int	sh;

	__device__ __forceinline__ explicit LaneConsts(const CoreParams &kp)
	{
		c.sign = vgpr_const(0x80000000u);
		c.p30 = vgpr_const(0x40000000u);
		rbw = vgpr_const(kp.round_bit);
		up = 32 - kp.iw;
		down = up - kp.in_shl;
		sh = kp.pw_shl;
	}
};

// One vector through the converter: the per-vector body of topolar_lj_sweep
// (cordic_device.h; everything between its prefetch and its two stores)
// restated, because the sweep stores what it computes.  Built from the same
// pieces in the same order; rm, rp are the words the sweep would store to
// omag[g], oph[g].
template <int NLIVE, bool DYN, bool UG, bool PLAIN>
__device__ __forceinline__ void pol_lj_vector(const CoreParams &kp, const LaneConsts &ln,
		const i32x4 tx, const i32x4 ty, i32x4 &rm, u32x4 &rp)
{
	const PolLjRegs &c = ln.c;
	const int up = ln.up, down = ln.down;
	int64_t x[kVec], y[kVec], p[kVec];
#pragma unroll
	for (int v = 0; v < kVec; v++) {
		// the ports (e = sext(i, IW) << in_shl), the fold as four
		// multiply-adds, the quadrant phase p0
		const int32_t ex = (int32_t)((uint32_t)tx[v] << up) >> down;
		const int32_t ey = (int32_t)((uint32_t)ty[v] << up) >> down;
		const int32_t mx = (int32_t)op_and_or((uint32_t)ex, c.p30, c.sign);
		const int32_t my = (int32_t)op_and_or((uint32_t)ey, c.p30, c.sign);
		const int32_t nmy = (int32_t)((uint32_t)my ^ c.sign);
		x[v] = op_mul(ex, mx);
		op_mad(x[v], ey, my);
		y[v] = op_mul(ey, mx);
		op_mad(y[v], ex, nmy);
		const uint32_t l = ((uint32_t)mx ^ c.sign) >> 1;
		p[v] = op_mul(nmy, (int32_t)l);
	}
	if (PLAIN || down >= 2) {	// stage 1: pol_stage1_lj (WW <= 32) ...
#pragma unroll
		for (int v = 0; v < kVec; v++)
			pol_stage1_lj(x[v], y[v], p[v], kp.angle[0], c);
	} else {			// ... or pol_stage1_lj_early (WW 33, 34)
#pragma unroll
		for (int v = 0; v < kVec; v++)
			pol_stage1_lj_early(x[v], y[v], p[v], kp.angle[0], c);
	}

	PolTmp m[kVec];
#if CORDIC_STAGE_YIELD
#pragma unroll
	for (int v = 0; v < kVec; v++)
		asm volatile("" : "=v"(m[v].t), "=v"(m[v].nt), "=v"(m[v].sy), "=v"(m[v].sx),
				"=s"(m[v].cc));
#endif
	PolChainLJ<NLIVE, 1, DYN>::run(x, y, p, c, kp, m);

	if (PLAIN || (kp.r >= 2 && kp.r <= 31)) {	// rounding at the 2^30 scale ...
#pragma unroll
		for (int v = 0; v < kVec; v++) {
			const uint32_t xh = (uint32_t)((uint64_t)x[v] >> 32);
			uint32_t b;
			asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(b)
				: "v"(xh), "s"(kp.r - 2), "v"(ln.rbw));
			op_mad_s(x[v], 0x40000000u, (int32_t)(b + (uint32_t)kp.round_base));
			rm[v] = (int32_t)((uint64_t)x[v] >> 32) >> (kp.r - 2);
		}
	} else {					// ... or round_to_ow on 64 bits
#pragma unroll
		for (int v = 0; v < kVec; v++)
			rm[v] = round_to_ow<int64_t>(x[v] >> 30, kp);
	}
#pragma unroll
	for (int v = 0; v < kVec; v++) {		// the phase word
		const uint32_t acc = (uint32_t)((uint64_t)p[v] >> 30);
		rp[v] = (acc + 0x80000000u) >> kp.pw_shl;
	}
	apply_unit_gain<UG>(rm, kp);
}

// sext_PW((a - b) mod 2^PW) with sh = 32 - PW
__device__ __forceinline__ int32_t step_of(uint32_t a, uint32_t b, int sh)
{
	return (int32_t)((a - b) << sh) >> sh;
}

// (phase0 + *d_last) mod 2^PW: the phase in front of sample 0 of a job
__device__ __forceinline__ uint32_t phase_in_front(uint32_t phase0,
		const uint32_t *d_last, int sh)
{
	return (phase0 + (d_last ? *d_last : 0u)) & (0xffffffffu >> sh);
}

// ONE tile, swept by a block of kBlock = 256 threads: nvec >= 1 vectors of one
// job and, in front of them, the halo -- the last vector of the tile before,
// converted again and not stored.  Element `at` of xin, yin, omag, ofreq is the
// halo and lane j of the sweep (j = 256 * pass + thread) has element at + j:
// lane 0 converts the halo, so the tile's first vector finds its predecessor
// where every other one does.  A bank passes pointers ONE VECTOR IN FRONT of
// the tile and at = 0, 32 bits wide; the single call passes pointers one vector
// in front of its arrays and the tile's first vector as a size_t (see there).
// j itself, and everything compared with it, is 32 bits wide either way.  The
// halo phase is the same arithmetic on the same inputs as the neighbour's own,
// so the result does not depend on how a job was cut or on the grid.  first: the
// tile begins at sample 0 of its job; there is no such vector, lane 0 loads
// nothing and holds (phase0 + *d_last) mod 2^PW instead.  That lane alone reads
// *d_last, and nothing here writes it.
//
// IO (Io32 / Io16, cordic_device.h; deduced from the tag behind `par`) is the
// container of the four sample arrays and of nothing else: a lane's 4 samples
// are one 16-byte or one 8-byte access per array, at any element alignment
// (the vector typedefs carry the element's), widened behind the load and
// narrowed in front of the store, and "one vector in front" is 16 or 8 bytes.
// The prefetched vectors wait in the container's own type (two registers per
// array for Io16), so Io32 is the loop it was.  Everything between load and
// store -- pol_lj_vector, the DPP move, the barrier, the edge words, step_of,
// phase_in_front -- is 32-bit in either; so are phase0 and *d_last.
//
// A tile takes nvec / 256 + 1 passes, the same for every thread of the block.
// A lane converts its 4 samples by pol_lj_vector and needs one more phase, the
// last one of the lane in front:
//   * inside a wave it comes from lane - 1 by one DPP move (wave_shr:1), whose
//     lane 0 keeps the value handed in;
//   * that value is the last phase of the wave in front -- wave w - 1 of this
//     pass, or wave 3 of the pass before -- through one LDS word per wave,
//     edge[par][wave].
// The words are double-buffered by `par`, which flips with every pass and is
// carried from tile to tile by the caller, so a pass has ONE barrier: a word
// written in pass i was last read in pass i - 2 (waves 1..3, behind that pass's
// barrier) or at the top of pass i - 1 (wave 0, in front of its barrier), and
// every wave has passed barrier i - 1 before any writes.  The argument counts
// the block's passes, whatever tile they belong to; pass 0 of a tile uses no
// word of the pass in front (the one its wave 0 reads is the halo lane's).
template <int NLIVE, bool DYN, bool UG, bool PLAIN, typename IDX, typename IO>
__device__ __forceinline__ void sweep_tile(const CoreParams &kp, const LaneConsts &ln,
		const typename IO::ivec *xin, const typename IO::ivec *yin,
		typename IO::ivec *omag, typename IO::ivec *ofreq,
		const IDX at, const uint32_t nvec, const bool first, const uint32_t phase0,
		const uint32_t *d_last, uint32_t (*edge)[kBlock / 64], unsigned &par, IO)
{
	const unsigned tid = threadIdx.x, lane = tid & 63u;
	// (the same in all of a wave's lanes: said so, it stays in a scalar)
	const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int sh = ln.sh;

	uint32_t prev = 0;	// the lane in front of sample 0 alone needs it
	if (first && tid == 0)
		prev = phase_in_front(phase0, d_last, sh);
	uint32_t j = tid;
	IDX g = at + tid;	// (= at + j)
	typename IO::ivec nx{}, ny{};	// software prefetch, afresh per tile (as
	if (j <= nvec && !(first && j == 0)) {	// topolar_lj_jobs)
		nx = CORDIC_LOAD_IN(&xin[g]);
		ny = CORDIC_LOAD_IN(&yin[g]);
	}
	// (thread 0's vector is behind the end: so is everyone's)
	for (uint32_t k0 = 0; k0 <= nvec; k0 += kBlock, j += kBlock, g += kBlock) {
		const i32x4 tx = IO::widen(nx), ty = IO::widen(ny);
		if (j + kBlock <= nvec) {
			nx = CORDIC_LOAD_IN(&xin[g + kBlock]);
			ny = CORDIC_LOAD_IN(&yin[g + kBlock]);
		}
		i32x4 rm;
		u32x4 rp;
		pol_lj_vector<NLIVE, DYN, UG, PLAIN>(kp, ln, tx, ty, rm, rp);

		uint32_t last = rp[3];
		if (first && j == 0)	// in front of sample 0
			last = prev;
		if (lane == 63)
			edge[par][wave] = last;
		uint32_t front = 0;
		if (wave == 0)		// (pass 0: the halo lane's, unused)
			front = edge[par ^ 1][kBlock / 64 - 1];
		__syncthreads();
		if (wave != 0)
			front = edge[par][wave - 1];
		par ^= 1;
		// wave_shr:1 -- lane l gets lane l - 1's `last`, lane 0 keeps
		// `front`
		const uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp(
			(int)front, (int)last, 0x138, 0xf, 0xf, false);
		i32x4 rf;
		rf[0] = step_of(rp[0], before, sh);
#pragma unroll
		for (int v = 1; v < kVec; v++)
			rf[v] = step_of(rp[v], rp[v - 1], sh);
		if (j != 0 && j <= nvec) {	// (not the halo)
			CORDIC_STORE_OUT(true, &omag[g], IO::narrow(rm));
			CORDIC_STORE_OUT(true, &ofreq[g], IO::narrow(rf));
		}
	}
}

// ONE tail (DemodTail), by one lane: its at most 4 samples gathered into one
// zero-padded vector, converted by the same pol_lj_vector instance as the
// sweep, differenced, stored; then *d_last.  A job without a whole vector reads
// its *d_last here, in the same lane, before writing it; every other job's was
// read by the sweep, in the launch in front.  IO (a tag, as in sweep_tile): the
// container of the four sample arrays, loaded and stored one element -- a word
// or a short -- at a time.
template <int NLIVE, bool DYN, bool UG, bool PLAIN, typename IO>
__device__ __forceinline__ void tail_of(const CoreParams &kp, const DemodTail d, IO)
{
	typedef typename IO::ielem ielem;
	const LaneConsts ln(kp);
	const ielem *x = reinterpret_cast<const ielem *>((uintptr_t)d.x);
	const ielem *y = reinterpret_cast<const ielem *>((uintptr_t)d.y);
	ielem *omag = reinterpret_cast<ielem *>((uintptr_t)d.mag);
	ielem *ofreq = reinterpret_cast<ielem *>((uintptr_t)d.freq);
	uint32_t *lp = reinterpret_cast<uint32_t *>((uintptr_t)d.last);
	i32x4 tx{}, ty{};
#pragma unroll
	for (int v = 0; v < kVec; v++)
		if ((uint32_t)v < d.count) {
			tx[v] = x[v];
			ty[v] = y[v];
		}
	i32x4 rm;
	u32x4 rp;
	pol_lj_vector<NLIVE, DYN, UG, PLAIN>(kp, ln, tx, ty, rm, rp);
	// element 0 only lends its phase when a whole vector was in front
	uint32_t p = rp[0];
	if (d.first) {
		p = phase_in_front(d.phase0, lp, ln.sh);
		omag[0] = (ielem)rm[0];
		ofreq[0] = (ielem)step_of(rp[0], p, ln.sh);
		p = rp[0];
	}
#pragma unroll
	for (int v = 1; v < kVec; v++)
		if ((uint32_t)v < d.count) {
			omag[v] = (ielem)rm[v];
			ofreq[v] = (ielem)step_of(rp[v], p, ln.sh);
			p = rp[v];
		}
	if (lp)
		*lp = p;
}

// ---- host: which instance serves a core
template <int NLIVE, bool DYN, bool UG, bool PLAIN>
struct Instance {
	static constexpr int nlive = NLIVE;
	static constexpr bool dyn = DYN, ug = UG, plain = PLAIN;
};

// Calls f with the Instance of the core: the choice of launch_pol_lj_jobs
// (cordic_inst_pol_lj.hip) -- 20 and 29 live stages on static PLAIN instances
// (WW <= 32, rounding at the 2^30 scale), every other core on the dynamic-exit
// one -- and unit gain on a dynamic-exit instance of its own, as launch_pol_lj
// has it.  (CORDIC_FORCE_DYN is launch_pol_lj's knob alone.)  The container
// comes as a tag: Io32 here, Io16 below.
template <typename F>
void with_instance(const cordic_config &cfg, const CoreParams &kp, F &&f, Io32)
{
	if (kp.post_mul != 0)		// CORDIC_FLAG_UNIT_GAIN
		return f(Instance<kDynStages, true, true, false>{});
	const bool plain = (32 - kp.iw) - kp.in_shl >= 2 && kp.r >= 2 && kp.r <= 31;
	switch (plain ? cfg.nlive : -1) {
	case 20: return f(Instance<20, false, false, true>{});
	case 29: return f(Instance<29, false, false, true>{});
	default: return f(Instance<kDynStages, true, false, false>{});
	}
}

// Io16: a core that a *16 call accepts has IW, OW, PW <= 16 and with them at
// most about 13 live stages (r2p 16 16 2 16 -1: WW 24, 13 stages), so the
// static 20- and 29-stage instances never apply: the dynamic-exit instance and
// its unit-gain twin serve every such core.
template <typename F>
void with_instance(const cordic_config &, const CoreParams &kp, F &&f, Io16)
{
	if (kp.post_mul != 0)		// CORDIC_FLAG_UNIT_GAIN
		return f(Instance<kDynStages, true, true, false>{});
	return f(Instance<kDynStages, true, false, false>{});
}

} // namespace fmd
} // namespace cordic_amd
#endif // __HIPCC__
#endif

