// cordic_hostargs.h -- argument checks that the FM units' entry points share
// (cordic_fm_demod.hip, cordic_fm_mix.hip, cordic_table_fm.hip): byte ranges and
// the rule "no output range over another output or any input", the whole check
// of an I/Q call with tuning words, the span of a single call's block and the
// environment's cap on a grid.  Plain C++ that touches no device, so that a
// stand-alone program can run it under a sanitizer (tests/test_hostargs.py).
// (A bank of many jobs sorts its ranges instead: BankRanges, cordic_bank_host.h.)
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_HOSTARGS_H
#define CORDIC_HOSTARGS_H

#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace cordic_amd {

struct Range {
	uintptr_t lo;
	size_t	bytes;
};

// (an optional array that is not there is an empty range)
inline Range range_of(const void *p, size_t bytes)
{
	return Range{reinterpret_cast<uintptr_t>(p), p ? bytes : 0};
}

inline bool hits(const Range &a, const Range &b)
{
	return a.bytes && b.bytes && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes;
}

// 1: an output range lies over another output range or over an input range.
// inplace: out[0] may begin where in[0] begins -- the one pair a call can
// declare safe (cordic_phase_accumulate with d_phase == d_fcw).
template <size_t NOUT, size_t NIN>
inline bool outputs_overlap(const Range (&out)[NOUT], const Range (&in)[NIN],
		bool inplace = false)
{
	for (size_t i = 0; i < NOUT; i++) {
		for (size_t j = i + 1; j < NOUT; j++)
			if (hits(out[i], out[j]))
				return true;
		for (size_t j = 0; j < NIN; j++)
			if (hits(out[i], in[j]) && !(inplace && i == 0 && j == 0
					&& out[0].lo == in[0].lo))
				return true;
	}
	return false;
}

// The check of an I/Q call with per-sample tuning words (the FM mixer, the
// tuned FM receiver), n > 0 samples of `esize` bytes (4 or 2): d_fcw, the two
// sample inputs, the two sample outputs and d_work are there (d_pm, d_acc and
// d_last may be NULL), n <= SIZE_MAX >> 4, the words on the grid of 4, the
// sample arrays on that of esize, d_work on that of 16, and no output range --
// the two arrays, the words at d_acc and d_last, the `work_bytes` of d_work --
// over another output or any input, by the true byte ranges.  out_shift: the
// two output arrays hold n >> out_shift elements (the decimating mixer).
// interleaved: the two sample inputs are ONE array at d_x, I and Q by turns --
// there, on the grid of a complex sample (2 * esize), 2 * esize * n bytes --
// and d_y is not looked at (the *_c16 receivers); the outputs stay two arrays
// unless out_interleaved says the same of them (the *_c16 mixers): ONE array at
// d_o0 on the grid of a complex sample, 2 * esize * (n >> out_shift) bytes, and
// d_o1 is not looked at.
inline bool iq_call_ok(size_t n, const void *d_acc, const void *d_last,
		const void *d_fcw, const void *d_pm, const void *d_x, const void *d_y,
		const void *d_o0, const void *d_o1, size_t esize, const void *d_work,
		size_t work_bytes, unsigned out_shift = 0, bool interleaved = false,
		bool out_interleaved = false)
{
	if (interleaved)
		d_y = nullptr;
	if (out_interleaved)
		d_o1 = nullptr;
	if (!d_fcw || !d_x || (!d_y && !interleaved) || !d_o0 || (!d_o1 && !out_interleaved)
			|| !d_work || n > (~(size_t)0 >> 4))
		return false;
	const uintptr_t words = reinterpret_cast<uintptr_t>(d_fcw)
		| reinterpret_cast<uintptr_t>(d_pm) | reinterpret_cast<uintptr_t>(d_acc)
		| reinterpret_cast<uintptr_t>(d_last);
	const uintptr_t samples = reinterpret_cast<uintptr_t>(d_x)
		| reinterpret_cast<uintptr_t>(d_y) | reinterpret_cast<uintptr_t>(d_o0)
		| reinterpret_cast<uintptr_t>(d_o1);
	if ((words & 3u) || (samples & (esize - 1))
			|| (reinterpret_cast<uintptr_t>(d_work) & 15u)
			|| (interleaved && (reinterpret_cast<uintptr_t>(d_x) & (2 * esize - 1)))
			|| (out_interleaved && (reinterpret_cast<uintptr_t>(d_o0) & (2 * esize - 1))))
		return false;
	const size_t nout = n >> out_shift;
	const Range out[5] = {range_of(d_o0, nout * esize * (out_interleaved ? 2 : 1)),
		range_of(d_o1, nout * esize),
		range_of(d_acc, 4), range_of(d_last, 4), range_of(d_work, work_bytes)};
	const Range in[4] = {range_of(d_fcw, n * 4), range_of(d_pm, n * 4),
		range_of(d_x, n * esize * (interleaved ? 2 : 1)), range_of(d_y, n * esize)};
	return !outputs_overlap(out, in);
}

// The span of a single call of n > 0 samples on at most `cap` blocks: every
// block owns `span` consecutive samples -- whole passes of `pass`, less the
// `halo` samples in front that a receiver's block computes again -- and the
// last one what is left; grid <= cap.  A span of p passes yields p * pass -
// halo samples, at least p * (pass - halo): p for at most `cap` spans.
struct CallSpan {
	size_t	span, grid;
};
inline CallSpan call_span(size_t n, size_t cap, size_t pass, size_t halo)
{
	const size_t yield1 = pass - halo;
	const size_t npass = (n + yield1 - 1) / yield1;
	const size_t per_block = (npass + cap - 1) / cap;
	const size_t span = per_block * pass - halo;
	return CallSpan{span, (n + span - 1) / span};
}

// min(cap, the value of the environment variable `name`) for values >= 1; read
// at every call (the CORDIC_*_MAX_BLOCKS test and A/B knobs)
inline size_t env_block_cap(const char *name, size_t cap)
{
	if (const char *e = std::getenv(name)) {
		const long v = std::strtol(e, nullptr, 10);
		if (v >= 1 && (size_t)v < cap)
			cap = (size_t)v;
	}
	return cap;
}

} // namespace cordic_amd
#endif
