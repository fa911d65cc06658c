// cordic_hostargs.h -- argument checks that the FM units' entry points share
// (cordic_fm_demod.hip, cordic_fm_mix.hip, cordic_table_fm.hip): byte ranges and
// the rule "no output range over another output or any input", and the
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
