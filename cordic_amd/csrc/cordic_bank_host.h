// cordic_bank_host.h -- what the creates of the "many small jobs" handles share
// (job sets; FM banks, cordic_fm_demod_bank.h and cordic_fm_mix_bank.h): the
// overlap rule over sorted byte ranges, the tile-length rule, the power-of-two
// knob.  Plain C++ that touches no device, so that a stand-alone program can run
// it under a sanitizer (tests/test_bank_host.py).
//
// No kernel of the DESIGN section 4.4 sweep lives here, so tools/build_stamp.py
// does not hash this unit.
#ifndef CORDIC_BANK_HOST_H
#define CORDIC_BANK_HOST_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace cordic_amd {

// The byte ranges of a bank's arrays.  No output range may overlap another
// output range or any input range; inputs may alias.  Found by sorting the
// ranges by address: a range that begins inside an earlier one is an overlap,
// which is refused unless both are inputs.
struct BankRanges {
	struct R { uint64_t lo, hi; bool out; };
	std::vector<R> r;
	// false: the range wraps around the end of the address space
	bool add(uint64_t addr, uint64_t bytes, bool is_output)
	{
		if (bytes > ~(uint64_t)0 - addr)
			return false;
		r.push_back(R{addr, addr + bytes, is_output});
		return true;
	}
	bool outputs_clear()
	{
		std::sort(r.begin(), r.end(),
			[](const R &a, const R &b) { return a.lo < b.lo; });
		uint64_t any_end = 0, out_end = 0;	// ends of the ranges in front
		for (const R &a : r) {
			if (a.lo < (a.out ? any_end : out_end))
				return false;
			any_end = std::max(any_end, a.hi);
			if (a.out)
				out_end = std::max(out_end, a.hi);
		}
		return true;
	}
};

// The tile-length rule: the longest tile that still gives every resident block
// (`blocks_per_cu` on each of `cus` CUs; cus <= 0: 256) four of them: what such
// a tile holds of a bank of `total`, in the units of `total` ...
inline uint64_t bank_tile_room(uint64_t total, int cus, int blocks_per_cu)
{
	return total / ((uint64_t)(cus > 0 ? cus : 256) * (uint64_t)blocks_per_cu * 4u);
}
// ... and in passes of `unit` each, in the steps 1, 2, 4, ... max
inline uint32_t bank_passes(uint64_t total, int cus, int blocks_per_cu,
		uint32_t unit, uint32_t max)
{
	const uint64_t per = bank_tile_room(total, cus, blocks_per_cu) / unit;
	uint32_t p = 1;
	while (p < max && (uint64_t)p * 2 <= per)
		p <<= 1;
	return p;
}

// An environment variable's value `e` (NULL: not set) that forces P: a power
// of two within 1 .. max replaces `p`, anything else keeps it.
inline uint32_t bank_forced_passes(const char *e, uint32_t max, uint32_t p)
{
	const long v = e ? std::strtol(e, nullptr, 10) : 0;
	return (v >= 1 && v <= (long)max && !(v & (v - 1))) ? (uint32_t)v : p;
}

} // namespace cordic_amd
#endif
