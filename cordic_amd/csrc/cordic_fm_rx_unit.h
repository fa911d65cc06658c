// cordic_fm_rx_unit.h -- the tuned FM receiver's units: ONE list of the <LJ,
// container> pairs its four launch-2 kernels are instantiated for, in the order
// of fmx::Unit (cordic_fm_mix.h).  Each of cordic_fm_rx.hip,
// cordic_fm_rx_decim.hip, cordic_fm_rx_bank.hip and cordic_fm_rx_bank_decim.hip
// is compiled once per entry, -DCORDIC_FMRX_UNIT=<position> (the Makefile's
// pattern rule; 0, the default, also holds launch 1 and the host side), so that
// the sixteen objects build beside each other.  From the list come
//   - the compiled unit's kUnitLj, UnitIo and the suffix of its ONE entry point
//     (FMRX_ENTRY(launch_rx) is launch_rx_lj29 in unit 1),
//   - the declarations of all sixteen entry points, one function type per call
//     shape (the plain forms take k and ignore it),
//   - the tables [decimating][unit] that launch_fm_rx and launch_fmrx_bank index
//     by fmx::unit_of, expanded there.
// A new container is one more entry here, one more value of fmx::Unit and one
// more suffix in the Makefile's FMRX_UNITS.  For hipcc only.
#ifndef CORDIC_FM_RX_UNIT_H
#define CORDIC_FM_RX_UNIT_H

#include "cordic_fm_rx.h"

#ifdef __HIPCC__

// X(suffix, LJ, IO)
#define CORDIC_FMRX_UNITS(X) \
	X(lj30, 30, Io32) X(lj29, 29, Io32) X(io16, 30, Io16) X(c16, 30, fmx::IoC16)

#ifndef CORDIC_FMRX_UNIT
#define CORDIC_FMRX_UNIT 0	// the position in the list
#endif

namespace cordic_amd {

struct RxSpan;		// (cordic_fm_rx_bank.h)

namespace fmrx {

using namespace dev;

// an entry's position, by its suffix
namespace unit_at {
#define X(sfx, lj, io) sfx,
enum { CORDIC_FMRX_UNITS(X) kCount };
#undef X
}
constexpr int kUnits = unit_at::kCount;

// ... is the enum's value: what fmx::unit_of answers for a core of that LJ (WW
// 35 is LJ 29) on that container
template <int I> struct UnitAt;
#define X(sfx, lj, io) \
	template <> struct UnitAt<unit_at::sfx> { \
		static constexpr int kLj = lj; \
		typedef io Io; \
	}; \
	static_assert(fmx::unit_of(lj == 29 ? 35 : 34, sizeof(io::ielem), fmx::is_iq<io>::value) \
		== unit_at::sfx, "the list is in the order of fmx::Unit");
CORDIC_FMRX_UNITS(X)
#undef X

// the compiled unit's <LJ, container> ...
constexpr int kUnitLj = UnitAt<CORDIC_FMRX_UNIT>::kLj;
typedef UnitAt<CORDIC_FMRX_UNIT>::Io UnitIo;

// ... and its suffix: the list's suffixes as arguments, the unit's picked
#define FMRX_PICK0(a, ...) a
#define FMRX_PICK1(a, b, ...) b
#define FMRX_PICK2(a, b, c, ...) c
#define FMRX_PICK3(a, b, c, d, ...) d
#define FMRX_PICK_(i, ...) FMRX_PICK##i(__VA_ARGS__)
#define FMRX_PICK(i, ...) FMRX_PICK_(i, __VA_ARGS__)
#define FMRX_SUFFIX_OF(sfx, lj, io) sfx,
#define FMRX_SUFFIX FMRX_PICK(CORDIC_FMRX_UNIT, CORDIC_FMRX_UNITS(FMRX_SUFFIX_OF))
#define FMRX_PASTE_(stem, sfx) stem##_##sfx
#define FMRX_PASTE(stem, sfx) FMRX_PASTE_(stem, sfx)
#define FMRX_ENTRY(stem) FMRX_PASTE(stem, FMRX_SUFFIX)
static_assert(unit_at::FMRX_SUFFIX == CORDIC_FMRX_UNIT, "the suffix is this unit's");

// The entry points: each launches its kernel's instance for nlive live stages
// around fmx::with_stages; false: no instance, nothing enqueued.  log2r: the
// decimating forms' k in 1 .. 8; the plain forms ignore it.
typedef bool RxLaunch(int nlive, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const RxArgs &a, uint32_t log2r);
typedef bool BankLaunch(int nlive, unsigned grid, size_t lds, hipStream_t st,
		const CoreParams &kp, const DirArgs &da, const RxSpan *spans,
		uint32_t nspans, const uint32_t *start, const uint32_t *part,
		const uint32_t *prev, const uint32_t *ckmem, uint32_t xw, uint32_t log2r);
#define X(sfx, lj, io) \
	RxLaunch launch_rx_##sfx, launch_rxd_##sfx; \
	BankLaunch launch_rxbank_##sfx, launch_rxbank_decim_##sfx;
CORDIC_FMRX_UNITS(X)
#undef X

} // namespace fmrx
} // namespace cordic_amd
#endif // __HIPCC__
#endif
