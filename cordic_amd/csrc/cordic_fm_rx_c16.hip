// cordic_fm_rx_c16.hip -- the tuned FM receiver's <30, IoC16> instances
// (interleaved int16 I/Q in, int16 arrays out; cordic_plan_fm_rx_c16):
// cordic_fm_rx.hip compiled as a unit of its own, beside the others.
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps;
// .private_segment_fixed_size is 0 for every instance):
//   live stages               13   16   19   20   24   27   29
//   fm_rx_xydir<30, N, IoC16> 106  106  106  106  108  110  111
//   ... <30, N, Io16>         106  106  106  106  108  111  111
// within 128: 4 waves per SIMD, the grid's 4 blocks per CU (kFmrxBlocksPerCu).
// profiles/r24/fm_rx_c16.txt.
#define CORDIC_FMRX_UNIT 0xc16
#include "cordic_fm_rx.hip"
