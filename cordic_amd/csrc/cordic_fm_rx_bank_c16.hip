// cordic_fm_rx_bank_c16.hip -- the receiver banks' <30, IoC16> instances
// (interleaved int16 I/Q in, int16 arrays out; cordic_rxbank_create_c16):
// cordic_fm_rx_bank.hip compiled as a unit of its own.
//
// Registers (.vgpr_count of the gfx950 code objects, -O3, --save-temps;
// .private_segment_fixed_size is 0 for every instance):
//   live stages                   13   16   19   20   24   27   29
//   fm_rxbank_xydir<30, N, IoC16> 132  142  133  133  134  137  137
//   ... <30, N, Io16>             130  132  131  131  132  135  135
// above 128 as the twin's are: the banks' grid is sized for 3 blocks per CU
// (kFmrxbBlocksPerCu), which holds up to 168.
// profiles/r24/fm_rx_c16.txt.
#define CORDIC_FMRXB_UNIT 0xc16
#include "cordic_fm_rx_bank.hip"
