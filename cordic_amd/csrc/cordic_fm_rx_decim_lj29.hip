// cordic_fm_rx_decim_lj29.hip -- the decimating FM receiver's <29, Io32>
// instances (WW 35 plans): cordic_fm_rx_decim.hip compiled as a unit of its own.
#define CORDIC_FMRXD_UNIT 29
#include "cordic_fm_rx_decim.hip"
