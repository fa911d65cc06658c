// cordic_fm_rx_decim_io16.hip -- the decimating FM receiver's <30, Io16>
// instances (int16 arrays): cordic_fm_rx_decim.hip compiled as a unit of its own.
#define CORDIC_FMRXD_UNIT 16
#include "cordic_fm_rx_decim.hip"
