// cordic_fm_rx_bank_decim_lj29.hip -- the decimating receiver banks' <29, Io32>
// instances (WW 35 plans): cordic_fm_rx_bank_decim.hip compiled as a unit of
// its own.
#define CORDIC_FMRXBD_UNIT 29
#include "cordic_fm_rx_bank_decim.hip"
