// cordic_fm_rx_bank_decim_io16.hip -- the decimating receiver banks' <30, Io16>
// instances (int16 arrays): cordic_fm_rx_bank_decim.hip compiled as a unit of
// its own.
#define CORDIC_FMRXBD_UNIT 16
#include "cordic_fm_rx_bank_decim.hip"
