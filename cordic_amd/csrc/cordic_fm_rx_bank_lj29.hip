// cordic_fm_rx_bank_lj29.hip -- the receiver banks' <29, Io32> instances (WW 35
// plans): cordic_fm_rx_bank.hip compiled as a unit of its own, beside the others.
#define CORDIC_FMRXB_UNIT 29
#include "cordic_fm_rx_bank.hip"
