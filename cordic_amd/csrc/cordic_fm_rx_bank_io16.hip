// cordic_fm_rx_bank_io16.hip -- the receiver banks' <30, Io16> instances (int16
// arrays): cordic_fm_rx_bank.hip compiled as a unit of its own, beside the others.
#define CORDIC_FMRXB_UNIT 16
#include "cordic_fm_rx_bank.hip"
