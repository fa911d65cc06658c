// cordic_fm_rx_io16.hip -- the tuned FM receivers <30, Io16> instances (int16
// arrays): cordic_fm_rx.hip compiled as a unit of its own, beside the others.
#define CORDIC_FMRX_UNIT 16
#include "cordic_fm_rx.hip"
