// cordic_fm_rx_lj29.hip -- the tuned FM receivers <29, Io32> instances (WW 35
// plans): cordic_fm_rx.hip compiled as a unit of its own, beside the others.
#define CORDIC_FMRX_UNIT 29
#include "cordic_fm_rx.hip"
