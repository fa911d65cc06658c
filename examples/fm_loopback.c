/* fm_loopback.c -- plain C caller of both halves of an FM link on the device
 * (include/cordic_amd.h, "frequency- and phase-modulated oscillators" and "FM
 * demodulation"): cordic_table_fm turns one tuning word per sample into a
 * quadrature pair on a quarter-wave table (rtl/quarterwav.v), cordic_fm_demod
 * turns the pair back into the phase step per sample on the converter
 * (rtl/topolar.v).  The transmitter's phase has PW_TX = 18 bits and the
 * converter's PW_RX = 32, so a tuning word f comes back as f << 14, give or
 * take the table's amplitude quantisation and the converter's phase error.
 * Prints the worst deviation of the recovered step from the tuning word.
 *
 *   gcc -std=c99 -I include -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       examples/fm_loopback.c -L cordic_amd -lcordic_amd -L /opt/rocm/lib \
 *       -lamdhip64 -Wl,-rpath,$PWD/cordic_amd -o tools/fm_loopback
 *   tools/fm_loopback [-l LOG2_SAMPLES]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "cordic_amd.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != CORDIC_OK) { \
	fprintf(stderr, "%s: %s\n", #call, cordic_strerror(rc_)); return 1; } } while (0)
#define HIP(call) do { if ((call) != hipSuccess) { \
	fprintf(stderr, "%s failed\n", #call); return 1; } } while (0)

enum { PW_TX = 18, OW_TX = 24 };

int main(int argc, char **argv)
{
	int lg = 20;
	for (int k = 1; k < argc; k += 2) {
		if (k + 1 < argc && !strcmp(argv[k], "-l")) lg = atoi(argv[k + 1]);
		else lg = -1;
	}
	if (lg < 4 || lg > 26) {
		fprintf(stderr, "usage: %s [-l LOG2_SAMPLES (4 .. 26)]\n", argv[0]);
		return 2;
	}
	const size_t n = ((size_t)1 << lg) + 3;	/* (no multiple of anything) */

	cordic_table_config tc;
	cordic_config conv;
	CHECK(cordic_table_config_init(&tc, CORDIC_QTR, -1, OW_TX, PW_TX));
	/* a converter whose inputs are as wide as the table's outputs */
	CHECK(cordic_config_init(&conv, CORDIC_R2P, OW_TX, 24, 2, -1, 20));
	cordic_table *osc;
	CHECK(cordic_table_create(&tc, &osc));
	int32_t fused = 0, tile = 0;
	CHECK(cordic_fm_demod_info(&conv, &fused, &tile));
	const int up = (int)conv.pw - PW_TX;	/* PW_RX - PW_TX */

	/* the message: a two-tone FSK with a slow ramp on top, in units of
	 * 2 pi / 2^PW_TX per sample, both signs */
	uint32_t *fcw = malloc(n * sizeof *fcw);
	int32_t *freq = malloc(n * sizeof *freq);
	if (!fcw || !freq) return 1;
	for (size_t i = 0; i < n; i++) {
		const int32_t f = ((i / 37) & 1 ? 1500 : -900) + (int32_t)((i >> 8) % 257);
		fcw[i] = (uint32_t)f;
	}
	uint32_t *d_fcw, *d_last;
	int32_t *d_i, *d_q, *d_mag, *d_freq;
	void *d_wtx, *d_wrx;
	HIP(hipMalloc((void **)&d_fcw, n * 4));
	HIP(hipMalloc((void **)&d_i, n * 4));
	HIP(hipMalloc((void **)&d_q, n * 4));
	HIP(hipMalloc((void **)&d_mag, n * 4));
	HIP(hipMalloc((void **)&d_freq, n * 4));
	HIP(hipMalloc((void **)&d_last, 4));
	HIP(hipMalloc(&d_wtx, cordic_fm_workspace(n)));
	HIP(hipMalloc(&d_wrx, cordic_fm_demod_workspace(n)));
	HIP(hipMemcpy(d_fcw, fcw, n * 4, hipMemcpyHostToDevice));
	HIP(hipMemset(d_last, 0, 4));

	/* transmit: d_q = sine, d_i = cosine of the accumulated phase (start 0);
	 * receive: the phase in front of sample 0 is 0 too, so freq[0] is the
	 * phase of the first sample itself */
	CHECK(cordic_table_fm(osc, n, d_fcw, NULL, 0, NULL, d_q, d_i, d_wtx, NULL));
	CHECK(cordic_fm_demod(&conv, n, d_i, d_q, 0, d_last, d_mag, d_freq, d_wrx, NULL));
	HIP(hipDeviceSynchronize());
	HIP(hipMemcpy(freq, d_freq, n * 4, hipMemcpyDeviceToHost));

	/* sample i of the pair sits at the phase accumulated BEFORE fcw[i]: the
	 * step into sample i is fcw[i - 1] */
	long long worst = 0;
	size_t at = 0;
	for (size_t i = 1; i < n; i++) {
		const long long want = (long long)(int32_t)fcw[i - 1] * (1LL << up);
		long long d = (long long)freq[i] - want;
		if (d < 0) d = -d;
		if (d > worst) { worst = d; at = i; }
	}
	printf("%zu samples, QTR table PW %d OW %d -> r2p IW %d PW %d (%s, tile %d)\n",
		n, PW_TX, OW_TX, (int)conv.iw, (int)conv.pw,
		fused ? "fused kernel" : "fallback", (int)tile);
	printf("worst |recovered step - tuning word| = %lld of 2^%d per turn "
		"(%.4f tuning-word LSBs), at sample %zu\n", worst, (int)conv.pw,
		(double)worst / (double)(1LL << up), at);
	cordic_table_destroy(osc);
	hipFree(d_fcw); hipFree(d_i); hipFree(d_q); hipFree(d_mag); hipFree(d_freq);
	hipFree(d_last); hipFree(d_wtx); hipFree(d_wrx);
	free(fcw); free(freq);
	return 0;
}
