/* ddc_receiver.c -- plain C caller of a DECIMATING 16-bit receiver bank
 * (cordic_rxbank_create_decim16; include/cordic_amd.h, "Decimating receiver
 * banks"): the chain of examples/ddc_channeliser.c -- tune, decimate by R = 8,
 * discriminate, CHANNELS short int16 blocks per round -- as ONE bank, two
 * launches a round, without the decimated I/Q array in between.  The
 * oscillator's accumulator and the discriminator's last phase are carried from
 * round to round in a d_acc and a d_last word per channel (phase0 = dphase0 =
 * 0).
 *
 * The reference is ddc_channeliser.c's chain itself: a decimating mixer bank
 * into a demodulation bank, four launches a round, with words of their own.
 * Every magnitude and frequency of every round, and every d_acc and d_last
 * word after the last round, must be the same.  Exit status 0 on equality.
 *
 *   gcc -std=c99 -I include -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       examples/ddc_receiver.c -L cordic_amd -lcordic_amd -L /opt/rocm/lib \
 *       -lamdhip64 -Wl,-rpath,$PWD/cordic_amd -o tools/ddc_receiver
 *   tools/ddc_receiver [-c CHANNELS] [-l BLOCK_SAMPLES] [-r ROUNDS]
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

enum { IW = 16, LOG2R = 3, R = 1 << LOG2R };

static uint32_t lcg(uint32_t *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s;
}

/* the LO's tuning word of channel c at sample i of its stream
 * (ddc_channeliser.c) */
static uint32_t tuning(size_t c, size_t i)
{
	return (uint32_t)((int32_t)(c % 97) * 1234567 - 40000000
		+ (int32_t)((i >> 6) % 129) * 4001 + ((i / 29) & 1 ? 77777 : -55555));
}

int main(int argc, char **argv)
{
	long channels = 256, block = 1504, rounds = 3;
	for (int k = 1; k < argc; k += 2) {
		if (k + 1 < argc && !strcmp(argv[k], "-c")) channels = atol(argv[k + 1]);
		else if (k + 1 < argc && !strcmp(argv[k], "-l")) block = atol(argv[k + 1]);
		else if (k + 1 < argc && !strcmp(argv[k], "-r")) rounds = atol(argv[k + 1]);
		else channels = -1;
	}
	if (channels < 1 || channels > 4096 || block < R || block > (1 << 20) || block % R
			|| rounds < 1 || rounds > 64) {
		fprintf(stderr, "usage: %s [-c CHANNELS (1 .. 4096)] [-l BLOCK_SAMPLES "
			"(%d .. 2^20, a multiple of %d)] [-r ROUNDS (1 .. 64)]\n", argv[0], R, R);
		return 2;
	}
	const size_t C = (size_t)channels, L = (size_t)block, n = C * L;
	const size_t M = L >> LOG2R, m = C * M;		/* decimated */

	cordic_config rot, conv;
	CHECK(cordic_config_init(&rot, CORDIC_P2R, IW, IW, 2, -1, -1));
	CHECK(cordic_config_init(&conv, CORDIC_R2P, IW, IW, 2, 16, -1));
	cordic_plan *plan;
	CHECK(cordic_plan_create(&rot, &plan));

	uint32_t *fcw = malloc(n * sizeof *fcw);
	int16_t *iq = malloc(2 * n * sizeof *iq);
	int16_t *got = malloc(2 * m * sizeof *got), *want = malloc(2 * m * sizeof *want);
	uint32_t *wa = malloc(4 * C * sizeof *wa);
	cordic_fmrx_job16 *rjobs = malloc(C * sizeof *rjobs);
	cordic_fmmix_job16 *mjobs = malloc(C * sizeof *mjobs);
	cordic_demod_job16 *djobs = malloc(C * sizeof *djobs);
	if (!fcw || !iq || !got || !want || !wa || !rjobs || !mjobs || !djobs) return 1;
	/* d_in: [i | q] at the input rate; d_out: the receiver bank's [mag | freq]
	 * at the decimated rate; d_ref: the chain's [tuned i | tuned q | mag | freq]
	 * at the decimated rate; d_words: [acc | last] of the receiver bank, then of
	 * the chain */
	uint32_t *d_fcw, *d_words;
	int16_t *d_in, *d_out, *d_ref;
	HIP(hipMalloc((void **)&d_fcw, n * 4));
	HIP(hipMalloc((void **)&d_in, 2 * n * 2));
	HIP(hipMalloc((void **)&d_out, 2 * m * 2));
	HIP(hipMalloc((void **)&d_ref, 4 * m * 2));
	HIP(hipMalloc((void **)&d_words, 4 * C * 4));
	HIP(hipMemset(d_words, 0, 4 * C * 4));
	uint32_t *d_acc = d_words, *d_last = d_words + C, *d_racc = d_words + 2 * C,
		*d_rlast = d_words + 3 * C;

	for (size_t c = 0; c < C; c++) {
		memset(&rjobs[c], 0, sizeof rjobs[c]);
		rjobs[c].d_fcw = d_fcw + c * L;
		rjobs[c].d_xval = d_in + c * L;
		rjobs[c].d_yval = d_in + n + c * L;
		rjobs[c].d_omag = d_out + c * M;	/* n >> k elements per job */
		rjobs[c].d_ofreq = d_out + m + c * M;
		rjobs[c].d_acc = d_acc + c;
		rjobs[c].d_last = d_last + c;
		rjobs[c].n = L;
		memset(&mjobs[c], 0, sizeof mjobs[c]);
		mjobs[c].d_fcw = d_fcw + c * L;
		mjobs[c].d_xval = d_in + c * L;
		mjobs[c].d_yval = d_in + n + c * L;
		mjobs[c].d_oxval = d_ref + c * M;
		mjobs[c].d_oyval = d_ref + m + c * M;
		mjobs[c].d_acc = d_racc + c;
		mjobs[c].n = L;
		memset(&djobs[c], 0, sizeof djobs[c]);
		djobs[c].d_xval = d_ref + c * M;
		djobs[c].d_yval = d_ref + m + c * M;
		djobs[c].d_omag = d_ref + 2 * m + c * M;
		djobs[c].d_ofreq = d_ref + 3 * m + c * M;
		djobs[c].d_last = d_rlast + c;
		djobs[c].n = M;
	}
	cordic_rxbank *rx;
	cordic_mixbank *mix;
	cordic_demodbank *dem;
	CHECK(cordic_rxbank_create_decim16(plan, &conv, LOG2R, C, rjobs, &rx));
	CHECK(cordic_mixbank_create_decim16(plan, LOG2R, C, mjobs, &mix));
	CHECK(cordic_demodbank_create16(&conv, C, djobs, &dem));
	uint64_t samples;
	uint32_t spans;
	int32_t fused, tile;
	CHECK(cordic_rxbank_info(rx, &samples, &spans, &fused, &tile));

	uint32_t seed = 12345;
	size_t bad = 0;
	for (size_t r = 0; r < (size_t)rounds; r++) {
		for (size_t c = 0; c < C; c++)
			for (size_t i = 0; i < L; i++)
				fcw[c * L + i] = tuning(c, r * L + i);
		for (size_t k = 0; k < 2 * n; k++)	/* full-scale IW-bit samples */
			iq[k] = (int16_t)((int32_t)(lcg(&seed) >> (32 - IW)) - (1 << (IW - 1)));
		HIP(hipMemcpy(d_fcw, fcw, n * 4, hipMemcpyHostToDevice));
		HIP(hipMemcpy(d_in, iq, 2 * n * 2, hipMemcpyHostToDevice));
		/* every channel's block through its receiver: two launches ... */
		CHECK(cordic_rxbank_run(rx, NULL));
		/* ... and through the chain of two banks: four */
		CHECK(cordic_mixbank_run(mix, NULL));
		CHECK(cordic_demodbank_run(dem, NULL));
		HIP(hipDeviceSynchronize());
		HIP(hipMemcpy(got, d_out, 2 * m * 2, hipMemcpyDeviceToHost));
		HIP(hipMemcpy(want, d_ref + 2 * m, 2 * m * 2, hipMemcpyDeviceToHost));
		for (size_t k = 0; k < 2 * m; k++)
			bad += got[k] != want[k];
	}
	HIP(hipMemcpy(wa, d_words, 4 * C * 4, hipMemcpyDeviceToHost));
	for (size_t k = 0; k < 2 * C; k++)
		bad += wa[k] != wa[2 * C + k];
	printf("%zu channels x %zu samples x %ld rounds, decimated by %d to %zu, on int16; "
		"receiver bank: %llu samples, %u spans of passes of %d (%s)\n", C, L, rounds, R,
		M, (unsigned long long)samples, spans, (int)tile,
		fused ? "fused, two launches per round" : "one by one");
	printf("%zu shorts or words differ from the decimating mixer bank into the "
		"demodulation bank\n", bad);
	cordic_rxbank_destroy(rx);
	cordic_mixbank_destroy(mix);
	cordic_demodbank_destroy(dem);
	cordic_plan_destroy(plan);
	hipFree(d_fcw); hipFree(d_in); hipFree(d_out); hipFree(d_ref); hipFree(d_words);
	free(fcw); free(iq); free(got); free(want); free(wa); free(rjobs); free(mjobs);
	free(djobs);
	return bad ? 1 : 0;
}
