/* fm_channeliser.c -- plain C caller of an FM demodulation bank
 * (include/cordic_amd.h, "FM demodulation banks"): the block that ends a
 * channeliser's receive chain when its channels carry FM.  CHANNELS short
 * blocks per round; cordic_table_fm (a quarter-wave table, rtl/quarterwav.v)
 * makes each channel's quadrature pair from one tuning word per sample, its
 * accumulator carried from round to round in a d_acc word per channel; ONE
 * cordic_demodbank over all channels, each with a d_last word of its own and
 * phase0 = 0, turns every round's pairs back into the phase step per sample --
 * two launches per round, no host work between rounds.  The transmitter's
 * phase has PW_TX = 18 bits and the converter's PW_RX = 32, so a tuning word f
 * comes back as f << 14, give or take the table's amplitude quantisation and
 * the converter's phase error (examples/fm_loopback.c does the same for one
 * channel in one call).  Prints the worst deviation over all channels and
 * rounds, the first sample of every later round -- whose predecessor is the
 * last sample of the round before -- included; only the very first sample of a
 * channel has no step to compare (its "step" is its own phase, and a
 * quarter-wave table starts half a phase LSB off zero).  Exit status 0 when
 * that deviation is under half a tuning-word LSB, so that rounding recovers
 * every tuning word.
 *
 *   gcc -std=c99 -I include -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       examples/fm_channeliser.c -L cordic_amd -lcordic_amd -L /opt/rocm/lib \
 *       -lamdhip64 -Wl,-rpath,$PWD/cordic_amd -o tools/fm_channeliser
 *   tools/fm_channeliser [-c CHANNELS] [-l BLOCK_SAMPLES] [-r ROUNDS]
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

/* the message of channel c at sample i of its stream: a two-tone FSK with a
 * slow ramp on top and an offset per channel, in units of 2 pi / 2^PW_TX per
 * sample, both signs */
static int32_t message(size_t c, size_t i)
{
	return ((i / 37) & 1 ? 1500 : -900) + (int32_t)((i >> 8) % 257)
		+ (int32_t)(c % 64) * 17 - 500;
}

int main(int argc, char **argv)
{
	long channels = 256, block = 4099, rounds = 4;
	for (int k = 1; k < argc; k += 2) {
		if (k + 1 < argc && !strcmp(argv[k], "-c")) channels = atol(argv[k + 1]);
		else if (k + 1 < argc && !strcmp(argv[k], "-l")) block = atol(argv[k + 1]);
		else if (k + 1 < argc && !strcmp(argv[k], "-r")) rounds = atol(argv[k + 1]);
		else channels = -1;
	}
	if (channels < 1 || channels > 4096 || block < 1 || block > (1 << 20)
			|| rounds < 1 || rounds > 64) {
		fprintf(stderr, "usage: %s [-c CHANNELS (1 .. 4096)] [-l BLOCK_SAMPLES "
			"(1 .. 2^20)] [-r ROUNDS (1 .. 64)]\n", argv[0]);
		return 2;
	}
	const size_t C = (size_t)channels, L = (size_t)block, n = C * L;

	cordic_table_config tc;
	cordic_config conv;
	CHECK(cordic_table_config_init(&tc, CORDIC_QTR, -1, OW_TX, PW_TX));
	/* a converter whose inputs are as wide as the table's outputs */
	CHECK(cordic_config_init(&conv, CORDIC_R2P, OW_TX, 24, 2, -1, 20));
	cordic_table *osc;
	CHECK(cordic_table_create(&tc, &osc));
	const int up = (int)conv.pw - PW_TX;	/* PW_RX - PW_TX */

	uint32_t *fcw = malloc(n * sizeof *fcw);
	int32_t *freq = malloc(n * sizeof *freq);
	uint32_t *before = malloc(C * sizeof *before);	/* last word of the round before */
	cordic_demod_job *jobs = malloc(C * sizeof *jobs);
	if (!fcw || !freq || !before || !jobs) return 1;
	uint32_t *d_fcw, *d_acc, *d_last;
	int32_t *d_i, *d_q, *d_mag, *d_freq;
	void *d_wtx;
	HIP(hipMalloc((void **)&d_fcw, n * 4));
	HIP(hipMalloc((void **)&d_i, n * 4));
	HIP(hipMalloc((void **)&d_q, n * 4));
	HIP(hipMalloc((void **)&d_mag, n * 4));
	HIP(hipMalloc((void **)&d_freq, n * 4));
	HIP(hipMalloc((void **)&d_acc, C * 4));
	HIP(hipMalloc((void **)&d_last, C * 4));
	HIP(hipMalloc(&d_wtx, cordic_fm_workspace(L)));
	/* transmitter and receiver start at phase 0 */
	HIP(hipMemset(d_acc, 0, C * 4));
	HIP(hipMemset(d_last, 0, C * 4));

	/* channel c's block of a round sits at [c * L, (c + 1) * L): for an odd L
	 * the blocks are off the 16-byte grid, which a bank serves all the same */
	for (size_t c = 0; c < C; c++) {
		memset(&jobs[c], 0, sizeof jobs[c]);
		jobs[c].d_xval = d_i + c * L;
		jobs[c].d_yval = d_q + c * L;
		jobs[c].d_omag = d_mag + c * L;
		jobs[c].d_ofreq = d_freq + c * L;
		jobs[c].d_last = d_last + c;
		jobs[c].n = L;
	}
	cordic_demodbank *bank;
	CHECK(cordic_demodbank_create(&conv, C, jobs, &bank));
	uint64_t samples;
	uint32_t tiles, tail_jobs;
	int32_t fused, tile;
	CHECK(cordic_demodbank_info(bank, &samples, &tiles, &tail_jobs, &fused, &tile));

	long long worst = 0;
	size_t at_c = 0, at_i = 0;
	for (size_t r = 0; r < (size_t)rounds; r++) {
		for (size_t c = 0; c < C; c++) {
			before[c] = r ? fcw[c * L + L - 1] : 0;
			for (size_t i = 0; i < L; i++)
				fcw[c * L + i] = (uint32_t)message(c, r * L + i);
		}
		HIP(hipMemcpy(d_fcw, fcw, n * 4, hipMemcpyHostToDevice));
		/* transmit: d_q = sine, d_i = cosine of the accumulated phase */
		for (size_t c = 0; c < C; c++)
			CHECK(cordic_table_fm(osc, L, d_fcw + c * L, NULL, 0, d_acc + c,
				d_q + c * L, d_i + c * L, d_wtx, NULL));
		/* receive: every channel's block in one run */
		CHECK(cordic_demodbank_run(bank, NULL));
		HIP(hipDeviceSynchronize());
		HIP(hipMemcpy(freq, d_freq, n * 4, hipMemcpyDeviceToHost));
		/* sample i of a pair sits at the phase accumulated BEFORE fcw[i]:
		 * the step into sample i is fcw[i - 1], across rounds as well */
		for (size_t c = 0; c < C; c++)
			for (size_t i = r ? 0 : 1; i < L; i++) {
				const uint32_t f = i ? fcw[c * L + i - 1] : before[c];
				const long long want = (long long)(int32_t)f * (1LL << up);
				long long d = (long long)freq[c * L + i] - want;
				if (d < 0) d = -d;
				if (d > worst) { worst = d; at_c = c; at_i = r * L + i; }
			}
	}
	printf("%zu channels x %zu samples x %ld rounds, QTR table PW %d OW %d -> r2p "
		"IW %d PW %d; bank: %llu samples, %u tiles of %d, %u tail jobs (%s)\n",
		C, L, rounds, PW_TX, OW_TX, (int)conv.iw, (int)conv.pw,
		(unsigned long long)samples, tiles, (int)tile, tail_jobs,
		fused ? "fused, two launches per round" : "one by one");
	printf("worst |recovered step - tuning word| = %lld of 2^%d per turn "
		"(%.4f tuning-word LSBs), channel %zu sample %zu\n", worst, (int)conv.pw,
		(double)worst / (double)(1LL << up), at_c, at_i);
	cordic_demodbank_destroy(bank);
	cordic_table_destroy(osc);
	hipFree(d_fcw); hipFree(d_i); hipFree(d_q); hipFree(d_mag); hipFree(d_freq);
	hipFree(d_acc); hipFree(d_last); hipFree(d_wtx);
	free(fcw); free(freq); free(before); free(jobs);
	/* a clean loop-back: rounding recovers every tuning word */
	return 2 * worst < (1LL << up) ? 0 : 1;
}
