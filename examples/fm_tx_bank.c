/* fm_tx_bank.c -- plain C caller of an FM oscillator bank
 * (include/cordic_amd.h, "FM oscillator banks") in front of an FM demodulation
 * bank: the link of examples/fm_channeliser.c with its transmit half run as a
 * bank as well.  CHANNELS short blocks per round; ONE cordic_fmbank over all
 * channels makes every channel's quadrature pair from one tuning word per
 * sample (a quarter-wave table, rtl/quarterwav.v), each channel's accumulator
 * carried from round to round in a d_acc word of its own with phase0 = 0; ONE
 * cordic_demodbank turns every round's pairs back into the phase step per
 * sample.  A round is four launches, whatever the number of channels, with no
 * host work between the two banks.
 *
 * The first round also runs the per-channel cordic_table_fm calls -- two
 * launches per channel -- into a second set of arrays and compares every
 * sample and every d_acc word with the bank's.  As in fm_channeliser.c the
 * transmitter's phase has PW_TX = 18 bits and the converter's PW_RX = 32, so a
 * tuning word f comes back as f << 14, give or take the table's amplitude
 * quantisation and the converter's phase error.  Exit status 0 when no word
 * differs and the worst deviation of a recovered step is under half a
 * tuning-word LSB, so that rounding recovers every tuning word.
 *
 *   gcc -std=c99 -I include -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       examples/fm_tx_bank.c -L cordic_amd -lcordic_amd -L /opt/rocm/lib \
 *       -lamdhip64 -Wl,-rpath,$PWD/cordic_amd -o tools/fm_tx_bank
 *   tools/fm_tx_bank [-c CHANNELS] [-l BLOCK_SAMPLES] [-r ROUNDS]
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

/* the message of channel c at sample i of its stream: as fm_channeliser.c */
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
	int32_t *a = malloc(n * sizeof *a), *b = malloc(n * sizeof *b);
	uint32_t *before = malloc(C * sizeof *before);	/* last word of the round before */
	uint32_t *acc = malloc(2 * C * sizeof *acc);
	cordic_fmosc_job *tx = malloc(C * sizeof *tx);
	cordic_demod_job *rx = malloc(C * sizeof *rx);
	if (!fcw || !freq || !a || !b || !before || !acc || !tx || !rx) return 1;
	uint32_t *d_fcw, *d_acc, *d_acc1, *d_last;
	int32_t *d_i, *d_q, *d_i1, *d_q1, *d_mag, *d_freq;
	void *d_wtx;
	HIP(hipMalloc((void **)&d_fcw, n * 4));
	HIP(hipMalloc((void **)&d_i, n * 4));
	HIP(hipMalloc((void **)&d_q, n * 4));
	HIP(hipMalloc((void **)&d_i1, n * 4));
	HIP(hipMalloc((void **)&d_q1, n * 4));
	HIP(hipMalloc((void **)&d_mag, n * 4));
	HIP(hipMalloc((void **)&d_freq, n * 4));
	HIP(hipMalloc((void **)&d_acc, C * 4));
	HIP(hipMalloc((void **)&d_acc1, C * 4));
	HIP(hipMalloc((void **)&d_last, C * 4));
	HIP(hipMalloc(&d_wtx, cordic_fm_workspace(L)));
	/* transmitter and receiver start at phase 0 */
	HIP(hipMemset(d_acc, 0, C * 4));
	HIP(hipMemset(d_acc1, 0, C * 4));
	HIP(hipMemset(d_last, 0, C * 4));

	/* channel c's block of a round sits at [c * L, (c + 1) * L): for an odd L
	 * the blocks are off the 16-byte grid, which both banks serve all the same */
	for (size_t c = 0; c < C; c++) {
		memset(&tx[c], 0, sizeof tx[c]);
		tx[c].d_fcw = d_fcw + c * L;
		tx[c].d_sin = d_q + c * L;	/* d_q = sine, d_i = cosine */
		tx[c].d_cos = d_i + c * L;
		tx[c].d_acc = d_acc + c;
		tx[c].n = L;
		memset(&rx[c], 0, sizeof rx[c]);
		rx[c].d_xval = d_i + c * L;
		rx[c].d_yval = d_q + c * L;
		rx[c].d_omag = d_mag + c * L;
		rx[c].d_ofreq = d_freq + c * L;
		rx[c].d_last = d_last + c;
		rx[c].n = L;
	}
	cordic_fmbank *txbank;
	cordic_demodbank *rxbank;
	CHECK(cordic_table_fmbank_create(osc, C, tx, &txbank));
	CHECK(cordic_demodbank_create(&conv, C, rx, &rxbank));
	uint64_t tx_samples, rx_samples;
	uint32_t spans, tiles, tail_jobs;
	int32_t span, fused, tile;
	CHECK(cordic_fmbank_info(txbank, &tx_samples, &spans, &span));
	CHECK(cordic_demodbank_info(rxbank, &rx_samples, &tiles, &tail_jobs, &fused, &tile));

	long long worst = 0;
	size_t at_c = 0, at_i = 0, differ = 0;
	for (size_t r = 0; r < (size_t)rounds; r++) {
		for (size_t c = 0; c < C; c++) {
			before[c] = r ? fcw[c * L + L - 1] : 0;
			for (size_t i = 0; i < L; i++)
				fcw[c * L + i] = (uint32_t)message(c, r * L + i);
		}
		HIP(hipMemcpy(d_fcw, fcw, n * 4, hipMemcpyHostToDevice));
		/* transmit: every channel's block in one run of two launches ... */
		CHECK(cordic_fmbank_run(txbank, NULL));
		/* ... receive: every channel's block in one run */
		CHECK(cordic_demodbank_run(rxbank, NULL));
		HIP(hipDeviceSynchronize());
		HIP(hipMemcpy(freq, d_freq, n * 4, hipMemcpyDeviceToHost));
		if (r == 0) {
			/* the per-channel calls on arrays of their own: the same bits */
			for (size_t c = 0; c < C; c++)
				CHECK(cordic_table_fm(osc, L, d_fcw + c * L, NULL, 0, d_acc1 + c,
					d_q1 + c * L, d_i1 + c * L, d_wtx, NULL));
			HIP(hipDeviceSynchronize());
			HIP(hipMemcpy(a, d_q, n * 4, hipMemcpyDeviceToHost));
			HIP(hipMemcpy(b, d_q1, n * 4, hipMemcpyDeviceToHost));
			for (size_t i = 0; i < n; i++)
				differ += a[i] != b[i];
			HIP(hipMemcpy(a, d_i, n * 4, hipMemcpyDeviceToHost));
			HIP(hipMemcpy(b, d_i1, n * 4, hipMemcpyDeviceToHost));
			for (size_t i = 0; i < n; i++)
				differ += a[i] != b[i];
			HIP(hipMemcpy(acc, d_acc, C * 4, hipMemcpyDeviceToHost));
			HIP(hipMemcpy(acc + C, d_acc1, C * 4, hipMemcpyDeviceToHost));
			for (size_t c = 0; c < C; c++)
				differ += acc[c] != acc[C + c];
		}
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
		"IW %d PW %d\n", C, L, rounds, PW_TX, OW_TX, (int)conv.iw, (int)conv.pw);
	printf("transmit bank: %llu samples, %u spans of %d (two launches per round); "
		"receive bank: %llu samples, %u tiles of %d, %u tail jobs (%s)\n",
		(unsigned long long)tx_samples, spans, (int)span,
		(unsigned long long)rx_samples, tiles, (int)tile, tail_jobs,
		fused ? "fused, two launches per round" : "one by one");
	printf("bank against %zu cordic_table_fm calls in round 0: %zu words differ\n",
		C, differ);
	printf("worst |recovered step - tuning word| = %lld of 2^%d per turn "
		"(%.4f tuning-word LSBs), channel %zu sample %zu\n", worst, (int)conv.pw,
		(double)worst / (double)(1LL << up), at_c, at_i);
	cordic_fmbank_destroy(txbank);
	cordic_demodbank_destroy(rxbank);
	cordic_table_destroy(osc);
	hipFree(d_fcw); hipFree(d_i); hipFree(d_q); hipFree(d_i1); hipFree(d_q1);
	hipFree(d_mag); hipFree(d_freq); hipFree(d_acc); hipFree(d_acc1); hipFree(d_last);
	hipFree(d_wtx);
	free(fcw); free(freq); free(a); free(b); free(before); free(acc); free(tx); free(rx);
	/* the bank's bits are the single calls', and the loop-back is clean:
	 * rounding recovers every tuning word */
	return differ == 0 && 2 * worst < (1LL << up) ? 0 : 1;
}
