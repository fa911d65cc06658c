/* afc_receiver.c -- plain C caller of a receiver bank (include/cordic_amd.h,
 * "Receiver banks"): the whole receive chain of a channeliser whose every
 * channel has a local oscillator of its own -- an AFC or Costas loop, a Doppler
 * correction, a de-chirp -- in front of its FM discriminator.  CHANNELS short
 * blocks per round.  ONE cordic_rxbank over all channels rotates each
 * channel's I/Q block by the running sum of that channel's tuning words and
 * turns it into magnitude and phase step per sample, the oscillator carried
 * from round to round in a d_acc word per channel and the discriminator in a
 * d_last word per channel (phase0 = dphase0 = 0).  Two launches per round for
 * all channels, and the tuned I/Q is never stored.
 *
 * The same chain then runs as examples/afc_channeliser.c has it -- ONE mixer
 * bank into ONE demodulation bank, four launches and an intermediate I/Q array,
 * on arrays and words of their own -- and every output sample of every round,
 * and every d_acc and d_last word after the last round, must be the same.
 * Exit status 0 on equality.
 *
 *   gcc -std=c99 -I include -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       examples/afc_receiver.c -L cordic_amd -lcordic_amd -L /opt/rocm/lib \
 *       -lamdhip64 -Wl,-rpath,$PWD/cordic_amd -o tools/afc_receiver
 *   tools/afc_receiver [-c CHANNELS] [-l BLOCK_SAMPLES] [-r ROUNDS]
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

enum { IW = 24 };

static uint32_t lcg(uint32_t *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s;
}

/* the LO's tuning word of channel c at sample i of its stream: the channel's
 * offset, a slow sweep and a dither, 2 pi / 2^32 per unit, both signs */
static uint32_t tuning(size_t c, size_t i)
{
	return (uint32_t)((int32_t)(c % 97) * 1234567 - 40000000
		+ (int32_t)((i >> 6) % 129) * 4001 + ((i / 29) & 1 ? 77777 : -55555));
}

int main(int argc, char **argv)
{
	long channels = 256, block = 1500, rounds = 3;
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

	cordic_config rot, conv;
	CHECK(cordic_config_init(&rot, CORDIC_P2R, IW, IW, 2, -1, -1));
	/* a converter whose inputs are as wide as the rotator's outputs */
	CHECK(cordic_config_init(&conv, CORDIC_R2P, IW, IW, 2, -1, 20));
	cordic_plan *plan;
	CHECK(cordic_plan_create(&rot, &plan));

	uint32_t *fcw = malloc(n * sizeof *fcw);
	int32_t *iq = malloc(2 * n * sizeof *iq);
	int32_t *got = malloc(2 * n * sizeof *got), *want = malloc(2 * n * sizeof *want);
	uint32_t *wa = malloc(4 * C * sizeof *wa);
	cordic_fmmix_job *mjobs = malloc(C * sizeof *mjobs);
	cordic_demod_job *djobs = malloc(C * sizeof *djobs);
	cordic_fmrx_job *rjobs = malloc(C * sizeof *rjobs);
	if (!fcw || !iq || !got || !want || !wa || !mjobs || !djobs || !rjobs) return 1;
	/* d_in: [i | q]; d_out: [mag | freq] of the receiver bank; d_ref: [tuned i |
	 * tuned q | mag | freq] of the two banks; d_words: [acc | last] of the
	 * receiver bank, then of the two banks */
	uint32_t *d_fcw, *d_words;
	int32_t *d_in, *d_out, *d_ref;
	HIP(hipMalloc((void **)&d_fcw, n * 4));
	HIP(hipMalloc((void **)&d_in, 2 * n * 4));
	HIP(hipMalloc((void **)&d_out, 2 * n * 4));
	HIP(hipMalloc((void **)&d_ref, 4 * n * 4));
	HIP(hipMalloc((void **)&d_words, 4 * C * 4));
	/* every oscillator and every discriminator starts at phase 0 */
	HIP(hipMemset(d_words, 0, 4 * C * 4));
	uint32_t *d_acc = d_words, *d_last = d_words + C, *d_racc = d_words + 2 * C,
		*d_rlast = d_words + 3 * C;

	/* channel c's block of a round sits at [c * L, (c + 1) * L): for an odd L
	 * the blocks are off the 16-byte grid, which all three banks serve */
	for (size_t c = 0; c < C; c++) {
		memset(&rjobs[c], 0, sizeof rjobs[c]);
		rjobs[c].d_fcw = d_fcw + c * L;
		rjobs[c].d_xval = d_in + c * L;
		rjobs[c].d_yval = d_in + n + c * L;
		rjobs[c].d_omag = d_out + c * L;
		rjobs[c].d_ofreq = d_out + n + c * L;
		rjobs[c].d_acc = d_acc + c;
		rjobs[c].d_last = d_last + c;
		rjobs[c].n = L;
		memset(&mjobs[c], 0, sizeof mjobs[c]);
		mjobs[c].d_fcw = d_fcw + c * L;
		mjobs[c].d_xval = d_in + c * L;
		mjobs[c].d_yval = d_in + n + c * L;
		mjobs[c].d_oxval = d_ref + c * L;
		mjobs[c].d_oyval = d_ref + n + c * L;
		mjobs[c].d_acc = d_racc + c;
		mjobs[c].n = L;
		memset(&djobs[c], 0, sizeof djobs[c]);
		djobs[c].d_xval = d_ref + c * L;
		djobs[c].d_yval = d_ref + n + c * L;
		djobs[c].d_omag = d_ref + 2 * n + c * L;
		djobs[c].d_ofreq = d_ref + 3 * n + c * L;
		djobs[c].d_last = d_rlast + c;
		djobs[c].n = L;
	}
	cordic_rxbank *rx;
	cordic_mixbank *mix;
	cordic_demodbank *dem;
	CHECK(cordic_rxbank_create(plan, &conv, C, rjobs, &rx));
	CHECK(cordic_mixbank_create(plan, C, mjobs, &mix));
	CHECK(cordic_demodbank_create(&conv, C, djobs, &dem));
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
			iq[k] = (int32_t)(lcg(&seed) >> (32 - IW)) - (1 << (IW - 1));
		HIP(hipMemcpy(d_fcw, fcw, n * 4, hipMemcpyHostToDevice));
		HIP(hipMemcpy(d_in, iq, 2 * n * 4, hipMemcpyHostToDevice));
		/* every channel's block through its LO and its discriminator */
		CHECK(cordic_rxbank_run(rx, NULL));
		/* the same through the two banks */
		CHECK(cordic_mixbank_run(mix, NULL));
		CHECK(cordic_demodbank_run(dem, NULL));
		HIP(hipDeviceSynchronize());
		HIP(hipMemcpy(got, d_out, 2 * n * 4, hipMemcpyDeviceToHost));
		HIP(hipMemcpy(want, d_ref + 2 * n, 2 * n * 4, hipMemcpyDeviceToHost));
		for (size_t k = 0; k < 2 * n; k++)
			bad += got[k] != want[k];
	}
	HIP(hipMemcpy(wa, d_words, 4 * C * 4, hipMemcpyDeviceToHost));
	for (size_t k = 0; k < 2 * C; k++)
		bad += wa[k] != wa[2 * C + k];
	printf("%zu channels x %zu samples x %ld rounds, p2r IW %d PW %d -> r2p IW %d PW "
		"%d; receiver bank: %llu samples, %u spans, passes of %d (%s)\n", C, L, rounds,
		(int)rot.iw, (int)rot.pw, (int)conv.iw, (int)conv.pw,
		(unsigned long long)samples, spans, (int)tile,
		fused ? "fused, two launches per round" : "one by one");
	printf("%zu words differ from the mixer bank into the demodulation bank\n", bad);
	cordic_rxbank_destroy(rx);
	cordic_mixbank_destroy(mix);
	cordic_demodbank_destroy(dem);
	cordic_plan_destroy(plan);
	hipFree(d_fcw); hipFree(d_in); hipFree(d_out); hipFree(d_ref); hipFree(d_words);
	free(fcw); free(iq); free(got); free(want); free(wa); free(mjobs); free(djobs);
	free(rjobs);
	return bad ? 1 : 0;
}
