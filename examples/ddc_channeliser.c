/* ddc_channeliser.c -- plain C caller of a DECIMATING 16-bit FM mixer bank in
 * front of a 16-bit FM demodulation bank (cordic_mixbank_create_decim16,
 * cordic_demodbank_create16; include/cordic_amd.h, "Decimating FM mixer banks",
 * "FM demodulation banks"): a digital down-converter per channel.  CHANNELS
 * short int16 blocks per round.  ONE cordic_mixbank over all channels tunes
 * each channel's I/Q block by the running sum of that channel's tuning words
 * -- the accumulator carried from round to round in a d_acc word per channel
 * (phase0 = 0) -- sums R = 8 consecutive tuned samples (k = 3) and keeps one;
 * ONE cordic_demodbank turns the decimated blocks, BLOCK_SAMPLES / 8 long, into
 * magnitude and phase step, the last phase carried in a d_last word per
 * channel.  Four launches per round for all channels; the full-rate tuned I/Q
 * is never stored and the discriminators run at an eighth of the input rate.
 *
 * The reference runs channel by channel: one cordic_plan_fm_mix16 call at the
 * full rate, the sums of 8 and the floor on the HOST, and one
 * cordic_fm_demod16 call on what the host made, with words of their own.
 * Every output sample of every round, and every d_acc and d_last word after
 * the last round, must be the same.  Exit status 0 on equality.
 *
 *   gcc -std=c99 -I include -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       examples/ddc_channeliser.c -L cordic_amd -lcordic_amd -L /opt/rocm/lib \
 *       -lamdhip64 -Wl,-rpath,$PWD/cordic_amd -o tools/ddc_channeliser
 *   tools/ddc_channeliser [-c CHANNELS] [-l BLOCK_SAMPLES] [-r ROUNDS]
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

/* the LO's tuning word of channel c at sample i of its stream: the channel's
 * offset, a slow sweep and a dither, 2 pi / 2^32 per unit, both signs */
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
	int16_t *iq = malloc(2 * n * sizeof *iq), *full = malloc(2 * n * sizeof *full);
	int16_t *got = malloc(4 * m * sizeof *got), *want = malloc(4 * m * sizeof *want);
	uint32_t *wa = malloc(4 * C * sizeof *wa);
	cordic_fmmix_job16 *mjobs = malloc(C * sizeof *mjobs);
	cordic_demod_job16 *djobs = malloc(C * sizeof *djobs);
	if (!fcw || !iq || !full || !got || !want || !wa || !mjobs || !djobs) return 1;
	/* d_in: [i | q] at the input rate; d_full: the reference's tuned [i | q] at
	 * the input rate; d_out / d_ref: [tuned i | tuned q | mag | freq] at the
	 * decimated rate, of the banks and of the reference; d_words: [acc | last]
	 * of the banks, then of the reference */
	uint32_t *d_fcw, *d_words;
	int16_t *d_in, *d_full, *d_out, *d_ref;
	void *d_wmix, *d_wdem;
	HIP(hipMalloc((void **)&d_fcw, n * 4));
	HIP(hipMalloc((void **)&d_in, 2 * n * 2));
	HIP(hipMalloc((void **)&d_full, 2 * n * 2));
	HIP(hipMalloc((void **)&d_out, 4 * m * 2));
	HIP(hipMalloc((void **)&d_ref, 4 * m * 2));
	HIP(hipMalloc((void **)&d_words, 4 * C * 4));
	HIP(hipMalloc(&d_wmix, cordic_plan_fm_mix16_workspace(plan, L)));
	HIP(hipMalloc(&d_wdem, cordic_fm_demod_workspace(M)));
	HIP(hipMemset(d_words, 0, 4 * C * 4));
	uint32_t *d_acc = d_words, *d_last = d_words + C, *d_racc = d_words + 2 * C,
		*d_rlast = d_words + 3 * C;

	for (size_t c = 0; c < C; c++) {
		memset(&mjobs[c], 0, sizeof mjobs[c]);
		mjobs[c].d_fcw = d_fcw + c * L;
		mjobs[c].d_xval = d_in + c * L;
		mjobs[c].d_yval = d_in + n + c * L;
		mjobs[c].d_oxval = d_out + c * M;	/* n >> k elements per job */
		mjobs[c].d_oyval = d_out + m + c * M;
		mjobs[c].d_acc = d_acc + c;
		mjobs[c].n = L;
		memset(&djobs[c], 0, sizeof djobs[c]);
		djobs[c].d_xval = d_out + c * M;
		djobs[c].d_yval = d_out + m + c * M;
		djobs[c].d_omag = d_out + 2 * m + c * M;
		djobs[c].d_ofreq = d_out + 3 * m + c * M;
		djobs[c].d_last = d_last + c;
		djobs[c].n = M;
	}
	cordic_mixbank *mix;
	cordic_demodbank *dem;
	CHECK(cordic_mixbank_create_decim16(plan, LOG2R, C, mjobs, &mix));
	CHECK(cordic_demodbank_create16(&conv, C, djobs, &dem));
	uint64_t samples;
	uint32_t spans;
	int32_t fused, tile;
	CHECK(cordic_mixbank_info(mix, &samples, &spans, &fused, &tile));
	int32_t dfused;
	CHECK(cordic_demodbank_info(dem, NULL, NULL, NULL, &dfused, NULL));

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
		/* every channel's block through its decimating LO and its discriminator */
		CHECK(cordic_mixbank_run(mix, NULL));
		CHECK(cordic_demodbank_run(dem, NULL));
		/* the reference: the mixer at the full rate, channel by channel ... */
		for (size_t c = 0; c < C; c++)
			CHECK(cordic_plan_fm_mix16(plan, L, d_fcw + c * L, NULL, 0, d_racc + c,
				d_in + c * L, d_in + n + c * L, d_full + c * L, d_full + n + c * L,
				d_wmix, NULL));
		HIP(hipDeviceSynchronize());
		HIP(hipMemcpy(full, d_full, 2 * n * 2, hipMemcpyDeviceToHost));
		/* ... the sums of R and the floor on the host (L is a multiple of R, so
		 * the groups of [i | q] as one array are the channels' own) ... */
		for (size_t j = 0; j < 2 * m; j++) {
			int32_t s = 0;
			for (size_t i = 0; i < R; i++)
				s += full[j * R + i];
			/* floor: toward minus infinity */
			want[j] = (int16_t)((s - (s < 0 ? R - 1 : 0)) / R);
		}
		HIP(hipMemcpy(d_ref, want, 2 * m * 2, hipMemcpyHostToDevice));
		/* ... and the discriminator on them */
		for (size_t c = 0; c < C; c++)
			CHECK(cordic_fm_demod16(&conv, M, d_ref + c * M, d_ref + m + c * M, 0,
				d_rlast + c, d_ref + 2 * m + c * M, d_ref + 3 * m + c * M, d_wdem,
				NULL));
		HIP(hipDeviceSynchronize());
		HIP(hipMemcpy(got, d_out, 4 * m * 2, hipMemcpyDeviceToHost));
		HIP(hipMemcpy(want, d_ref, 4 * m * 2, hipMemcpyDeviceToHost));
		for (size_t k = 0; k < 4 * m; k++)
			bad += got[k] != want[k];
	}
	HIP(hipMemcpy(wa, d_words, 4 * C * 4, hipMemcpyDeviceToHost));
	for (size_t k = 0; k < 2 * C; k++)
		bad += wa[k] != wa[2 * C + k];
	printf("%zu channels x %zu samples x %ld rounds, decimated by %d to %zu, on int16; "
		"mixer bank: %llu samples, %u spans of at most %d (%s); demodulation bank: "
		"%s\n", C, L, rounds, R, M, (unsigned long long)samples, spans, (int)tile,
		fused ? "fused, two launches per round" : "one by one",
		dfused ? "fused, two launches per round" : "one by one");
	printf("%zu shorts or words differ from the chain run channel by channel\n", bad);
	cordic_mixbank_destroy(mix);
	cordic_demodbank_destroy(dem);
	cordic_plan_destroy(plan);
	hipFree(d_fcw); hipFree(d_in); hipFree(d_full); hipFree(d_out); hipFree(d_ref);
	hipFree(d_words); hipFree(d_wmix); hipFree(d_wdem);
	free(fcw); free(iq); free(full); free(got); free(want); free(wa); free(mjobs);
	free(djobs);
	return bad ? 1 : 0;
}
