/* ddc_c16.c -- plain C caller of a decimating FM mixer bank on INTERLEAVED
 * int16 I/Q, in and out (include/cordic_amd.h, "FM mixer on INTERLEAVED int16
 * I/Q"): a digital down-converter that hands the decimated baseband on in the
 * form the capture arrived in.  The capture buffer -- complex int16, I0 Q0 I1
 * Q1 .., CHANNELS blocks of BLOCK complex samples one behind the other -- goes
 * through ONE cordic_mixbank_create_decim_c16 bank at R = 2^k: every channel is
 * tuned by the running sum of its own tuning words and summed by R, in two
 * launches a round, into one interleaved output buffer; the oscillator is
 * carried from round to round in a d_acc word per channel.  Nobody splits the
 * capture or interleaves the result on the device.
 *
 * The same rounds then run through cordic_plan_fm_mix_decim16, one call per
 * channel, on two arrays that this program splits ON THE HOST, with words of
 * their own; every output short of every round and every word after the last
 * round must be the same.  Exit status 0 on equality.
 *
 *   gcc -std=c99 -I include -I /opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       examples/ddc_c16.c -L cordic_amd -lcordic_amd -L /opt/rocm/lib \
 *       -lamdhip64 -Wl,-rpath,$PWD/cordic_amd -o tools/ddc_c16
 *   tools/ddc_c16 [-c CHANNELS] [-l BLOCK_SAMPLES] [-k LOG2R] [-r ROUNDS]
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

static uint32_t lcg(uint32_t *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s;
}

/* the LO's tuning word of channel c at sample i of its stream */
static uint32_t tuning(size_t c, size_t i)
{
	return (uint32_t)((int32_t)(c % 97) * 1234567 - 40000000
		+ (int32_t)((i >> 6) % 129) * 4001 + ((i / 29) & 1 ? 77777 : -55555));
}

int main(int argc, char **argv)
{
	long channels = 256, block = 1536, log2r = 3, rounds = 3;
	for (int k = 1; k < argc; k += 2) {
		if (k + 1 < argc && !strcmp(argv[k], "-c")) channels = atol(argv[k + 1]);
		else if (k + 1 < argc && !strcmp(argv[k], "-l")) block = atol(argv[k + 1]);
		else if (k + 1 < argc && !strcmp(argv[k], "-k")) log2r = atol(argv[k + 1]);
		else if (k + 1 < argc && !strcmp(argv[k], "-r")) rounds = atol(argv[k + 1]);
		else channels = -1;
	}
	if (channels < 1 || channels > 4096 || block < 1 || block > (1 << 20) || log2r < 0
			|| log2r > 8 || block % (1L << log2r) || rounds < 1 || rounds > 64) {
		fprintf(stderr, "usage: %s [-c CHANNELS (1 .. 4096)] [-l BLOCK_SAMPLES (1 .. 2^20, "
			"a multiple of 2^LOG2R)] [-k LOG2R (0 .. 8)] [-r ROUNDS (1 .. 64)]\n", argv[0]);
		return 2;
	}
	const size_t C = (size_t)channels, L = (size_t)block, n = C * L;
	const uint32_t K = (uint32_t)log2r;
	const size_t M = L >> K, m = C * M;		/* decimated samples */

	/* 16-bit ports: the container of the *16 and *_c16 forms */
	cordic_config rot;
	CHECK(cordic_config_init(&rot, CORDIC_P2R, 16, 16, 2, 16, 16));
	cordic_plan *plan;
	CHECK(cordic_plan_create(&rot, &plan));

	uint32_t *fcw = malloc(n * sizeof *fcw);
	int16_t *iq = malloc(2 * n * sizeof *iq), *xy = malloc(2 * n * sizeof *xy);
	int16_t *got = malloc(2 * m * sizeof *got), *want = malloc(2 * m * sizeof *want);
	uint32_t *wa = malloc(2 * C * sizeof *wa);
	cordic_fmmix_job_c16 *jobs = malloc(C * sizeof *jobs);
	if (!fcw || !iq || !xy || !got || !want || !wa || !jobs) return 1;
	/* d_iq: the capture buffer; d_oiq: the bank's decimated baseband, interleaved;
	 * d_xy: [x | y], split on the host; d_ref: [ox | oy] of the single calls;
	 * d_words: the d_acc words of the bank, then of the single calls */
	uint32_t *d_fcw, *d_words;
	int16_t *d_iq, *d_oiq, *d_xy, *d_ref;
	void *d_work;
	const size_t wbytes = cordic_plan_fm_mix_decim16_workspace(plan, L, K);
	HIP(hipMalloc((void **)&d_fcw, n * 4));
	HIP(hipMalloc((void **)&d_iq, 2 * n * 2));
	HIP(hipMalloc((void **)&d_oiq, 2 * m * 2));
	HIP(hipMalloc((void **)&d_xy, 2 * n * 2));
	HIP(hipMalloc((void **)&d_ref, 2 * m * 2));
	HIP(hipMalloc((void **)&d_words, 2 * C * 4));
	HIP(hipMalloc(&d_work, wbytes ? wbytes : 16));
	/* every oscillator starts at phase 0 */
	HIP(hipMemset(d_words, 0, 2 * C * 4));
	uint32_t *d_acc = d_words, *d_racc = d_words + C;

	/* channel c's block of a round is complex samples [c * L, (c + 1) * L) of the
	 * capture buffer, and [c * M, (c + 1) * M) of the baseband */
	for (size_t c = 0; c < C; c++) {
		memset(&jobs[c], 0, sizeof jobs[c]);
		jobs[c].d_fcw = d_fcw + c * L;
		jobs[c].d_iq = d_iq + 2 * c * L;
		jobs[c].d_oiq = d_oiq + 2 * c * M;
		jobs[c].d_acc = d_acc + c;
		jobs[c].n = L;
	}
	cordic_mixbank *ddc;
	CHECK(cordic_mixbank_create_decim_c16(plan, K, C, jobs, &ddc));
	uint64_t samples;
	uint32_t spans;
	int32_t fused, tile;
	CHECK(cordic_mixbank_info(ddc, &samples, &spans, &fused, &tile));

	uint32_t seed = 12345;
	size_t bad = 0;
	for (size_t r = 0; r < (size_t)rounds; r++) {
		for (size_t c = 0; c < C; c++)
			for (size_t i = 0; i < L; i++)
				fcw[c * L + i] = tuning(c, r * L + i);
		for (size_t k = 0; k < 2 * n; k++)	/* full-scale 16-bit samples */
			iq[k] = (int16_t)((int32_t)(lcg(&seed) >> 16) - 32768);
		for (size_t i = 0; i < n; i++) {	/* the split, for the reference only */
			xy[i] = iq[2 * i];
			xy[n + i] = iq[2 * i + 1];
		}
		HIP(hipMemcpy(d_fcw, fcw, n * 4, hipMemcpyHostToDevice));
		HIP(hipMemcpy(d_iq, iq, 2 * n * 2, hipMemcpyHostToDevice));
		HIP(hipMemcpy(d_xy, xy, 2 * n * 2, hipMemcpyHostToDevice));
		/* the capture buffer as it came, all channels in two launches */
		CHECK(cordic_mixbank_run(ddc, NULL));
		/* the same, channel by channel, from the split arrays */
		for (size_t c = 0; c < C; c++)
			CHECK(cordic_plan_fm_mix_decim16(plan, L, K, d_fcw + c * L, NULL, 0, d_racc + c,
				d_xy + c * L, d_xy + n + c * L, d_ref + c * M, d_ref + m + c * M, d_work,
				NULL));
		HIP(hipDeviceSynchronize());
		HIP(hipMemcpy(got, d_oiq, 2 * m * 2, hipMemcpyDeviceToHost));
		HIP(hipMemcpy(want, d_ref, 2 * m * 2, hipMemcpyDeviceToHost));
		for (size_t j = 0; j < m; j++)
			bad += (got[2 * j] != want[j]) + (got[2 * j + 1] != want[m + j]);
	}
	HIP(hipMemcpy(wa, d_words, 2 * C * 4, hipMemcpyDeviceToHost));
	for (size_t c = 0; c < C; c++)
		bad += wa[c] != wa[C + c];
	printf("%zu channels x %zu complex int16 samples x %ld rounds, R = %u, p2r IW %d PW %d; "
		"interleaved mixer bank: %llu samples, %u spans, passes of %d (%s)\n", C, L,
		rounds, 1u << K, (int)rot.iw, (int)rot.pw, (unsigned long long)samples, spans,
		(int)tile, fused ? "fused, two launches per round" : "one by one");
	printf("%zu shorts and words differ from cordic_plan_fm_mix_decim16 per channel on split "
		"arrays\n", bad);
	cordic_mixbank_destroy(ddc);
	cordic_plan_destroy(plan);
	hipFree(d_fcw); hipFree(d_iq); hipFree(d_oiq); hipFree(d_xy); hipFree(d_ref);
	hipFree(d_words); hipFree(d_work);
	free(fcw); free(iq); free(xy); free(got); free(want); free(wa); free(jobs);
	return bad ? 1 : 0;
}
