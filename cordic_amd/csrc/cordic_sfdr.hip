// cordic_sfdr.hip -- the second half of the reference benches' report: the
// spurious free dynamic range of a full sweep, by a double-precision FFT on
// the device.
//
// bench/cpp/cordic_tb.cpp:340-371 and bench/cpp/quadtbl_tb.cpp:185-219 copy
// one turn of the phase ramp's outputs into a complex array, transform it with
// FFTW (bench/cpp/fftw.c) and compare bin 1 -- the tone -- with the largest
// other bin; both give up at PW >= 26 because the host runs out of room.  Here
// the 2^lgn complex doubles stay on the device: two buffers of 16 B * 2^lgn,
// an out-of-place Stockham autosort transform between them (no bit reversal
// pass), one launch per radix-4 stage and one radix-2 stage when lgn is odd,
// then one reduction kernel for the spur.
//
// Twiddles are fp64 sincospi of a dyadic fraction p / n (exact argument,
// exact reduction): no recurrence, so nothing drifts over 2^28 butterflies.
//
// Nothing here is on the product's data path: these kernels read what the
// engine wrote.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "cordic_amd.h"
#include "cordic_internal.h"

namespace cordic_amd {
namespace {

constexpr int kFBlock = 256;

struct SpurSlot {
	double spur;			// max |X[k]|^2 over this block's k != 1
	unsigned long long bin;		// lowest k that attains it
};

__device__ __forceinline__ double2 cmul(double2 a, double2 w)
{
	return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// e^{-2 pi i k p / n} for dyadic p / n: the argument of sincospi is exact
__device__ __forceinline__ double2 twiddle(double frac)
{
	double sn, cs;
	sincospi(-2.0 * frac, &sn, &cs);
	return make_double2(cs, sn);
}

// cordic_tb.cpp:349-352: sample index0 + i is x + j y
__global__ __launch_bounds__(kFBlock) void sfdr_load_iq(double2 *__restrict__ buf,
		size_t n, unsigned long long index0, const int32_t *__restrict__ re,
		const int32_t *__restrict__ im)
{
	const size_t stride = (size_t)gridDim.x * kFBlock;
	for (size_t i = (size_t)blockIdx.x * kFBlock + threadIdx.x; i < n; i += stride)
		buf[index0 + i] = make_double2((double)re[i], (double)im[i]);
}

// quadtbl_tb.cpp:194-197: outpt[k] = (s[(k + N/4) & (N-1)], s[k]), i.e. sample
// k is the imaginary part of point k and the real part of point k - N/4
__global__ __launch_bounds__(kFBlock) void sfdr_load_sine(double *__restrict__ buf,
		size_t n, unsigned long long index0, const int32_t *__restrict__ s,
		unsigned long long nfft)
{
	const size_t stride = (size_t)gridDim.x * kFBlock;
	for (size_t i = (size_t)blockIdx.x * kFBlock + threadIdx.x; i < n; i += stride) {
		const unsigned long long k = index0 + i;
		const double v = (double)s[i];
		buf[2 * k + 1] = v;
		buf[2 * ((k - (nfft >> 2)) & (nfft - 1))] = v;
	}
}

// One radix-4 Stockham stage: the transform of length n (stride s, n * s = N)
// becomes four of length n / 4 (stride 4 s).  Butterfly t = q + s p reads
// x[t + k N/4], k = 0..3 (always coalesced) and writes y[q + s (4 p + k)].
__global__ __launch_bounds__(kFBlock) void sfdr_radix4(const double2 *__restrict__ x,
		double2 *__restrict__ y, unsigned long long quarter, int lgs, int lgn)
{
	const unsigned long long smask = (1ull << lgs) - 1;
	const size_t stride = (size_t)gridDim.x * kFBlock;
	const double inv_n = 1.0 / (double)(1ull << lgn);	// a power of two: exact
	for (unsigned long long t = (size_t)blockIdx.x * kFBlock + threadIdx.x;
			t < quarter; t += stride) {
		const unsigned long long q = t & smask, p = t >> lgs;
		const double2 a = x[t], b = x[t + quarter], c = x[t + 2 * quarter],
			d = x[t + 3 * quarter];
		const double2 apc = make_double2(a.x + c.x, a.y + c.y);
		const double2 amc = make_double2(a.x - c.x, a.y - c.y);
		const double2 bpd = make_double2(b.x + d.x, b.y + d.y);
		// j (b - d)
		const double2 jbmd = make_double2(-(b.y - d.y), b.x - d.x);
		const double f = (double)p * inv_n;
		const double2 w1 = twiddle(f), w2 = twiddle(2.0 * f), w3 = twiddle(3.0 * f);
		double2 *o = y + (q + ((4 * p) << lgs));
		o[0] = make_double2(apc.x + bpd.x, apc.y + bpd.y);
		o[1ull << lgs] = cmul(make_double2(amc.x - jbmd.x, amc.y - jbmd.y), w1);
		o[2ull << lgs] = cmul(make_double2(apc.x - bpd.x, apc.y - bpd.y), w2);
		o[3ull << lgs] = cmul(make_double2(amc.x + jbmd.x, amc.y + jbmd.y), w3);
	}
}

// The last stage when lgn is odd: N/2 transforms of length 2, no twiddles.
__global__ __launch_bounds__(kFBlock) void sfdr_radix2(const double2 *__restrict__ x,
		double2 *__restrict__ y, unsigned long long half)
{
	const size_t stride = (size_t)gridDim.x * kFBlock;
	for (unsigned long long t = (size_t)blockIdx.x * kFBlock + threadIdx.x;
			t < half; t += stride) {
		const double2 a = x[t], b = x[t + half];
		y[t] = make_double2(a.x + b.x, a.y + b.y);
		y[t + half] = make_double2(a.x - b.x, a.y - b.y);
	}
}

// cordic_tb.cpp:357-366: master = |X[1]|^2, spur = the largest other bin.  One
// slot per block (overwritten, not accumulated); the host takes their maximum.
__global__ __launch_bounds__(kFBlock) void sfdr_spur(const double2 *__restrict__ x,
		unsigned long long nfft, SpurSlot *slots, double *master)
{
	__shared__ double red[kFBlock / 64];
	__shared__ unsigned long long reda[kFBlock / 64];
	double m = -1.0;
	unsigned long long am = ~0ull;
	const size_t stride = (size_t)gridDim.x * kFBlock;
	for (unsigned long long k = (size_t)blockIdx.x * kFBlock + threadIdx.x;
			k < nfft; k += stride) {
		const double2 v = x[k];
		const double e = v.x * v.x + v.y * v.y;
		if (k == 1)
			*master = e;
		else if (e > m) { m = e; am = k; }	// k ascends: lowest on ties
	}
	for (int off = 32; off; off >>= 1) {
		const double o = __shfl_down(m, off, 64);
		const unsigned long long b = __shfl_down(am, off, 64);
		if (o > m || (o == m && b < am)) { m = o; am = b; }
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0) { red[wave] = m; reda[wave] = am; }
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < kFBlock / 64; w++)
			if (red[w] > m || (red[w] == m && reda[w] < am)) { m = red[w]; am = reda[w]; }
		slots[blockIdx.x].spur = m;
		slots[blockIdx.x].bin = am;
	}
}

} // namespace
} // namespace cordic_amd

using namespace cordic_amd;

struct cordic_sfdr {
	int lgn = 0;
	unsigned long long n = 0;	// 2^lgn
	double2 *buf[2] = {nullptr, nullptr};
	SpurSlot *d_slots = nullptr;	// grid slots, then one double: |X[1]|^2
	int grid = 0;
	int device = 0;
	unsigned long long loaded = 0;	// samples loaded since the last transform
	int result = -1;		// buffer that holds the last transform, -1: none
};

static int grid_of(const cordic_sfdr *s, unsigned long long work)
{
	const unsigned long long want = (work + kFBlock - 1) / kFBlock;
	return (int)(want < (unsigned long long)s->grid ? want : (unsigned long long)s->grid);
}

int cordic_sfdr_create(int lgn, cordic_sfdr **out)
{
	if (!out || lgn < 1 || lgn > 30)
		return CORDIC_ERR_ARGS;
	cordic_sfdr *s = new (std::nothrow) cordic_sfdr;
	if (!s)
		return CORDIC_ERR_NOMEM;
	s->lgn = lgn;
	s->n = 1ull << lgn;
	hipDeviceProp_t prop;
	if (hipGetDevice(&s->device) != hipSuccess ||
	    hipGetDeviceProperties(&prop, s->device) != hipSuccess) {
		delete s;
		return CORDIC_ERR_DEVICE;
	}
	s->grid = prop.multiProcessorCount * 8;
	const size_t bytes = (size_t)s->n * sizeof(double2);
	if (hipMalloc((void **)&s->buf[0], bytes) != hipSuccess ||
	    hipMalloc((void **)&s->buf[1], bytes) != hipSuccess ||
	    hipMalloc((void **)&s->d_slots, (size_t)s->grid * sizeof(SpurSlot)
			+ sizeof(double)) != hipSuccess) {
		(void)hipGetLastError();
		cordic_sfdr_destroy(s);
		return CORDIC_ERR_NOMEM;
	}
	*out = s;
	return CORDIC_OK;
}

void cordic_sfdr_destroy(cordic_sfdr *s)
{
	if (!s)
		return;
	for (int k = 0; k < 2; k++)
		if (s->buf[k])
			(void)hipFree(s->buf[k]);
	if (s->d_slots)
		(void)hipFree(s->d_slots);
	delete s;
}

// range and handle checks of the two loads; 1 = nothing to do
static int load_check(cordic_sfdr *s, size_t n, uint64_t index0, const void *a,
		const void *b)
{
	if (!s)
		return CORDIC_ERR_ARGS;
	if (index0 > s->n || n > s->n - index0)
		return CORDIC_ERR_ARGS;
	if (n == 0)
		return 1;
	if (!a || !b)
		return CORDIC_ERR_ARGS;
	int dev;
	if (hipGetDevice(&dev) != hipSuccess)
		return CORDIC_ERR_DEVICE;
	if (dev != s->device)
		return CORDIC_ERR_ARGS;
	return CORDIC_OK;
}

int cordic_sfdr_load_iq(cordic_sfdr *s, size_t n, uint64_t index0,
		const int32_t *d_re, const int32_t *d_im, void *stream)
{
	if (int rc = load_check(s, n, index0, d_re, d_im))
		return rc < 0 ? rc : CORDIC_OK;
	(void)hipGetLastError();
	hipLaunchKernelGGL(sfdr_load_iq, dim3(grid_of(s, n)), dim3(kFBlock), 0,
		static_cast<hipStream_t>(stream), s->buf[0], n,
		(unsigned long long)index0, d_re, d_im);
	if (hipGetLastError() != hipSuccess)
		return CORDIC_ERR_DEVICE;
	s->loaded += n;
	s->result = -1;
	return CORDIC_OK;
}

int cordic_sfdr_load_sine(cordic_sfdr *s, size_t n, uint64_t index0,
		const int32_t *d_sin, void *stream)
{
	if (int rc = load_check(s, n, index0, d_sin, d_sin))
		return rc < 0 ? rc : CORDIC_OK;
	(void)hipGetLastError();
	hipLaunchKernelGGL(sfdr_load_sine, dim3(grid_of(s, n)), dim3(kFBlock), 0,
		static_cast<hipStream_t>(stream), reinterpret_cast<double *>(s->buf[0]),
		n, (unsigned long long)index0, d_sin, s->n);
	if (hipGetLastError() != hipSuccess)
		return CORDIC_ERR_DEVICE;
	s->loaded += n;
	s->result = -1;
	return CORDIC_OK;
}

int cordic_sfdr_run(cordic_sfdr *s, cordic_sfdr_result *out, void *stream)
{
	if (!s || !out)
		return CORDIC_ERR_ARGS;
	if (s->loaded != s->n)
		return CORDIC_ERR_ARGS;
	int dev;
	if (hipGetDevice(&dev) != hipSuccess)
		return CORDIC_ERR_DEVICE;
	if (dev != s->device)
		return CORDIC_ERR_ARGS;
	hipStream_t st = static_cast<hipStream_t>(stream);
	(void)hipGetLastError();
	int cur = 0, lgs = 0;
	for (int lg = s->lgn; lg >= 2; lg -= 2, lgs += 2, cur ^= 1)
		hipLaunchKernelGGL(sfdr_radix4, dim3(grid_of(s, s->n >> 2)), dim3(kFBlock),
			0, st, s->buf[cur], s->buf[cur ^ 1], s->n >> 2, lgs, lg);
	if (s->lgn & 1) {
		hipLaunchKernelGGL(sfdr_radix2, dim3(grid_of(s, s->n >> 1)), dim3(kFBlock),
			0, st, s->buf[cur], s->buf[cur ^ 1], s->n >> 1);
		cur ^= 1;
	}
	const int grid = grid_of(s, s->n);
	double *d_master = reinterpret_cast<double *>(s->d_slots + s->grid);
	hipLaunchKernelGGL(sfdr_spur, dim3(grid), dim3(kFBlock), 0, st, s->buf[cur],
		s->n, s->d_slots, d_master);
	if (hipGetLastError() != hipSuccess)
		return CORDIC_ERR_DEVICE;
	// the input buffer has been written over: a new sweep is loaded afresh
	s->loaded = 0;
	s->result = cur;
	std::vector<SpurSlot> h((size_t)grid + 1);
	if (hipStreamSynchronize(st) != hipSuccess ||
	    hipMemcpy(h.data(), s->d_slots, (size_t)grid * sizeof(SpurSlot),
			hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(&h[grid], d_master, sizeof(double),
			hipMemcpyDeviceToHost) != hipSuccess) {
		s->result = -1;
		return CORDIC_ERR_DEVICE;
	}
	std::memset(out, 0, sizeof *out);
	out->n = s->n;
	std::memcpy(&out->master, &h[grid], sizeof(double));
	double spur = -1.0;
	unsigned long long bin = ~0ull;
	for (int k = 0; k < grid; k++)
		if (h[k].spur > spur || (h[k].spur == spur && h[k].bin < bin)) {
			spur = h[k].spur;
			bin = h[k].bin;
		}
	out->spur = spur;
	out->spur_bin = bin;
	// cordic_tb.cpp:368-369
	out->sfdr_dbc = 10 * std::log(out->master / out->spur) / std::log(10.);
	return CORDIC_OK;
}

int cordic_sfdr_bins(cordic_sfdr *s, uint64_t first, uint64_t count,
		double *host_re_im)
{
	if (!s || s->result < 0)
		return CORDIC_ERR_ARGS;
	if (first > s->n || count > s->n - first)
		return CORDIC_ERR_ARGS;
	if (count == 0)
		return CORDIC_OK;
	if (!host_re_im)
		return CORDIC_ERR_ARGS;
	if (hipMemcpy(host_re_im, s->buf[s->result] + first,
			(size_t)count * sizeof(double2), hipMemcpyDeviceToHost) != hipSuccess)
		return CORDIC_ERR_DEVICE;
	return CORDIC_OK;
}
