// cordic_quality_sine.hip -- the acceptance statistic of the sine-producing
// cores (-t qtbl / tbl / qtr), reduced on the device, and the public
// cordic_quality_* entry points over both kinds of handle.
//
// bench/cpp/quadtbl_tb.cpp:146-179 judges the quadratic core by ONE maximum,
// |sin(2 pi p / 2^PW) (2^(OW-1) - 1) - o|, and reports the extreme outputs; the
// plain tables have no bench at all.  quality_sine below reduces that over
// arrays the engine wrote, in per-block slots the block itself merges call
// after call (no atomics, fixed grid), as cordic_quality.hip does for the
// CORDIC cores.  There are no sums in it, so a sweep fed in pieces gives the
// bytes of the same sweep fed at once.
//
// A sine handle is a cordic_quality with a mode no CORDIC core has and slots
// of its own.  cordic_quality.hip -- one of the sources the committed sweep
// was measured on (tools/build_stamp.py) -- is compiled as part of THIS
// translation unit, unchanged, with its handle-taking entry points under
// other names; the public ones are defined at the end of this file and send
// each handle to the code that owns it.
//
// Nothing here is on the product's data path: these kernels read what the
// engine wrote.
#include "cordic_amd.h"

#define cordic_quality_destroy	quality_base_destroy
#define cordic_quality_reset	quality_base_reset
#define cordic_quality_p2r	quality_base_p2r
#define cordic_quality_nco	quality_base_nco
#define cordic_quality_r2p	quality_base_r2p
#define cordic_quality_p2r_result	quality_base_p2r_result
#define cordic_quality_r2p_result	quality_base_r2p_result
#include "cordic_quality.hip"
#undef cordic_quality_destroy
#undef cordic_quality_reset
#undef cordic_quality_p2r
#undef cordic_quality_nco
#undef cordic_quality_r2p
#undef cordic_quality_p2r_result
#undef cordic_quality_r2p_result

namespace cordic_amd {
namespace {

// quadtbl_tb.cpp:146-170: the sine cores' statistic has no sums, only a
// maximum (with the sample and phase it was seen at) and the extreme output
// values, so a block's slot -- and the result -- does not depend on how a
// sweep was cut into calls.
struct SSlot {
	double err;			// max |sin * scale - o|, -1: none yet
	unsigned long long arg;		// sample index of it (lowest on ties)
	uint32_t phase;			// its PW-bit phase
	int32_t maxv, minv;		// both start at 0 (:147)
	int32_t pad;
};

struct SParams {
	int ow;
	double scale;		// 2^(OW-1) - 1
	double two_inv_2pw;	// 2 * 2^-PW
	uint32_t pmask;		// 2^PW - 1
};

template <bool NCO, typename T>
__global__ __launch_bounds__(kQBlock) void quality_sine(SParams sp, size_t n,
		const uint32_t *__restrict__ phase, uint32_t phase0, uint32_t fcw,
		unsigned long long index0, const T *__restrict__ val,
		unsigned long long base, SSlot *slots)
{
	__shared__ SSlot red[kQBlock / 64];
	double mx = -1.0;
	unsigned long long amx = ~0ull;
	uint32_t pmx = 0;
	int32_t hi = 0, lo = 0;
	const size_t stride = (size_t)gridDim.x * kQBlock;
	for (size_t i = (size_t)blockIdx.x * kQBlock + threadIdx.x; i < n; i += stride) {
		uint32_t p;
		if (NCO)
			p = phase0 + (uint32_t)(index0 + i) * fcw;
		else
			p = phase[i];
		p &= sp.pmask;
		const int32_t o = q_sext((int32_t)val[i], sp.ow);
		// ph = pdata * 2 pi / 2^PW (:155-156): sinpi reduces exactly, which
		// also makes the bench's (int) of a PW = 32 phase immaterial.
		// Separate roundings (no fma): one sample, one value, on every path
		const double dsin = __dmul_rn(sinpi((double)p * sp.two_inv_2pw), sp.scale);
		const double err = fabs(__dsub_rn(dsin, (double)o));	// :163
		if (err > mx) { mx = err; amx = base + i; pmx = p; }
		hi = o > hi ? o : hi;					// :166-169
		lo = o < lo ? o : lo;
	}
	for (int off = 32; off; off >>= 1) {
		const double oe = __shfl_down(mx, off, 64);
		const unsigned long long oa = __shfl_down(amx, off, 64);
		const uint32_t op = __shfl_down(pmx, off, 64);
		if (oe > mx || (oe == mx && oa < amx)) { mx = oe; amx = oa; pmx = op; }
		const int32_t oh = __shfl_down(hi, off, 64), ol = __shfl_down(lo, off, 64);
		hi = oh > hi ? oh : hi;
		lo = ol < lo ? ol : lo;
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0) {
		red[wave].err = mx; red[wave].arg = amx; red[wave].phase = pmx;
		red[wave].maxv = hi; red[wave].minv = lo;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		SSlot s = slots[blockIdx.x];
		for (int w = 0; w < kQBlock / 64; w++) {
			if (red[w].err > s.err || (red[w].err == s.err && red[w].arg < s.arg)) {
				s.err = red[w].err; s.arg = red[w].arg; s.phase = red[w].phase;
			}
			s.maxv = red[w].maxv > s.maxv ? red[w].maxv : s.maxv;
			s.minv = red[w].minv < s.minv ? red[w].minv : s.minv;
		}
		slots[blockIdx.x] = s;
	}
}

} // namespace
} // namespace cordic_amd

constexpr int kSineMode = -1000;	// cfg.mode of a sine handle

struct SineQuality : cordic_quality {
	SParams sp{};
	SSlot *d_sslots = nullptr;
	int pw = 0, ow = 0;
	double tbl_err = 0.0;
	bool judged = false;
};

static SineQuality *as_sine(cordic_quality *q)
{
	return (q && q->cfg.mode == kSineMode) ? static_cast<SineQuality *>(q) : nullptr;
}

static int zero_sine_slots(SineQuality *q, hipStream_t st)
{
	std::vector<SSlot> z((size_t)q->grid);
	for (auto &s : z) {
		std::memset(&s, 0, sizeof s);
		s.err = -1.0;
		s.arg = ~0ull;
	}
	// pageable source: hipMemcpyAsync returns once it has been staged
	if (hipMemcpyAsync(q->d_sslots, z.data(), z.size() * sizeof(SSlot),
			hipMemcpyHostToDevice, st) != hipSuccess)
		return CORDIC_ERR_DEVICE;
	if (hipStreamSynchronize(st) != hipSuccess)
		return CORDIC_ERR_DEVICE;
	q->count = 0;
	q->kind = -1;
	return CORDIC_OK;
}

static int create_sine(int pw, int ow, double tbl_err, bool judged,
		cordic_quality **out)
{
	SineQuality *q = new (std::nothrow) SineQuality;
	if (!q)
		return CORDIC_ERR_NOMEM;
	std::memset(&q->cfg, 0, sizeof q->cfg);
	q->cfg.mode = kSineMode;
	q->pw = pw; q->ow = ow;
	q->tbl_err = tbl_err;
	q->judged = judged;
	q->sp.ow = ow;
	q->sp.scale = (double)((1ll << (ow - 1)) - 1);		// quadtbl_tb.cpp:157
	q->sp.two_inv_2pw = std::ldexp(1.0, 1 - pw);
	q->sp.pmask = (pw >= 32) ? 0xffffffffu : ((1u << pw) - 1u);
	hipDeviceProp_t prop;
	if (hipGetDevice(&q->device) != hipSuccess ||
	    hipGetDeviceProperties(&prop, q->device) != hipSuccess) {
		delete q;
		return CORDIC_ERR_DEVICE;
	}
	q->grid = prop.multiProcessorCount * 8;
	if (hipMalloc((void **)&q->d_sslots, (size_t)q->grid * sizeof(SSlot)) != hipSuccess) {
		delete q;
		return CORDIC_ERR_DEVICE;
	}
	if (int rc = zero_sine_slots(q, nullptr)) {
		cordic_quality_destroy(q);
		return rc;
	}
	*out = q;
	return CORDIC_OK;
}

int cordic_quality_create_quad(const cordic_quad_config *cfg, cordic_quality **out)
{
	if (!cfg || !out || !quad_sane(*cfg))
		return CORDIC_ERR_ARGS;
	return create_sine(cfg->pw, cfg->ow, cfg->tbl_err, true, out);
}

int cordic_quality_create_table(const cordic_table_config *cfg, cordic_quality **out)
{
	if (!cfg || !out || !table_sane(*cfg))
		return CORDIC_ERR_ARGS;
	return create_sine(cfg->pw, cfg->ow, 0.0, false, out);
}

template <bool NCO, typename T>
static int sine_common(cordic_quality *h, size_t n, const uint32_t *phase,
		uint32_t phase0, uint32_t fcw, uint64_t index0, const T *val,
		void *stream)
{
	SineQuality *q = as_sine(h);
	if (!q)
		return CORDIC_ERR_ARGS;
	if (sizeof(T) == 2 && q->ow > 16)
		return CORDIC_ERR_CONTAINER;
	if (n == 0)
		return CORDIC_OK;
	if (!val || (!NCO && !phase))
		return CORDIC_ERR_ARGS;
	(void)hipGetLastError();
	hipLaunchKernelGGL((quality_sine<NCO, T>), dim3(q->grid), dim3(kQBlock), 0,
		static_cast<hipStream_t>(stream), q->sp, n, phase, phase0, fcw,
		(unsigned long long)index0, val, q->count, q->d_sslots);
	if (hipGetLastError() != hipSuccess)
		return CORDIC_ERR_DEVICE;
	q->count += n;
	q->kind = 2;
	return CORDIC_OK;
}

int cordic_quality_sine(cordic_quality *q, size_t n, const uint32_t *d_phase,
		const int32_t *d_val, void *stream)
{
	return sine_common<false>(q, n, d_phase, 0, 0, 0, d_val, stream);
}

int cordic_quality_sine16(cordic_quality *q, size_t n, const uint32_t *d_phase,
		const int16_t *d_val, void *stream)
{
	return sine_common<false>(q, n, d_phase, 0, 0, 0, d_val, stream);
}

int cordic_quality_sine_nco(cordic_quality *q, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, const int32_t *d_val, void *stream)
{
	return sine_common<true>(q, n, nullptr, phase0, fcw, index0, d_val, stream);
}

int cordic_quality_sine_nco16(cordic_quality *q, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, const int16_t *d_val, void *stream)
{
	return sine_common<true>(q, n, nullptr, phase0, fcw, index0, d_val, stream);
}

int cordic_quality_sine_result(cordic_quality *handle, cordic_sine_quality *r)
{
	SineQuality *q = as_sine(handle);
	if (!q || !r)
		return CORDIC_ERR_ARGS;
	if (q->kind != 2 || q->count == 0)
		return CORDIC_ERR_ARGS;
	std::vector<SSlot> h((size_t)q->grid);
	if (hipDeviceSynchronize() != hipSuccess ||
	    hipMemcpy(h.data(), q->d_sslots, h.size() * sizeof(SSlot),
			hipMemcpyDeviceToHost) != hipSuccess)
		return CORDIC_ERR_DEVICE;
	SSlot m;
	std::memset(&m, 0, sizeof m);
	m.err = -1.0;
	m.arg = ~0ull;
	for (const SSlot &s : h) {
		if (s.err > m.err || (s.err == m.err && s.arg < m.arg)) {
			m.err = s.err; m.arg = s.arg; m.phase = s.phase;
		}
		m.maxv = s.maxv > m.maxv ? s.maxv : m.maxv;
		m.minv = s.minv < m.minv ? s.minv : m.minv;
	}
	std::memset(r, 0, sizeof *r);		// padding too: results compare bytewise
	r->n = q->count;
	r->max_err = m.err;
	r->max_err_index = m.arg;
	r->max_err_phase = m.phase;
	r->max_val = m.maxv;
	r->min_val = m.minv;
	r->scale = q->sp.scale;
	r->tbl_err = q->tbl_err;
	// quadtbl_tb.cpp:176
	r->limit = q->judged ? std::fabs(q->tbl_err) + 2. : 0.0;
	r->judged = q->judged;
	r->pass = q->judged ? !(std::fabs(r->max_err) > r->limit) : 1;
	return CORDIC_OK;
}

// ------------------------------- the public entry points over both handles

void cordic_quality_destroy(cordic_quality *h)
{
	SineQuality *q = as_sine(h);
	if (!q) {
		quality_base_destroy(h);
		return;
	}
	if (q->d_sslots)
		(void)hipFree(q->d_sslots);
	delete q;
}

int cordic_quality_reset(cordic_quality *h, void *stream)
{
	if (SineQuality *q = as_sine(h))
		return zero_sine_slots(q, static_cast<hipStream_t>(stream));
	return quality_base_reset(h, stream);
}

int cordic_quality_p2r(cordic_quality *q, size_t n, const int32_t *d_xval,
		const int32_t *d_yval, int32_t xval, int32_t yval,
		const uint32_t *d_phase, const int32_t *d_oxval,
		const int32_t *d_oyval, void *stream)
{
	if (as_sine(q))
		return CORDIC_ERR_ARGS;
	return quality_base_p2r(q, n, d_xval, d_yval, xval, yval, d_phase, d_oxval,
			d_oyval, stream);
}

int cordic_quality_nco(cordic_quality *q, size_t n, uint32_t phase0, uint32_t fcw,
		uint64_t index0, int32_t xval, int32_t yval,
		const int32_t *d_oxval, const int32_t *d_oyval, void *stream)
{
	if (as_sine(q))
		return CORDIC_ERR_ARGS;
	return quality_base_nco(q, n, phase0, fcw, index0, xval, yval, d_oxval,
			d_oyval, stream);
}

int cordic_quality_r2p(cordic_quality *q, size_t n, const int32_t *d_xval,
		const int32_t *d_yval, int32_t imag, const int32_t *d_omag,
		const uint32_t *d_ophase, void *stream)
{
	if (as_sine(q))
		return CORDIC_ERR_ARGS;
	return quality_base_r2p(q, n, d_xval, d_yval, imag, d_omag, d_ophase, stream);
}

int cordic_quality_p2r_result(cordic_quality *q, cordic_p2r_quality *out)
{
	if (as_sine(q))
		return CORDIC_ERR_ARGS;
	return quality_base_p2r_result(q, out);
}

int cordic_quality_r2p_result(cordic_quality *q, cordic_r2p_quality *out)
{
	if (as_sine(q))
		return CORDIC_ERR_ARGS;
	return quality_base_r2p_result(q, out);
}
