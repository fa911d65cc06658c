// cordic_devmem.h -- host-only helpers of the C ABI units (cordic_abi*.cpp,
// cordic_fm_demod_bank.hip): device memory of the handles, the stream-capture
// queries, a handle's device, the skeleton of the FM bank handles and the span
// table of the two prefix-sum ones.  Handles
// are C structs that their *_destroy functions free; nothing here owns memory.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <vector>

#include "cordic_amd.h"
#include "cordic_span_bank.h"

// frees the non-null ones of its pointers, then nulls them
template <typename... T> static void dev_free(T *&...p)
{
	((p ? (void)hipFree(p) : (void)0, p = nullptr), ...);
}

// Device memory that `fill` has written, or a clean failure: nothing stays
// allocated, *dst is null and the runtime's sticky error is cleared.  Zero bytes
// succeed and leave *dst null.  Whether a failure is fatal is the caller's
// business.
template <typename T, typename F>
static bool dev_filled(T **dst, size_t bytes, F fill)
{
	*dst = nullptr;
	if (!bytes)
		return true;
	if (hipMalloc((void **)dst, bytes) == hipSuccess && fill() == hipSuccess)
		return true;
	dev_free(*dst);
	(void)hipGetLastError();
	return false;
}

// a device copy of a host array
template <typename T>
static bool dev_upload(const void *src, size_t bytes, T **dst)
{
	return dev_filled(dst, bytes,
		[=] { return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice); });
}

// zeroed device memory
template <typename T> static bool dev_zalloc(T **dst, size_t bytes)
{
	return dev_filled(dst, bytes, [=] { return hipMemset(*dst, 0, bytes); });
}

// Is `stream` being captured?  (The null stream is not asked.)  A failed query
// answers false, sets *query_failed where the caller gave one and leaves no
// sticky error behind.  Two policies, by what the caller does with the answer:
//   - it only CHOOSES by it and then enqueues on the stream anyway (a tile
//     queue's slot, the one-shot batches): pass nullptr, a failed query counts
//     as "not capturing" and whatever is wrong with the stream comes back as
//     the status of that launch;
//   - its work would go wrong inside a capture without any call failing
//     (cordic_oscbank_retune: the copy would become a graph node that reads a
//     host mirror rewritten by then): it has to KNOW, and answers a failed
//     query with CORDIC_ERR_DEVICE.
static inline bool stream_capturing(void *stream, bool *query_failed)
{
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	const bool failed = stream && hipStreamIsCapturing(
			static_cast<hipStream_t>(stream), &cs) != hipSuccess;
	if (failed)
		(void)hipGetLastError();
	if (query_failed)
		*query_failed = failed;
	return !failed && cs != hipStreamCaptureStatusNone;
}

// The legacy (null) stream, whose capture a create's blocking uploads may not
// enter.  This one does ask the null stream; the runtime says yes by the status
// or, where another stream's capture makes the legacy stream unusable, by the
// error below.  Any other failure is "not capturing": the uploads report it.
static inline bool legacy_stream_capturing()
{
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	const hipError_t ce = hipStreamIsCapturing(nullptr, &cs);
	(void)hipGetLastError();
	return ce == hipErrorStreamCaptureImplicit
		|| (ce == hipSuccess && cs != hipStreamCaptureStatusNone);
}

// the current device, for a handle to record; -1 and no sticky error: none
static inline int current_device()
{
	int dev = -1;
	return hipGetDevice(&dev) == hipSuccess ? dev : ((void)hipGetLastError(), -1);
}

// Is the device that a handle recorded current?  (Its tables hold device
// addresses.)  CORDIC_ERR_DEVICE: none is, CORDIC_ERR_ARGS: another one is.
static inline int device_is_current(int device)
{
	const int dev = current_device();
	return dev < 0 ? CORDIC_ERR_DEVICE : dev == device ? CORDIC_OK : CORDIC_ERR_ARGS;
}

// the CUs of the current device (cordic_jobs_fused.hip), or 256 and no sticky error
namespace cordic_amd { int jobs_cus_now(); }
static inline int cus_or_256()
{
	const int cus = cordic_amd::jobs_cus_now();
	return cus > 0 ? cus : ((void)hipGetLastError(), 256);
}

// ---- What cordic_demodbank (cordic_fm_demod_bank.hip) and cordic_mixbank
// (cordic_abi_fm.cpp) share: a bank runs FUSED, from descriptor tables that its
// create cuts and uploads, or ONE BY ONE through the single call of its kind.
template <typename Job> struct BankHandle {
	bool	fused = false;
	int	device = -1, cus = 0;	// (cus: of a fused bank's device, at create)
	uint64_t samples = 0;
	// one by one: the non-empty jobs and the workspace of the longest
	std::vector<Job> jobs;
	void	*d_work = nullptr;
};

// The head of a create, behind the argument checks: makes the handle B (a
// BankHandle<Job>) and finishes one that runs one by one (work_bytes(n): the
// single call's workspace).  A fused one the caller cuts for, or frees.
template <typename B, typename Job, typename WorkBytes>
static int bank_begin(size_t njobs, const Job *jobs, bool fused,
		WorkBytes work_bytes, B **out)
{
	if (legacy_stream_capturing())	// (blocking uploads below)
		return CORDIC_ERR_UNSUPPORTED;
	B *b = new (std::nothrow) B;
	if (!b)
		return CORDIC_ERR_NOMEM;
	b->fused = fused;
	b->device = current_device();
	size_t longest = 0;
	for (size_t k = 0; k < njobs; k++) {
		b->samples += jobs[k].n;
		if (jobs[k].n > longest)
			longest = (size_t)jobs[k].n;
		if (!fused && jobs[k].n)
			b->jobs.push_back(jobs[k]);
	}
	b->cus = fused ? cus_or_256() : 0;
	if (!fused && !dev_zalloc(&b->d_work, work_bytes(longest))) {
		delete b;
		return CORDIC_ERR_DEVICE;
	}
	*out = b;
	return CORDIC_OK;
}

// ---- What cordic_mixbank (cordic_abi_fm.cpp) and cordic_fmbank
// (cordic_abi_table.cpp) share, the prefix-sum banks (cordic_span_bank.h): the
// span table on the device and the workspace of a run, [start words, one per
// non-empty job | partial sums, one per span | SpanRule::words further latched
// words per non-empty job].
template <typename SPAN> struct SpanTable {
	SPAN	*d_spans = nullptr;
	uint32_t *d_words = nullptr;
	uint32_t nspans = 0, nstarts = 0;
	uint32_t *start() const { return d_words; }
	uint32_t *part() const { return d_words + nstarts; }
	uint32_t *more() const { return d_words + nstarts + nspans; }
	void	free() { dev_free(d_spans, d_words); }
};

// The tail of a create, behind its own argument checks: the base span for
// `total_units` on `cus` CUs with `per_cu` resident blocks each, or what the
// environment variable `env_base` forces, into *base (for *_info); the span cap
// of `rule`, or what `env_cap` lowers it to; then cuts, uploads and allocates.
// CORDIC_OK; CORDIC_ERR_ARGS: more than 2^32 - 1 spans; CORDIC_ERR_DEVICE: an
// upload failed, and nothing stays allocated.
template <typename SPAN, typename Jobs>
static int span_table_build(SpanTable<SPAN> *t, const char *env_base,
		const char *env_cap, const cordic_amd::SpanRule &rule, uint64_t total_units,
		int cus, int per_cu, size_t njobs, Jobs jobs, uint32_t *base)
{
	using namespace cordic_amd;
	*base = span_forced_base(rule, std::getenv(env_base),
			span_base_units(rule, total_units, cus, per_cu));
	const uint32_t cap = span_forced_cap(rule, std::getenv(env_cap));
	if (span_count(rule, njobs, jobs, *base, cap) > 0xffffffffull)
		return CORDIC_ERR_ARGS;
	std::vector<SPAN> spans;
	span_cut(rule, njobs, jobs, *base, cap, &spans, &t->nstarts);
	t->nspans = (uint32_t)spans.size();
	if (!dev_upload(spans.data(), spans.size() * sizeof(SPAN), &t->d_spans)
			|| !dev_zalloc(&t->d_words,
				((size_t)t->nstarts * (1 + rule.words) + t->nspans)
					* sizeof(uint32_t))) {
		t->free();
		return CORDIC_ERR_DEVICE;
	}
	return CORDIC_OK;
}

// A run: on the handle's device, the fused launches or the kept jobs through `each`
template <typename Job, typename Fused, typename Each>
static int bank_run(const BankHandle<Job> &b, Fused fused, Each each)
{
	if (int rc = device_is_current(b.device))
		return rc;
	if (b.fused)
		return fused();
	for (const Job &jb : b.jobs)
		if (int rc = each(jb))
			return rc;
	return CORDIC_OK;
}
