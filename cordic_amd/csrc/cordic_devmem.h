// cordic_devmem.h -- host-only helpers of the C ABI units (cordic_abi*.cpp):
// device memory of the handles, and the one stream-capture query.  The handles
// are C structs that their *_destroy functions free; nothing here owns memory.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

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
