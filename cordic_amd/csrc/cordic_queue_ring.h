// cordic_queue_ring.h -- the tile queues a plan, table or quadratic handle
// lends to its launches (host only; cordic_abi.cpp with cordic_abi_plan.h,
// cordic_abi_table.cpp).
#pragma once
#include <cstdlib>
#include <mutex>

#include "cordic_amd.h"
#include "cordic_devmem.h"

// Tile queues of the seeded kernel (CORDIC_QUEUE_BYTES of device counters,
// zeroed once here and left zeroed by every kernel that used them).  Two
// launches must never share a block of counters while either is running, so a
// slot is handed out again only once the launch that used it has COMPLETED:
//   - eager launches draw from slots [0, kEagerSlots) round robin: each slot
//     carries an event recorded right behind its kernel; a launch that gets a
//     slot whose previous user may still be running is ordered behind it on
//     the device (same stream: nothing to do; other stream: the stream waits
//     for the event) -- the host never waits and may run ahead of the GPU by
//     any number of launches;
//   - a launch issued while its stream is being CAPTURED keeps its slot baked
//     into the graph node and may be replayed at any later time, so it takes a
//     slot from [kEagerSlots, kQueueSlots) that is never handed out again
//     (at most kQueueSlots - kEagerSlots = 208 captured launches per handle
//     for its lifetime; further ones run the static sweep, -5...-8 %, and are
//     counted: cordic_*_queue_info).  A graph exec never runs concurrently
//     with itself, so one slot per captured node is enough; two execs
//     instantiated from the SAME captured graph share the node's slot and
//     must not run concurrently (include/cordic_amd.h says so).
// Stream identity is never taken from the handle's address (a destroyed
// stream's address can be reused): a slot whose event has not completed is
// always waited for on the device, whatever stream asks.
// (Inline and templates only: cordic_abi_plan.h puts a ring into a handle that
// two units share.)
namespace cordic_amd {
constexpr unsigned kQueueSlots = 256;
constexpr unsigned kEagerSlots = 48;

struct QueueRing {
	enum State : unsigned char { FREE, CLAIMED, RECORDED, RETIRED };
	uint32_t *d = nullptr;		// kQueueSlots x CORDIC_QUEUE_BYTES
	mutable std::mutex mu;
	mutable hipEvent_t ev[kEagerSlots] = {};
	mutable State state[kQueueSlots] = {};
	mutable State prev[kEagerSlots] = {};	// state before the pending claim
	mutable unsigned next = 0, next_captured = kEagerSlots;
	mutable unsigned long long fallbacks = 0;	// launches that got no slot

	bool alloc()
	{
		if (!dev_zalloc(&d, (size_t)kQueueSlots * CORDIC_QUEUE_BYTES))
			return false;
		for (unsigned k = 0; k < kEagerSlots; k++)
			if (hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) {
				release();
				return false;
			}
		return true;
	}
	void info(cordic_queue_info *out) const
	{
		std::lock_guard<std::mutex> lock(mu);
		out->eager_slots = d ? (int32_t)kEagerSlots : 0;
		out->captured_capacity = d ? (int32_t)(kQueueSlots - kEagerSlots) : 0;
		out->captured_used = (int32_t)(next_captured - kEagerSlots);
		out->fallback_launches = fallbacks;
	}
	void release()
	{
		for (unsigned k = 0; k < kEagerSlots; k++)
			if (ev[k]) {
				(void)hipEventDestroy(ev[k]);
				ev[k] = nullptr;
			}
		dev_free(d);
	}
	uint32_t *ptr(int slot) const
	{
		return slot < 0 ? nullptr
			: d + (size_t)(slot % (int)kQueueSlots) * (CORDIC_QUEUE_BYTES / 4);
	}
	// a slot no launch in flight uses, or -1 (the caller then launches
	// without a queue)
	int claim(void *stream) const
	{
		if (!d)
			return -1;
		// A/B switch (measurement only): the round-2 behaviour, slots handed
		// out round-robin without looking at what is still in flight
		static const bool unchecked = [] {
			const char *e = std::getenv("CORDIC_QUEUE_UNCHECKED");
			return e && e[0] == '1';
		}();
		if (unchecked) {
			std::lock_guard<std::mutex> lock(mu);
			const unsigned k = next;
			next = (next + 1) % kQueueSlots;
			return (int)k + (int)kQueueSlots;	// launched() ignores it
		}
		const bool capturing = stream_capturing(stream, nullptr);
		std::lock_guard<std::mutex> lock(mu);
		if (capturing) {
			if (next_captured >= kQueueSlots) {
				fallbacks++;
				return -1;
			}
			state[next_captured] = RETIRED;
			return (int)next_captured++;
		}
		// round robin; a slot whose last launch may still be running is
		// made safe ON THE DEVICE: this stream waits for that launch's
		// event (on the stream that recorded it the wait is free: stream
		// order already serialises the two kernels).  No host wait, and the
		// host may run any number of launches ahead of the GPU without
		// losing the queue.
		for (unsigned i = 0; i < kEagerSlots; i++) {
			const unsigned k = (next + i) % kEagerSlots;
			if (state[k] == CLAIMED || state[k] == RETIRED)
				continue;	// another thread is launching on it
			if (state[k] == RECORDED && hipEventQuery(ev[k]) != hipSuccess) {
				(void)hipGetLastError();	// hipErrorNotReady
				if (hipStreamWaitEvent(static_cast<hipStream_t>(stream),
						ev[k], 0) != hipSuccess) {
					(void)hipGetLastError();
					continue;
				}
			}
			prev[k] = state[k];
			state[k] = CLAIMED;
			next = (k + 1) % kEagerSlots;
			return (int)k;
		}
		fallbacks++;
		return -1;
	}
	// after the launch that uses `slot` has been enqueued (rc = its status)
	void launched(int slot, void *stream, int rc) const
	{
		if (slot < 0 || slot >= (int)kEagerSlots)
			return;
		std::lock_guard<std::mutex> lock(mu);
		if (rc != CORDIC_OK)
			// nothing new ran on it: what was there before the claim
			// stands -- a RECORDED slot keeps its pending event, so the
			// earlier launch is still waited for by the next taker
			state[slot] = prev[slot];
		else if (hipEventRecord(ev[slot], static_cast<hipStream_t>(stream)) == hipSuccess)
			state[slot] = RECORDED;
		else
			state[slot] = RETIRED;	// cannot tell when it is free again
	}
};

// launch with a tile queue no other launch in flight is using
template <typename F> int with_queue(const QueueRing &ring, void *stream, F launch)
{
	const int slot = ring.claim(stream);
	const int rc = launch(ring.ptr(slot));
	ring.launched(slot, stream, rc);
	return rc;
}

// cordic_{plan,table,quad}_queue_info: every such handle has its ring in `queues`
template <typename H> int queue_info(const H *h, cordic_queue_info *info)
{
	if (!h || !info)
		return CORDIC_ERR_ARGS;
	h->queues.info(info);
	return CORDIC_OK;
}
} // namespace cordic_amd
