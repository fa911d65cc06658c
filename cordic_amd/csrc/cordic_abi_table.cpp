// cordic_abi_table.cpp -- the C ABI's table-driven sine cores on the device:
// table and quadratic handles, their lookups and oscillators (the modulated
// ones included), and the oscillator banks and FM oscillator banks cut for them
// (include/cordic_amd.h;
// the cores' host side: cordic_abi.cpp).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <new>
#include <vector>

#include "cordic_amd.h"
#include "cordic_devmem.h"
#include "cordic_internal.h"
#include "cordic_queue_ring.h"
#include "cordic_table_bank.h"
#include "cordic_table_fm.h"
#include "cordic_table_fm_bank.h"
#include "cordic_table_nco.h"

using namespace cordic_amd;

// ------------------------------------------------------------- table cores
struct cordic_table {
	cordic_table_config cfg;
	int32_t *d_tbl = nullptr;
	// optional packed copy for the LDS kernel (cordic_kernels.hip:
	// table_lookup_lds): mode 1 = quarter-wave table as is, 2 = full-wave
	// table folded to its first quadrant (+ the peak entry)
	int16_t *d_lds16 = nullptr;
	int	lds_mode = 0, lds_entries = 0;
	QueueRing queues;	// optional: without it the chunk-per-block sweep runs

	SineCore core() const
	{
		SineCore c;
		c.t = cfg;
		c.d_tbl = d_tbl;
		c.d_lds16 = d_lds16;
		c.lds_mode = lds_mode;
		c.lds_entries = lds_entries;
		return c;
	}
};

namespace {
// A packed int16 table of at most 64 KiB (+ one entry) if the core allows it.
// For -t tbl the fold is only used when every one of the 2^PW entries is
// reproduced by it.
bool pack_for_lds(const cordic_table_config &c, const std::vector<int32_t> &t,
		std::vector<int16_t> *out, int *mode)
{
	if (c.pw < 4)
		return false;
	const int quarter = 1 << (c.pw - 2);
	if (quarter > 32768)
		return false;
	// OW <= 16: a packed int16 copy (modes 1 / 2, two blocks per CU); wider
	// outputs: the 32-bit entries themselves (modes 3 / 4, 128 KiB for 2^15
	// entries, one block per CU), read from the table in HBM by the kernel
	const bool wide = c.ow > 16;
	if (c.kind == CORDIC_QTR) {
		if (!wide) {
			out->resize((size_t)quarter);
			for (int k = 0; k < quarter; k++)
				(*out)[(size_t)k] = (int16_t)t[(size_t)k];
		}
		*mode = wide ? 3 : 1;
		return true;
	}
	const int n = 1 << c.pw;
	for (int i = 0; i < n; i++) {
		const int q = i >> (c.pw - 2), j = i & (quarter - 1);
		int32_t v = t[(size_t)((q & 1) ? quarter - j : j)];
		if (q & 2)
			v = -v;
		if (v != t[(size_t)i])
			return false;
	}
	if (!wide) {
		out->resize((size_t)quarter + 1);
		for (int k = 0; k <= quarter; k++)
			(*out)[(size_t)k] = (int16_t)t[(size_t)k];
	}
	*mode = wide ? 4 : 2;
	return true;
}
} // namespace

int cordic_table_create(const cordic_table_config *cfg, cordic_table **tbl)
{
	if (!cfg || !tbl || !table_sane(*cfg))
		return CORDIC_ERR_ARGS;
	std::vector<int32_t> host((size_t)cfg->entries);
	int rc = table_fill(*cfg, host.data(), host.size());
	if (rc != CORDIC_OK)
		return rc;
	cordic_table *t = new (std::nothrow) cordic_table;
	if (!t)
		return CORDIC_ERR_NOMEM;
	t->cfg = *cfg;
	if (!dev_upload(host.data(), host.size() * 4, &t->d_tbl)) {
		delete t;
		return CORDIC_ERR_DEVICE;
	}
	std::vector<int16_t> packed;
	int mode = 0;
	if (pack_for_lds(*cfg, host, &packed, &mode)) {
		const int quarter = 1 << (cfg->pw - 2);
		if (mode >= 3) {
			// the kernel fills its LDS copy from d_tbl itself
			t->lds_mode = mode;
			t->lds_entries = quarter + (mode == 4 ? 1 : 0);
		} else if (dev_upload(packed.data(), packed.size() * 2, &t->d_lds16)) {
			// optional: on failure the L2 gather kernel serves the table
			t->lds_mode = mode;
			t->lds_entries = (int)packed.size();
		}
	}
	if (!t->queues.alloc())
		(void)hipGetLastError();
	*tbl = t;
	return CORDIC_OK;
}

int cordic_table_queue_info(const cordic_table *tbl, cordic_queue_info *info)
{
	return queue_info(tbl, info);
}

void cordic_table_destroy(cordic_table *tbl)
{
	if (!tbl)
		return;
	tbl->queues.release();
	dev_free(tbl->d_tbl, tbl->d_lds16);
	delete tbl;
}

int cordic_table_lds_mode(const cordic_table *tbl)
{
	return tbl ? tbl->lds_mode : CORDIC_ERR_ARGS;
}

int cordic_table_lookup(const cordic_table *tbl, size_t n,
		const uint32_t *d_phase, int32_t *d_val, void *stream)
{
	if (!tbl)
		return CORDIC_ERR_ARGS;
	return with_queue(tbl->queues, stream, [&](uint32_t *q) {
		return launch_table_lookup(tbl->cfg, tbl->d_tbl, n, d_phase, d_val,
				stream, tbl->d_lds16, tbl->lds_mode, tbl->lds_entries, q);
	});
}

// ---------------------------------------- oscillators on either sine core
// The argument checks of the oscillator calls of either core `h`, then its
// store-only launch (cordic_table_nco.hip), queued and counted like the
// lookup's.
template <typename H>
static int nco_call(const H *h, size_t n, uint32_t phase0, uint32_t fcw,
		uint64_t index0, void *d_sin, void *d_cos, bool io16, void *stream)
{
	if (!h)
		return CORDIC_ERR_ARGS;
	if (io16 && h->cfg.ow > 16)
		return CORDIC_ERR_CONTAINER;
	if (n == 0)
		return CORDIC_OK;
	if (!d_sin)
		return CORDIC_ERR_ARGS;
	return with_queue(h->queues, stream, [&](uint32_t *q) {
		return launch_sine_nco(h->core(), n, phase0, fcw, index0, d_sin, d_cos,
				io16, stream, q);
	});
}

// The argument checks of the modulated oscillator calls of either core `h`,
// then their two launches (cordic_table_fm.hip).  No tile queue: these calls
// take none and count nowhere.
template <typename H>
static int fm_call(const H *h, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, void *d_sin,
		void *d_cos, bool io16, void *d_work, void *stream)
{
	if (!h)
		return CORDIC_ERR_ARGS;
	if (io16 && h->cfg.ow > 16)
		return CORDIC_ERR_CONTAINER;
	if (n == 0)
		return CORDIC_OK;
	if (!d_fcw || !d_sin || !d_work)
		return CORDIC_ERR_ARGS;
	return launch_sine_fm(h->core(), n, d_fcw, d_pm, phase0, d_acc, d_sin, d_cos,
			io16, d_work, stream);
}

int cordic_table_nco(const cordic_table *tbl, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, int32_t *d_sin, int32_t *d_cos,
		void *stream)
{
	return nco_call(tbl, n, phase0, fcw, index0, d_sin, d_cos, false, stream);
}

int cordic_table_nco16(const cordic_table *tbl, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, int16_t *d_sin, int16_t *d_cos,
		void *stream)
{
	return nco_call(tbl, n, phase0, fcw, index0, d_sin, d_cos, true, stream);
}

int cordic_table_fm(const cordic_table *tbl, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, int32_t *d_sin,
		int32_t *d_cos, void *d_work, void *stream)
{
	return fm_call(tbl, n, d_fcw, d_pm, phase0, d_acc, d_sin, d_cos, false,
			d_work, stream);
}

int cordic_table_fm16(const cordic_table *tbl, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, int16_t *d_sin,
		int16_t *d_cos, void *d_work, void *stream)
{
	return fm_call(tbl, n, d_fcw, d_pm, phase0, d_acc, d_sin, d_cos, true,
			d_work, stream);
}

// ------------------------------------------------- quadratic sine core
struct cordic_quad {
	cordic_quad_config cfg;
	int32_t *d_tab = nullptr;	// entries x {C, L, Q, 0}
	QueueRing queues;

	SineCore core() const
	{
		SineCore c;
		c.quad = true;
		c.q = cfg;
		c.d_tbl = d_tab;
		return c;
	}
};

int cordic_quad_create(const cordic_quad_config *cfg, cordic_quad **core)
{
	if (!cfg || !core || !quad_sane(*cfg))
		return CORDIC_ERR_ARGS;
	const size_t n = (size_t)cfg->entries;
	std::vector<int32_t> c(n), l(n), q(n), packed(n * 4);
	int rc = quad_fill(*cfg, c.data(), l.data(), q.data(), n);
	if (rc != CORDIC_OK)
		return rc;
	for (size_t k = 0; k < n; k++) {
		packed[4 * k] = c[k];
		packed[4 * k + 1] = l[k];
		packed[4 * k + 2] = q[k];
		packed[4 * k + 3] = 0;
	}
	cordic_quad *h = new (std::nothrow) cordic_quad;
	if (!h)
		return CORDIC_ERR_NOMEM;
	h->cfg = *cfg;
	if (!dev_upload(packed.data(), packed.size() * 4, &h->d_tab)) {
		delete h;
		return CORDIC_ERR_DEVICE;
	}
	if (!h->queues.alloc())
		(void)hipGetLastError();
	*core = h;
	return CORDIC_OK;
}

int cordic_quad_queue_info(const cordic_quad *core, cordic_queue_info *info)
{
	return queue_info(core, info);
}

void cordic_quad_destroy(cordic_quad *core)
{
	if (!core)
		return;
	core->queues.release();
	dev_free(core->d_tab);
	delete core;
}

int cordic_quad_lookup(const cordic_quad *core, size_t n, const uint32_t *d_phase,
		int32_t *d_sin, void *stream)
{
	if (!core)
		return CORDIC_ERR_ARGS;
	return with_queue(core->queues, stream, [&](uint32_t *q) {
		return launch_quad_lookup(core->cfg, core->d_tab, n, d_phase, d_sin,
				stream, q);
	});
}

int cordic_quad_nco(const cordic_quad *core, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, int32_t *d_sin, int32_t *d_cos,
		void *stream)
{
	return nco_call(core, n, phase0, fcw, index0, d_sin, d_cos, false, stream);
}

int cordic_quad_nco16(const cordic_quad *core, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, int16_t *d_sin, int16_t *d_cos,
		void *stream)
{
	return nco_call(core, n, phase0, fcw, index0, d_sin, d_cos, true, stream);
}

int cordic_quad_fm(const cordic_quad *core, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, int32_t *d_sin,
		int32_t *d_cos, void *d_work, void *stream)
{
	return fm_call(core, n, d_fcw, d_pm, phase0, d_acc, d_sin, d_cos, false,
			d_work, stream);
}

int cordic_quad_fm16(const cordic_quad *core, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, int16_t *d_sin,
		int16_t *d_cos, void *d_work, void *stream)
{
	return fm_call(core, n, d_fcw, d_pm, phase0, d_acc, d_sin, d_cos, true,
			d_work, stream);
}

// ------------------------------------------------------- oscillator banks
// Many oscillator jobs of one table / quadratic core in one launch
// (include/cordic_amd.h, "oscillator banks"; kernel: cordic_table_bank.hip).
// The host cuts the jobs' output streams into tiles and edges once; tunings
// stay a per-job device array that cordic_oscbank_retune rewrites in place.
struct cordic_oscbank {
	// the core and its handle's tile queues: the handle must outlive the bank
	SineCore core;
	const QueueRing *queues = nullptr;
	int	device = -1;
	bool	io16 = false;
	// host mirror of the device tunings, the source of retune's copy.  It is
	// pageable memory on purpose: the runtime reads a pageable source of a
	// host-to-device copy into its own staging before hipMemcpyAsync returns
	// (only pinned sources are read later, in stream order), so the mirror
	// may be overwritten by the next retune, or freed by destroy, as soon as
	// the call is back -- also when the CALLER's array is pinned memory.
	// "The values are taken before the call returns" rests on that.
	std::vector<cordic_osc_tuning> tunings;
	OscTile *d_tiles = nullptr;
	OscEdge *d_edges = nullptr;
	cordic_osc_tuning *d_tunings = nullptr;
	BankTables tabs;
	uint64_t samples = 0;
	uint32_t edge_samples = 0;
};

namespace {
// `core` and `queues`: those of the table or quadratic handle the bank is for
int oscbank_create(const SineCore &core, const QueueRing *queues, size_t njobs,
		const cordic_osc_job *jobs, cordic_oscbank **out, bool io16)
{
	if (!out || (njobs && !jobs))
		return CORDIC_ERR_ARGS;
	if (io16 && core.ow() > 16)
		return CORDIC_ERR_CONTAINER;
	if (core.quad && core.lds_bytes() > 64 * 1024)
		return CORDIC_ERR_UNSUPPORTED;
	if (njobs > 0xffffffffull)
		return CORDIC_ERR_ARGS;
	const unsigned esize = io16 ? 2 : 4;
	const uint64_t W = 16 / esize;
	const uint32_t quarter = core.quarter();
	// one output stream of a job, cut on its own address
	struct Stream { uint64_t addr, n, head, nvec; uint32_t job, lead; };
	std::vector<Stream> streams;
	uint64_t samples = 0, total_vecs = 0;
	for (size_t k = 0; k < njobs; k++) {
		const cordic_osc_job &jb = jobs[k];
		if (jb.n == 0)
			continue;
		const uintptr_t s = (uintptr_t)jb.d_sin, c = (uintptr_t)jb.d_cos;
		if (!s || (s & (esize - 1)) || (c & (esize - 1))
				|| jb.n > (~(uint64_t)0 - (s > c ? s : c)) / esize)
			return CORDIC_ERR_ARGS;
		for (int q = 0; q < (c ? 2 : 1); q++) {
			Stream st;
			st.addr = q ? c : s;
			st.n = jb.n;
			st.head = head_elems((uintptr_t)st.addr, esize);
			if (st.head > st.n) st.head = st.n;
			st.nvec = (st.n - st.head) / W;
			st.job = (uint32_t)k;
			st.lead = q ? quarter : 0u;
			streams.push_back(st);
			samples += jb.n;
			total_vecs += st.nvec;
		}
	}
	// no two output ranges may overlap: sorted by address, each against its
	// successor
	std::sort(streams.begin(), streams.end(),
		[](const Stream &a, const Stream &b) { return a.addr < b.addr; });
	for (size_t k = 1; k < streams.size(); k++)
		if (streams[k - 1].addr + streams[k - 1].n * esize > streams[k].addr)
			return CORDIC_ERR_ARGS;
	int resident = sine_bank_resident(core);
	if (resident < 0) {
		(void)hipGetLastError();
		resident = 512;
	}
	uint64_t with_vecs = 0;
	for (const Stream &st : streams)
		with_vecs += st.nvec != 0;
	const uint32_t shift = bank_tile_shift(total_vecs, with_vecs, (uint64_t)resident);
	const uint64_t T = (uint64_t)1 << shift;
	uint64_t ntiles = 0;
	for (const Stream &st : streams)
		ntiles += (st.nvec + T - 1) / T;
	// (at most two edges per stream: the edge list and its samples stay
	// within 32 bits as well)
	if (ntiles > 0xffffffffull || streams.size() > 0x0fffffffull)
		return CORDIC_ERR_ARGS;
	// (the streams are in address order and do not overlap: so are the tiles)
	std::vector<OscTile> tiles;
	std::vector<OscEdge> edges;
	tiles.reserve((size_t)ntiles);
	uint64_t edge_samples = 0;
	for (const Stream &st : streams) {
		if (st.head) {
			edges.push_back(OscEdge{st.addr, 0u, (uint32_t)st.head, st.job, st.lead});
			edge_samples += st.head;
		}
		for (uint64_t v0 = 0; v0 < st.nvec; v0 += T) {
			const uint64_t live = st.nvec - v0 < T ? st.nvec - v0 : T;
			const uint64_t first = st.head + v0 * W;
			tiles.push_back(OscTile{st.addr + first * esize, (uint32_t)first,
				(uint32_t)live, st.job, st.lead});
		}
		const uint64_t done = st.head + st.nvec * W;
		if (done < st.n) {
			edges.push_back(OscEdge{st.addr + done * esize, (uint32_t)done,
				(uint32_t)(st.n - done), st.job, st.lead});
			edge_samples += st.n - done;
		}
	}
	cordic_oscbank *b = new (std::nothrow) cordic_oscbank;
	if (!b)
		return CORDIC_ERR_NOMEM;
	b->core = core;
	b->queues = queues;
	b->io16 = io16;
	b->samples = samples;
	b->edge_samples = (uint32_t)edge_samples;
	b->tunings.resize(njobs);
	for (size_t k = 0; k < njobs; k++)
		b->tunings[k] = cordic_osc_tuning{jobs[k].phase0, jobs[k].fcw, jobs[k].index0};
	b->device = current_device();
	if (!dev_upload(tiles.data(), tiles.size() * sizeof(OscTile), &b->d_tiles)
			|| !dev_upload(edges.data(), edges.size() * sizeof(OscEdge), &b->d_edges)
			|| !dev_upload(b->tunings.data(), njobs * sizeof(cordic_osc_tuning),
				&b->d_tunings)) {
		cordic_oscbank_destroy(b);
		return CORDIC_ERR_DEVICE;
	}
	b->tabs.tiles = b->d_tiles;
	b->tabs.edges = b->d_edges;
	b->tabs.tunings = b->d_tunings;
	b->tabs.ntiles = (uint32_t)tiles.size();
	b->tabs.nedges = (uint32_t)edges.size();
	b->tabs.tile_shift = shift;
	*out = b;
	return CORDIC_OK;
}

int oscbank_create16(const SineCore &core, const QueueRing *queues, size_t njobs,
		const cordic_osc_job16 *jobs, cordic_oscbank **out)
{
	static_assert(sizeof(cordic_osc_job16) == sizeof(cordic_osc_job)
		&& offsetof(cordic_osc_job16, phase0) == offsetof(cordic_osc_job, phase0)
		&& offsetof(cordic_osc_job16, fcw) == offsetof(cordic_osc_job, fcw)
		&& offsetof(cordic_osc_job16, index0) == offsetof(cordic_osc_job, index0)
		&& offsetof(cordic_osc_job16, n) == offsetof(cordic_osc_job, n)
		&& offsetof(cordic_osc_job16, d_sin) == offsetof(cordic_osc_job, d_sin)
		&& offsetof(cordic_osc_job16, d_cos) == offsetof(cordic_osc_job, d_cos),
		"cordic_osc_job16 is cordic_osc_job with 16-bit sample pointers");
	if (!out || (njobs && !jobs))
		return CORDIC_ERR_ARGS;
	// same layout; the pointers are never dereferenced on the host and every
	// address is computed in bytes
	std::vector<cordic_osc_job> wide(njobs);
	for (size_t k = 0; k < njobs; k++) {
		const cordic_osc_job16 &a = jobs[k];
		wide[k] = cordic_osc_job{a.phase0, a.fcw, a.index0, a.n,
			reinterpret_cast<int32_t *>(a.d_sin), reinterpret_cast<int32_t *>(a.d_cos)};
	}
	return oscbank_create(core, queues, njobs, wide.data(), out, true);
}

} // namespace

int cordic_table_bank_create(const cordic_table *tbl, size_t njobs,
		const cordic_osc_job *jobs, cordic_oscbank **bank)
{
	if (!tbl)
		return CORDIC_ERR_ARGS;
	return oscbank_create(tbl->core(), &tbl->queues, njobs, jobs, bank, false);
}

int cordic_table_bank_create16(const cordic_table *tbl, size_t njobs,
		const cordic_osc_job16 *jobs, cordic_oscbank **bank)
{
	if (!tbl)
		return CORDIC_ERR_ARGS;
	return oscbank_create16(tbl->core(), &tbl->queues, njobs, jobs, bank);
}

int cordic_quad_bank_create(const cordic_quad *core, size_t njobs,
		const cordic_osc_job *jobs, cordic_oscbank **bank)
{
	if (!core)
		return CORDIC_ERR_ARGS;
	return oscbank_create(core->core(), &core->queues, njobs, jobs, bank, false);
}

int cordic_quad_bank_create16(const cordic_quad *core, size_t njobs,
		const cordic_osc_job16 *jobs, cordic_oscbank **bank)
{
	if (!core)
		return CORDIC_ERR_ARGS;
	return oscbank_create16(core->core(), &core->queues, njobs, jobs, bank);
}

void cordic_oscbank_destroy(cordic_oscbank *bank)
{
	if (!bank)
		return;
	dev_free(bank->d_tiles, bank->d_edges, bank->d_tunings);
	delete bank;
}

int cordic_oscbank_info(const cordic_oscbank *bank, uint64_t *samples,
		uint32_t *tiles, uint32_t *edge_samples)
{
	if (!bank)
		return CORDIC_ERR_ARGS;
	if (samples) *samples = bank->samples;
	if (tiles) *tiles = bank->tabs.ntiles;
	if (edge_samples) *edge_samples = bank->edge_samples;
	return CORDIC_OK;
}

int cordic_oscbank_run(const cordic_oscbank *bank, uint64_t index_offset,
		void *stream)
{
	if (!bank)
		return CORDIC_ERR_ARGS;
	if (int rc = device_is_current(bank->device))
		return rc;
	if (bank->samples == 0)
		return CORDIC_OK;
	// (PW <= 32: the low 32 bits of a sample index are all that matters)
	const uint32_t off = (uint32_t)index_offset;
	return with_queue(*bank->queues, stream, [&](uint32_t *q) {
		return launch_sine_bank(bank->core, bank->tabs, off, bank->io16, stream, q);
	});
}

int cordic_oscbank_retune(cordic_oscbank *bank, size_t first, size_t count,
		const cordic_osc_tuning *tunings, void *stream)
{
	if (!bank || first > bank->tunings.size()
			|| count > bank->tunings.size() - first || (count && !tunings))
		return CORDIC_ERR_ARGS;
	if (int rc = device_is_current(bank->device))
		return rc;
	bool query_failed = false;
	const bool capturing = stream_capturing(stream, &query_failed);
	if (query_failed)
		return CORDIC_ERR_DEVICE;
	if (capturing)
		return CORDIC_ERR_UNSUPPORTED;
	if (count == 0)
		return CORDIC_OK;
	std::copy(tunings, tunings + count, bank->tunings.begin() + (long)first);
	if (hipMemcpyAsync(bank->d_tunings + first, bank->tunings.data() + first,
			count * sizeof(cordic_osc_tuning), hipMemcpyHostToDevice,
			static_cast<hipStream_t>(stream)) != hipSuccess) {
		(void)hipGetLastError();
		return CORDIC_ERR_DEVICE;
	}
	return CORDIC_OK;
}

// ---------------------------------------------------- FM oscillator banks
// Many modulated oscillator jobs of one table / quadratic core in two launches
// (include/cordic_amd.h, "FM oscillator banks"; the cutter and the kernels:
// cordic_table_fm_bank.h, cordic_table_fm_bank.hip).  There is no one-by-one
// path: every core the single call serves is served from the span table.
struct cordic_fmbank {
	SineCore core;		// the handle's: it must outlive the bank
	int	device = -1, cus = 0;	// (cus: of the device, at create)
	bool	io16 = false;		// the jobs' outputs hold int16
	uint64_t samples = 0;
	uint32_t tiles = 0;		// T, the tiles of a base span
	SpanTable<FmSpan> spans;
};

namespace {
// all four creates: `h` is the table or quadratic handle, `jobs` either job
// struct (FmJobs, cordic_table_fm_bank.h)
template <typename H>
int fmbank_create(const H *h, size_t njobs, FmJobs jobs, cordic_fmbank **bank)
{
	const bool io16 = jobs.j16 != nullptr;	// (no jobs at all: the 32-bit rules)
	if (!h || !bank || (njobs && jobs.none()))
		return CORDIC_ERR_ARGS;
	const SineCore core = h->core();
	if (io16 && core.ow() > 16)
		return CORDIC_ERR_CONTAINER;
	if (core.quad && core.lds_bytes() > 64 * 1024)
		return CORDIC_ERR_UNSUPPORTED;
	if (!core.sane() || njobs >= ((size_t)1 << 28) || !fmob_jobs_valid(njobs, jobs))
		return CORDIC_ERR_ARGS;
	(void)hipGetLastError();	// (a stale error is not this call's)
	if (legacy_stream_capturing())	// (blocking uploads below)
		return CORDIC_ERR_UNSUPPORTED;
	uint64_t samples = 0, tiles = 0;
	for (size_t k = 0; k < njobs; k++) {
		samples += jobs.n(k) * (jobs.n(k) && jobs.quadrature(k) ? 2u : 1u);
		tiles += span_units_of(kFmobRule, jobs.n(k));
	}
	const int cus = cus_or_256();
	int per_cu = 1;
	if (tiles)
		if (int rc = fmob_resident(core, io16, &per_cu))
			return rc;
	cordic_fmbank *b = new (std::nothrow) cordic_fmbank;
	if (!b)
		return CORDIC_ERR_NOMEM;
	b->core = core;
	b->device = current_device();
	b->cus = cus;
	b->io16 = io16;
	b->samples = samples;
	if (int rc = span_table_build(&b->spans, "CORDIC_FMOB_TILES",
			"CORDIC_FMOB_MAX_SPANS", kFmobRule, tiles, cus, per_cu, njobs, jobs,
			&b->tiles)) {
		cordic_fmbank_destroy(b);
		return rc;
	}
	*bank = b;
	return CORDIC_OK;
}
} // namespace

int cordic_table_fmbank_create(const cordic_table *tbl, size_t njobs,
		const cordic_fmosc_job *jobs, cordic_fmbank **bank)
{
	return fmbank_create(tbl, njobs, jobs, bank);
}

int cordic_table_fmbank_create16(const cordic_table *tbl, size_t njobs,
		const cordic_fmosc_job16 *jobs, cordic_fmbank **bank)
{
	return fmbank_create(tbl, njobs, jobs, bank);
}

int cordic_quad_fmbank_create(const cordic_quad *core, size_t njobs,
		const cordic_fmosc_job *jobs, cordic_fmbank **bank)
{
	return fmbank_create(core, njobs, jobs, bank);
}

int cordic_quad_fmbank_create16(const cordic_quad *core, size_t njobs,
		const cordic_fmosc_job16 *jobs, cordic_fmbank **bank)
{
	return fmbank_create(core, njobs, jobs, bank);
}

void cordic_fmbank_destroy(cordic_fmbank *bank)
{
	if (!bank)
		return;
	bank->spans.free();
	delete bank;
}

int cordic_fmbank_info(const cordic_fmbank *bank, uint64_t *samples,
		uint32_t *spans, int32_t *tile)
{
	if (!bank)
		return CORDIC_ERR_ARGS;
	if (samples) *samples = bank->samples;
	if (spans) *spans = bank->spans.nspans;
	if (tile) *tile = (int32_t)(bank->tiles * kFmobRule.unit);
	return CORDIC_OK;
}

int cordic_fmbank_run(const cordic_fmbank *bank, void *stream)
{
	if (!bank)
		return CORDIC_ERR_ARGS;
	(void)hipGetLastError();
	if (int rc = device_is_current(bank->device))
		return rc;
	const SpanTable<FmSpan> &t = bank->spans;
	return launch_fmosc_bank(bank->core, t.d_spans, t.nspans, t.start(), t.part(),
		bank->cus, bank->io16, stream);
}
