// cordic_abi_clocked.cpp -- the C ABI's clocked views of a core: the pipelined
// cores tick by tick (cordic_stream) and the sequential cores' handshake
// (cordic_seq); include/cordic_amd.h, kernels: cordic_stream.hip.
#include <hip/hip_runtime_api.h>

#include <new>
#include <vector>

#include "cordic_amd.h"
#include "cordic_devmem.h"
#include "cordic_internal.h"

using namespace cordic_amd;

// Scratch of the clocked views.  cordic_*_reserve sizes it up front; a *_ticks
// call that needs more grows it IN STREAM ORDER on the caller's stream
// (hipFreeAsync / hipMallocAsync): earlier kernels of that stream still see the
// old block, no other stream is stalled and nothing synchronises the device.
// (Not inside a stream capture: reserve first, then capture.)  `s` is either
// view's state: StreamState or SeqState.
template <typename S> static int grow_workspace(S &s, size_t need, void *stream)
{
	if (need <= s.ws_bytes)
		return CORDIC_OK;
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (s.ws && hipFreeAsync(s.ws, st) != hipSuccess)
		return CORDIC_ERR_DEVICE;
	s.ws = nullptr;
	s.ws_bytes = 0;
	if (hipMallocAsync(&s.ws, need, st) != hipSuccess) {
		s.ws = nullptr;
		return CORDIC_ERR_DEVICE;
	}
	s.ws_bytes = need;
	return CORDIC_OK;
}

// cordic_*_reserve: the same scratch, sized before the first *_ticks call
template <typename S> static int reserve_workspace(S &s, size_t need)
{
	if (need <= s.ws_bytes)
		return CORDIC_OK;
	// kernels of earlier calls may still be using the old scratch
	if (hipDeviceSynchronize() != hipSuccess)
		return CORDIC_ERR_DEVICE;
	dev_free(s.ws);
	s.ws_bytes = 0;
	if (hipMalloc(&s.ws, need) != hipSuccess)
		return CORDIC_ERR_DEVICE;
	s.ws_bytes = need;
	return CORDIC_OK;
}

// ------------------------------------------------- clocked view (stream)
struct cordic_stream {
	cordic_config cfg;
	StreamState st;
	int latency = 0;
};

void cordic_stream_destroy(cordic_stream *s)
{
	if (!s)
		return;
	StreamState &t = s->st;
	dev_free(t.hx, t.hy, t.hph, t.haux, t.epoch, t.born_phase, t.ws);
	delete s;
}

int cordic_stream_create(const cordic_config *cfg, cordic_stream **out)
{
	if (!cfg || !out)
		return CORDIC_ERR_ARGS;
	if (cfg->mode != CORDIC_P2R && cfg->mode != CORDIC_R2P)
		return CORDIC_ERR_MODE;
	if (!config_sane(*cfg))
		return CORDIC_ERR_ARGS;
	cordic_stream *s = new (std::nothrow) cordic_stream;
	if (!s)
		return CORDIC_ERR_NOMEM;
	s->cfg = *cfg;
	const int L = cfg->nstages + 2;
	s->latency = L;
	StreamState &t = s->st;
	bool ok = dev_zalloc(&t.hx, (size_t)L * 4) && dev_zalloc(&t.hy, (size_t)L * 4)
		&& dev_zalloc(&t.hph, (size_t)L * 4) && dev_zalloc(&t.haux, (size_t)L)
		&& dev_zalloc(&t.epoch, 4);
	// rtl/topolar.v:235-243 on cleared registers: the phase accumulator of a
	// stage born at reset still collects angle[i] of every live stage it
	// passes; after e enabled clocks the output register shows the one born
	// in register NSTAGES-e+1 (cordic_stream.hip).  Skipped stages
	// (rtl/topolar.v:217-225) add nothing.
	std::vector<uint32_t> born((size_t)L + 1, 0u);
	const uint32_t pmask = (cfg->pw >= 32) ? 0xffffffffu : ((1u << cfg->pw) - 1u);
	for (int e = 1; e <= L - 1; e++) {
		uint32_t acc = 0;
		for (int i = cfg->nstages - e + 1; i < cfg->nstages; i++)
			if (i >= 0 && i < cfg->nlive)
				acc += cfg->angle[i];
		born[(size_t)e] = acc & pmask;
	}
	ok = ok && dev_upload(born.data(), born.size() * 4, &t.born_phase);
	if (!ok) {
		cordic_stream_destroy(s);
		return CORDIC_ERR_DEVICE;
	}
	*out = s;
	return CORDIC_OK;
}

size_t cordic_stream_workspace(size_t ticks) { return stream_workspace_bytes(ticks); }

int cordic_stream_reserve(cordic_stream *s, size_t max_ticks)
{
	if (!s)
		return CORDIC_ERR_ARGS;
	return reserve_workspace(s->st, stream_workspace_bytes(max_ticks));
}

int cordic_stream_latency(const cordic_stream *s) { return s ? s->latency : CORDIC_ERR_ARGS; }

int cordic_stream_reset(cordic_stream *s, void *stream)
{
	if (!s)
		return CORDIC_ERR_ARGS;
	return (hipMemsetAsync(s->st.epoch, 0, 4,
			static_cast<hipStream_t>(stream)) == hipSuccess)
		? CORDIC_OK : CORDIC_ERR_DEVICE;
}

int cordic_stream_ticks(cordic_stream *s, size_t ticks, const uint8_t *d_ce,
		const uint8_t *d_reset, const uint8_t *d_aux, const int32_t *d_xval,
		const int32_t *d_yval, const uint32_t *d_phase, int32_t *d_out0,
		int32_t *d_out1, uint8_t *d_oaux, void *stream)
{
	if (!s)
		return CORDIC_ERR_ARGS;
	if (int rc = grow_workspace(s->st, stream_workspace_bytes(ticks), stream))
		return rc;
	return launch_stream_ticks(s->cfg, s->st, ticks, d_ce, d_reset, d_aux,
			d_xval, d_yval, d_phase, d_out0, d_out1, d_oaux, stream);
}

// ------------------------------------- handshake view, sequential cores
struct cordic_seq {
	cordic_config cfg;
	SeqState st;
};

void cordic_seq_destroy(cordic_seq *s)
{
	if (!s)
		return;
	SeqState &t = s->st;
	dev_free(t.c, t.px, t.py, t.pph, t.paux, t.l0, t.l1, t.la, t.violations,
			t.ws, t.lit);
	delete s;
}

int cordic_seq_create(const cordic_config *cfg, cordic_seq **out)
{
	if (!cfg || !out)
		return CORDIC_ERR_ARGS;
	if (cfg->mode != CORDIC_SP2R && cfg->mode != CORDIC_SR2P)
		return CORDIC_ERR_MODE;
	if (!config_sane(*cfg))
		return CORDIC_ERR_ARGS;
	cordic_seq *s = new (std::nothrow) cordic_seq;
	if (!s)
		return CORDIC_ERR_NOMEM;
	s->cfg = *cfg;
	SeqState &t = s->st;
	bool ok = dev_zalloc(&t.violations, 8) && dev_zalloc(&t.c, 4)
		&& dev_zalloc(&t.px, 4) && dev_zalloc(&t.py, 4) && dev_zalloc(&t.pph, 4)
		&& dev_zalloc(&t.paux, 4) && dev_zalloc(&t.l0, 4) && dev_zalloc(&t.l1, 4)
		&& dev_zalloc(&t.la, 4);
	// register-level state for off-protocol stretches: power-on registers
	// and the padded arctan table
	std::vector<unsigned char> image(seq_literal_bytes());
	seq_literal_init(*cfg, image.data());
	ok = ok && dev_upload(image.data(), image.size(), &t.lit);
	if (!ok) {
		cordic_seq_destroy(s);
		return CORDIC_ERR_DEVICE;
	}
	*out = s;
	return CORDIC_OK;
}

size_t cordic_seq_workspace(size_t ticks) { return seq_workspace_bytes(ticks); }

int cordic_seq_reserve(cordic_seq *s, size_t max_ticks)
{
	if (!s)
		return CORDIC_ERR_ARGS;
	return reserve_workspace(s->st, seq_workspace_bytes(max_ticks));
}

int cordic_seq_ticks(cordic_seq *s, size_t ticks, const uint8_t *d_stb,
		const uint8_t *d_reset, const uint8_t *d_aux, const int32_t *d_xval,
		const int32_t *d_yval, const uint32_t *d_phase, int32_t *d_out0,
		int32_t *d_out1, uint8_t *d_busy, uint8_t *d_done, uint8_t *d_oaux,
		void *stream)
{
	if (!s)
		return CORDIC_ERR_ARGS;
	if (int rc = grow_workspace(s->st, seq_workspace_bytes(ticks), stream))
		return rc;
	return launch_seq_ticks(s->cfg, s->st, ticks, d_stb, d_reset, d_aux, d_xval,
			d_yval, d_phase, d_out0, d_out1, d_busy, d_done, d_oaux,
			stream);
}

int cordic_seq_violations(cordic_seq *s, uint64_t *count)
{
	if (!s || !count)
		return CORDIC_ERR_ARGS;
	unsigned long long v = 0;
	if (hipDeviceSynchronize() != hipSuccess
			|| hipMemcpy(&v, s->st.violations, 8, hipMemcpyDeviceToHost)
				!= hipSuccess)
		return CORDIC_ERR_DEVICE;
	*count = v;
	return CORDIC_OK;
}
