// cordic_abi_fm.cpp -- the plan-side FM layer of the extern "C" surface
// (include/cordic_amd.h): the FM mixer and the decimating mixer, the FM mixer
// banks, the tuned FM receiver in all its forms (int32, int16, interleaved
// int16; plain and decimating) and the receiver banks.  The plan itself lives in
// cordic_abi.cpp (cordic_abi_plan.h).  Argument checks, the choice between a
// fused launcher (cordic_fm_mix.h, cordic_fm_rx.h and their banks' headers) and
// the fallback put together from other entry points, and that fallback's place
// inside d_work, by the layout functions next to the workspace rules.  A call's
// form -- container, interleaved, k -- travels as one FmForm (cordic_fm_mix.h).
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <new>
#include <vector>

#include "cordic_abi_plan.h"
#include "cordic_amd.h"
#include "cordic_bank_host.h"
#include "cordic_devmem.h"
#include "cordic_fm_mix.h"
#include "cordic_fm_mix_bank.h"
#include "cordic_fm_rx.h"
#include "cordic_fm_rx_decim.h"
#include "cordic_fm_rx_bank.h"
#include "cordic_internal.h"

using namespace cordic_amd;

constexpr FmForm kForm32 = {4, false, 0}, kForm16 = {2, false, 0}, kFormC16 = {2, true, 0};

// the form at k
static constexpr FmForm decim(FmForm f, uint32_t log2r)
{
	return FmForm{f.container, f.iq, log2r};
}

static unsigned char *bytes_at(void *d_work, size_t at)
{
	return static_cast<unsigned char *>(d_work) + at;
}

// <NAME>=1 in the environment: a test and A/B knob, read where it is asked
static bool knob_set(const char *name)
{
	const char *e = std::getenv(name);
	return e && e[0] == '1';
}

// ---- the FM mixer: per-sample tuning words accumulated inside the rotator
// (cordic_fm_mix.h)
static int fm_mix_plan_ok(const cordic_plan *plan)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	if (plan->cfg.mode != CORDIC_P2R && plan->cfg.mode != CORDIC_SP2R)
		return CORDIC_ERR_MODE;
	return config_sane(plan->cfg) ? CORDIC_OK : CORDIC_ERR_ARGS;
}

// the plan, its mode, then the container (the tuning words stay 32-bit: any PW)
static int fm_mix_ok(const cordic_plan *plan, FmForm f)
{
	if (int rc = fm_mix_plan_ok(plan))
		return rc;
	return f.io16() ? fits16(plan->cfg, false) : CORDIC_OK;
}

// the mixer's own call, k = 0, on the form's container: its path ...
static bool fm_mix_fused(const cordic_plan *plan, FmForm f)
{
	return f.io16() ? fmx_is_fused16(plan->cfg, plan->d_dir, plan->dx)
		: fmx_is_fused(plan->cfg, plan->d_dir, plan->dx);
}

// ... and its workspace
static size_t fm_mix_work_bytes(const cordic_plan *plan, FmForm f, size_t n)
{
	return f.io16() ? fmx16_work_bytes(fm_mix_fused(plan, kForm16), fm_mix_fused(plan, kForm32), n)
		: fmx_work_bytes(fm_mix_fused(plan, kForm32), n);
}

size_t cordic_plan_fm_mix_workspace(const cordic_plan *plan, size_t n)
{
	if (fm_mix_ok(plan, kForm32) != CORDIC_OK)
		return 0;
	return fm_mix_work_bytes(plan, kForm32, n);
}

int cordic_plan_fm_mix_info(const cordic_plan *plan, int32_t *fused, int32_t *tile)
{
	if (int rc = fm_mix_plan_ok(plan))
		return rc;
	const bool f = fm_mix_fused(plan, kForm32);
	if (fused)
		*fused = f ? 1 : 0;
	if (tile)
		*tile = f ? (int32_t)kFmxPass : 0;
	return CORDIC_OK;
}

int cordic_plan_fm_mix(const cordic_plan *plan, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc,
		const int32_t *d_xval, const int32_t *d_yval, int32_t *d_oxval,
		int32_t *d_oyval, void *d_work, void *stream)
{
	if (int rc = fm_mix_plan_ok(plan))
		return rc;
	if (n == 0)
		return CORDIC_OK;
	const bool fused = fm_mix_fused(plan, kForm32);
	if (int rc = fmx_check_call(n, d_fcw, d_pm, d_acc, d_xval, d_yval, d_oxval,
			d_oyval, 4, d_work, fmx_work_bytes(fused, n)))
		return rc;
	if (fused)
		return launch_fm_mix(plan->cfg, plan->d_dir, plan->dx, n, d_fcw, d_pm,
			phase0, d_acc, d_xval, d_yval, d_oxval, d_oyval, 4, d_work, stream);
	// the fallback: the phases into the workspace, behind the accumulator's own
	// scratch, and the rotator on them
	uint32_t *ph = reinterpret_cast<uint32_t *>(bytes_at(d_work, kFmxPhaseAt));
	if (int rc = cordic_phase_accumulate(n, d_fcw, d_pm, phase0, d_acc, ph, d_work,
			stream))
		return rc;
	return cordic_plan_p2r(plan, n, d_xval, d_yval, ph, d_oxval, d_oyval, stream);
}

// ---- the same on int16 I/Q arrays
size_t cordic_plan_fm_mix16_workspace(const cordic_plan *plan, size_t n)
{
	if (fm_mix_ok(plan, kForm16) != CORDIC_OK)
		return 0;
	return fm_mix_work_bytes(plan, kForm16, n);
}

int cordic_plan_fm_mix16(const cordic_plan *plan, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc,
		const int16_t *d_xval, const int16_t *d_yval, int16_t *d_oxval,
		int16_t *d_oyval, void *d_work, void *stream)
{
	if (int rc = fm_mix_ok(plan, kForm16))
		return rc;
	if (n == 0)
		return CORDIC_OK;
	if (int rc = fmx_check_call(n, d_fcw, d_pm, d_acc, d_xval, d_yval, d_oxval,
			d_oyval, 2, d_work, fm_mix_work_bytes(plan, kForm16, n)))
		return rc;
	if (fm_mix_fused(plan, kForm16))
		return launch_fm_mix(plan->cfg, plan->d_dir, plan->dx, n, d_fcw, d_pm,
			phase0, d_acc, d_xval, d_yval, d_oxval, d_oyval, 2, d_work, stream);
	// the fallback: the 32-bit call on widened copies, all of it in d_work, and
	// the low halves of what it wrote
	const Fmx16Layout at = fmx16_layout(fm_mix_work_bytes(plan, kForm32, n), n);
	int32_t *wx = reinterpret_cast<int32_t *>(bytes_at(d_work, at.x));
	int32_t *wy = reinterpret_cast<int32_t *>(bytes_at(d_work, at.y));
	int32_t *wox = reinterpret_cast<int32_t *>(bytes_at(d_work, at.ox));
	int32_t *woy = reinterpret_cast<int32_t *>(bytes_at(d_work, at.oy));
	if (int rc = launch_fmx_widen(n, d_xval, d_yval, wx, wy, stream))
		return rc;
	if (int rc = cordic_plan_fm_mix(plan, n, d_fcw, d_pm, phase0, d_acc, wx, wy, wox,
			woy, d_work, stream))
		return rc;
	return launch_fmx_narrow(n, wox, woy, d_oxval, d_oyval, stream);
}

// cordic_plan_fm_mix or cordic_plan_fm_mix16, by the form's container
static int fm_mix_call(const cordic_plan *plan, FmForm f, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, const void *d_xval,
		const void *d_yval, void *d_oxval, void *d_oyval, void *d_work, void *stream)
{
	if (f.io16())
		return cordic_plan_fm_mix16(plan, n, d_fcw, d_pm, phase0, d_acc,
			static_cast<const int16_t *>(d_xval), static_cast<const int16_t *>(d_yval),
			static_cast<int16_t *>(d_oxval), static_cast<int16_t *>(d_oyval), d_work,
			stream);
	return cordic_plan_fm_mix(plan, n, d_fcw, d_pm, phase0, d_acc,
		static_cast<const int32_t *>(d_xval), static_cast<const int32_t *>(d_yval),
		static_cast<int32_t *>(d_oxval), static_cast<int32_t *>(d_oyval), d_work,
		stream);
}

// ---- the decimating mixer: integrate-and-dump by 2^log2r behind the rotator
// (cordic_fm_mix.h), on either container.  CORDIC_FMXD_FALLBACK=1 in the
// environment (read at every single call and workspace query; a test and A/B
// knob) sends a fused plan's single call through the fallback.  The workspace
// grows with it and a call cannot see the size of the caller's buffer, so it
// has to be set before the query as well as before the call, as
// tools/bench_fm_mix_decim.py does.  Banks ignore it.
static bool fm_mix_decim_fused(const cordic_plan *plan, FmForm f)
{
	if (knob_set("CORDIC_FMXD_FALLBACK"))
		return false;
	return fm_mix_fused(plan, f);
}

// a plan that the call accepts; 0 where the call would fail.  (k = 0: the
// mixer's own workspace, whatever `fused` says.)  An interleaved form: the
// twin's where it is fused, else the twin's fallback with the four split arrays
// behind it (fmx_c16_layout).
static size_t fm_mix_decim_work_bytes(const cordic_plan *plan, FmForm f, bool fused,
		size_t n)
{
	if (f.iq) {
		const bool fu = f.log2r ? fused : fm_mix_fused(plan, f);
		const size_t twin = fm_mix_decim_work_bytes(plan, f.split(), fu, n);
		return twin ? fmx_c16_work_bytes(fu, twin, n, f.log2r) : 0;
	}
	const size_t mix = fm_mix_work_bytes(plan, f, n);
	if (!fmxd_shape_ok(n, f.log2r))
		return 0;
	return f.log2r ? fmxd_work_bytes(fused, mix, n, f.esize()) : mix;
}

static int fm_mix_decim(const cordic_plan *plan, FmForm f, size_t n,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc,
		const void *d_xval, const void *d_yval, void *d_oxval, void *d_oyval,
		void *d_work, void *stream, bool fused);

// The interleaved forms (f.iq; the shape is checked): d_iq and d_oiq.  k = 0 is
// the plain call, on the plan's own path; `fused` is a decimating call's.
static int fm_mix_iq(const cordic_plan *plan, FmForm f, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, const void *d_iq,
		void *d_oiq, void *d_work, void *stream, bool fused)
{
	if (n == 0)
		return CORDIC_OK;
	if (!f.log2r)
		fused = fm_mix_fused(plan, f);
	if (int rc = fmx_check_call(n, d_fcw, d_pm, d_acc, d_iq, nullptr, d_oiq, nullptr,
			f.esize(), d_work, fm_mix_decim_work_bytes(plan, f, fused, n), f.log2r, true))
		return rc;
	if (fused)
		return launch_fm_mix(plan->cfg, plan->d_dir, plan->dx, n, d_fcw, d_pm, phase0,
			d_acc, d_iq, nullptr, d_oiq, nullptr, f.esize(), d_work, stream, f.log2r, true);
	// the fallback: one split launch into two arrays behind the twin's
	// workspace, the twin itself from them into two more, one interleave launch
	const FmForm twin = f.split();
	const FmxC16Layout at = fmx_c16_layout(fm_mix_decim_work_bytes(plan, twin, false, n), n,
		f.log2r);
	int16_t *x = reinterpret_cast<int16_t *>(bytes_at(d_work, at.x));
	int16_t *y = reinterpret_cast<int16_t *>(bytes_at(d_work, at.y));
	int16_t *ox = reinterpret_cast<int16_t *>(bytes_at(d_work, at.ox));
	int16_t *oy = reinterpret_cast<int16_t *>(bytes_at(d_work, at.oy));
	if (int rc = launch_fmrx_split_c16(n, static_cast<const int16_t *>(d_iq), x, y, stream))
		return rc;
	if (int rc = fm_mix_decim(plan, twin, n, d_fcw, d_pm, phase0, d_acc, x, y, ox, oy,
			d_work, stream, false))
		return rc;
	return launch_fmx_interleave_c16(n >> f.log2r, ox, oy, static_cast<int16_t *>(d_oiq),
		stream);
}

// f.iq: d_xval is d_iq, d_oxval is d_oiq, d_yval and d_oyval are not looked at
static int fm_mix_decim(const cordic_plan *plan, FmForm f, size_t n,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc,
		const void *d_xval, const void *d_yval, void *d_oxval, void *d_oyval,
		void *d_work, void *stream, bool fused)
{
	if (!fmxd_shape_ok(n, f.log2r))
		return CORDIC_ERR_ARGS;
	if (f.iq)
		return fm_mix_iq(plan, f, n, d_fcw, d_pm, phase0, d_acc, d_xval, d_oxval, d_work,
			stream, fused);
	if (f.log2r == 0 || n == 0)	// the mixer itself: its bits, its launches
		return fm_mix_call(plan, f, n, d_fcw, d_pm, phase0, d_acc, d_xval, d_yval,
			d_oxval, d_oyval, d_work, stream);
	if (int rc = fmx_check_call(n, d_fcw, d_pm, d_acc, d_xval, d_yval, d_oxval, d_oyval,
			f.esize(), d_work, fm_mix_decim_work_bytes(plan, f, fused, n), f.log2r))
		return rc;
	if (fused)
		return launch_fm_mix(plan->cfg, plan->d_dir, plan->dx, n, d_fcw, d_pm, phase0,
			d_acc, d_xval, d_yval, d_oxval, d_oyval, f.esize(), d_work, stream, f.log2r);
	// the fallback: the mixer's call into two full-rate arrays behind its own
	// workspace, then the sums
	const FmxdLayout at = fmxd_layout(fm_mix_work_bytes(plan, f, n), n, f.esize());
	void *tx = bytes_at(d_work, at.tx), *ty = bytes_at(d_work, at.ty);
	if (int rc = fm_mix_call(plan, f, n, d_fcw, d_pm, phase0, d_acc, d_xval, d_yval, tx,
			ty, d_work, stream))
		return rc;
	return launch_fmx_decimate(n, f.log2r, f.esize(), tx, ty, d_oxval, d_oyval, stream);
}

size_t cordic_plan_fm_mix_decim_workspace(const cordic_plan *plan, size_t n, uint32_t log2r)
{
	const FmForm f = decim(kForm32, log2r);
	if (fm_mix_ok(plan, f) != CORDIC_OK)
		return 0;
	return fm_mix_decim_work_bytes(plan, f, fm_mix_decim_fused(plan, f), n);
}

size_t cordic_plan_fm_mix_decim16_workspace(const cordic_plan *plan, size_t n,
		uint32_t log2r)
{
	const FmForm f = decim(kForm16, log2r);
	if (fm_mix_ok(plan, f) != CORDIC_OK)
		return 0;
	return fm_mix_decim_work_bytes(plan, f, fm_mix_decim_fused(plan, f), n);
}

int cordic_plan_fm_mix_decim(const cordic_plan *plan, size_t n, uint32_t log2r,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc,
		const int32_t *d_xval, const int32_t *d_yval, int32_t *d_oxval,
		int32_t *d_oyval, void *d_work, void *stream)
{
	const FmForm f = decim(kForm32, log2r);
	if (int rc = fm_mix_ok(plan, f))
		return rc;
	return fm_mix_decim(plan, f, n, d_fcw, d_pm, phase0, d_acc, d_xval, d_yval, d_oxval,
		d_oyval, d_work, stream, fm_mix_decim_fused(plan, f));
}

int cordic_plan_fm_mix_decim16(const cordic_plan *plan, size_t n, uint32_t log2r,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc,
		const int16_t *d_xval, const int16_t *d_yval, int16_t *d_oxval,
		int16_t *d_oyval, void *d_work, void *stream)
{
	const FmForm f = decim(kForm16, log2r);
	if (int rc = fm_mix_ok(plan, f))
		return rc;
	return fm_mix_decim(plan, f, n, d_fcw, d_pm, phase0, d_acc, d_xval, d_yval, d_oxval,
		d_oyval, d_work, stream, fm_mix_decim_fused(plan, f));
}

// ---- the mixer on interleaved int16 I/Q, in and out: the *16 twins with d_iq
// and d_oiq in the place of the four sample pointers (cordic_fm_mix.h)
int cordic_plan_fm_mix_c16_info(const cordic_plan *plan, int32_t *fused, int32_t *tile)
{
	if (int rc = fm_mix_ok(plan, kFormC16))
		return rc;
	const bool f = fm_mix_fused(plan, kFormC16);
	if (fused)
		*fused = f ? 1 : 0;
	if (tile)
		*tile = f ? (int32_t)kFmxPass : 0;
	return CORDIC_OK;
}

size_t cordic_plan_fm_mix_decim_c16_workspace(const cordic_plan *plan, size_t n,
		uint32_t log2r)
{
	const FmForm f = decim(kFormC16, log2r);
	if (fm_mix_ok(plan, f) != CORDIC_OK)
		return 0;
	return fm_mix_decim_work_bytes(plan, f, fm_mix_decim_fused(plan, f), n);
}

size_t cordic_plan_fm_mix_c16_workspace(const cordic_plan *plan, size_t n)
{
	return cordic_plan_fm_mix_decim_c16_workspace(plan, n, 0);
}

int cordic_plan_fm_mix_decim_c16(const cordic_plan *plan, size_t n, uint32_t log2r,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc,
		const int16_t *d_iq, int16_t *d_oiq, void *d_work, void *stream)
{
	const FmForm f = decim(kFormC16, log2r);
	if (int rc = fm_mix_ok(plan, f))
		return rc;
	return fm_mix_decim(plan, f, n, d_fcw, d_pm, phase0, d_acc, d_iq, nullptr, d_oiq,
		nullptr, d_work, stream, fm_mix_decim_fused(plan, f));
}

int cordic_plan_fm_mix_c16(const cordic_plan *plan, size_t n, const uint32_t *d_fcw,
		const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, const int16_t *d_iq,
		int16_t *d_oiq, void *d_work, void *stream)
{
	return cordic_plan_fm_mix_decim_c16(plan, n, 0, d_fcw, d_pm, phase0, d_acc, d_iq,
		d_oiq, d_work, stream);
}

// ---- FM mixer banks: many of those jobs in two launches
// (cordic_fm_mix_bank.h)
struct cordic_mixbank : BankHandle<cordic_fmmix_job> {
	const cordic_plan *plan = nullptr;	// the caller's; outlives the bank
	FmForm	form;				// the jobs' container; iq: d_xval / d_oxval are
						// interleaved I/Q (_c16); log2r > 0: a decimating bank
	uint32_t passes = 0;
	SpanTable<MixSpan> spans;		// fused
};

// The create of the two plan-side banks (mixer, receiver), 32- and 16-bit:
// `jobs` is the bank's view of either job struct (MixJobs, RxJobs), `form` what
// they say of every call, `core_ok` the check of the plan (and converter),
// `fused` the whole bank's path, `work_bytes` a job's workspace one by one,
// `finish` what a fused bank still needs behind its span table.  TR
// (MixBankTraits, RxBankTraits, next to the views): the job check, the span rule
// (of the view: a decimating receiver bank's halo follows its k), the knobs'
// names, the blocks per CU.
// The checks come in this order, each bank's documented order of status codes.
template <typename TR, typename Bank, typename Jobs, typename Ok, typename Fused,
	typename Work, typename Finish>
static int plan_bank_create(const cordic_plan *plan, size_t njobs, Jobs jobs, FmForm form,
		Bank **bank, Ok core_ok, Fused fused, Work work_bytes, void (*destroy)(Bank *),
		Finish finish)
{
	if (!bank || (njobs && jobs.none()))
		return CORDIC_ERR_ARGS;
	if (int rc = core_ok())
		return rc;
	if (njobs >= ((size_t)1 << 28) || !TR::jobs_valid(njobs, jobs))
		return CORDIC_ERR_ARGS;
	(void)hipGetLastError();	// (a stale error is not this call's)
	// the handle keeps its jobs in the 32-bit struct, whatever the container
	typedef typename decltype(Bank::jobs)::value_type Job;
	std::vector<Job> wide;
	const Job *flat = jobs.j32;
	if (form.io16()) {
		wide.reserve(njobs);
		for (size_t k = 0; k < njobs; k++)
			wide.push_back(jobs[k]);
		flat = wide.data();
	}
	Bank *b = nullptr;
	if (int rc = bank_begin(njobs, flat, fused(), work_bytes, &b))
		return rc;
	b->plan = plan;
	b->form = form;
	int rc = CORDIC_OK;
	if (b->fused) {
		const SpanRule rule = TR::rule_of(jobs);
		uint64_t passes = 0;
		for (size_t k = 0; k < njobs; k++)
			passes += span_units_of(rule, jobs.n(k));
		rc = span_table_build(&b->spans, TR::passes, TR::max_spans, rule, passes,
			b->cus, TR::blocks_per_cu, njobs, jobs, &b->passes);
	}
	if (!rc)
		rc = finish(b);
	if (rc) {
		destroy(b);
		return rc;
	}
	*bank = b;
	return CORDIC_OK;
}

// all six creates: `jobs` is either job struct (MixJobs, cordic_fm_mix_bank.h;
// no jobs at all: the 32-bit rules)
static int mixbank_create(const cordic_plan *plan, size_t njobs, MixJobs jobs,
		cordic_mixbank **bank)
{
	const FmForm f = {jobs.j16 ? 2u : 4u, jobs.iq, jobs.log2r};
	return plan_bank_create<MixBankTraits>(plan, njobs, jobs, f, bank,
		[&] { return fm_mix_ok(plan, f); }, [&] { return fm_mix_fused(plan, f); },
		[&](size_t n) { return fm_mix_decim_work_bytes(plan, f, false, n); },
		cordic_mixbank_destroy, [](cordic_mixbank *) { return CORDIC_OK; });
}

int cordic_mixbank_create(const cordic_plan *plan, size_t njobs,
		const cordic_fmmix_job *jobs, cordic_mixbank **bank)
{
	return mixbank_create(plan, njobs, jobs, bank);
}

int cordic_mixbank_create16(const cordic_plan *plan, size_t njobs,
		const cordic_fmmix_job16 *jobs, cordic_mixbank **bank)
{
	return mixbank_create(plan, njobs, jobs, bank);
}

int cordic_mixbank_create_decim(const cordic_plan *plan, uint32_t log2r, size_t njobs,
		const cordic_fmmix_job *jobs, cordic_mixbank **bank)
{
	return mixbank_create(plan, njobs, MixJobs(jobs, log2r), bank);
}

int cordic_mixbank_create_decim16(const cordic_plan *plan, uint32_t log2r, size_t njobs,
		const cordic_fmmix_job16 *jobs, cordic_mixbank **bank)
{
	return mixbank_create(plan, njobs, MixJobs(jobs, log2r), bank);
}

// the interleaved creates: the jobs as 16-bit ones whose d_xval is d_iq and
// whose d_oxval is d_oiq (fmxb_from_c16); the checks keep mixbank_create's order
static int mixbank_create_c16(const cordic_plan *plan, uint32_t log2r, size_t njobs,
		const cordic_fmmix_job_c16 *jobs, cordic_mixbank **bank)
{
	if (!bank || (njobs && !jobs))
		return CORDIC_ERR_ARGS;
	// the plan, its mode and its container, then the count, as mixbank_create
	// has them -- in front of the copy, which is then at most 2^28 jobs
	if (int rc = fm_mix_ok(plan, kFormC16))
		return rc;
	if (njobs >= ((size_t)1 << 28))
		return CORDIC_ERR_ARGS;
	std::vector<cordic_fmmix_job16> split;
	try {
		split.resize(njobs + 1);
	} catch (const std::bad_alloc &) {	// (nothing is thrown across the C ABI)
		return CORDIC_ERR_NOMEM;
	}
	for (size_t k = 0; k < njobs; k++)
		split[k] = fmxb_from_c16(jobs[k]);
	// (NULL jobs with njobs == 0: NULL on, as _create16 would see it)
	const cordic_fmmix_job16 *j16 = jobs ? split.data() : nullptr;
	return mixbank_create(plan, njobs, MixJobs(j16, log2r, true), bank);
}

int cordic_mixbank_create_c16(const cordic_plan *plan, size_t njobs,
		const cordic_fmmix_job_c16 *jobs, cordic_mixbank **bank)
{
	return mixbank_create_c16(plan, 0, njobs, jobs, bank);
}

int cordic_mixbank_create_decim_c16(const cordic_plan *plan, uint32_t log2r, size_t njobs,
		const cordic_fmmix_job_c16 *jobs, cordic_mixbank **bank)
{
	return mixbank_create_c16(plan, log2r, njobs, jobs, bank);
}

void cordic_mixbank_destroy(cordic_mixbank *bank)
{
	if (!bank)
		return;
	bank->spans.free();
	dev_free(bank->d_work);
	delete bank;
}

int cordic_mixbank_info(const cordic_mixbank *bank, uint64_t *samples,
		uint32_t *spans, int32_t *fused, int32_t *tile)
{
	if (!bank)
		return CORDIC_ERR_ARGS;
	if (samples) *samples = bank->samples;
	if (spans) *spans = bank->spans.nspans;
	if (fused) *fused = bank->fused ? 1 : 0;
	if (tile) *tile = bank->fused ? (int32_t)(bank->passes * kFmxbRule.unit) : 0;
	return CORDIC_OK;
}

int cordic_mixbank_run(const cordic_mixbank *bank, void *stream)
{
	if (!bank)
		return CORDIC_ERR_ARGS;
	(void)hipGetLastError();
	const cordic_plan *plan = bank->plan;
	const FmForm f = bank->form;
	return bank_run(*bank, [&] {
		const SpanTable<MixSpan> &t = bank->spans;
		return launch_fmx_bank(plan->cfg, plan->d_dir, plan->dx, t.d_spans, t.nspans,
			t.start(), t.part(), bank->cus, f.io16(), stream, f.log2r, f.iq);
	}, [&](const cordic_fmmix_job &jb) {
		// (log2r 0: the mixer's own call, cordic_plan_fm_mix or _mix16; an
		// interleaved job's d_xval / d_oxval carry its d_iq / d_oiq)
		return fm_mix_decim(plan, f, (size_t)jb.n, jb.d_fcw, jb.d_pm, jb.phase0,
			jb.d_acc, jb.d_xval, jb.d_yval, jb.d_oxval, jb.d_oyval, bank->d_work, stream,
			false);
	});
}

// ---- the tuned FM receiver: that mixer and the FM discriminator in one kernel
// (cordic_fm_rx.h), with the integrate-and-dump by 2^k between them where the
// form has a k (cordic_fm_rx_decim.h), on int32, int16 or -- the *_c16 forms,
// the *16 twins with d_iq in the place of d_xval / d_yval -- interleaved int16
// input.  The status codes are those of the two calls, the mixer's first: the
// plan (ARGS, MODE), then the converter (ARGS, MODE, ARGS) and, for the 16-bit
// forms, the plan's container, then the converter's; then the shape, then the
// ranges.
static int fm_rx_ok(const cordic_plan *plan, const cordic_config *conv, FmForm f)
{
	if (!plan || !conv)
		return CORDIC_ERR_ARGS;
	if (int rc = fm_mix_plan_ok(plan))
		return rc;
	if (int rc = fmd_check_core(conv))
		return rc;
	if (!f.io16())
		return CORDIC_OK;
	if (int rc = fits16(plan->cfg, false))
		return rc;
	return fits16(*conv, true);
}

// The path of a single call.  Fused where the mixer is and the converter is
// served; an interleaved form where its twin is, with the twin's launches and
// workspace (the <30, IoC16> instances of launch 2).  CORDIC_FMRXD_FALLBACK=1 in
// the environment (read at every decimating single call and workspace query, as
// CORDIC_FMXD_FALLBACK is: set it before both) sends a fused pair's decimating
// call through the fallback; it does not reach k = 0, and banks ignore it
// (they ask at k = 0).
static bool fm_rx_fused(const cordic_plan *plan, const cordic_config *conv, FmForm f)
{
	if (f.log2r && knob_set("CORDIC_FMRXD_FALLBACK"))
		return false;
	return fm_mix_fused(plan, f) && fmrx_conv_is_fused(*conv);
}

// The workspace of a pair that the call accepts; 0 where the call would fail.
// Not fused: [the mixer call's workspace, as its _workspace query answers | the
// fallback's arrays], and for an interleaved form the split arrays behind that.
// one_by_one: of a bank that runs its jobs by this call -- the fallback's, at
// its largest, whatever the A/B knobs say at run.
static size_t fm_rx_work_bytes(const cordic_plan *plan, const cordic_config *conv,
		FmForm f, size_t n, bool one_by_one)
{
	if (!fmxd_shape_ok(n, f.log2r))
		return 0;
	const bool fused = !one_by_one && fm_rx_fused(plan, conv, f);
	const bool mix_fused = !one_by_one && f.log2r && fm_mix_decim_fused(plan, f);
	// (the mixer call of the fallback is the split one's, whatever the input)
	const size_t twin = fmrxd_work_bytes(fused,
		fm_mix_decim_work_bytes(plan, f.split(), mix_fused, n), n, f.log2r, f.esize());
	return f.iq ? fmrx_c16_work_bytes(fused, twin, n) : twin;
}

static size_t fm_rx_workspace(const cordic_plan *plan, const cordic_config *conv, FmForm f,
		size_t n)
{
	return fm_rx_ok(plan, conv, f) == CORDIC_OK ? fm_rx_work_bytes(plan, conv, f, n, false) : 0;
}

static int fm_rx_info(const cordic_plan *plan, const cordic_config *conv,
		int32_t *fused, int32_t *tile, FmForm f)
{
	if (int rc = fm_rx_ok(plan, conv, f))
		return rc;
	const bool fu = fm_rx_fused(plan, conv, f);
	if (fused)
		*fused = fu ? 1 : 0;
	if (tile)
		*tile = fu ? (int32_t)kFmrxPass : 0;
	return CORDIC_OK;
}

// cordic_fm_demod or cordic_fm_demod16, by the form's container
static int fm_demod_call(const cordic_config *conv, FmForm f, size_t n, const void *d_xval,
		const void *d_yval, uint32_t dphase0, uint32_t *d_last, void *d_omag,
		void *d_ofreq, void *d_work, void *stream)
{
	if (f.io16())
		return cordic_fm_demod16(conv, n, static_cast<const int16_t *>(d_xval),
			static_cast<const int16_t *>(d_yval), dphase0, d_last,
			static_cast<int16_t *>(d_omag), static_cast<int16_t *>(d_ofreq), d_work, stream);
	return cordic_fm_demod(conv, n, static_cast<const int32_t *>(d_xval),
		static_cast<const int32_t *>(d_yval), dphase0, d_last,
		static_cast<int32_t *>(d_omag), static_cast<int32_t *>(d_ofreq), d_work, stream);
}

// Every single call, and a bank's job run one by one.  f.iq: d_xval is d_iq and
// d_yval is not looked at.  k = 0 is the receiver itself: its bits, its launches.
static int fm_rx(const cordic_plan *plan, const cordic_config *conv, FmForm f, size_t n,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const void *d_xval, const void *d_yval, uint32_t dphase0,
		uint32_t *d_last, void *d_omag, void *d_ofreq, void *d_work, void *stream)
{
	if (int rc = fm_rx_ok(plan, conv, f))
		return rc;
	if (!fmxd_shape_ok(n, f.log2r))
		return CORDIC_ERR_ARGS;
	if (n == 0)
		return CORDIC_OK;
	const bool fused = fm_rx_fused(plan, conv, f);
	if (int rc = fmrx_check_call(f, n, d_fcw, d_pm, d_acc, d_xval, d_yval, d_last, d_omag,
			d_ofreq, d_work, fm_rx_work_bytes(plan, conv, f, n, false)))
		return rc;
	if (fused)
		return launch_fm_rx(plan->cfg, plan->d_dir, plan->dx, *conv, f, n, d_fcw, d_pm,
			phase0, d_acc, d_xval, d_yval, dphase0, d_last, d_omag, d_ofreq, d_work,
			stream);
	if (f.iq) {
		// the interleaved forms' fallback: one split launch into two arrays
		// behind the twin's workspace, then the twin itself from them
		const FmForm twin = f.split();
		const FmrxC16Layout at = fmrx_c16_layout(fm_rx_work_bytes(plan, conv, twin, n, false),
			n);
		int16_t *x = reinterpret_cast<int16_t *>(bytes_at(d_work, at.x));
		int16_t *y = reinterpret_cast<int16_t *>(bytes_at(d_work, at.y));
		if (int rc = launch_fmrx_split_c16(n, static_cast<const int16_t *>(d_xval), x, y,
				stream))
			return rc;
		return fm_rx(plan, conv, twin, n, d_fcw, d_pm, phase0, d_acc, x, y, dphase0,
			d_last, d_omag, d_ofreq, d_work, stream);
	}
	// the fallback: the two calls of the definition -- the (decimating) mixer
	// into two arrays of m = n >> k elements inside d_work, the discriminator
	// from them
	const size_t m = n >> f.log2r;
	const bool mix_fused = f.log2r && fm_mix_decim_fused(plan, f);
	const FmrxLayout at = fmrx_layout(fm_mix_decim_work_bytes(plan, f, mix_fused, n), m,
		f.esize());
	void *tx = bytes_at(d_work, at.tx), *ty = bytes_at(d_work, at.ty);
	if (int rc = fm_mix_decim(plan, f, n, d_fcw, d_pm, phase0, d_acc, d_xval, d_yval, tx,
			ty, d_work, stream, mix_fused))
		return rc;
	return fm_demod_call(conv, f, m, tx, ty, dphase0, d_last, d_omag, d_ofreq,
		bytes_at(d_work, at.demod), stream);
}

size_t cordic_plan_fm_rx_workspace(const cordic_plan *plan, const cordic_config *conv,
		size_t n)
{
	return fm_rx_workspace(plan, conv, kForm32, n);
}

size_t cordic_plan_fm_rx16_workspace(const cordic_plan *plan, const cordic_config *conv,
		size_t n)
{
	return fm_rx_workspace(plan, conv, kForm16, n);
}

size_t cordic_plan_fm_rx_c16_workspace(const cordic_plan *plan, const cordic_config *conv,
		size_t n)
{
	return fm_rx_workspace(plan, conv, kFormC16, n);
}

size_t cordic_plan_fm_rx_decim_workspace(const cordic_plan *plan,
		const cordic_config *conv, size_t n, uint32_t log2r)
{
	return fm_rx_workspace(plan, conv, decim(kForm32, log2r), n);
}

size_t cordic_plan_fm_rx_decim16_workspace(const cordic_plan *plan,
		const cordic_config *conv, size_t n, uint32_t log2r)
{
	return fm_rx_workspace(plan, conv, decim(kForm16, log2r), n);
}

size_t cordic_plan_fm_rx_decim_c16_workspace(const cordic_plan *plan,
		const cordic_config *conv, size_t n, uint32_t log2r)
{
	return fm_rx_workspace(plan, conv, decim(kFormC16, log2r), n);
}

int cordic_plan_fm_rx_info(const cordic_plan *plan, const cordic_config *conv,
		int32_t *fused, int32_t *tile)
{
	return fm_rx_info(plan, conv, fused, tile, kForm32);
}

int cordic_plan_fm_rx16_info(const cordic_plan *plan, const cordic_config *conv,
		int32_t *fused, int32_t *tile)
{
	return fm_rx_info(plan, conv, fused, tile, kForm16);
}

int cordic_plan_fm_rx_c16_info(const cordic_plan *plan, const cordic_config *conv,
		int32_t *fused, int32_t *tile)
{
	return fm_rx_info(plan, conv, fused, tile, kFormC16);
}

int cordic_plan_fm_rx(const cordic_plan *plan, const cordic_config *conv, size_t n,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const int32_t *d_xval, const int32_t *d_yval,
		uint32_t dphase0, uint32_t *d_last, int32_t *d_omag, int32_t *d_ofreq,
		void *d_work, void *stream)
{
	return fm_rx(plan, conv, kForm32, n, d_fcw, d_pm, phase0, d_acc, d_xval, d_yval,
		dphase0, d_last, d_omag, d_ofreq, d_work, stream);
}

int cordic_plan_fm_rx16(const cordic_plan *plan, const cordic_config *conv, size_t n,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const int16_t *d_xval, const int16_t *d_yval,
		uint32_t dphase0, uint32_t *d_last, int16_t *d_omag, int16_t *d_ofreq,
		void *d_work, void *stream)
{
	return fm_rx(plan, conv, kForm16, n, d_fcw, d_pm, phase0, d_acc, d_xval, d_yval,
		dphase0, d_last, d_omag, d_ofreq, d_work, stream);
}

int cordic_plan_fm_rx_c16(const cordic_plan *plan, const cordic_config *conv, size_t n,
		const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const int16_t *d_iq, uint32_t dphase0, uint32_t *d_last,
		int16_t *d_omag, int16_t *d_ofreq, void *d_work, void *stream)
{
	return fm_rx(plan, conv, kFormC16, n, d_fcw, d_pm, phase0, d_acc, d_iq, nullptr,
		dphase0, d_last, d_omag, d_ofreq, d_work, stream);
}

int cordic_plan_fm_rx_decim(const cordic_plan *plan, const cordic_config *conv, size_t n,
		uint32_t log2r, const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const int32_t *d_xval, const int32_t *d_yval,
		uint32_t dphase0, uint32_t *d_last, int32_t *d_omag, int32_t *d_ofreq,
		void *d_work, void *stream)
{
	return fm_rx(plan, conv, decim(kForm32, log2r), n, d_fcw, d_pm, phase0, d_acc, d_xval,
		d_yval, dphase0, d_last, d_omag, d_ofreq, d_work, stream);
}

int cordic_plan_fm_rx_decim16(const cordic_plan *plan, const cordic_config *conv, size_t n,
		uint32_t log2r, const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0,
		uint32_t *d_acc, const int16_t *d_xval, const int16_t *d_yval,
		uint32_t dphase0, uint32_t *d_last, int16_t *d_omag, int16_t *d_ofreq,
		void *d_work, void *stream)
{
	return fm_rx(plan, conv, decim(kForm16, log2r), n, d_fcw, d_pm, phase0, d_acc, d_xval,
		d_yval, dphase0, d_last, d_omag, d_ofreq, d_work, stream);
}

int cordic_plan_fm_rx_decim_c16(const cordic_plan *plan, const cordic_config *conv,
		size_t n, uint32_t log2r, const uint32_t *d_fcw, const uint32_t *d_pm,
		uint32_t phase0, uint32_t *d_acc, const int16_t *d_iq, uint32_t dphase0,
		uint32_t *d_last, int16_t *d_omag, int16_t *d_ofreq, void *d_work, void *stream)
{
	return fm_rx(plan, conv, decim(kFormC16, log2r), n, d_fcw, d_pm, phase0, d_acc, d_iq,
		nullptr, dphase0, d_last, d_omag, d_ofreq, d_work, stream);
}

// ---- receiver banks: many of those jobs in two launches (cordic_fm_rx_bank.h)
struct cordic_rxbank : BankHandle<cordic_fmrx_job> {
	const cordic_plan *plan = nullptr;	// the caller's; outlives the bank
	cordic_config conv;			// a copy
	FmForm	form;				// the jobs' container; iq: d_xval is interleaved
						// I/Q (_c16); log2r > 0: a decimating bank
	uint32_t passes = 0;
	SpanTable<RxSpan> spans;		// fused
	uint32_t *d_conv = nullptr;		// fused: conv's kernel parameters
};

// all six creates: `jobs` is either job struct with the bank's k (RxJobs,
// cordic_fm_rx_bank.h; no jobs at all: the 32-bit rules); a fused bank uploads
// the converter's kernel parameters behind its span table.  The bank's path is
// the plain call's: the fallback knob does not reach it.
static int rxbank_create(const cordic_plan *plan, const cordic_config *conv,
		size_t njobs, RxJobs jobs, cordic_rxbank **bank)
{
	const FmForm f = {jobs.j16 ? 2u : 4u, jobs.iq, jobs.log2r};
	return plan_bank_create<RxBankTraits>(plan, njobs, jobs, f, bank,
		[&] { return fm_rx_ok(plan, conv, f); },
		[&] { return fm_rx_fused(plan, conv, f.plain()); },
		[&](size_t n) { return fm_rx_work_bytes(plan, conv, f, n, true); },
		cordic_rxbank_destroy, [&](cordic_rxbank *b) {
			b->conv = *conv;
			return b->fused ? fmrxb_upload_conv(b->conv, &b->d_conv) : CORDIC_OK;
		});
}

int cordic_rxbank_create_decim(const cordic_plan *plan, const cordic_config *conv,
		uint32_t log2r, size_t njobs, const cordic_fmrx_job *jobs, cordic_rxbank **bank)
{
	return rxbank_create(plan, conv, njobs, RxJobs(jobs, log2r), bank);
}

int cordic_rxbank_create_decim16(const cordic_plan *plan, const cordic_config *conv,
		uint32_t log2r, size_t njobs, const cordic_fmrx_job16 *jobs,
		cordic_rxbank **bank)
{
	return rxbank_create(plan, conv, njobs, RxJobs(jobs, log2r), bank);
}

int cordic_rxbank_create(const cordic_plan *plan, const cordic_config *conv,
		size_t njobs, const cordic_fmrx_job *jobs, cordic_rxbank **bank)
{
	return rxbank_create(plan, conv, njobs, jobs, bank);
}

int cordic_rxbank_create16(const cordic_plan *plan, const cordic_config *conv,
		size_t njobs, const cordic_fmrx_job16 *jobs, cordic_rxbank **bank)
{
	return rxbank_create(plan, conv, njobs, jobs, bank);
}

// the interleaved creates: the jobs as 16-bit ones whose d_xval is d_iq
// (fmrxb_from_c16); the checks keep rxbank_create's order
static int rxbank_create_c16(const cordic_plan *plan, const cordic_config *conv,
		uint32_t log2r, size_t njobs, const cordic_fmrx_job_c16 *jobs,
		cordic_rxbank **bank)
{
	if (!bank || (njobs && !jobs))
		return CORDIC_ERR_ARGS;
	if (njobs >= ((size_t)1 << 28)) {	// (refused before that many are copied)
		const int rc = fm_rx_ok(plan, conv, kFormC16);
		return rc ? rc : CORDIC_ERR_ARGS;
	}
	std::vector<cordic_fmrx_job16> split(njobs + 1);
	for (size_t k = 0; k < njobs; k++)
		split[k] = fmrxb_from_c16(jobs[k]);
	// (NULL jobs with njobs == 0: NULL on, as _create16 would see it)
	const cordic_fmrx_job16 *j16 = jobs ? split.data() : nullptr;
	return rxbank_create(plan, conv, njobs, RxJobs(j16, log2r, true), bank);
}

int cordic_rxbank_create_c16(const cordic_plan *plan, const cordic_config *conv,
		size_t njobs, const cordic_fmrx_job_c16 *jobs, cordic_rxbank **bank)
{
	return rxbank_create_c16(plan, conv, 0, njobs, jobs, bank);
}

int cordic_rxbank_create_decim_c16(const cordic_plan *plan, const cordic_config *conv,
		uint32_t log2r, size_t njobs, const cordic_fmrx_job_c16 *jobs,
		cordic_rxbank **bank)
{
	return rxbank_create_c16(plan, conv, log2r, njobs, jobs, bank);
}

void cordic_rxbank_destroy(cordic_rxbank *bank)
{
	if (!bank)
		return;
	bank->spans.free();
	dev_free(bank->d_work, bank->d_conv);
	delete bank;
}

int cordic_rxbank_info(const cordic_rxbank *bank, uint64_t *samples, uint32_t *spans,
		int32_t *fused, int32_t *tile)
{
	if (!bank)
		return CORDIC_ERR_ARGS;
	if (samples) *samples = bank->samples;
	if (spans) *spans = bank->spans.nspans;
	if (fused) *fused = bank->fused ? 1 : 0;
	if (tile) *tile = bank->fused ? (int32_t)kFmrxPass : 0;
	return CORDIC_OK;
}

int cordic_rxbank_run(const cordic_rxbank *bank, void *stream)
{
	if (!bank)
		return CORDIC_ERR_ARGS;
	(void)hipGetLastError();
	const cordic_plan *plan = bank->plan;
	return bank_run(*bank, [&] {
		const SpanTable<RxSpan> &t = bank->spans;
		return launch_fmrx_bank(plan->cfg, plan->d_dir, plan->dx, bank->d_conv,
			t.d_spans, t.nspans, t.start(), t.part(), t.more(), bank->cus, bank->form,
			stream);
	}, [&](const cordic_fmrx_job &jb) {
		// (an interleaved job's d_xval carries its d_iq: fmrxb_from_c16)
		return fm_rx(plan, &bank->conv, bank->form, (size_t)jb.n, jb.d_fcw, jb.d_pm,
			jb.phase0, jb.d_acc, jb.d_xval, jb.d_yval, jb.dphase0, jb.d_last, jb.d_omag,
			jb.d_ofreq, bank->d_work, stream);
	});
}
