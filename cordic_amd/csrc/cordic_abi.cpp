// cordic_abi.cpp -- the extern "C" surface declared in include/cordic_amd.h:
// plans, job sets, the int16 calls, the config and stateless wrappers.  (The
// plan-side FM layer -- mixer, receiver and their banks: cordic_abi_fm.cpp;
// table, quadratic and oscillator-bank handles: cordic_abi_table.cpp; the
// clocked views: cordic_abi_clocked.cpp.)  Thin by
// design: argument checks, then the host layer (cordic_config.cpp) or the
// device launchers (cordic_kernels.hip).
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

#include "cordic_abi_plan.h"
#include "cordic_amd.h"
#include "cordic_devmem.h"
#include "cordic_internal.h"
#include "cordic_jobs_fused.h"
#include "cordic_queue_ring.h"

using namespace cordic_amd;

// scratch words that hold any core's seed table (seeds, leaves, direction
// tails) and any core's direction tables: cordic_plan.cpp fills them
constexpr size_t kSeedTableWords = 4 + 4096 * 4 + 4096 * 2
		+ 4 + kDtMaxLevels * (6 + 2 * 4096 + 2 * 256);
constexpr size_t kDirTableWords = 4 + kDxMaxLevels * (6 + 2 * 4096 + 2 * 256);

// ------------------------------------------------------------------- plans
// (the handle: cordic_abi_plan.h)
int cordic_last_kernel(void) { return g_last_kernel; }

int cordic_plan_create(const cordic_config *cfg, cordic_plan **plan)
{
	if (!cfg || !plan)
		return CORDIC_ERR_ARGS;
	if (cfg->mode < CORDIC_P2R || cfg->mode > CORDIC_SR2P)
		return CORDIC_ERR_MODE;
	if (!config_sane(*cfg))
		return CORDIC_ERR_ARGS;
	cordic_plan *p = new (std::nothrow) cordic_plan;
	if (!p)
		return CORDIC_ERR_NOMEM;
	p->cfg = *cfg;
	std::vector<uint32_t> words(kSeedTableWords);
	const size_t nw = build_seed_table(*cfg, CORDIC_SEED_STAGES, words.data(),
			words.size(), &p->dt);
	if (nw) {
		if (!dev_upload(words.data(), nw * 4, &p->d_table) || !p->queues.alloc()) {
			cordic_plan_destroy(p);
			return CORDIC_ERR_DEVICE;
		}
		p->m = (int)words[0];
		p->S = (int)words[1];
		p->nbuckets = (int)words[2];
		p->nleaves = (int)words[3];
		// CORDIC_SEED_IMAGES=0: every block computes its prologue (A/B)
		const char *e = std::getenv("CORDIC_SEED_IMAGES");
		if (!(e && e[0] == '0' && e[1] == 0))
			p->images = seed_images_create();	// (NULL: not fatal)
	}
	// direction tables for per-sample vectors (cordic_plan_p2r); independent
	// of the seed table
	std::vector<uint32_t> dw(kDirTableWords);
	const size_t dn = build_dir_table(*cfg, dw.data(), dw.size(), &p->dx);
	if (!dev_upload(dw.data(), dn * 4, &p->d_dir))
		p->dx = DxInfo{};	// not fatal: cordic_p2r's kernel serves
	*plan = p;
	return CORDIC_OK;
}

int cordic_plan_dir_info(const cordic_plan *plan, int32_t *ngroups, int32_t stages[5])
{
	if (!plan || !ngroups)
		return CORDIC_ERR_ARGS;
	*ngroups = plan->d_dir ? plan->dx.n : 0;
	if (stages)
		for (int g = 0; g < kDxMaxLevels; g++)
			stages[g] = g < *ngroups ? plan->dx.lv[g].t : 0;
	return CORDIC_OK;
}

// the plan's direction tables for the per-sample-vector kernels
static void attach_dirs(const cordic_plan *plan, RotatorJob &j)
{
	j.dir_table = plan->d_dir;
	j.dx = plan->dx;
	j.min_samples = plan->min_samples.load(std::memory_order_relaxed);
}

int cordic_plan_p2r(const cordic_plan *plan, size_t n, const int32_t *d_xval,
		const int32_t *d_yval, const uint32_t *d_phase, int32_t *d_oxval,
		int32_t *d_oyval, void *stream)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	RotatorJob j;
	j.x = d_xval; j.y = d_yval; j.phase = d_phase;
	j.ox = d_oxval; j.oy = d_oyval; j.n = n;
	attach_dirs(plan, j);
	return launch_rotator(plan->cfg, Feed::PhaseArray_XYArray, j, stream);
}

int cordic_plan_mix(const cordic_plan *plan, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, const int32_t *d_xval,
		const int32_t *d_yval, int32_t *d_oxval, int32_t *d_oyval, void *stream)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	RotatorJob j;
	j.x = d_xval; j.y = d_yval;
	j.phase0 = phase0; j.fcw = fcw; j.index0 = index0; j.xy_nco = true;
	j.ox = d_oxval; j.oy = d_oyval; j.n = n;
	attach_dirs(plan, j);
	return launch_rotator(plan->cfg, Feed::PhaseArray_XYArray, j, stream);
}


int cordic_plan_queue_info(const cordic_plan *plan, cordic_queue_info *info)
{
	return queue_info(plan, info);
}

void cordic_plan_destroy(cordic_plan *plan)
{
	if (!plan)
		return;
	dev_free(plan->d_table, plan->d_dir);
	seed_images_destroy(plan->images);
	plan->queues.release();
	delete plan;
}

const cordic_config *cordic_plan_config(const cordic_plan *plan)
{
	return plan ? &plan->cfg : nullptr;
}

int cordic_plan_seed_info(const cordic_plan *plan, int32_t *stages,
		int32_t *nleaves, int32_t *nbuckets)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	if (stages) *stages = plan->m;
	if (nleaves) *nleaves = plan->nleaves;
	if (nbuckets) *nbuckets = plan->nbuckets;
	return CORDIC_OK;
}

int cordic_plan_tail_info(const cordic_plan *plan, int32_t *ngroups,
		int32_t stages[4])
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	if (ngroups) *ngroups = plan->dt.n;
	if (stages)
		for (int g = 0; g < 4; g++)
			stages[g] = g < plan->dt.n ? plan->dt.lv[g].t : 0;
	return CORDIC_OK;
}

static void attach_seed(const cordic_plan *plan, RotatorJob &j)
{
	j.seed_table = plan->d_table;
	j.seed_m = plan->m;
	j.seed_S = plan->S;
	j.seed_nbuckets = plan->nbuckets;
	j.seed_nleaves = plan->nleaves;
	j.dt = plan->dt;
	j.images = plan->images;
	j.min_samples = plan->min_samples.load(std::memory_order_relaxed);
}

// a constant-vector launch of the plan: seeded, with a tile queue of its own
// (an int16 one is noted for cordic_plan_prepare)
static int launch_seeded(const cordic_plan *plan, Feed feed, RotatorJob &j,
		void *stream)
{
	attach_seed(plan, j);
	if (j.io16)
		plan->io16_used.store(true, std::memory_order_relaxed);
	return with_queue(plan->queues, stream, [&](uint32_t *q) {
		j.queue = q;
		return launch_rotator(plan->cfg, feed, j, stream);
	});
}

int cordic_plan_prepare(const cordic_plan *plan, int32_t xval, int32_t yval,
		void *stream)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	if (!plan->d_table || !plan->images)
		return CORDIC_ERR_UNSUPPORTED;
	int rc = CORDIC_OK;
	// the image of the 32-bit arrays' container and -- only once the plan has
	// served an int16 call: an image takes one of its eight write-once slots
	// -- the int16 arrays' 
	for (int io16 = 0; io16 < 2; io16++) {
		if (io16 && (plan->cfg.iw > 16 || plan->cfg.ow > 16
				|| !plan->io16_used.load(std::memory_order_relaxed)))
			break;
		RotatorJob j;
		j.x0 = xval; j.y0 = yval;
		j.io16 = io16 != 0;
		j.prepare_only = true;
		attach_seed(plan, j);
		// the image of the instance a QUEUED launch runs (the ordinary case;
		// a launch without a queue runs the dynamic-exit instance and keeps
		// its own): any counter block stands for "queued" here -- build mode
		// never touches it
		j.queue = plan->queues.d;
		const int r = launch_rotator(plan->cfg, Feed::PhaseArray_ConstXY, j, stream);
		if (!io16)
			rc = r;
	}
	// a set-up call: it returns with the image COMPLETE (one block, ~15 us),
	// so that a capture begun right behind it may use it
	if (rc == CORDIC_OK && !seed_images_settle(plan->images))
		rc = CORDIC_ERR_DEVICE;
	return rc;
}

// ------------------------------------------------------------- job sets
// Many small jobs in one launch (include/cordic_amd.h, "job sets").  The host
// cuts the batch into the seeded kernel's tiles once and keeps the table on
// the device; running the set is then ONE launch of the dynamic-exit instance
// (+ one small launch for trailing samples), whatever the number of jobs.
struct cordic_jobset {
	int	kind = 0;		// enum cordic_jobs_kind
	int	device = 0;
	std::vector<cordic_job> jobs;	// host copy: the one-by-one fallback
	uint32_t *d_tiles = nullptr, *d_tails = nullptr;
	JobTables tabs;
	cordic_config cfg;		// of the plan it was cut for (PW decides NCO words)
	// cordic_jobset_create16: the sample arrays (and the pointers of `jobs`)
	// are int16 / uint16 ones
	bool	io16 = false;
	// enum cordic_jobs_path of the latest run (runs take the set const)
	mutable std::atomic<int> path{CORDIC_JOBS_PATH_NONE};
};

namespace {
// one-shot batches (cordic_plan_*_batch): the set has to outlive the launch
// that reads it; it is parked here with an event and freed by a later call
// once that event has completed (or by cordic_jobset_reap / process exit)
struct Parked { cordic_jobset *set; hipEvent_t done; };
std::mutex g_parked_mu;
std::vector<Parked> g_parked;

void reap_parked(bool wait)
{
	std::vector<Parked> dead;
	{
		std::lock_guard<std::mutex> lock(g_parked_mu);
		for (size_t k = 0; k < g_parked.size();) {
			Parked &p = g_parked[k];
			const hipError_t e = wait ? hipEventSynchronize(p.done)
						  : hipEventQuery(p.done);
			// (only a launch that is KNOWN to have passed gives its tables
			// back: an event in an error state says nothing about who still
			// reads them, and the set then stays parked for good)
			if (e == hipSuccess) {
				dead.push_back(p);
				g_parked.erase(g_parked.begin() + (long)k);
			} else {
				(void)hipGetLastError();
				k++;
			}
		}
	}
	for (Parked &p : dead) {
		(void)hipEventDestroy(p.done);
		cordic_jobset_destroy(p.set);
	}
}

// same core?  field by field: the PODs come from different places and their
// padding bytes are nobody's business
bool same_core(const cordic_config &a, const cordic_config &b)
{
	if (a.mode != b.mode || a.iw != b.iw || a.ow != b.ow || a.nextra != b.nextra
			|| a.ww != b.ww || a.pw != b.pw || a.nstages != b.nstages
			|| a.nlive != b.nlive || a.needs_wrap != b.needs_wrap
			|| a.flags != b.flags)
		return false;
	for (int i = 0; i < a.nstages && i < CORDIC_AMD_MAX_STAGES; i++)
		if (a.angle[i] != b.angle[i])
			return false;
	return true;
}

// Tile length (vectors) of the data-fed kinds: whole passes of a 256-thread
// block, as long as the seeded kernels' tiles where the tile-length rule
// (cordic_bank_host.h; 8 resident blocks per CU) allows, shorter below.
// CORDIC_JOBS_TILE_PASSES=<1, 2, 4 or 8> in the environment (read at create; a
// test and A/B knob like the banks' CORDIC_*_PASSES) forces a tile of that many
// passes; anything else keeps the rule's choice.  The bits do not depend on it.
uint32_t xy_tile_vecs(uint64_t total_vecs)
{
	const uint64_t per = bank_tile_room(total_vecs, cus_or_256(), 8);
	const uint32_t rule = (uint32_t)std::min<uint64_t>(kJobTileVecs,
		std::max<uint64_t>(kJobPassVecs, per / kJobPassVecs * kJobPassVecs));
	return kJobPassVecs * bank_forced_passes(std::getenv("CORDIC_JOBS_TILE_PASSES"),
		kJobTileVecs / kJobPassVecs, rule / kJobPassVecs);
}

// esize: bytes per sample of every array of the jobs -- 4, or 2 for the sets of
// cordic_jobset_create16 (whose cordic_job16 has cordic_job's layout)
int jobset_create(const cordic_plan *plan, int kind, size_t njobs,
		const cordic_job *jobs, cordic_jobset **out, unsigned esize)
{
	if (!plan || !out || (njobs && !jobs) || kind < CORDIC_JOBS_PHASE_ARRAYS
			|| kind > CORDIC_JOBS_MIX)
		return CORDIC_ERR_ARGS;
	const uintptr_t amask = esize - 1;
	// address of sample s of an array
	auto at = [esize](const void *p, uint64_t s) -> uint64_t {
		return (uint64_t)((uintptr_t)p + (uintptr_t)s * esize);
	};
	const bool rot = plan->cfg.mode == CORDIC_P2R || plan->cfg.mode == CORDIC_SP2R;
	if (rot == (kind == CORDIC_JOBS_R2P))
		return CORDIC_ERR_MODE;
	const bool xy = kind >= CORDIC_JOBS_R2P;	// per-sample vectors from memory
	const bool phase_array = kind == CORDIC_JOBS_PHASE_ARRAYS
			|| kind == CORDIC_JOBS_P2R_XY;
	const bool gen_phase = kind == CORDIC_JOBS_NCO || kind == CORDIC_JOBS_MIX;
	std::vector<TileDesc> tiles;
	std::vector<TailDesc> tails;
	std::vector<TileDescXY> xtiles, xtails;
	uint64_t samples = 0, vecs = 0;
	const int sh = 32 - plan->cfg.pw;
	for (size_t k = 0; k < njobs; k++) {
		const cordic_job &jb = jobs[k];
		if (jb.n == 0)
			continue;
		if (!jb.d_oxval || !jb.d_oyval || (phase_array && !jb.d_phase)
				|| (xy && (!jb.d_xval || !jb.d_yval))
				|| ((uintptr_t)jb.d_oxval & amask) || ((uintptr_t)jb.d_oyval & amask)
				|| (phase_array && ((uintptr_t)jb.d_phase & amask))
				|| (xy && (((uintptr_t)jb.d_xval & amask)
					|| ((uintptr_t)jb.d_yval & amask))))
			return CORDIC_ERR_ARGS;
		samples += jb.n;
		vecs += jb.n / 4;
	}
	const uint32_t tile_vecs = xy ? xy_tile_vecs(vecs) : kJobTileVecs;
	for (size_t k = 0; k < njobs; k++) {
		const cordic_job &jb = jobs[k];
		if (jb.n == 0)
			continue;
		const uint64_t nvec = jb.n / 4;
		// the phase of sample s of the job, left-justified (NCO / MIX jobs)
		auto nco_word = [&](uint64_t s) -> uint64_t {
			const uint32_t f = jb.fcw << sh;
			const uint32_t p = (jb.phase0 << sh) + (uint32_t)(jb.index0 + s) * f;
			return ((uint64_t)f << 32) | p;
		};
		auto in_word = [&](uint64_t s) -> uint64_t {
			return gen_phase ? nco_word(s)
				: phase_array ? at(jb.d_phase, s) : 0;
		};
		auto xy_desc = [&](uint64_t s, uint32_t live) {
			TileDescXY d{};
			d.in0 = at(jb.d_xval, s);
			d.in1 = at(jb.d_yval, s);
			d.in2 = in_word(s);
			d.o0 = at(jb.d_oxval, s);
			d.o1 = at(jb.d_oyval, s);
			d.live = live;
			return d;
		};
		for (uint64_t v0 = 0; v0 < nvec; v0 += tile_vecs) {
			const uint32_t live = (uint32_t)(nvec - v0 < tile_vecs ? nvec - v0 : tile_vecs);
			if (xy) {
				xtiles.push_back(xy_desc(v0 * 4, live));
				continue;
			}
			TileDesc d{};
			d.in = in_word(v0 * 4);
			d.ox = at(jb.d_oxval, v0 * 4);
			d.oy = at(jb.d_oyval, v0 * 4);
			d.live = live;
			tiles.push_back(d);
		}
		for (uint64_t s = nvec * 4; s < jb.n; s++) {
			if (xy) {
				xtails.push_back(xy_desc(s, 0));
				continue;
			}
			TailDesc d{};
			d.in = in_word(s);
			d.ox = at(jb.d_oxval, s);
			d.oy = at(jb.d_oyval, s);
			tails.push_back(d);
		}
		if (tiles.size() > 0x7fffffffu || tails.size() > 0x7fffffffu
				|| xtiles.size() > 0x7fffffffu || xtails.size() > 0x7fffffffu)
			return CORDIC_ERR_ARGS;
	}
	cordic_jobset *set = new (std::nothrow) cordic_jobset;
	if (!set)
		return CORDIC_ERR_NOMEM;
	set->kind = kind;
	set->cfg = plan->cfg;
	set->io16 = esize == 2;
	set->jobs.assign(jobs, jobs + njobs);
	set->device = current_device();
	const bool up = xy
		? dev_upload(xtiles.data(), xtiles.size() * sizeof(TileDescXY), &set->d_tiles)
			&& dev_upload(xtails.data(), xtails.size() * sizeof(TileDescXY), &set->d_tails)
		: dev_upload(tiles.data(), tiles.size() * sizeof(TileDesc), &set->d_tiles)
			&& dev_upload(tails.data(), tails.size() * sizeof(TailDesc), &set->d_tails);
	if (!up) {
		cordic_jobset_destroy(set);
		return CORDIC_ERR_DEVICE;
	}
	set->tabs.tiles = set->d_tiles;
	set->tabs.ntiles = (uint32_t)(xy ? xtiles.size() : tiles.size());
	set->tabs.tails = set->d_tails;
	set->tabs.ntails = (uint32_t)(xy ? xtails.size() : tails.size());
	set->tabs.samples = samples;
	*out = set;
	return CORDIC_OK;
}
} // namespace

int cordic_jobset_create(const cordic_plan *plan, int kind, size_t njobs,
		const cordic_job *jobs, cordic_jobset **out)
{
	return jobset_create(plan, kind, njobs, jobs, out, 4);
}

int cordic_jobset_create16(const cordic_plan *plan, int kind, size_t njobs,
		const cordic_job16 *jobs, cordic_jobset **out)
{
	static_assert(sizeof(cordic_job16) == sizeof(cordic_job)
		&& offsetof(cordic_job16, d_phase) == offsetof(cordic_job, d_phase)
		&& offsetof(cordic_job16, phase0) == offsetof(cordic_job, phase0)
		&& offsetof(cordic_job16, fcw) == offsetof(cordic_job, fcw)
		&& offsetof(cordic_job16, index0) == offsetof(cordic_job, index0)
		&& offsetof(cordic_job16, d_oxval) == offsetof(cordic_job, d_oxval)
		&& offsetof(cordic_job16, d_oyval) == offsetof(cordic_job, d_oyval)
		&& offsetof(cordic_job16, n) == offsetof(cordic_job, n)
		&& offsetof(cordic_job16, d_xval) == offsetof(cordic_job, d_xval)
		&& offsetof(cordic_job16, d_yval) == offsetof(cordic_job, d_yval),
		"cordic_job16 is cordic_job with 16-bit sample pointers");
	if (!plan || !out || (njobs && !jobs) || kind < CORDIC_JOBS_PHASE_ARRAYS
			|| kind > CORDIC_JOBS_MIX)
		return CORDIC_ERR_ARGS;
	// (the constant-vector kinds would need the seeded kernel's tile form on
	// 16-bit arrays)
	if (kind < CORDIC_JOBS_R2P)
		return CORDIC_ERR_UNSUPPORTED;
	const bool rot = plan->cfg.mode == CORDIC_P2R || plan->cfg.mode == CORDIC_SP2R;
	if (rot == (kind == CORDIC_JOBS_R2P))
		return CORDIC_ERR_MODE;
	if (int rc = fits16(plan->cfg, kind != CORDIC_JOBS_MIX))
		return rc;
	// the set keeps its jobs as cordic_job: same layout, the pointers are never
	// dereferenced on the host and every address is computed in bytes
	std::vector<cordic_job> wide(njobs);
	for (size_t k = 0; k < njobs; k++) {
		const cordic_job16 &a = jobs[k];
		cordic_job &b = wide[k];
		b.d_phase = reinterpret_cast<const uint32_t *>(a.d_phase);
		b.phase0 = a.phase0; b.fcw = a.fcw; b.index0 = a.index0;
		b.d_oxval = reinterpret_cast<int32_t *>(a.d_oxval);
		b.d_oyval = reinterpret_cast<int32_t *>(a.d_oyval);
		b.n = a.n;
		b.d_xval = reinterpret_cast<const int32_t *>(a.d_xval);
		b.d_yval = reinterpret_cast<const int32_t *>(a.d_yval);
	}
	return jobset_create(plan, kind, njobs, wide.data(), out, 2);
}

void cordic_jobset_destroy(cordic_jobset *set)
{
	if (!set)
		return;
	dev_free(set->d_tiles, set->d_tails);
	delete set;
}

int cordic_jobset_info(const cordic_jobset *set, uint64_t *samples,
		uint32_t *tiles, uint32_t *tail_samples)
{
	if (!set)
		return CORDIC_ERR_ARGS;
	if (samples) *samples = set->tabs.samples;
	if (tiles) *tiles = set->tabs.ntiles;
	if (tail_samples) *tail_samples = set->tabs.ntails;
	return CORDIC_OK;
}

int cordic_jobset_path(const cordic_jobset *set, int32_t *path)
{
	if (!set || !path)
		return CORDIC_ERR_ARGS;
	*path = set->path.load(std::memory_order_relaxed);
	return CORDIC_OK;
}

// Run a set: the fused launch where `fused` has one for this core, else (it
// says CORDIC_ERR_UNSUPPORTED) the non-empty jobs one by one through `each`,
// which gives the same results; the path taken is noted in the set.
template <typename Fused, typename Each>
static int fused_or_each(const cordic_jobset *set, Fused fused, Each each)
{
	int rc = fused();
	if (rc == CORDIC_OK)
		set->path.store(CORDIC_JOBS_PATH_FUSED, std::memory_order_relaxed);
	if (rc != CORDIC_ERR_UNSUPPORTED)
		return rc;
	set->path.store(CORDIC_JOBS_PATH_ONE_BY_ONE, std::memory_order_relaxed);
	for (const cordic_job &jb : set->jobs) {
		if (jb.n == 0)
			continue;
		rc = each(jb);
		if (rc != CORDIC_OK)
			return rc;
	}
	return CORDIC_OK;
}

int cordic_plan_run_jobs(const cordic_plan *plan, const cordic_jobset *set,
		int32_t xval, int32_t yval, void *stream)
{
	if (!plan || !set)
		return CORDIC_ERR_ARGS;
	// cut for this core (the tile table holds PW-scaled phase words) and for
	// this device (it holds device addresses)?
	if (int rc = device_is_current(set->device))
		return rc;
	if (!same_core(set->cfg, plan->cfg))
		return CORDIC_ERR_ARGS;
	const int kind = set->kind;
	// a data-fed job through the single call of its kind (taken where that
	// call runs the generic kernel on this core)
	auto each_xy = [&](const cordic_job &jb) {
		if (kind == CORDIC_JOBS_R2P)
			return launch_topolar(plan->cfg, (size_t)jb.n, jb.d_xval, jb.d_yval,
				jb.d_oxval, reinterpret_cast<uint32_t *>(jb.d_oyval), stream,
				set->io16);
		if (!set->io16)
			return kind == CORDIC_JOBS_MIX
				? cordic_plan_mix(plan, (size_t)jb.n, jb.phase0, jb.fcw, jb.index0,
					jb.d_xval, jb.d_yval, jb.d_oxval, jb.d_oyval, stream)
				: cordic_plan_p2r(plan, (size_t)jb.n, jb.d_xval, jb.d_yval,
					jb.d_phase, jb.d_oxval, jb.d_oyval, stream);
		const int16_t *x = reinterpret_cast<const int16_t *>(jb.d_xval);
		const int16_t *y = reinterpret_cast<const int16_t *>(jb.d_yval);
		int16_t *ox = reinterpret_cast<int16_t *>(jb.d_oxval);
		int16_t *oy = reinterpret_cast<int16_t *>(jb.d_oyval);
		return kind == CORDIC_JOBS_MIX
			? cordic_plan_mix16(plan, (size_t)jb.n, jb.phase0, jb.fcw, jb.index0,
				x, y, ox, oy, stream)
			: cordic_plan_p2r16(plan, (size_t)jb.n, x, y,
				reinterpret_cast<const uint16_t *>(jb.d_phase), ox, oy, stream);
	};
	if (set->io16)
		return fused_or_each(set, [&] {
			return launch_xy_jobs16(plan->cfg, kind, set->tabs, stream);
		}, each_xy);
	if (kind >= CORDIC_JOBS_R2P) {
		RotatorJob j;
		if (kind != CORDIC_JOBS_R2P)
			attach_dirs(plan, j);
		return fused_or_each(set, [&] {
			// the instances of launch_xy_jobs first, then the tile forms of
			// the other single-call kernels (cordic_jobs_fused.h)
			const int rc = launch_xy_jobs(plan->cfg, kind, j, set->tabs, stream);
			return rc != CORDIC_ERR_UNSUPPORTED ? rc
				: launch_xy_jobs_fused(plan->cfg, kind, j, set->tabs, stream);
		}, each_xy);
	}
	const Feed feed = kind == CORDIC_JOBS_NCO ? Feed::Nco_ConstXY
						  : Feed::PhaseArray_ConstXY;
	RotatorJob j;
	j.x0 = xval; j.y0 = yval;
	attach_seed(plan, j);
	// (one by one: no seeded kernel for this core, or no tile queue to be had
	// right now)
	return fused_or_each(set, [&] {
		return with_queue(plan->queues, stream, [&](uint32_t *q) {
			j.queue = q;
			return launch_rotator_jobs(plan->cfg, feed, j, set->tabs, stream);
		});
	}, [&](const cordic_job &jb) {
		return feed == Feed::Nco_ConstXY
			? cordic_plan_nco(plan, (size_t)jb.n, jb.phase0, jb.fcw, jb.index0,
				xval, yval, jb.d_oxval, jb.d_oyval, stream)
			: cordic_plan_p2r_const(plan, (size_t)jb.n, xval, yval, jb.d_phase,
				jb.d_oxval, jb.d_oyval, stream);
	});
}

static int run_batch_once(const cordic_plan *plan, int kind, size_t njobs,
		const cordic_job *jobs, int32_t xval, int32_t yval, void *stream)
{
	// cutting a set allocates and copies (blocking): not inside a capture --
	// and the graph would outlive the tables this call frees behind its launch
	if (stream_capturing(stream, nullptr))
		return CORDIC_ERR_UNSUPPORTED;
	reap_parked(false);
	cordic_jobset *set = nullptr;
	if (int rc = cordic_jobset_create(plan, kind, njobs, jobs, &set))
		return rc;
	const int rc = cordic_plan_run_jobs(plan, set, xval, yval, stream);
	// the tables have to stay until the launch has read them
	hipEvent_t done = nullptr;
	if (hipEventCreateWithFlags(&done, hipEventDisableTiming) == hipSuccess
			&& hipEventRecord(done, static_cast<hipStream_t>(stream)) == hipSuccess) {
		std::lock_guard<std::mutex> lock(g_parked_mu);
		g_parked.push_back(Parked{set, done});
	} else {
		(void)hipGetLastError();
		if (done) (void)hipEventDestroy(done);
		(void)hipStreamSynchronize(static_cast<hipStream_t>(stream));
		cordic_jobset_destroy(set);
	}
	return rc;
}

int cordic_plan_p2r_const_batch(const cordic_plan *plan, size_t njobs,
		const cordic_job *jobs, int32_t xval, int32_t yval, void *stream)
{
	return run_batch_once(plan, CORDIC_JOBS_PHASE_ARRAYS, njobs, jobs, xval, yval,
			stream);
}

int cordic_plan_nco_batch(const cordic_plan *plan, size_t njobs,
		const cordic_job *jobs, int32_t xval, int32_t yval, void *stream)
{
	return run_batch_once(plan, CORDIC_JOBS_NCO, njobs, jobs, xval, yval, stream);
}

int cordic_plan_r2p_batch(const cordic_plan *plan, size_t njobs,
		const cordic_job *jobs, void *stream)
{
	return run_batch_once(plan, CORDIC_JOBS_R2P, njobs, jobs, 0, 0, stream);
}

int cordic_plan_p2r_batch(const cordic_plan *plan, size_t njobs,
		const cordic_job *jobs, void *stream)
{
	return run_batch_once(plan, CORDIC_JOBS_P2R_XY, njobs, jobs, 0, 0, stream);
}

int cordic_plan_mix_batch(const cordic_plan *plan, size_t njobs,
		const cordic_job *jobs, void *stream)
{
	return run_batch_once(plan, CORDIC_JOBS_MIX, njobs, jobs, 0, 0, stream);
}

void cordic_jobset_reap(void) { reap_parked(true); }

int cordic_plan_set_min_samples(cordic_plan *plan, long long min_samples)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	plan->min_samples.store(min_samples < 0 ? -1 : min_samples,
			std::memory_order_relaxed);
	return CORDIC_OK;
}

int cordic_plan_image_info(const cordic_plan *plan, int32_t *held, uint64_t *hits,
		uint64_t *misses)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	seed_images_info(plan->images, held, hits, misses);
	return CORDIC_OK;
}

int cordic_plan_p2r_const(const cordic_plan *plan, size_t n, int32_t xval,
		int32_t yval, const uint32_t *d_phase, int32_t *d_oxval,
		int32_t *d_oyval, void *stream)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	RotatorJob j;
	j.x0 = xval; j.y0 = yval; j.phase = d_phase;
	j.ox = d_oxval; j.oy = d_oyval; j.n = n;
	return launch_seeded(plan, Feed::PhaseArray_ConstXY, j, stream);
}

int cordic_plan_nco(const cordic_plan *plan, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, int32_t xval, int32_t yval,
		int32_t *d_oxval, int32_t *d_oyval, void *stream)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	RotatorJob j;
	j.x0 = xval; j.y0 = yval; j.phase0 = phase0; j.fcw = fcw;
	j.index0 = index0; j.ox = d_oxval; j.oy = d_oyval; j.n = n;
	return launch_seeded(plan, Feed::Nco_ConstXY, j, stream);
}

// 16-bit containers: the job carries the int16 / uint16 arrays behind its
// int32 pointers (cordic_internal.h: RotatorJob::io16)
namespace {
template <typename T> const int32_t *as_i32(const T *p)
{
	return reinterpret_cast<const int32_t *>(p);
}
template <typename T> int32_t *as_i32(T *p)
{
	return reinterpret_cast<int32_t *>(p);
}
RotatorJob job16(const int16_t *x, const int16_t *y, const uint16_t *phase,
		int16_t *ox, int16_t *oy, size_t n)
{
	RotatorJob j;
	j.x = as_i32(x); j.y = as_i32(y);
	j.phase = reinterpret_cast<const uint32_t *>(phase);
	j.ox = as_i32(ox); j.oy = as_i32(oy);
	j.n = n;
	j.io16 = true;
	return j;
}
} // namespace

int cordic_p2r16(const cordic_config *cfg, size_t n, const int16_t *d_xval,
		const int16_t *d_yval, const uint16_t *d_phase, int16_t *d_oxval,
		int16_t *d_oyval, void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	if (int rc = fits16(*cfg, true))
		return rc;
	RotatorJob j = job16(d_xval, d_yval, d_phase, d_oxval, d_oyval, n);
	return launch_rotator(*cfg, Feed::PhaseArray_XYArray, j, stream);
}

int cordic_p2r16_const(const cordic_config *cfg, size_t n, int32_t xval,
		int32_t yval, const uint16_t *d_phase, int16_t *d_oxval,
		int16_t *d_oyval, void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	if (int rc = fits16(*cfg, true))
		return rc;
	RotatorJob j = job16(nullptr, nullptr, d_phase, d_oxval, d_oyval, n);
	j.x0 = xval; j.y0 = yval;
	return launch_rotator(*cfg, Feed::PhaseArray_ConstXY, j, stream);
}

int cordic_nco16(const cordic_config *cfg, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, int32_t xval, int32_t yval,
		int16_t *d_oxval, int16_t *d_oyval, void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	if (int rc = fits16(*cfg, false))
		return rc;
	RotatorJob j = job16(nullptr, nullptr, nullptr, d_oxval, d_oyval, n);
	j.x0 = xval; j.y0 = yval; j.phase0 = phase0; j.fcw = fcw;
	j.index0 = index0;
	return launch_rotator(*cfg, Feed::Nco_ConstXY, j, stream);
}

int cordic_r2p16(const cordic_config *cfg, size_t n, const int16_t *d_xval,
		const int16_t *d_yval, int16_t *d_omag, uint16_t *d_ophase,
		void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	if (int rc = fits16(*cfg, true))
		return rc;
	return launch_topolar(*cfg, n, as_i32(d_xval), as_i32(d_yval),
			as_i32(d_omag), reinterpret_cast<uint32_t *>(d_ophase),
			stream, true);
}

int cordic_plan_p2r16_const(const cordic_plan *plan, size_t n, int32_t xval,
		int32_t yval, const uint16_t *d_phase, int16_t *d_oxval,
		int16_t *d_oyval, void *stream)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	if (int rc = fits16(plan->cfg, true))
		return rc;
	RotatorJob j = job16(nullptr, nullptr, d_phase, d_oxval, d_oyval, n);
	j.x0 = xval; j.y0 = yval;
	return launch_seeded(plan, Feed::PhaseArray_ConstXY, j, stream);
}

int cordic_plan_nco16(const cordic_plan *plan, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, int32_t xval, int32_t yval,
		int16_t *d_oxval, int16_t *d_oyval, void *stream)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	if (int rc = fits16(plan->cfg, false))
		return rc;
	RotatorJob j = job16(nullptr, nullptr, nullptr, d_oxval, d_oyval, n);
	j.x0 = xval; j.y0 = yval; j.phase0 = phase0; j.fcw = fcw;
	j.index0 = index0;
	return launch_seeded(plan, Feed::Nco_ConstXY, j, stream);
}

int cordic_mix16(const cordic_config *cfg, size_t n, uint32_t phase0, uint32_t fcw,
		uint64_t index0, const int16_t *d_xval, const int16_t *d_yval,
		int16_t *d_oxval, int16_t *d_oyval, void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	if (int rc = fits16(*cfg, false))
		return rc;
	RotatorJob j = job16(d_xval, d_yval, nullptr, d_oxval, d_oyval, n);
	j.phase0 = phase0; j.fcw = fcw; j.index0 = index0; j.xy_nco = true;
	return launch_rotator(*cfg, Feed::PhaseArray_XYArray, j, stream);
}

// (the plan forms run the kernel of cordic_p2r16: the direction tables are for
// the left-justified 64-bit container and are not attached)
int cordic_plan_mix16(const cordic_plan *plan, size_t n, uint32_t phase0,
		uint32_t fcw, uint64_t index0, const int16_t *d_xval,
		const int16_t *d_yval, int16_t *d_oxval, int16_t *d_oyval, void *stream)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	return cordic_mix16(&plan->cfg, n, phase0, fcw, index0, d_xval, d_yval,
			d_oxval, d_oyval, stream);
}

int cordic_plan_p2r16(const cordic_plan *plan, size_t n, const int16_t *d_xval,
		const int16_t *d_yval, const uint16_t *d_phase, int16_t *d_oxval,
		int16_t *d_oyval, void *stream)
{
	if (!plan)
		return CORDIC_ERR_ARGS;
	return cordic_p2r16(&plan->cfg, n, d_xval, d_yval, d_phase, d_oxval, d_oyval,
			stream);
}

// ---------------------- host side of the table and quadratic sine cores
// (their device handles: cordic_abi_table.cpp)
int cordic_table_config_init(cordic_table_config *cfg, int kind, int iw, int ow,
		int phase_bits)
{
	return table_derive(cfg, kind, iw, ow, phase_bits);
}

int cordic_table_values(const cordic_table_config *cfg, int32_t *out, size_t cap)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	return table_fill(*cfg, out, cap);
}

int cordic_quad_config_init(cordic_quad_config *cfg, int iw, int ow, int xtra,
		int phase_bits)
{
	return quad_build_from_cli(cfg, iw, ow, xtra, phase_bits);
}

int cordic_quad_config_init_core(cordic_quad_config *cfg, int phase_bits, int ow,
		int nxtra)
{
	return quad_build_core(cfg, phase_bits, ow, nxtra);
}

int cordic_quad_tables(const cordic_quad_config *cfg, int32_t *ctbl,
		int32_t *ltbl, int32_t *qtbl, size_t cap)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	return quad_fill(*cfg, ctbl, ltbl, qtbl, cap);
}

int cordic_quad_write_header(const cordic_quad_config *cfg, const char *name,
		char *buf, size_t cap)
{
	return quad_write_header(cfg, name, buf, cap);
}

size_t cordic_dir_table(const cordic_config *cfg, uint32_t *buf, size_t cap_words)
{
	if (!cfg)
		return 0;
	if (!buf || cap_words == 0) {
		std::vector<uint32_t> tmp(kDirTableWords);
		return build_dir_table(*cfg, tmp.data(), tmp.size(), nullptr);
	}
	return build_dir_table(*cfg, buf, cap_words, nullptr);
}

size_t cordic_seed_table(const cordic_config *cfg, uint32_t *buf, size_t cap_words)
{
	if (!cfg)
		return 0;
	if (!buf || cap_words == 0) {
		std::vector<uint32_t> tmp(kSeedTableWords);
		return build_seed_table(*cfg, CORDIC_SEED_STAGES, tmp.data(), tmp.size());
	}
	return build_seed_table(*cfg, CORDIC_SEED_STAGES, buf, cap_words);
}

extern "C" {

int cordic_abi_version(void) { return CORDIC_AMD_ABI_VERSION; }

const char *cordic_strerror(int status) { return status_text(status); }

int cordic_config_init(cordic_config *cfg, int mode, int iw, int ow, int xtra,
		int phase_bits, int nstages)
{
	return build_from_cli(cfg, mode, iw, ow, xtra, phase_bits, nstages);
}

int cordic_config_init_core(cordic_config *cfg, int mode, int nstages, int iw,
		int ow, int nxtra, int phase_bits)
{
	return build_core(cfg, mode, nstages, iw, ow, nxtra, phase_bits);
}

int cordic_config_from_args(cordic_config *cfg, int argc,
		const char *const *argv, char *fname, size_t fname_cap,
		int *c_header)
{
	return parse_args(cfg, argc, argv, fname, fname_cap, c_header);
}

int cordic_config_write_header(const cordic_config *cfg, const char *name,
		char *buf, size_t cap)
{
	return write_header(cfg, name, buf, cap);
}

int cordic_nextlg(unsigned vl) { return next_lg(vl); }
double cordic_gain(int nstages) { return rotation_gain(nstages); }
uint32_t cordic_gain_annihilator(int nstages) { return gain_annihilator(nstages); }
uint32_t cordic_config_gain_annihilator(const cordic_config *cfg)
{
	return cfg ? core_gain_annihilator(*cfg) : 0u;
}
double cordic_phase_variance(int nstages, int phase_bits)
{
	return phase_variance(nstages, phase_bits);
}
double cordic_transform_quantization_variance(int nstages, int xtrabits,
		int dropped_bits)
{
	return quantization_variance(nstages, xtrabits, dropped_bits);
}
int cordic_angles(int nstages, int phase_bits, uint32_t *out)
{
	if (!out || nstages < 0 || phase_bits < 3 || phase_bits > 32)
		return CORDIC_ERR_ARGS;
	for (int k = 0; k < nstages; k++)
		out[k] = arctan_entry((unsigned)k, phase_bits);
	return CORDIC_OK;
}
int cordic_calc_stages_ww(int working_width, int phase_bits)
{
	return stages_for(phase_bits, working_width);
}
int cordic_calc_stages(int phase_bits) { return stages_for(phase_bits, -1); }
int cordic_calc_phase_bits(int output_width) { return phase_bits_for(output_width); }

// ------------------------------------------------------------------ device

int cordic_p2r(const cordic_config *cfg, size_t n, const int32_t *d_xval,
		const int32_t *d_yval, const uint32_t *d_phase, int32_t *d_oxval,
		int32_t *d_oyval, void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	RotatorJob j;
	j.x = d_xval; j.y = d_yval; j.phase = d_phase;
	j.ox = d_oxval; j.oy = d_oyval; j.n = n;
	return launch_rotator(*cfg, Feed::PhaseArray_XYArray, j, stream);
}

int cordic_p2r_const(const cordic_config *cfg, size_t n, int32_t xval,
		int32_t yval, const uint32_t *d_phase, int32_t *d_oxval,
		int32_t *d_oyval, void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	RotatorJob j;
	j.x0 = xval; j.y0 = yval; j.phase = d_phase;
	j.ox = d_oxval; j.oy = d_oyval; j.n = n;
	return launch_rotator(*cfg, Feed::PhaseArray_ConstXY, j, stream);
}

int cordic_nco(const cordic_config *cfg, size_t n, uint32_t phase0, uint32_t fcw,
		uint64_t index0, int32_t xval, int32_t yval, int32_t *d_oxval,
		int32_t *d_oyval, void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	RotatorJob j;
	j.x0 = xval; j.y0 = yval; j.phase0 = phase0; j.fcw = fcw;
	j.index0 = index0; j.ox = d_oxval; j.oy = d_oyval; j.n = n;
	return launch_rotator(*cfg, Feed::Nco_ConstXY, j, stream);
}

int cordic_mix(const cordic_config *cfg, size_t n, uint32_t phase0, uint32_t fcw,
		uint64_t index0, const int32_t *d_xval, const int32_t *d_yval,
		int32_t *d_oxval, int32_t *d_oyval, void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	RotatorJob j;
	j.x = d_xval; j.y = d_yval;
	j.phase0 = phase0; j.fcw = fcw; j.index0 = index0; j.xy_nco = true;
	j.ox = d_oxval; j.oy = d_oyval; j.n = n;
	return launch_rotator(*cfg, Feed::PhaseArray_XYArray, j, stream);
}

int cordic_r2p(const cordic_config *cfg, size_t n, const int32_t *d_xval,
		const int32_t *d_yval, int32_t *d_omag, uint32_t *d_ophase,
		void *stream)
{
	if (!cfg)
		return CORDIC_ERR_ARGS;
	return launch_topolar(*cfg, n, d_xval, d_yval, d_omag, d_ophase, stream);
}

// cordic_p2r_host / cordic_r2p_host: cordic_host.cpp (chunked copy pipeline)

int cordic_fill_phase_ramp(uint32_t *d_phase, size_t n, uint64_t index0,
		int shift, void *stream)
{
	return launch_fill_phase_ramp(d_phase, n, index0, shift, stream);
}

int cordic_fill_iq_ramp(int32_t *d_x, int32_t *d_y, size_t n, uint64_t index0,
		uint32_t mulx, uint32_t muly, int bits, void *stream)
{
	return launch_fill_iq_ramp(d_x, d_y, n, index0, mulx, muly, bits, stream);
}

int cordic_digest_u32(const uint32_t *d_words, size_t n, uint64_t index0,
		uint64_t *d_digest, void *stream)
{
	return launch_digest_u32(d_words, n, index0, d_digest, stream);
}

} // extern "C"
