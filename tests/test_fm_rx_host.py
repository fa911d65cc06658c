"""The tuned FM receiver's interface (cordic_plan_fm_rx and its twins;
include/cordic_amd.h): what needs no GPU -- the declarations, the export, the
binding, the status codes in their documented order and the workspace sizes."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cordic_amd as ca
import test_fm_demod as DEM
import test_fm_mix as MIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_plan_fm_rx_workspace", "cordic_plan_fm_rx16_workspace",
         "cordic_plan_fm_rx_info", "cordic_plan_fm_rx16_info", "cordic_plan_fm_rx",
         "cordic_plan_fm_rx16")
SIZES = (0, 1, 255, 256, 257, 1 << 20, 1 << 33)


def declared(text, decl):
    toks = re.findall(r"\w+|[^\w\s]", decl)
    out = ""
    for a, b in zip(toks, toks[1:] + [""]):
        out += re.escape(a)
        out += r"\s+" if re.match(r"\w", a) and re.match(r"\w", b) else r"\s*"
    return re.search(out, text) is not None


def test_the_six_functions_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    head = "const cordic_plan *plan, const cordic_config *conv, "
    for w in ("", "16"):
        assert declared(text, "size_t cordic_plan_fm_rx%s_workspace(%ssize_t n);" % (w, head))
        assert declared(text, "int cordic_plan_fm_rx%s_info(%sint32_t *fused, "
                              "int32_t *tile);" % (w, head))
        t = "int%s_t" % (w or "32")
        assert declared(text, (
            "int cordic_plan_fm_rx%s(%ssize_t n, const uint32_t *d_fcw, const uint32_t "
            "*d_pm, uint32_t phase0, uint32_t *d_acc, const T *d_xval, const T *d_yval, "
            "uint32_t dphase0, uint32_t *d_last, T *d_omag, T *d_ofreq, void *d_work, "
            "void *stream);" % (w, head)).replace("T", t))
    # behind the FM mixer banks, in front of the clocked view
    assert text.index("cordic_mixbank_create16(") < text.index("cordic_plan_fm_rx_workspace(")
    assert text.index("cordic_plan_fm_rx16(") < text.index("clocked view (streaming shim)")
    from cordic_amd import _native
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
        assert name in _native.ABI
    for name in ("fm_rx", "fm_rx16", "fm_rx_info", "fm_rx16_info", "fm_rx_workspace",
                 "fm_rx16_workspace"):
        assert callable(getattr(ca.Plan, name))
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_header_with_the_new_block_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { const cordic_plan *p = 0; const cordic_config *c = 0;\n'
        'int32_t f, t; int32_t *a = 0; int16_t *h = 0; uint32_t *w = 0;\n'
        'size_t b = cordic_plan_fm_rx_workspace(p, c, 8) + cordic_plan_fm_rx16_workspace(p, c, 8);\n'
        'return cordic_plan_fm_rx_info(p, c, &f, &t) + cordic_plan_fm_rx16_info(p, c, &f, &t)\n'
        ' + cordic_plan_fm_rx(p, c, 0, w, w, 0, w, a, a, 0, w, a, a, 0, 0)\n'
        ' + cordic_plan_fm_rx16(p, c, 0, w, w, 0, w, h, h, 0, w, h, h, 0, 0) + (int)b; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def rx(L, w, plan, conv, n=0):
    return getattr(L, "cordic_plan_fm_rx" + w)(plan, conv, n, None, None, 0, None, None,
                                              None, 0, None, None, None, None, None)


def test_null_handles_and_modes_are_refused_without_a_device_in_the_documented_order():
    """(the WW 38 plan has no seed table and needs no device)"""
    L = ca.lib()
    plan = ca.Plan(MIX.both("ww38")[0])
    cfg3 = DEM.both("cfg3")[0]
    rot = MIX.both("ww38")[0]                       # a rotator as the converter
    for w in ("", "16"):
        info = getattr(L, "cordic_plan_fm_rx%s_info" % w)
        size = getattr(L, "cordic_plan_fm_rx%s_workspace" % w)
        f, t = C.c_int32(-5), C.c_int32(-5)
        for p, c, want in ((None, cfg3.ref, ca.ERR_ARGS), (plan._h, None, ca.ERR_ARGS),
                           (None, None, ca.ERR_ARGS), (plan._h, rot.ref, ca.ERR_MODE)):
            assert info(p, c, C.byref(f), C.byref(t)) == want
            assert (f.value, t.value) == (-5, -5)
            assert size(p, c, 1 << 20) == 0
            for n in (0, 8):
                assert rx(L, w, p, c, n) == want
    # the mixer's mode first: a converter handed in as the plan
    conv_plan = ca.Plan(DEM.both("r2p32")[0])       # WW 40: no device either
    assert L.cordic_plan_fm_rx_info(conv_plan._h, rot.ref, None, None) == ca.ERR_MODE
    assert L.cordic_plan_fm_rx_info(conv_plan._h, cfg3.ref, None, None) == ca.ERR_MODE
    conv_plan.close()
    # the 16-bit form: the containers behind the modes
    assert L.cordic_plan_fm_rx16_info(plan._h, cfg3.ref, None, None) == ca.ERR_CONTAINER
    assert L.cordic_plan_fm_rx16_info(plan._h, rot.ref, None, None) == ca.ERR_MODE
    assert rx(L, "16", plan._h, cfg3.ref, 0) == ca.ERR_CONTAINER
    # a good pair: not fused, either out-pointer may be NULL, n = 0 is a no-op
    assert plan.fm_rx_info(cfg3) == (0, 0)
    assert L.cordic_plan_fm_rx_info(plan._h, cfg3.ref, None, None) == 0
    assert rx(L, "", plan._h, cfg3.ref, 0) == 0
    # with n > 0 the arrays are asked for, on the host
    assert rx(L, "", plan._h, cfg3.ref, 8) == ca.ERR_ARGS
    plan.close()


# (entry point, container, interleaved, decimating)
SINGLE_CALLS = (("cordic_plan_fm_rx", 4, False, False), ("cordic_plan_fm_rx16", 2, False, False),
                ("cordic_plan_fm_rx_c16", 2, True, False),
                ("cordic_plan_fm_rx_decim", 4, False, True),
                ("cordic_plan_fm_rx_decim16", 2, False, True),
                ("cordic_plan_fm_rx_decim_c16", 2, True, True))
# the cases of the *_c16 forms that tests/test_fm_rx_c16_host.py pins already
PINNED_C16 = {"NULL plan", "NULL converter", "converter in a p2r mode", "plan too wide",
              "converter's PW too wide", "k = 9", "n no multiple of 2^k"}


def test_the_status_codes_of_all_six_single_calls_and_their_queries_in_one_table():
    """Every single-call receiver entry point and its _workspace query on the
    arguments that are refused before the device is touched, in the order
    include/cordic_amd.h documents: the plan (ARGS, MODE), the converter (ARGS,
    MODE), the plan's container, the converter's, then the shape.  The sample
    arrays are in place (addresses that are never dereferenced), so that ARGS
    for a shape is not the ranges' ARGS; every query answers 0."""
    import test_fm_demod16 as DEM16
    import test_fm_mix16 as MIX16
    L = ca.lib()
    wide = ca.Plan(MIX.both("ww38")[0])             # IW 32: no 16-bit container
    narrow = ca.Plan(MIX16.both("n9")[0])
    polar = ca.Plan(DEM.both("r2p32")[0])           # a converter handed in as the plan
    cfg3 = DEM.both("cfg3")[0]                      # IW 24, PW 24: a wide converter
    conv16 = ca.Config.from_cli(*DEM16.CORES["io16"][0])
    rot = MIX.both("ww38")[0]                       # a rotator as the converter
    a = 0x100000
    for name, es, iq, decim in SINGLE_CALLS:
        plan, conv = (wide, cfg3) if es == 4 else (narrow, conv16)
        cases = [("NULL plan", None, conv.ref, 3, 1024, ca.ERR_ARGS),
                 ("NULL converter", plan._h, None, 3, 1024, ca.ERR_ARGS),
                 ("plan in an r2p mode", polar._h, conv.ref, 3, 1024, ca.ERR_MODE),
                 ("converter in a p2r mode", plan._h, rot.ref, 3, 1024, ca.ERR_MODE)]
        if es == 2:
            cases += [("plan too wide", wide._h, conv.ref, 3, 1024, ca.ERR_CONTAINER),
                      ("converter's PW too wide", plan._h, cfg3.ref, 3, 1024,
                       ca.ERR_CONTAINER)]
        if decim:
            cases += [("k = 9", plan._h, conv.ref, 9, 1024, ca.ERR_ARGS),
                      ("n no multiple of 2^k", plan._h, conv.ref, 3, 1020, ca.ERR_ARGS)]
        for what, p, c, k, n, want in cases:
            if iq and what in PINNED_C16:
                continue
            ks = (k,) if decim else ()
            xy = (2 * a,) if iq else (2 * a, 3 * a)
            rest = (a, None, 0, None) + xy + (0, None, 4 * a, 5 * a, 6 * a, None)
            got = getattr(L, name)(p, c, n, *ks, *rest)
            assert got == want, (name, what, got)
            assert getattr(L, name + "_workspace")(p, c, n, *ks) == 0, (name, what)
            if what != "n no multiple of 2^k":      # in front of "n = 0 is a no-op"
                assert getattr(L, name)(p, c, 0, *ks, *rest) == want, (name, what)
    for h in (wide, narrow, polar):
        h.close()


def test_the_workspace_of_a_pair_that_is_not_fused_holds_the_two_arrays():
    plan = ca.Plan(MIX.both("ww38")[0])
    cfg3 = DEM.both("cfg3")[0]
    last = 0
    for n in SIZES:
        w = plan.fm_rx_workspace(cfg3, n)
        assert w % 16 == 0 and w >= last and (w == 0) == (n == 0), n
        assert w <= 13 * n + 65536 + 128, n
        if n:
            assert w >= plan.fm_mix_workspace(n) + 8 * n + ca.fm_demod_workspace(n), n
        last = w
    plan.close()


def test_the_binding_asks_the_caller_for_the_scratch():
    import torch
    plan = ca.Plan(MIX.both("ww38")[0])
    cfg3 = DEM.both("cfg3")[0]
    a = (0x1000, 0x2000, 0x3000, 0x4000, 0x5000)
    with pytest.raises(TypeError):
        plan.fm_rx(cfg3, *a, n=8)
    short = torch.zeros(plan.fm_rx_workspace(cfg3, 8) - 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        plan.fm_rx(cfg3, *a, short, n=8)
    plan.close()


# ---------------------------------------------------------------- the banks' host layer

FIELDS = ("d_fcw", "d_pm", "d_xval", "d_yval", "d_omag", "d_ofreq", "d_acc", "d_last", "n",
          "phase0", "dphase0", "reserved")


def test_the_job_structs_are_88_bytes_and_their_fields_lie_where_gcc_puts_them(tmp_path):
    from cordic_amd import _native
    src, exe = tmp_path / "o.c", tmp_path / "o"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "cordic_amd.h"\n'
        'int main(void) {\n'
        + "".join('printf("%%zu %%zu\\n", offsetof(cordic_fmrx_job, %s), '
                  'offsetof(cordic_fmrx_job16, %s));\n' % (f, f) for f in FIELDS)
        + 'printf("%zu %zu\\n", sizeof(cordic_fmrx_job), sizeof(cordic_fmrx_job16));\n'
          'return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                        os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [tuple(map(int, l.split())) for l in
            subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n") if l]
    assert rows[-1] == (88, 88) and C.sizeof(_native._CFmRxJob) == 88
    for f, row in zip(FIELDS, rows):
        assert row[0] == row[1] == getattr(_native._CFmRxJob, f).offset, f
    assert [r[0] for r in rows[:-1]] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80]


PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "cordic_fm_rx_bank.h"
#include "cordic_fm_mix_bank.h"
#include "cordic_fm_demod_bank.h"
#include "cordic_table_fm_bank.h"
#include "cordic_fm_rx_decim.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced: job k's arrays lie 2^24 bytes apart
static const uintptr_t kBase = 0x100000000u;
template <typename J> static J rx_job(size_t k, uint64_t n)
{
	J j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t b = kBase + (uintptr_t)k * 0x10000000u;
	const uintptr_t es = sizeof *j.d_xval;
	j.d_fcw = (const uint32_t *)(b + 4 * (k % 4));
	j.d_pm = k % 2 ? (const uint32_t *)(b + 0x1000000u + 4 * (k % 3)) : nullptr;
	j.d_xval = (decltype(j.d_xval))(b + 0x2000000u + es * (k % 5));
	j.d_yval = (decltype(j.d_yval))(b + 0x3000000u + es * (k % 7));
	j.d_omag = (decltype(j.d_omag))(b + 0x4000000u + es * (k % 3));
	j.d_ofreq = (decltype(j.d_ofreq))(b + 0x5000000u + es * (k % 2));
	j.d_acc = k % 3 ? (uint32_t *)(0x6000000000u + 32 * k) : nullptr;
	j.d_last = k % 4 ? (uint32_t *)(0x6000000000u + 32 * k + 16) : nullptr;
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u);
	j.dphase0 = (uint32_t)(k * 0x85ebca77u);
	return j;
}

// the rx rule cuts ragged jobs so that the spans tile [0, n) of every job in
// order, never across a job's end, each with its halo inside the job
template <typename J>
static void check_cut(const std::vector<J> &jobs, uint32_t base, uint32_t cap)
{
	const SpanRule &r = kFmrxbRule;
	const uint64_t es = sizeof *jobs.data()->d_xval;
	std::vector<RxSpan> spans;
	uint32_t live = 0;
	span_cut(r, jobs.size(), RxJobs(jobs.data()), base, cap, &spans, &live);
	EXPECT(spans.size() == span_count(r, jobs.size(), RxJobs(jobs.data()), base, cap));
	size_t at = 0;
	uint32_t seen = 0;
	for (size_t k = 0; k < jobs.size(); k++) {
		const J &jb = jobs[k];
		if (!jb.n)
			continue;
		const uint64_t uj = span_job_units(r, jb.n, base, cap);
		const uint64_t yield = uj * 1024 - 4;
		EXPECT(uj >= base && (uj == base || span_spans_of(r, jb.n, uj / 2) > cap));
		EXPECT(span_spans_of(r, jb.n, uj) <= cap);
		const uint32_t part0 = (uint32_t)at;
		uint64_t s0 = 0;
		for (uint32_t idx = 0; s0 < jb.n; idx++, at++) {
			EXPECT(at < spans.size());
			if (at >= spans.size())
				return;
			const RxSpan &d = spans[at];
			const bool last = s0 + d.n == jb.n;
			EXPECT(d.n >= 1 && d.n <= yield && s0 + d.n <= jb.n);
			EXPECT(last || d.n == yield);	// only a job's last span is short
			EXPECT(s0 == 0 || s0 >= 4);	// the halo lies inside the job
			EXPECT(d.fcw == (uintptr_t)jb.d_fcw + 4 * s0);
			EXPECT(d.pm == (jb.d_pm ? (uintptr_t)jb.d_pm + 4 * s0 : 0));
			EXPECT(d.x == (uintptr_t)jb.d_xval + es * s0);
			EXPECT(d.y == (uintptr_t)jb.d_yval + es * s0);
			EXPECT(d.mag == (uintptr_t)jb.d_omag + es * s0);
			EXPECT(d.freq == (uintptr_t)jb.d_ofreq + es * s0);
			EXPECT(d.acc == (uintptr_t)jb.d_acc && d.last == (uintptr_t)jb.d_last);
			EXPECT(d.phase0 == jb.phase0 && d.dphase0 == jb.dphase0);
			EXPECT(d.start == seen && d.part0 == part0 && d.idx == idx);
			EXPECT(d.flags == ((s0 ? 0u : kSpanFirst) | (last ? kSpanLast : 0u)));
			s0 += d.n;
		}
		EXPECT(s0 == jb.n);
		seen++;
	}
	EXPECT(at == spans.size() && live == seen);
}

template <typename J> static void cuts()
{
	const uint64_t ns[] = {1, 4, 0, 1019, 1020, 1021, 2040, 2041, 5 * 1024 + 3, 0, 3,
		4096ull * 1020, 4096ull * 1020 + 1, 65536, 1500};
	std::vector<J> jobs;
	for (uint64_t n : ns)
		jobs.push_back(rx_job<J>(jobs.size(), n));
	EXPECT(fmrxb_jobs_valid(jobs.size(), RxJobs(jobs.data())));
	for (uint32_t base : {1u, 2u, 4u, 16u})
		for (uint32_t cap : {4096u, 2u, 1u, 7u})
			check_cut(jobs, base, cap);
	// one-pass spans of 1020 samples; the job of 4096 * 1020 + 1 gets two-pass ones
	EXPECT(span_count(kFmrxbRule, jobs.size(), RxJobs(jobs.data()), 1, 4096)
		== 1 + 1 + 1 + 1 + 2 + 2 + 3 + 6 + 1 + 4096 + 2044 + 65 + 2);
}

// the job check: what it refuses, each on an otherwise good pair of jobs
template <typename J> static void checks()
{
	const uint64_t n = 64;
	auto valid = [](std::vector<J> v) { return fmrxb_jobs_valid(v.size(), RxJobs(v.data())); };
	const J a = rx_job<J>(1, n), b = rx_job<J>(2, n);
	const uintptr_t es = sizeof *a.d_xval;
	EXPECT(a.d_acc && a.d_last && b.d_acc && b.d_last);
	EXPECT(valid({a, b}));
	J t = b;
	t.d_last = a.d_last; EXPECT(!valid({a, t}));		// a shared d_last
	t = b; t.d_acc = a.d_acc; EXPECT(!valid({a, t}));	// a shared d_acc
	t = b; t.d_last = a.d_acc; EXPECT(!valid({a, t}));	// one's d_last is the other's d_acc
	t = a; t.d_last = t.d_acc; EXPECT(!valid({t, b}));	// ... or its own
	t = b; t.d_last = (uint32_t *)((uintptr_t)a.d_omag + es * (n - 2));
	EXPECT(!valid({a, t}));					// d_last inside another job's d_omag
	t = b; t.d_last = (uint32_t *)((uintptr_t)a.d_omag + es * n);
	EXPECT(valid({a, t}) == (((uintptr_t)t.d_last & 3u) == 0));	// just behind it: clear
	t = b; t.d_last = (uint32_t *)((uintptr_t)a.d_xval + 4);
	EXPECT(!valid({a, t}));					// ... inside an input
	t = b; t.d_omag = (decltype(t.d_omag))((uintptr_t)a.d_ofreq + es * (n - 1));
	EXPECT(!valid({a, t}));					// output over output
	t = b; t.d_ofreq = (decltype(t.d_ofreq))((uintptr_t)a.d_fcw + 4);
	EXPECT(!valid({a, t}));					// output over input
	t = b; t.d_xval = a.d_xval; t.d_yval = a.d_xval; t.d_fcw = a.d_fcw;
	EXPECT(valid({a, t}));					// inputs may alias
	// misaligned pointers
	t = b; t.d_last = (uint32_t *)((uintptr_t)t.d_last + 2); EXPECT(!valid({a, t}));
	t = b; t.d_acc = (uint32_t *)((uintptr_t)t.d_acc + 1); EXPECT(!valid({a, t}));
	t = b; t.d_fcw = (const uint32_t *)((uintptr_t)t.d_fcw + 2); EXPECT(!valid({a, t}));
	t = b; t.d_pm = (const uint32_t *)((uintptr_t)b.d_fcw + 0x800002u); EXPECT(!valid({a, t}));
	t = b; t.d_xval = (decltype(t.d_xval))((uintptr_t)t.d_xval + es / 2); EXPECT(!valid({a, t}));
	t = b; t.d_omag = (decltype(t.d_omag))((uintptr_t)t.d_omag + 1); EXPECT(!valid({a, t}));
	if (es == 2) {		// shorts sit on the 2-byte grid
		t = b; t.d_xval = (decltype(t.d_xval))((uintptr_t)t.d_xval + 2); EXPECT(valid({a, t}));
	}
	t = b; t.reserved = 1; EXPECT(!valid({a, t}));
	t = b; t.reserved = 1ull << 40; EXPECT(!valid({a, t}));
	t = b; t.n = (~(size_t)0 >> 4) + 1; EXPECT(!valid({a, t}));
	t = b; t.d_omag = nullptr; EXPECT(!valid({a, t}));
	t = b; t.d_fcw = nullptr; EXPECT(!valid({a, t}));
	t = b; t.d_pm = nullptr; t.d_acc = nullptr; t.d_last = nullptr; EXPECT(valid({a, t}));
	// a job of no samples is not looked at
	t = b; t.n = 0; t.d_last = a.d_last; t.reserved = 5; t.d_omag = nullptr; EXPECT(valid({a, t}));
}

// the three existing banks' checks answer as before on their own cases
static void others()
{
	const uint64_t n = 64;
	cordic_fmmix_job m0, m1;
	std::memset(&m0, 0, sizeof m0);
	m0.d_fcw = (const uint32_t *)0x10000; m0.d_xval = (const int32_t *)0x20000;
	m0.d_yval = (const int32_t *)0x30000; m0.d_oxval = (int32_t *)0x40000;
	m0.d_oyval = (int32_t *)0x50000; m0.d_acc = (uint32_t *)0x60000; m0.n = n;
	m1 = m0;
	m1.d_oxval = (int32_t *)0x48000; m1.d_oyval = (int32_t *)0x58000;
	m1.d_acc = (uint32_t *)0x60010;
	auto mix = [](cordic_fmmix_job a, cordic_fmmix_job b) {
		const cordic_fmmix_job v[2] = {a, b};
		return fmxb_jobs_valid(2, MixJobs(v));
	};
	EXPECT(mix(m0, m1));
	cordic_fmmix_job t = m1;
	t.d_acc = m0.d_acc; EXPECT(!mix(m0, t));
	t = m1; t.d_acc = (uint32_t *)0x60012; EXPECT(!mix(m0, t));
	t = m1; t.d_acc = (uint32_t *)((uintptr_t)m0.d_oxval + 8); EXPECT(!mix(m0, t));
	t = m1; t.d_oxval = (int32_t *)((uintptr_t)m0.d_oyval + 4 * (n - 1)); EXPECT(!mix(m0, t));
	t = m1; t.reserved = 1; EXPECT(!mix(m0, t));
	t = m1; t.d_acc = nullptr; EXPECT(mix(m0, t));

	cordic_demod_job d0, d1;
	std::memset(&d0, 0, sizeof d0);
	d0.d_xval = (const int32_t *)0x20000; d0.d_yval = (const int32_t *)0x30000;
	d0.d_omag = (int32_t *)0x40000; d0.d_ofreq = (int32_t *)0x50000;
	d0.d_last = (uint32_t *)0x60000; d0.n = n;
	d1 = d0;
	d1.d_omag = (int32_t *)0x48000; d1.d_ofreq = (int32_t *)0x58000;
	d1.d_last = (uint32_t *)0x60010;
	auto dem = [](cordic_demod_job a, cordic_demod_job b) {
		const cordic_demod_job v[2] = {a, b};
		return fmd_bank_jobs_valid(2, DemodJobs(v));
	};
	EXPECT(dem(d0, d1));
	cordic_demod_job u = d1;
	u.d_last = d0.d_last; EXPECT(!dem(d0, u));
	u = d1; u.d_last = (uint32_t *)0x60011; EXPECT(!dem(d0, u));
	u = d1; u.d_last = (uint32_t *)((uintptr_t)d0.d_ofreq + 4); EXPECT(!dem(d0, u));
	u = d1; u.d_omag = (int32_t *)((uintptr_t)d0.d_xval + 16); EXPECT(!dem(d0, u));
	u = d1; u.d_last = nullptr; EXPECT(dem(d0, u));

	cordic_fmosc_job o0, o1;
	std::memset(&o0, 0, sizeof o0);
	o0.d_fcw = (const uint32_t *)0x10000; o0.d_sin = (int32_t *)0x40000;
	o0.d_cos = (int32_t *)0x50000; o0.d_acc = (uint32_t *)0x60000; o0.n = n;
	o1 = o0;
	o1.d_sin = (int32_t *)0x48000; o1.d_cos = nullptr; o1.d_acc = (uint32_t *)0x60010;
	auto osc = [](cordic_fmosc_job a, cordic_fmosc_job b) {
		const cordic_fmosc_job v[2] = {a, b};
		return fmob_jobs_valid(2, FmJobs(v));
	};
	EXPECT(osc(o0, o1));
	cordic_fmosc_job w = o1;
	w.d_acc = o0.d_acc; EXPECT(!osc(o0, w));
	w = o1; w.d_acc = (uint32_t *)0x60013; EXPECT(!osc(o0, w));
	w = o1; w.d_sin = (int32_t *)((uintptr_t)o0.d_cos + 4 * (n - 1)); EXPECT(!osc(o0, w));
	w = o1; w.d_sin = nullptr; EXPECT(!osc(o0, w));

	// and their rules have neither a halo nor a second word
	EXPECT(kFmxbRule.halo == 0 && kFmxbRule.words == 0);
	EXPECT(kFmrxbRule.halo == 4 && kFmrxbRule.words == 1 && kFmrxbRule.unit == 1024);
	EXPECT(span_spans_of(kFmxbRule, 4096, 2) == 2 && span_spans_of(kFmxbRule, 4097, 2) == 3);
	EXPECT(span_job_units(kFmxbRule, 8 * 1024 + 1, 1, 4) == 4);
}

// ---- the fallbacks' places inside d_work (the layout functions next to the
// *_work_bytes rules): every part begins on the 16-byte grid, holds its bytes,
// ends where the next begins, and the last ends at what the rule returns --
// which is the closed form the rule had before it was written in terms of the
// layout
static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
struct Part { size_t at, bytes; };
template <size_t N>
static void parts_ok(const Part (&p)[N], size_t first, size_t end, size_t rule, size_t closed)
{
	EXPECT(p[0].at == first);
	for (size_t k = 0; k < N; k++) {
		const size_t next = k + 1 < N ? p[k + 1].at : end;
		EXPECT(p[k].at % 16 == 0);
		EXPECT(p[k].at + p[k].bytes <= next);		// no overlap
		EXPECT(p[k].at + up16(p[k].bytes) == next);	// and no hole of a grid step
	}
	EXPECT(end == rule && rule == closed);
}

static void layouts()
{
	const size_t ns[] = {1, 4, 1023, 1024, 1025, 4096};
	const uint32_t ks[] = {0, 1, 3, 8};
	for (size_t n : ns) {
		for (size_t es : {(size_t)4, (size_t)2}) {
			for (uint32_t k : ks) {
				if (n & (((size_t)1 << k) - 1))
					continue;
				const size_t m = n >> k;
				for (size_t mix : {(size_t)160, fmx_work_bytes(false, n), kFmxWorkBytes}) {
					// the receiver: [mixer workspace | tuned x | tuned y |
					// discriminator workspace], m elements in the arrays
					const FmrxLayout r = fmrx_layout(mix, m, es);
					const Part rp[] = {{r.tx, m * es}, {r.ty, m * es},
						{r.demod, fmd_work_bytes(m)}};
					const size_t closed = mix + 2 * up16(m * es) + fmd_work_bytes(m);
					parts_ok(rp, mix, r.end, fmrxd_work_bytes(false, mix, n, k, es), closed);
					if (k == 0)
						EXPECT(fmrx_work_bytes(false, mix, n, es) == closed);
					EXPECT(fmrxd_work_bytes(true, mix, n, k, es) == kFmrxWorkBytes);
					// the decimating mixer's own: [mixer workspace | tx | ty] at
					// the full rate
					const FmxdLayout d = fmxd_layout(mix, n, es);
					const Part dp[] = {{d.tx, n * es}, {d.ty, n * es}};
					parts_ok(dp, mix, d.end, fmxd_work_bytes(false, mix, n, es),
						mix + 2 * up16(n * es));
				}
			}
		}
		// the *_c16 split: [twin | x | y of n shorts], the twin's size rounded up
		for (size_t twin : {(size_t)16544, (size_t)16544 + 8, (size_t)1}) {
			const FmrxC16Layout c = fmrx_c16_layout(twin, n);
			const Part cp[] = {{c.x, n * 2}, {c.y, n * 2}};
			parts_ok(cp, up16(twin), c.end, fmrx_c16_work_bytes(false, twin, n),
				up16(twin) + 2 * up16(n * 2));
			EXPECT(fmrx_c16_work_bytes(true, twin, n) == twin);
		}
		// the 16-bit mixer: [the 32-bit call's workspace | x | y | ox | oy] as int32
		for (bool f32 : {false, true}) {
			const size_t mix = fmx_work_bytes(f32, n);
			const Fmx16Layout w = fmx16_layout(mix, n);
			const Part wp[] = {{w.x, n * 4}, {w.y, n * 4}, {w.ox, n * 4}, {w.oy, n * 4}};
			parts_ok(wp, mix, w.end, fmx16_work_bytes(false, f32, n), mix + 4 * up16(n * 4));
		}
	}
	EXPECT(fmrx_work_bytes(false, 160, 0, 4) == 0 && fmrx_c16_work_bytes(false, 0, 0) == 0
		&& fmxd_work_bytes(false, 160, 0, 2) == 0 && fmx16_work_bytes(false, false, 0) == 0);
}
static_assert(fmrx_layout(160, 1024 >> 3, 2).tx == 160
	&& fmrx_layout(160, 1024 >> 3, 2).ty == 160 + 256
	&& fmrx_layout(160, 1024 >> 3, 2).demod == 160 + 512
	&& fmrx_layout(160, 1024 >> 3, 2).end == 160 + 512 + fmd_work_bytes(128), "k = 3, shorts");
static_assert(fmrx_layout(32, 1025, 4).ty == 32 + 4112 && fmrxd_work_bytes(false, 32, 1025, 0, 4)
	== 32 + 2 * 4112 + fmd_work_bytes(1025), "a partial grid step behind each array");
static_assert(fmrx_c16_layout(24, 1023).x == 32 && fmrx_c16_layout(24, 1023).y == 32 + 2048
	&& fmrx_c16_work_bytes(false, 24, 1023) == 32 + 4096, "the twin's size rounded up");
static_assert(fmxd_layout(48, 4, 2).ty == 64 && fmxd_work_bytes(false, 48, 4, 2) == 80,
	"two arrays of one grid step");
static_assert(fmx16_layout(16, 1).oy == 16 + 48 && fmx16_layout(16, 1).end == 16 + 64,
	"four widened arrays");

int main()
{
	layouts();
	cuts<cordic_fmrx_job>();
	cuts<cordic_fmrx_job16>();
	checks<cordic_fmrx_job>();
	checks<cordic_fmrx_job16>();
	others();
	if (!failures)
		std::printf("rx bank host ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_rx_rule_and_the_job_checks_under_address_and_ub_sanitizers(tmp_path):
    """a stand-alone C++ program with its own main: no Python and no GPU in the
    checked process, as tests/test_span_bank_host.py"""
    src, exe = tmp_path / "rx_bank.cpp", tmp_path / "rx_bank"
    src.write_text(PROGRAM)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "cordic_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
         str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "rx bank host ok" in r.stdout


def test_the_prologue_and_the_chooser_are_shared_not_pasted():
    """one block prologue and one instance chooser for fm_mix_xydir,
    fm_mixbank_xydir, fm_rx_xydir, fm_rxbank_xydir and their decimating forms, in
    cordic_fm_mix.h; one list of the receiver's units, in cordic_fm_rx_unit.h"""
    import glob
    csrc = os.path.join(ROOT, "cordic_amd", "csrc")
    receivers = ("cordic_fm_rx.hip", "cordic_fm_rx_bank.hip", "cordic_fm_rx_decim.hip",
                 "cordic_fm_rx_bank_decim.hip")
    names = ("cordic_fm_mix.h", "cordic_fm_rx.h", "cordic_fm_demod.h", "cordic_fm_mix.hip",
             "cordic_fm_mix_bank.hip") + receivers + (
             "cordic_fm_mix_decim.hip", "cordic_fm_mix_bank_decim.hip")
    text = {n: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, n)).read()) for n in names}

    def places(pattern):
        return [n for n in names for _ in re.finditer(pattern, text[n])]

    # the switch over the stage counts (the macro's own definition aside)
    assert places(r"(?<!#define )FMX_STAGES\(X\)") == ["cordic_fm_mix.h"]
    assert places(r"__builtin_trap") == ["cordic_fm_mix.h"]
    # the staging of the tables: one call (its definition has no `<` behind the name)
    assert places(r"\bstage_tables<") == ["cordic_fm_mix.h"]
    # every kernel goes through the two pieces, and every launcher through the switch
    for unit in names[3:]:
        assert len(re.findall(r"\bblock_begin<LJ, NLIVE, IO>\(", text[unit])) == 1, unit
        assert len(re.findall(r"\bblock_ready<LJ, NLIVE>\(", text[unit])) == 1, unit
        assert len(re.findall(r"\bwith_stages\(", text[unit])) >= 1, unit
        assert "static_assert(LJ ==" not in text[unit], unit
        assert not re.search(r"switch\s*\(nlive\)", text[unit]), unit
    # "WW 35 is LJ 29" and "no Io16 at WW 35" have one home
    assert places(r"ww\s*(==|<|>=)\s*35") == ["cordic_fm_mix.h"] * 2

    # the receiver's units: no ladder over a unit macro in the four sources ...
    for unit in receivers:
        assert not re.search(r"#\s*elif[^\n]*UNIT", text[unit]), unit
        assert not re.search(r"#\s*define\s+CORDIC_FM\w*_UNIT\b", text[unit]), unit
        assert '#include "cordic_fm_rx_unit.h"' in text[unit], unit
    # ... the list defined once and expanded, never written out again: a suffix
    # behind the first stands in the list and nowhere else in the sources
    every = {os.path.basename(f): re.sub(r"//[^\n]*", "", open(f).read())
             for f in glob.glob(os.path.join(csrc, "*")) if f.endswith((".h", ".hip", ".cpp"))}
    defs = [n for n, t in every.items() for _ in re.finditer(r"#\s*define\s+CORDIC_FMRX_UNITS\b", t)]
    assert defs == ["cordic_fm_rx_unit.h"]
    unit_h = every["cordic_fm_rx_unit.h"]
    entries = re.findall(r"\bX\((\w+), (\d+), ([\w:]+)\)", unit_h[unit_h.index("CORDIC_FMRX_UNITS(X)"):]
                         .split("\n\n")[0])
    assert entries == [("lj30", "30", "Io32"), ("lj29", "29", "Io32"), ("io16", "30", "Io16"),
                       ("c16", "30", "fmx::IoC16")]
    assert "static_assert(fmx::unit_of(" in unit_h       # each position pinned to fmx::Unit
    for n, t in every.items():
        if n.startswith("cordic_fm_rx") or n == "cordic_fm_mix.h":
            hits = re.findall(r"\blaunch_rx\w*_(?:lj30|lj29|io16|c16)\b", t)
            assert not hits, (n, hits)
    for unit in ("cordic_fm_rx.hip", "cordic_fm_rx_bank.hip"):
        assert len(re.findall(r"CORDIC_FMRX_UNITS\((?:PLAIN|DECIM)\)", text[unit])) == 2, unit
    # ... no entry point named in a brace-initialised array
    for n, t in every.items():
        for m in re.finditer(r"=\s*\{[^;]*\}\s*;", t):
            assert not re.search(r"\blaunch_rx(d|bank)?\w*\b(?!##)", m.group(0)), (n, m.group(0))
    # ... and no source that only sets the macro and includes another
    for tail in ("lj29", "io16", "c16"):
        assert not glob.glob(os.path.join(csrc, "cordic_fm_rx*_%s.hip" % tail)), tail
    make = open(os.path.join(csrc, "Makefile")).read()
    assert make.count("-DCORDIC_FMRX_UNIT=") == 1
