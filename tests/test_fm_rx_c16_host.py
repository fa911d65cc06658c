"""The tuned FM receiver on interleaved int16 I/Q (cordic_plan_fm_rx_c16,
cordic_plan_fm_rx_decim_c16, cordic_rxbank_create_c16 and _create_decim_c16;
include/cordic_amd.h): what needs no GPU -- the declarations, the export, the
binding, the status codes in the *16 twins' order, the workspace sizes and the
banks' host layer on interleaved jobs."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cordic_amd as ca
import test_fm_demod as DEM
import test_fm_demod16 as DEM16
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
from test_fm_rx_host import SIZES, declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_plan_fm_rx_c16_workspace", "cordic_plan_fm_rx_c16_info",
         "cordic_plan_fm_rx_c16", "cordic_plan_fm_rx_decim_c16_workspace",
         "cordic_plan_fm_rx_decim_c16", "cordic_rxbank_create_c16",
         "cordic_rxbank_create_decim_c16")
FIELDS = ("d_fcw", "d_pm", "d_iq", "d_omag", "d_ofreq", "d_acc", "d_last", "n", "phase0",
          "dphase0", "reserved")


def io16():
    return ca.Config.from_cli(*DEM16.CORES["io16"][0])


def test_the_functions_and_the_struct_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    head = "const cordic_plan *plan, const cordic_config *conv, "
    tail = ("const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, "
            "const int16_t *d_iq, uint32_t dphase0, uint32_t *d_last, int16_t *d_omag, "
            "int16_t *d_ofreq, void *d_work, void *stream);")
    assert declared(text, "size_t cordic_plan_fm_rx_c16_workspace(%ssize_t n);" % head)
    assert declared(text, "int cordic_plan_fm_rx_c16_info(%sint32_t *fused, int32_t *tile);"
                    % head)
    assert declared(text, "int cordic_plan_fm_rx_c16(%ssize_t n, %s" % (head, tail))
    assert declared(text, "size_t cordic_plan_fm_rx_decim_c16_workspace(%ssize_t n, "
                          "uint32_t log2r);" % head)
    assert declared(text, "int cordic_plan_fm_rx_decim_c16(%ssize_t n, uint32_t log2r, %s"
                    % (head, tail))
    assert declared(text, "int cordic_rxbank_create_c16(%ssize_t njobs, const "
                          "cordic_fmrx_job_c16 *jobs, cordic_rxbank **bank);" % head)
    assert declared(text, "int cordic_rxbank_create_decim_c16(%suint32_t log2r, size_t njobs, "
                          "const cordic_fmrx_job_c16 *jobs, cordic_rxbank **bank);" % head)
    assert declared(text, "typedef struct cordic_fmrx_job_c16 { const uint32_t *d_fcw; ")
    # directly behind the decimating receiver banks, in front of the clocked view
    assert text.index("cordic_rxbank_create_decim16(") \
        < text.index("cordic_plan_fm_rx_c16_workspace(") \
        < text.index("cordic_rxbank_create_decim_c16(") \
        < text.index("clocked view (streaming shim)")
    from cordic_amd import _native
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
        assert name in _native.ABI
    for name in ("fm_rx_c16", "fm_rx_c16_info", "fm_rx_c16_workspace", "fm_rx_decim_c16",
                 "fm_rx_decim_c16_workspace"):
        assert callable(getattr(ca.Plan, name))
    assert "RxBankC16" in ca.__all__ and "log2r" in ca.RxBankC16.__init__.__code__.co_varnames
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_header_with_the_new_block_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { const cordic_plan *p = 0; const cordic_config *c = 0;\n'
        'int32_t f, t; int16_t *h = 0; uint32_t *w = 0; cordic_rxbank *b = 0;\n'
        'const cordic_fmrx_job_c16 *j = 0;\n'
        'size_t s = cordic_plan_fm_rx_c16_workspace(p, c, 8)\n'
        ' + cordic_plan_fm_rx_decim_c16_workspace(p, c, 8, 3);\n'
        'return cordic_plan_fm_rx_c16_info(p, c, &f, &t)\n'
        ' + cordic_plan_fm_rx_c16(p, c, 0, w, w, 0, w, h, 0, w, h, h, 0, 0)\n'
        ' + cordic_plan_fm_rx_decim_c16(p, c, 0, 3, w, w, 0, w, h, 0, w, h, h, 0, 0)\n'
        ' + cordic_rxbank_create_c16(p, c, 0, j, &b)\n'
        ' + cordic_rxbank_create_decim_c16(p, c, 3, 0, j, &b) + (int)s; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_job_struct_has_the_size_the_header_states_and_gcc_reports(tmp_path):
    from cordic_amd import _native
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    stated = re.search(r"\}\s*cordic_fmrx_job_c16\s*;\s*/\*\s*(\d+) bytes", text)
    assert stated
    src, exe = tmp_path / "o.c", tmp_path / "o"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "cordic_amd.h"\n'
        'int main(void) {\n'
        + "".join('printf("%%zu\\n", offsetof(cordic_fmrx_job_c16, %s));\n' % f
                  for f in FIELDS)
        + 'printf("%zu\\n", sizeof(cordic_fmrx_job_c16));\nreturn 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                        os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [int(l) for l in
            subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert rows[-1] == int(stated.group(1)) == 80 == C.sizeof(_native._CFmRxJobC16)
    assert rows[:-1] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72]
    for f, at in zip(FIELDS, rows):
        assert getattr(_native._CFmRxJobC16, f).offset == at, f


def rx(L, plan, conv, n=0, k=None, iq=None):
    if k is None:
        return L.cordic_plan_fm_rx_c16(plan, conv, n, None, None, 0, None, iq, 0, None, None,
                                       None, None, None)
    return L.cordic_plan_fm_rx_decim_c16(plan, conv, n, k, None, None, 0, None, iq, 0, None,
                                         None, None, None, None)


def test_the_status_codes_are_the_16_bit_twins_in_their_order_without_a_device():
    """(the WW 38 plan and the 9-stage 16-bit one have no seed table and need no
    device)"""
    L = ca.lib()
    wide = ca.Plan(MIX.both("ww38")[0])             # IW 32: no 16-bit container
    plan = ca.Plan(MIX16.both("n9")[0])
    conv, cfg3 = io16(), DEM.both("cfg3")[0]        # cfg3: IW 24, a wide converter
    rot = MIX.both("ww38")[0]                       # a rotator as the converter
    f, t = C.c_int32(-5), C.c_int32(-5)
    for p, c, want in ((None, conv.ref, ca.ERR_ARGS), (plan._h, None, ca.ERR_ARGS),
                       (None, None, ca.ERR_ARGS), (plan._h, rot.ref, ca.ERR_MODE),
                       (wide._h, rot.ref, ca.ERR_MODE),         # the mode in front of ...
                       (wide._h, conv.ref, ca.ERR_CONTAINER),   # ... the plan's container
                       (plan._h, cfg3.ref, ca.ERR_CONTAINER)):  # and the converter's
        assert L.cordic_plan_fm_rx_c16_info(p, c, C.byref(f), C.byref(t)) == want
        assert L.cordic_plan_fm_rx16_info(p, c, None, None) == want      # the twin's
        assert (f.value, t.value) == (-5, -5)
        assert L.cordic_plan_fm_rx_c16_workspace(p, c, 1 << 20) == 0
        assert L.cordic_plan_fm_rx_decim_c16_workspace(p, c, 1 << 20, 3) == 0
        for n in (0, 8):
            assert rx(L, p, c, n) == want
            assert rx(L, p, c, n, 3) == want
            assert rx(L, p, c, n, 9) == want        # in front of the shape
        if want != ca.ERR_CONTAINER:       # (no jobs at all: the 32-bit rules)
            b = C.c_void_p()
            assert L.cordic_rxbank_create_c16(p, c, 0, None, C.byref(b)) == want
            assert L.cordic_rxbank_create16(p, c, 0, None, C.byref(b)) == want
    # a converter handed in as the plan: the mixer's mode first
    conv_plan = ca.Plan(DEM.both("r2p32")[0])
    assert L.cordic_plan_fm_rx_c16_info(conv_plan._h, conv.ref, None, None) == ca.ERR_MODE
    conv_plan.close()
    # a good pair: not fused, n = 0 is a no-op, the shape, then the arrays
    assert plan.fm_rx_c16_info(conv) == plan.fm_rx16_info(conv) == (0, 0)
    assert L.cordic_plan_fm_rx_c16_info(plan._h, conv.ref, None, None) == 0
    assert rx(L, plan._h, conv.ref, 0) == 0 and rx(L, plan._h, conv.ref, 0, 8) == 0
    a = 0x10000
    for n, k in ((1024, 9), (0, 9), (1020, 3), (255, 8), (1, 1)):
        assert L.cordic_plan_fm_rx_decim_c16(plan._h, conv.ref, n, k, a, None, 0, None, 2 * a,
                                             0, None, 4 * a, 5 * a, 6 * a,
                                             None) == ca.ERR_ARGS, (n, k)
        assert L.cordic_plan_fm_rx_decim_c16_workspace(plan._h, conv.ref, n, k) == 0, (n, k)
    # NULL d_iq with n > 0 (everything else in place), and d_iq off its 4-byte grid
    for k in (None, 3):
        args = lambda iq: ((plan._h, conv.ref, 8) + (() if k is None else (k,))
                           + (a, None, 0, None, iq, 0, None, 4 * a, 5 * a, 6 * a, None))
        fn = L.cordic_plan_fm_rx_c16 if k is None else L.cordic_plan_fm_rx_decim_c16
        assert fn(*args(None)) == ca.ERR_ARGS
        assert fn(*args(2 * a + 2)) == ca.ERR_ARGS
    assert rx(L, plan._h, conv.ref, 8) == ca.ERR_ARGS
    # the bank's creates: a NULL bank pointer or NULL jobs first, then the pair
    b = C.c_void_p()
    assert L.cordic_rxbank_create_c16(plan._h, conv.ref, 0, None, None) == ca.ERR_ARGS
    assert L.cordic_rxbank_create_c16(wide._h, conv.ref, 2, None, C.byref(b)) == ca.ERR_ARGS
    assert L.cordic_rxbank_create_decim_c16(plan._h, rot.ref, 3, 0, None,
                                            C.byref(b)) == ca.ERR_MODE
    wide.close()
    plan.close()


def test_the_workspace_of_a_pair_that_is_not_fused_is_the_twins_and_two_arrays_of_shorts():
    a16 = lambda b: (b + 15) // 16 * 16
    plan, conv = ca.Plan(MIX16.both("n9")[0]), io16()
    assert plan.fm_rx16_info(conv) == (0, 0)
    last = 0
    for n in SIZES:
        w = plan.fm_rx_c16_workspace(conv, n)
        assert w % 16 == 0 and w >= last and (w == 0) == (n == 0), n
        assert w == (a16(plan.fm_rx16_workspace(conv, n)) + 2 * a16(2 * n) if n else 0), n
        assert w <= plan.fm_rx16_workspace(conv, n) + 4 * n + 32, n
        assert plan.fm_rx_decim_c16_workspace(conv, n, 0) == w, n
        last = w
    for k in (1, 3, 8):
        last = 0
        for n in sorted({0, 1 << k, 3 << k, 256, 1024, 1024 + (1 << k), 1 << 20, 1 << 33}):
            w = plan.fm_rx_decim_c16_workspace(conv, n, k)
            twin = plan.fm_rx_decim16_workspace(conv, n, k)
            assert w % 16 == 0 and w >= last and (w == 0) == (n == 0), (k, n)
            assert w == (a16(twin) + 2 * a16(2 * n) if n else 0), (k, n)
            assert w <= twin + 4 * n + 32, (k, n)
            last = w
    plan.close()


def test_the_binding_asks_for_shorts_and_for_the_scratch():
    import torch
    plan, conv = ca.Plan(MIX16.both("n9")[0]), io16()
    a32 = torch.zeros(16, dtype=torch.int32)
    a16 = torch.zeros(16, dtype=torch.int16)
    with pytest.raises((TypeError, ValueError)):    # an int32 tensor for iq
        plan.fm_rx_c16(conv, a32, a32, a16, a16, a16, n=8)
    with pytest.raises((TypeError, ValueError)):
        plan.fm_rx_decim_c16(conv, 3, a32, a32, a16, a16, a16, n=8)
    with pytest.raises((TypeError, ValueError)):    # ... or for an output
        plan.fm_rx_c16(conv, a32, a16, a32, a16, a16, n=8)
    with pytest.raises((TypeError, ValueError)):
        ca.RxBankC16(plan, conv, [(a32, None, a32, a16, a16, 8, 0, None, 0, None)])
    with pytest.raises(TypeError):                  # no scratch
        plan.fm_rx_c16(conv, 0x1000, 0x2000, 0x3000, 0x4000, n=8)
    short = torch.zeros(plan.fm_rx_c16_workspace(conv, 8) - 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        plan.fm_rx_c16(conv, 0x1000, 0x2000, 0x3000, 0x4000, short, n=8)
    plan.close()


# ---------------------------------------------------------------- the banks' host layer

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "cordic_fm_rx_bank.h"
#include "cordic_hostargs.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced
static cordic_fmrx_job_c16 job(size_t k, uint64_t n)
{
	cordic_fmrx_job_c16 j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t b = 0x100000000u + (uintptr_t)k * 0x10000000u;
	j.d_fcw = (const uint32_t *)(b + 4 * (k % 4));
	j.d_pm = k % 2 ? (const uint32_t *)(b + 0x1000000u) : nullptr;
	j.d_iq = (const int16_t *)(b + 0x2000000u + 4 * (k % 5));
	j.d_omag = (int16_t *)(b + 0x4000000u + 2 * (k % 3));
	j.d_ofreq = (int16_t *)(b + 0x5000000u + 2 * (k % 2));
	j.d_acc = (uint32_t *)(0x6000000000u + 32 * k);
	j.d_last = (uint32_t *)(0x6000000000u + 32 * k + 16);
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u);
	j.dphase0 = (uint32_t)(k * 0x85ebca77u);
	return j;
}

static bool valid(std::vector<cordic_fmrx_job_c16> v, uint32_t k = 0)
{
	std::vector<cordic_fmrx_job16> s;
	for (const auto &j : v)
		s.push_back(fmrxb_from_c16(j));
	return fmrxb_jobs_valid(s.size(), RxJobs(s.data(), k, true));
}

int main()
{
	const uint64_t n = 64;
	const cordic_fmrx_job_c16 a = job(1, n), b = job(2, n);
	EXPECT(valid({a, b}));
	cordic_fmrx_job_c16 t = b;
	// d_iq's range is 4 n bytes: an output in its second half is an overlap ...
	t.d_omag = (int16_t *)((uintptr_t)a.d_iq + 2 * n);	EXPECT(!valid({a, t}));
	t = b; t.d_ofreq = (int16_t *)((uintptr_t)a.d_iq + 4 * n - 2); EXPECT(!valid({a, t}));
	t = b; t.d_last = (uint32_t *)((uintptr_t)a.d_iq + 4 * n - 4); EXPECT(!valid({a, t}));
	t = b; t.d_acc = (uint32_t *)((uintptr_t)a.d_iq + 2 * n + 4); EXPECT(!valid({a, t}));
	// ... in its first half too, and just behind it is clear
	t = b; t.d_omag = (int16_t *)((uintptr_t)a.d_iq + 6); EXPECT(!valid({a, t}));
	t = b; t.d_omag = (int16_t *)((uintptr_t)a.d_iq + 4 * n); EXPECT(valid({a, t}));
	t = b; t.d_last = (uint32_t *)((uintptr_t)a.d_iq + 4 * n); EXPECT(valid({a, t}));
	// a job's own output in its own d_iq
	t = a; t.d_omag = (int16_t *)((uintptr_t)a.d_iq + 4 * n - 2); EXPECT(!valid({t, b}));
	// inputs may alias; d_iq sits on the 4-byte grid, any of it
	t = b; t.d_iq = a.d_iq; EXPECT(valid({a, t}));
	for (unsigned off = 0; off < 16; off++) {
		t = b; t.d_iq = (const int16_t *)((uintptr_t)b.d_iq + off);
		EXPECT(valid({a, t}) == (off % 4 == 0));
	}
	t = b; t.d_iq = nullptr; EXPECT(!valid({a, t}));
	t = b; t.d_omag = (int16_t *)((uintptr_t)b.d_omag + 1); EXPECT(!valid({a, t}));
	t = b; t.d_omag = (int16_t *)((uintptr_t)b.d_omag + 2); EXPECT(valid({a, t}));
	t = b; t.reserved = 1; EXPECT(!valid({a, t}));
	t = b; t.n = (~(size_t)0 >> 4) + 1; EXPECT(!valid({a, t}));
	t = b; t.n = 0; t.d_iq = nullptr; t.reserved = 5; EXPECT(valid({a, t}));
	// a decimating bank: n % R, k <= 8, outputs of n >> k shorts
	EXPECT(valid({a, b}, 3) && !valid({a, b}, 9));
	t = b; t.n = 68; EXPECT(valid({a, t}, 2) && !valid({a, t}, 3));
	t = b; t.d_last = (uint32_t *)((uintptr_t)a.d_omag + 2 * (n >> 3) + 2);
	EXPECT(valid({a, t}, 3) == (((uintptr_t)t.d_last & 3u) == 0) && !valid({a, t}, 0));

	// the spans: x carries d_iq at 4 bytes a sample, the outputs 2 (>> k), y nothing
	for (uint32_t k : {0u, 3u}) {
		std::vector<cordic_fmrx_job16> s = {fmrxb_from_c16(job(0, 5 * 1024 + 8)),
			fmrxb_from_c16(job(3, 0)), fmrxb_from_c16(job(4, 1024))};
		const SpanRule r = fmrxb_rule(k);
		std::vector<RxSpan> spans;
		uint32_t live = 0;
		span_cut(r, s.size(), RxJobs(s.data(), k, true), 1, 4096, &spans, &live);
		EXPECT(live == 2 && spans.size() == span_count(r, s.size(), RxJobs(s.data(), k, true), 1, 4096));
		uint64_t s0 = 0;
		size_t j = 0;
		for (const RxSpan &d : spans) {
			if (s0 == s[j].n) {
				s0 = 0;
				j = 2;
			}
			EXPECT(d.fcw == (uintptr_t)s[j].d_fcw + 4 * s0);
			EXPECT(d.x == (uintptr_t)s[j].d_xval + 4 * s0 && d.y == 0);
			EXPECT(d.mag == (uintptr_t)s[j].d_omag + 2 * (s0 >> k));
			EXPECT(d.freq == (uintptr_t)s[j].d_ofreq + 2 * (s0 >> k));
			EXPECT(s0 % ((uint64_t)1 << k) == 0 && (s0 == 0 || s0 >= r.halo));
			s0 += d.n;
		}
		EXPECT(j == 2 && s0 == s[2].n);
	}

	// the single call's check: d_iq in the place of the pair
	const uintptr_t A = 0x10000;
	auto ok = [&](const void *iq, const void *o0, const void *last, unsigned k = 0) {
		return iq_call_ok(n, nullptr, last, (void *)A, nullptr, iq, nullptr, o0,
			(void *)(5 * A), 2, (void *)(6 * A), 64, k, true);
	};
	EXPECT(ok((void *)(2 * A), (void *)(4 * A), nullptr));
	EXPECT(ok((void *)(2 * A + 4), (void *)(4 * A), nullptr));
	EXPECT(ok((void *)(2 * A + 12), (void *)(4 * A + 2), nullptr));
	EXPECT(!ok((void *)(2 * A + 2), (void *)(4 * A), nullptr));
	EXPECT(!ok(nullptr, (void *)(4 * A), nullptr));
	EXPECT(!ok((void *)(2 * A), (void *)(2 * A + 4 * n - 2), nullptr));
	EXPECT(ok((void *)(2 * A), (void *)(2 * A + 4 * n), nullptr));
	EXPECT(!ok((void *)(2 * A), (void *)(4 * A), (void *)(2 * A + 4 * n - 4)));
	EXPECT(ok((void *)(2 * A), (void *)(4 * A), (void *)(2 * A + 4 * n)));
	EXPECT(!ok((void *)(6 * A + 32), (void *)(4 * A), nullptr));	// d_work over d_iq
	// and the split form asks for d_y as before
	EXPECT(!iq_call_ok(n, nullptr, nullptr, (void *)A, nullptr, (void *)(2 * A), nullptr,
		(void *)(4 * A), (void *)(5 * A), 2, (void *)(6 * A), 64));
	EXPECT(iq_call_ok(n, nullptr, nullptr, (void *)A, nullptr, (void *)(2 * A + 2),
		(void *)(3 * A), (void *)(4 * A), (void *)(5 * A), 2, (void *)(6 * A), 64));
	if (!failures)
		std::printf("rx c16 host ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_job_checks_and_the_spans_of_interleaved_jobs_under_sanitizers(tmp_path):
    """a stand-alone C++ program with its own main: no Python and no GPU in the
    checked process, as tests/test_fm_rx_host.py"""
    src, exe = tmp_path / "rx_c16.cpp", tmp_path / "rx_c16"
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
    assert "rx c16 host ok" in r.stdout
