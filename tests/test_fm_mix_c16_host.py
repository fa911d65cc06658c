"""The FM mixer on interleaved int16 I/Q, in and out (cordic_plan_fm_mix_c16,
cordic_plan_fm_mix_decim_c16, cordic_mixbank_create_c16 and _create_decim_c16;
include/cordic_amd.h): what needs no GPU -- the declarations, the export, the
binding, the status codes in the *16 twins' order, the workspace sizes and the
banks' host layer on interleaved jobs."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cordic_amd as ca
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
from test_fm_rx_host import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cordic_plan_fm_mix_c16_info", "cordic_plan_fm_mix_c16_workspace",
         "cordic_plan_fm_mix_c16", "cordic_plan_fm_mix_decim_c16_workspace",
         "cordic_plan_fm_mix_decim_c16", "cordic_mixbank_create_c16",
         "cordic_mixbank_create_decim_c16")
FIELDS = ("d_fcw", "d_pm", "d_iq", "d_oiq", "d_acc", "n", "phase0", "reserved")
OFFSETS = [0, 8, 16, 24, 32, 40, 48, 52]


def test_the_functions_and_the_struct_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    tail = ("const uint32_t *d_fcw, const uint32_t *d_pm, uint32_t phase0, uint32_t *d_acc, "
            "const int16_t *d_iq, int16_t *d_oiq, void *d_work, void *stream);")
    assert declared(text, "int cordic_plan_fm_mix_c16_info(const cordic_plan *plan, "
                          "int32_t *fused, int32_t *tile);")
    assert declared(text, "size_t cordic_plan_fm_mix_c16_workspace(const cordic_plan *plan, "
                          "size_t n);")
    assert declared(text, "int cordic_plan_fm_mix_c16(const cordic_plan *plan, size_t n, " + tail)
    assert declared(text, "size_t cordic_plan_fm_mix_decim_c16_workspace(const cordic_plan "
                          "*plan, size_t n, uint32_t log2r);")
    assert declared(text, "int cordic_plan_fm_mix_decim_c16(const cordic_plan *plan, size_t n, "
                          "uint32_t log2r, " + tail)
    assert declared(text, "int cordic_mixbank_create_c16(const cordic_plan *plan, size_t njobs, "
                          "const cordic_fmmix_job_c16 *jobs, cordic_mixbank **bank);")
    assert declared(text, "int cordic_mixbank_create_decim_c16(const cordic_plan *plan, "
                          "uint32_t log2r, size_t njobs, const cordic_fmmix_job_c16 *jobs, "
                          "cordic_mixbank **bank);")
    assert declared(text, "typedef struct cordic_fmmix_job_c16 { const uint32_t *d_fcw; ")
    # a block of its own directly behind the receivers' *_c16 block, in front of
    # the clocked view
    assert text.index("cordic_rxbank_create_decim_c16(const") \
        < text.index("cordic_plan_fm_mix_c16_info(const") \
        < text.index("cordic_mixbank_create_decim_c16(const") \
        < text.index("clocked view (streaming shim)")
    between = text[text.index("cordic_rxbank_create_decim_c16(const"):
                   text.index("cordic_plan_fm_mix_c16_info(const")]
    # (nothing but the block's comment between the two; the last line is the
    # new declaration's own return type)
    assert not re.search(r"^(int|size_t|typedef)\b",
                         between.split(";", 1)[1].rsplit("\n", 1)[0], re.M)
    from cordic_amd import _native
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
        assert name in _native.ABI
    for name in ("fm_mix_c16", "fm_mix_c16_info", "fm_mix_c16_workspace", "fm_mix_decim_c16",
                 "fm_mix_decim_c16_workspace"):
        assert callable(getattr(ca.Plan, name))
    assert "MixBankC16" in ca.__all__
    assert "log2r" in ca.MixBankC16.__init__.__code__.co_varnames
    assert ca.MixBankC16.__init__.__defaults__ == (0,)
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


def test_the_header_with_the_new_block_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { const cordic_plan *p = 0;\n'
        'int32_t f, t; int16_t *h = 0; uint32_t *w = 0; cordic_mixbank *b = 0;\n'
        'const cordic_fmmix_job_c16 *j = 0;\n'
        'size_t s = cordic_plan_fm_mix_c16_workspace(p, 8)\n'
        ' + cordic_plan_fm_mix_decim_c16_workspace(p, 8, 3);\n'
        'return cordic_plan_fm_mix_c16_info(p, &f, &t)\n'
        ' + cordic_plan_fm_mix_c16(p, 0, w, w, 0, w, h, h, 0, 0)\n'
        ' + cordic_plan_fm_mix_decim_c16(p, 0, 3, w, w, 0, w, h, h, 0, 0)\n'
        ' + cordic_mixbank_create_c16(p, 0, j, &b)\n'
        ' + cordic_mixbank_create_decim_c16(p, 3, 0, j, &b) + (int)s; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_job_struct_has_the_layout_of_the_header_gcc_and_the_ctypes_mirror(tmp_path):
    from cordic_amd import _native
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    stated = re.search(r"\}\s*cordic_fmmix_job_c16\s*;\s*/\*\s*(\d+) bytes", text)
    assert stated
    body = text[text.index("typedef struct cordic_fmmix_job_c16 {"):stated.start()]
    # the header's comment states every offset next to its field
    said = [(m.group(1), int(m.group(2))) for m in
            re.finditer(r"\*?(\w+);\s*/\*\s*offset\s+(\d+)", body)]
    assert said == list(zip(FIELDS, OFFSETS))
    src, exe = tmp_path / "o.c", tmp_path / "o"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "cordic_amd.h"\n'
        'int main(void) {\n'
        + "".join('printf("%%zu\\n", offsetof(cordic_fmmix_job_c16, %s));\n' % f
                  for f in FIELDS)
        + 'printf("%zu\\n", sizeof(cordic_fmmix_job_c16));\nreturn 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I",
                        os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [int(l) for l in
            subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert rows[-1] == int(stated.group(1)) == 56 == C.sizeof(_native._CFmMixJobC16)
    assert rows[:-1] == OFFSETS
    for f, at in zip(FIELDS, rows):
        assert getattr(_native._CFmMixJobC16, f).offset == at, f


def mix(L, plan, n=0, k=None, iq=None, oiq=None):
    if k is None:
        return L.cordic_plan_fm_mix_c16(plan, n, None, None, 0, None, iq, oiq, None, None)
    return L.cordic_plan_fm_mix_decim_c16(plan, n, k, None, None, 0, None, iq, oiq, None, None)


def twin(L, plan, n=0, k=None):
    if k is None:
        return L.cordic_plan_fm_mix16(plan, n, None, None, 0, None, None, None, None, None,
                                      None, None)
    return L.cordic_plan_fm_mix_decim16(plan, n, k, None, None, 0, None, None, None, None,
                                        None, None, None)


def test_the_status_codes_are_the_16_bit_twins_in_their_order_without_a_device():
    """(the WW 38 plan, the 9-stage 16-bit one and the converter have no seed
    table and need no device)"""
    import test_fm_demod as DEM
    L = ca.lib()
    wide = ca.Plan(MIX.both("ww38")[0])             # IW 32: no 16-bit container
    plan = ca.Plan(MIX16.both("n9")[0])
    conv = ca.Plan(DEM.both("r2p32")[0])            # the wrong mode AND the wrong container
    f, t = C.c_int32(-5), C.c_int32(-5)
    for p, want in ((None, ca.ERR_ARGS), (conv._h, ca.ERR_MODE), (wide._h, ca.ERR_CONTAINER)):
        assert L.cordic_plan_fm_mix_c16_info(p, C.byref(f), C.byref(t)) == want
        assert (f.value, t.value) == (-5, -5)
        assert L.cordic_plan_fm_mix_c16_workspace(p, 1 << 20) == 0
        assert L.cordic_plan_fm_mix_decim_c16_workspace(p, 1 << 20, 3) == 0
        for n in (0, 8, 1021):
            assert mix(L, p, n) == want == twin(L, p, n)
            assert mix(L, p, n, 3) == want == twin(L, p, n, 3)   # in front of n % R
            assert mix(L, p, n, 9) == want == twin(L, p, n, 9)   # in front of k > 8
        b = C.c_void_p()
        if want != ca.ERR_CONTAINER:       # (no jobs at all: the 32-bit rules)
            assert L.cordic_mixbank_create_c16(p, 0, None, C.byref(b)) == want
            assert L.cordic_mixbank_create16(p, 0, None, C.byref(b)) == want
    conv.close()
    # a good plan: not fused, n = 0 is a no-op behind the shape, then the arrays
    assert plan.fm_mix_c16_info() == (0, 0) == plan.fm_mix_info()
    assert L.cordic_plan_fm_mix_c16_info(plan._h, None, None) == 0
    assert mix(L, plan._h, 0) == 0 == twin(L, plan._h, 0)
    assert mix(L, plan._h, 0, 8) == 0 == twin(L, plan._h, 0, 8)
    assert mix(L, plan._h, 0, 9) == ca.ERR_ARGS == twin(L, plan._h, 0, 9)
    a = 0x10000
    for n, k in ((1024, 9), (0, 9), (1020, 3), (255, 8), (1, 1)):
        assert L.cordic_plan_fm_mix_decim_c16(plan._h, n, k, a, None, 0, None, 2 * a, 4 * a,
                                              6 * a, None) == ca.ERR_ARGS, (n, k)
        assert L.cordic_plan_fm_mix_decim_c16_workspace(plan._h, n, k) == 0, (n, k)
    # NULL d_iq / d_oiq with n > 0 (everything else in place), and either one 2
    # bytes off its 4-byte grid
    for k in (None, 3):
        args = lambda iq, oiq: ((plan._h, 8) + (() if k is None else (k,))
                                + (a, None, 0, None, iq, oiq, 6 * a, None))
        fn = L.cordic_plan_fm_mix_c16 if k is None else L.cordic_plan_fm_mix_decim_c16
        assert fn(*args(None, 4 * a)) == ca.ERR_ARGS
        assert fn(*args(2 * a, None)) == ca.ERR_ARGS
        assert fn(*args(2 * a + 2, 4 * a)) == ca.ERR_ARGS
        assert fn(*args(2 * a, 4 * a + 2)) == ca.ERR_ARGS
        assert fn(*args(2 * a, 2 * a)) == ca.ERR_ARGS       # in place is not offered
    assert mix(L, plan._h, 8) == ca.ERR_ARGS
    # the bank's creates: a NULL bank pointer or NULL jobs first, then the plan
    b = C.c_void_p()
    assert L.cordic_mixbank_create_c16(plan._h, 0, None, None) == ca.ERR_ARGS
    assert L.cordic_mixbank_create_c16(wide._h, 2, None, C.byref(b)) == ca.ERR_ARGS
    assert L.cordic_mixbank_create_decim_c16(None, 3, 0, None, C.byref(b)) == ca.ERR_ARGS
    wide.close()
    plan.close()


def test_the_workspace_of_a_plan_that_is_not_fused_is_the_twins_and_four_arrays_of_shorts():
    a16 = lambda b: (b + 15) // 16 * 16
    plan = ca.Plan(MIX16.both("n9")[0])
    assert plan.fm_mix_info() == (0, 0)
    for k in (0, 1, 3, 8):
        last = 0
        for n in MIX16.SIZES:
            n = n >> k << k                 # (the multiples of R)
            w = plan.fm_mix_decim_c16_workspace(n, k)
            tw = plan.fm_mix_decim16_workspace(n, k)
            assert w % 16 == 0 and w >= last and (w == 0) == (n == 0), (k, n)
            assert w == (a16(tw) + 2 * a16(2 * n) + 2 * a16(2 * (n >> k)) if n else 0), (k, n)
            assert w <= tw + 4 * n + 4 * (n >> k) + 64, (k, n)
            if k == 0:
                assert tw == plan.fm_mix16_workspace(n)
                assert plan.fm_mix_c16_workspace(n) == w, n
            last = w
    for n in MIX16.SIZES:
        assert plan.fm_mix_decim_c16_workspace(n, 0) == plan.fm_mix_c16_workspace(n)
    plan.close()


def test_the_binding_asks_for_shorts_and_for_the_scratch():
    import torch
    plan = ca.Plan(MIX16.both("n9")[0])
    a32 = torch.zeros(16, dtype=torch.int32)
    a16 = torch.zeros(16, dtype=torch.int16)
    with pytest.raises((TypeError, ValueError)):    # an int32 tensor for iq
        plan.fm_mix_c16(a32, a32, a16, n=8)
    with pytest.raises((TypeError, ValueError)):    # ... or for oiq
        plan.fm_mix_c16(a32, a16, a32, n=8)
    with pytest.raises((TypeError, ValueError)):
        plan.fm_mix_decim_c16(3, a32, a32, a16, n=8)
    with pytest.raises((TypeError, ValueError)):
        plan.fm_mix_decim_c16(3, a32, a16, a32, n=8)
    with pytest.raises((TypeError, ValueError)):
        ca.MixBankC16(plan, [(a32, None, a32, a16, 8, 0, None)])
    with pytest.raises((TypeError, ValueError)):
        ca.MixBankC16(plan, [(a32, None, a16, a32, 8, 0, None)], log2r=3)
    with pytest.raises(TypeError):                  # no scratch
        plan.fm_mix_c16(0x1000, 0x2000, 0x3000, n=8)
    with pytest.raises(TypeError):
        plan.fm_mix_decim_c16(3, 0x1000, 0x2000, 0x3000, n=8)
    short = torch.zeros(plan.fm_mix_c16_workspace(8) - 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        plan.fm_mix_c16(0x1000, 0x2000, 0x3000, short, n=8)
    short = torch.zeros(plan.fm_mix_decim_c16_workspace(8, 3) - 16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        plan.fm_mix_decim_c16(3, 0x1000, 0x2000, 0x3000, short, n=8)
    plan.close()


# ---------------------------------------------------------------- the banks' host layer

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "cordic_fm_mix_bank.h"
#include "cordic_hostargs.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced
static cordic_fmmix_job_c16 job(size_t k, uint64_t n)
{
	cordic_fmmix_job_c16 j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t b = 0x100000000u + (uintptr_t)k * 0x10000000u;
	j.d_fcw = (const uint32_t *)(b + 4 * (k % 4));
	j.d_pm = k % 2 ? (const uint32_t *)(b + 0x1000000u) : nullptr;
	j.d_iq = (const int16_t *)(b + 0x2000000u + 4 * (k % 5));
	j.d_oiq = (int16_t *)(b + 0x4000000u + 4 * (k % 3));
	j.d_acc = (uint32_t *)(0x6000000000u + 32 * k);
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u);
	return j;
}

static bool valid(std::vector<cordic_fmmix_job_c16> v, uint32_t k = 0)
{
	std::vector<cordic_fmmix_job16> s;
	for (const auto &j : v)
		s.push_back(fmxb_from_c16(j));
	return fmxb_jobs_valid(s.size(), MixJobs(s.data(), k, true));
}

static int16_t *shorts(const void *p, uint64_t bytes)
{
	return (int16_t *)((uintptr_t)p + bytes);
}

int main()
{
	const uint64_t n = 64;
	const cordic_fmmix_job_c16 a = job(1, n), b = job(2, n);
	EXPECT(valid({a, b}));
	cordic_fmmix_job_c16 t = b;
	// d_iq's range is 4 n bytes: an output on its last short (the last dword
	// that holds it) is an overlap, and so is one in its second half ...
	t.d_oiq = shorts(a.d_iq, 4 * n - 4);		EXPECT(!valid({a, t}));
	t = b; t.d_oiq = shorts(a.d_iq, 2 * n);		EXPECT(!valid({a, t}));
	t = b; t.d_oiq = shorts(a.d_iq, 2 * n + 4);	EXPECT(!valid({a, t}));
	t = b; t.d_acc = (uint32_t *)shorts(a.d_iq, 4 * n - 4); EXPECT(!valid({a, t}));
	t = b; t.d_acc = (uint32_t *)shorts(a.d_iq, 2 * n + 8); EXPECT(!valid({a, t}));
	// ... and one that ENDS on its first short; one short behind the range is clear
	t = b; t.d_oiq = shorts(a.d_iq, 4); EXPECT(!valid({a, t}));
	t = b; t.d_oiq = (int16_t *)((uintptr_t)a.d_iq - 4 * n + 4); EXPECT(!valid({a, t}));
	t = b; t.d_oiq = (int16_t *)((uintptr_t)a.d_iq - 4 * n); EXPECT(valid({a, t}));
	t = b; t.d_oiq = shorts(a.d_iq, 4 * n); EXPECT(valid({a, t}));
	t = b; t.d_acc = (uint32_t *)shorts(a.d_iq, 4 * n); EXPECT(valid({a, t}));
	// the last short of another job's d_oiq, and just behind it
	t = b; t.d_oiq = shorts(a.d_oiq, 4 * n - 4); EXPECT(!valid({a, t}));
	t = b; t.d_acc = (uint32_t *)shorts(a.d_oiq, 4 * n - 4); EXPECT(!valid({a, t}));
	t = b; t.d_oiq = shorts(a.d_oiq, 4 * n); EXPECT(valid({a, t}));
	t = b; t.d_acc = (uint32_t *)shorts(a.d_oiq, 4 * n); EXPECT(valid({a, t}));
	// a job's own output over its own d_iq: in place is not offered
	t = a; t.d_oiq = (int16_t *)a.d_iq; EXPECT(!valid({t, b}));
	t = a; t.d_oiq = shorts(a.d_iq, 4 * n - 4); EXPECT(!valid({t, b}));
	// a shared d_acc; inputs may alias
	t = b; t.d_acc = a.d_acc; EXPECT(!valid({a, t}));
	t = b; t.d_iq = a.d_iq; EXPECT(valid({a, t}));
	// both sit on the 4-byte grid, any of it
	for (unsigned off = 0; off < 16; off += 2) {
		t = b; t.d_iq = shorts(b.d_iq, off);
		EXPECT(valid({a, t}) == (off % 4 == 0));
		t = b; t.d_oiq = shorts(b.d_oiq, off);
		EXPECT(valid({a, t}) == (off % 4 == 0));
	}
	t = b; t.d_iq = nullptr; EXPECT(!valid({a, t}));
	t = b; t.d_oiq = nullptr; EXPECT(!valid({a, t}));
	t = b; t.reserved = 1; EXPECT(!valid({a, t}));
	t = b; t.n = (~(size_t)0 >> 4) + 1; EXPECT(!valid({a, t}));
	// an empty job's pointers are not looked at
	t = b; t.n = 0; t.d_iq = nullptr; t.d_oiq = shorts(a.d_iq, 2); t.reserved = 5;
	t.d_acc = a.d_acc; EXPECT(valid({a, t}));
	// a decimating bank: n % R, k <= 8, d_oiq judged by 4 (n >> k) bytes
	EXPECT(valid({a, b}, 3) && !valid({a, b}, 9));
	t = b; t.n = 68; EXPECT(valid({a, t}, 2) && !valid({a, t}, 3));
	t = b; t.d_oiq = shorts(a.d_oiq, 4 * (n >> 3));
	EXPECT(valid({a, t}, 3) && !valid({a, t}, 2) && !valid({a, t}, 0));
	t = b; t.d_oiq = shorts(a.d_oiq, 4 * (n >> 3) - 4); EXPECT(!valid({a, t}, 3));
	t = b; t.d_acc = (uint32_t *)shorts(a.d_oiq, 4 * (n >> 3)); EXPECT(valid({a, t}, 3));
	// (d_iq keeps its 4 n bytes)
	t = b; t.d_oiq = shorts(a.d_iq, 4 * n - 4); EXPECT(!valid({a, t}, 3));

	// the spans: x carries d_iq at 4 bytes a sample, ox d_oiq at 4 (>> k), y and
	// oy nothing
	for (uint32_t k : {0u, 3u}) {
		std::vector<cordic_fmmix_job16> s = {fmxb_from_c16(job(0, 5 * 1024 + 8)),
			fmxb_from_c16(job(3, 0)), fmxb_from_c16(job(4, 1024))};
		EXPECT(fmxb_jobs_valid(s.size(), MixJobs(s.data(), k, true)));
		std::vector<MixSpan> spans;
		uint32_t live = 0;
		span_cut(kFmxbRule, s.size(), MixJobs(s.data(), k, true), 1, 4096, &spans, &live);
		EXPECT(live == 2 && spans.size() == 7
			&& spans.size() == span_count(kFmxbRule, s.size(), MixJobs(s.data(), k, true), 1, 4096));
		uint64_t s0 = 0;
		size_t j = 0;
		for (const MixSpan &d : spans) {
			if (s0 == s[j].n) {
				s0 = 0;
				j = 2;
			}
			EXPECT(d.fcw == (uintptr_t)s[j].d_fcw + 4 * s0);
			EXPECT(d.pm == (s[j].d_pm ? (uintptr_t)s[j].d_pm + 4 * s0 : 0));
			EXPECT(d.x == (uintptr_t)s[j].d_xval + 4 * s0 && d.y == 0);
			EXPECT(d.ox == (uintptr_t)s[j].d_oxval + 4 * (s0 >> k) && d.oy == 0);
			EXPECT(d.acc == (uintptr_t)s[j].d_acc && s0 % 1024 == 0);
			s0 += d.n;
		}
		EXPECT(j == 2 && s0 == s[2].n);
	}
	// (a split 16-bit job's spans are what they were)
	{
		cordic_fmmix_job16 q = fmxb_from_c16(job(0, 2048));
		q.d_yval = (const int16_t *)0x7000000000u;
		q.d_oyval = (int16_t *)0x7100000000u;
		std::vector<MixSpan> spans;
		span_cut(kFmxbRule, 1, MixJobs(&q, 3), 1, 4096, &spans, nullptr);
		EXPECT(spans.size() == 2 && spans[1].x == (uintptr_t)q.d_xval + 2048
			&& spans[1].y == (uintptr_t)q.d_yval + 2048
			&& spans[1].ox == (uintptr_t)q.d_oxval + 256
			&& spans[1].oy == (uintptr_t)q.d_oyval + 256);
	}

	// the single call's check: d_iq and d_oiq in the place of the four
	const uintptr_t A = 0x10000;
	auto okw = [&](const void *iq, const void *oiq, const void *acc, unsigned k,
			const void *work) {
		return iq_call_ok(n, acc, nullptr, (void *)A, nullptr, iq, nullptr, oiq, nullptr, 2,
			work, 64, k, true, true);
	};
	auto ok = [&](const void *iq, const void *oiq, const void *acc, unsigned k = 0) {
		return okw(iq, oiq, acc, k, (void *)(6 * A));
	};
	EXPECT(ok((void *)(2 * A), (void *)(4 * A), nullptr));
	for (unsigned off = 0; off < 16; off += 2) {
		EXPECT(ok((void *)(2 * A + off), (void *)(4 * A), nullptr) == (off % 4 == 0));
		EXPECT(ok((void *)(2 * A), (void *)(4 * A + off), nullptr) == (off % 4 == 0));
	}
	EXPECT(!ok(nullptr, (void *)(4 * A), nullptr));
	EXPECT(!ok((void *)(2 * A), nullptr, nullptr));
	EXPECT(!ok((void *)(2 * A), (void *)(2 * A), nullptr));			// in place
	EXPECT(!ok((void *)(2 * A), (void *)(2 * A + 4 * n - 4), nullptr));	// the last short
	EXPECT(!ok((void *)(2 * A), (void *)(2 * A + 2 * n), nullptr));		// the second half
	EXPECT(ok((void *)(2 * A), (void *)(2 * A + 4 * n), nullptr));		// tight behind it
	EXPECT(!ok((void *)(2 * A + 4), (void *)(2 * A - 4 * n + 8), nullptr));
	EXPECT(ok((void *)(2 * A + 4), (void *)(2 * A - 4 * n + 4), nullptr));	// tight in front
	EXPECT(!ok((void *)(2 * A), (void *)(4 * A), (void *)(2 * A + 4 * n - 4)));
	EXPECT(ok((void *)(2 * A), (void *)(4 * A), (void *)(2 * A + 4 * n)));
	EXPECT(!ok((void *)(2 * A), (void *)(4 * A), (void *)(4 * A + 4 * n - 4)));
	EXPECT(ok((void *)(2 * A), (void *)(4 * A), (void *)(4 * A + 4 * n)));
	// d_oiq of a decimating call is 4 (n >> k) bytes
	EXPECT(ok((void *)(2 * A), (void *)(4 * A), (void *)(4 * A + 4 * (n >> 3)), 3));
	EXPECT(!ok((void *)(2 * A), (void *)(4 * A), (void *)(4 * A + 4 * (n >> 3) - 4), 3));
	EXPECT(!ok((void *)(2 * A), (void *)(2 * A + 4 * n - 4), nullptr, 3));
	// d_work over either
	EXPECT(!ok((void *)(6 * A + 32), (void *)(4 * A), nullptr));
	EXPECT(!ok((void *)(2 * A), (void *)(6 * A + 48), nullptr));
	EXPECT(!okw((void *)(2 * A), (void *)(4 * A), nullptr, 0, (void *)(2 * A + 4 * n - 16)));
	EXPECT(okw((void *)(2 * A), (void *)(4 * A), nullptr, 0, (void *)(2 * A + 4 * n)));
	// and the receivers' form (interleaved in, two outputs) is what it was
	EXPECT(!iq_call_ok(n, nullptr, nullptr, (void *)A, nullptr, (void *)(2 * A), nullptr,
		(void *)(4 * A), nullptr, 2, (void *)(6 * A), 64, 0, true));
	EXPECT(iq_call_ok(n, nullptr, nullptr, (void *)A, nullptr, (void *)(2 * A), nullptr,
		(void *)(4 * A + 2), (void *)(5 * A), 2, (void *)(6 * A), 64, 0, true));
	if (!failures)
		std::printf("mix c16 host ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_job_checks_and_the_spans_of_interleaved_jobs_under_sanitizers(tmp_path):
    """a stand-alone C++ program with its own main: no Python and no GPU in the
    checked process, as tests/test_fm_rx_c16_host.py"""
    src, exe = tmp_path / "mix_c16.cpp", tmp_path / "mix_c16"
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
    assert "mix c16 host ok" in r.stdout
