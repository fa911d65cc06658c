"""FM oscillator banks (cordic_table_fmbank_create, cordic_quad_fmbank_create,
their ...16 forms, cordic_fmbank_destroy, _info, _run; include/cordic_amd.h):
many cordic_table_fm / cordic_quad_fm jobs of one core in two launches.
Expected values need no tolerance: per job numpy's wrapping cumulative sum
(expected() of tests/test_table_fm.py) feeds the oracle's lookup; in addition
the bank's bits must equal those of one single call per job on copies of the
same data."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
from test_fm_mix import _hip
from test_table_fm import (expected, words, phase_words, TableCore, QuadCore,
                           TABLES, QUADS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")
CREATES = ("cordic_table_fmbank_create", "cordic_table_fmbank_create16",
           "cordic_quad_fmbank_create", "cordic_quad_fmbank_create16")
NAMES = CREATES + ("cordic_fmbank_destroy", "cordic_fmbank_info", "cordic_fmbank_run")
FIELDS = ["d_fcw", "d_pm", "d_sin", "d_cos", "d_acc", "n", "phase0", "reserved"]
TILE = 4096
MAX_SPANS = 1024
KNOBS = ("CORDIC_FMOB_TILES", "CORDIC_FMOB_MAX_SPANS", "CORDIC_FMOB_MAX_BLOCKS")
M32 = 0xffffffff


def spans_of(n, tiles, cap=MAX_SPANS):
    """the cutter's rule (cordic_table_fm_bank.h) restated: spans of `tiles`
    tiles, doubled for this job alone until it has at most `cap` of them"""
    if n == 0:
        return 0
    nt = -(-n // TILE)
    while -(-nt // tiles) > cap:
        tiles *= 2
    return -(-nt // tiles)


# ---------------------------------------------------------------- no GPU

def test_the_bank_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    c = r"(\s*/\*.*?\*/)?\s*"
    for name, elem in (("cordic_fmosc_job", "int32_t"), ("cordic_fmosc_job16", "int16_t")):
        assert re.search(
            r"typedef\s+struct\s+%s\s*\{\s*" % name +
            r"const\s+uint32_t\s*\*\s*d_fcw\s*;" + c +
            r"const\s+uint32_t\s*\*\s*d_pm\s*;" + c +
            r"%s\s*\*\s*d_sin\s*,\s*\*\s*d_cos\s*;" % elem + c +
            r"uint32_t\s*\*\s*d_acc\s*;" + c +
            r"uint64_t\s+n\s*;" + c +
            r"uint32_t\s+phase0\s*;" + c +
            r"uint32_t\s+reserved\s*;" + c +
            r"\}\s*%s\s*;" % name, text, re.S), name
    assert re.search(r"typedef\s+struct\s+cordic_fmbank\s+cordic_fmbank\s*;", text)
    for name in CREATES:
        handle = ("cordic_table", "tbl") if "table" in name else ("cordic_quad", "core")
        job = "cordic_fmosc_job16" if name.endswith("16") else "cordic_fmosc_job"
        assert re.search(
            r"int\s+%s\s*\(\s*const\s+%s\s*\*\s*%s\s*,\s*size_t\s+njobs\s*,\s*"
            r"const\s+%s\s*\*\s*jobs\s*,\s*cordic_fmbank\s*\*\*\s*bank\s*\)\s*;"
            % (name, handle[0], handle[1], job), text), name
    assert re.search(r"void\s+cordic_fmbank_destroy\s*\(\s*cordic_fmbank\s*\*\s*bank"
                     r"\s*\)\s*;", text)
    assert re.search(
        r"int\s+cordic_fmbank_info\s*\(\s*const\s+cordic_fmbank\s*\*\s*bank\s*,"
        r"\s*uint64_t\s*\*\s*samples\s*,\s*uint32_t\s*\*\s*spans\s*,\s*int32_t\s*\*\s*"
        r"tile\s*\)\s*;", text)
    assert re.search(r"int\s+cordic_fmbank_run\s*\(\s*const\s+cordic_fmbank\s*\*"
                     r"\s*bank\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    # behind the FM oscillator block, in front of FM demodulation
    assert text.index("cordic_quad_fm16(") < text.index("cordic_table_fmbank_create(") \
        < text.index("FM demodulation")
    from cordic_amd import _native
    for name in NAMES:
        getattr(ca.lib(), name)             # AttributeError: not exported
        assert name in _native.ABI
    assert "FmBank" in ca.__all__ and callable(ca.FmBank)
    assert callable(ca.Table.fm_bank) and callable(ca.Quad.fm_bank)
    assert re.search(r"#define\s+CORDIC_AMD_ABI_VERSION\s+1\b", text)


@pytest.mark.parametrize("struct", ["cordic_fmosc_job", "cordic_fmosc_job16"])
def test_the_ctypes_mirror_has_the_layout_of_the_header(struct, tmp_path):
    """56 bytes, the field offsets from a compiled offsetof program"""
    from cordic_amd._native import _CFmOscJob
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "cordic_amd.h"\n'
        'int main(void) { printf("%%zu", sizeof(%s));\n' % struct
        + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in FIELDS)
        + 'return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    nums = [int(v) for v in r.stdout.split()]
    assert nums[0] == 56 == C.sizeof(_CFmOscJob)
    assert [f[0] for f in _CFmOscJob._fields_] == FIELDS
    assert [getattr(_CFmOscJob, f).offset for f in FIELDS] == nums[1:]
    assert nums[1:] == [0, 8, 16, 24, 32, 40, 48, 52]


def test_the_header_with_the_bank_block_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "cordic_amd.h"\n'
        'int main(void) { const cordic_table *t = 0; const cordic_quad *q = 0;\n'
        'cordic_fmosc_job j; cordic_fmosc_job16 k;\n'
        'cordic_fmbank *b = 0; uint64_t s; uint32_t n; int32_t l; int rc;\n'
        'char size_is_56[sizeof(cordic_fmosc_job) == 56\n'
        '	&& sizeof(cordic_fmosc_job16) == 56 ? 1 : -1];\n'
        'j.d_fcw = j.d_pm = 0; j.d_sin = j.d_cos = 0;\n'
        'j.d_acc = 0; j.n = 0; j.phase0 = 0; j.reserved = 0; (void)size_is_56;\n'
        'k.d_fcw = k.d_pm = 0; k.d_sin = k.d_cos = 0;\n'
        'k.d_acc = 0; k.n = 0; k.phase0 = 0; k.reserved = 0;\n'
        'rc = cordic_table_fmbank_create(t, 1, &j, &b);\n'
        'rc += cordic_table_fmbank_create16(t, 1, &k, &b);\n'
        'rc += cordic_quad_fmbank_create(q, 1, &j, &b);\n'
        'rc += cordic_quad_fmbank_create16(q, 1, &k, &b);\n'
        'rc += cordic_fmbank_info(b, &s, &n, &l);\n'
        'rc += cordic_fmbank_run(b, 0); cordic_fmbank_destroy(b); return rc; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                        "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_create_refuses_a_null_core_before_anything_is_looked_at():
    """(a core handle needs the device: the other NULLs and the job count are
    in the GPU tests)"""
    L = ca.lib()
    h = C.c_void_p(0x5a5a)
    job = ca._native._CFmOscJob()
    for name in CREATES:
        f = getattr(L, name)
        assert f(None, 0, None, C.byref(h)) == ca.ERR_ARGS
        assert f(None, 1, C.byref(job), C.byref(h)) == ca.ERR_ARGS
        assert f(None, 1 << 28, C.byref(job), C.byref(h)) == ca.ERR_ARGS
        assert f(None, 0, None, None) == ca.ERR_ARGS
    assert h.value == 0x5a5a                # no handle was made
    for core in (ca.Table(ca.QTR, -1, 16, 17, device=False), ca.Quad(device=False)):
        with pytest.raises(ca.CordicError) as e:
            core.fm_bank([])
        assert e.value.status == ca.ERR_ARGS


def test_info_run_and_destroy_on_a_null_handle():
    L = ca.lib()
    s, t, l = C.c_uint64(7), C.c_uint32(7), C.c_int32(7)
    assert L.cordic_fmbank_info(None, C.byref(s), C.byref(t), C.byref(l)) == ca.ERR_ARGS
    assert (s.value, t.value, l.value) == (7, 7, 7)
    assert L.cordic_fmbank_info(None, None, None, None) == ca.ERR_ARGS
    assert L.cordic_fmbank_run(None, None) == ca.ERR_ARGS
    L.cordic_fmbank_destroy(None)           # a no-op


def test_the_restated_cutter_rule():
    assert [spans_of(n, 1) for n in (0, 1, 4095, 4096, 4097, 5 * 4096 + 3)] \
        == [0, 1, 1, 1, 2, 6]
    assert [spans_of(n, 2) for n in (0, 1, 4095, 4096, 4097, 5 * 4096 + 3)] \
        == [0, 1, 1, 1, 1, 3]
    assert spans_of(9 * 4096, 1, 3) == 3 and spans_of(5 * 4096 + 3, 1, 3) == 3
    assert spans_of(1025 * 4096, 1) == 513 and spans_of(1024 * 4096, 1) == 1024


def test_the_tile_loop_is_shared_not_pasted():
    """one definition, in cordic_table_fm.h, called by both kernels"""
    head = open(os.path.join(CSRC, "cordic_table_fm.h")).read()
    assert len(re.findall(r"\bvoid\s+tile_loop\s*\(", head)) == 1
    assert len(re.findall(r"\bauto\s+load_tile\b", head)) == 1
    assert len(re.findall(r"\bauto\s+emit\b", head)) == 1
    for unit, kernel in (("cordic_table_fm.hip", "table_fm"),
                         ("cordic_table_fm_bank.hip", "table_fmbank")):
        body = open(os.path.join(CSRC, unit)).read()
        assert len(re.findall(r"\btile_loop<CORE, T>\(", body)) == 1, unit
        assert re.search(r"\bvoid\s+%s\s*\(" % kernel, body), unit
        code = re.sub(r"//[^\n]*", "", body)
        for pasted in ("__shfl_up", "load_tile", "emit(", "Words4 q = *",
                       "__builtin_nontemporal_store"):
            assert pasted not in code, (unit, pasted)
    stamp = open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert "cordic_table_fm_bank" not in stamp


# ---------------------------------------------------------------- GPU

S32, S16 = -0x5a5a5a5b, 0x5a5b             # sentinels
SENT_U = S32 & M32
PAD = 16                                   # sentinel elements around every output
LENGTHS = [0, 1, 5, 4095, 4096, 4097, 3 * 4096 + 7, (1 << 16) + 3]
PATTERNS = ("zero", "ones", "random", "fsk")


class Spec:
    """The host side of a bank: per job a length, a tuning pattern, whether it
    has phase words, a cosine and a d_acc, its phase0 and the word its d_acc
    holds before the first run.  Job j's sine sits j % W elements behind a
    16-byte boundary (W = 4 words or 8 shorts) and its cosine (3 * j + 1) % W,
    which is never the same; d_fcw sits (j + 1) % 4 words behind one and d_pm
    (j + 3) % 4."""

    def __init__(self, lengths, seed, with_acc=None, phase0=None, mixed=True):
        rng = np.random.default_rng(seed)
        self.ns = list(lengths)
        k = len(self.ns)
        # every (pm, cos, acc) combination in turn, shifted once per round of
        # the lengths so that a length meets another one the second time
        combo = lambda j: (j + j // 8) % 8 if mixed else 7
        self.has_pm = [bool(combo(j) & 1) for j in range(k)]
        self.has_cos = [bool(combo(j) & 2) for j in range(k)]
        self.has_acc = [bool(combo(j) & 4) if with_acc is None else with_acc
                        for j in range(k)]
        self.kind = [PATTERNS[(j + j // 4) % 4] for j in range(k)]
        self.phase0 = [int(v) | 0x80000000 for v in rng.integers(0, 1 << 32, k)] \
            if phase0 is None else [phase0] * k
        # a preset whose sum with phase0 wraps
        self.preset = [(int(v) | 0x80000000) for v in rng.integers(0, 1 << 32, k)]
        self.renew(seed + 1)

    def renew(self, seed):
        """new tuning and phase words for the same jobs"""
        self.fcw, self.pm = [], []
        for j, n in enumerate(self.ns):
            self.fcw.append(words(self.kind[j], n, seed + 17 * j))
            self.pm.append(phase_words("random", n, seed + 17 * j + 5)
                           if self.has_pm[j] else None)

    def samples(self):
        return sum(n * (2 if c else 1) for n, c in zip(self.ns, self.has_cos))

    def spans(self, tiles, cap=MAX_SPANS):
        return sum(spans_of(n, tiles, cap) for n in self.ns)


class DeviceBank:
    """`spec` on the device -- one arena of inputs, one of outputs between
    sentinels, four d_acc words per job -- and an FmBank over it"""

    def __init__(self, torch, core, spec, i16=False):
        from gpu_util import DEV
        self.torch, self.spec, self.i16 = torch, spec, i16
        self.W = W = 8 if i16 else 4
        self.sent = S16 if i16 else S32
        self.at_in, self.at_out = [], []
        cur_in, cur_out = 4, PAD
        for j, n in enumerate(spec.ns):
            f = (cur_in + 3) // 4 * 4 + (j + 1) % 4
            m = (f + n + 3) // 4 * 4 + (j + 3) % 4
            cur_in = m + n
            s = (cur_out + PAD + W - 1) // W * W + j % W
            c = (s + n + PAD + W - 1) // W * W + (3 * j + 1) % W
            cur_out = c + n
            self.at_in.append((f, m))
            self.at_out.append((s, c))
        self.ins = torch.zeros(cur_in + 8, dtype=torch.int32, device=DEV)
        self.outs = torch.full((cur_out + 2 * PAD,), self.sent,
                               dtype=torch.int16 if i16 else torch.int32, device=DEV)
        self.accs = torch.full((4 * max(1, len(spec.ns)),), S32, dtype=torch.int32,
                               device=DEV)
        self.upload()
        self.set_accs(spec.preset)
        jobs = []
        for j, n in enumerate(spec.ns):
            (f, m), (s, c) = self.at_in[j], self.at_out[j]
            jobs.append((self.ins[f:], self.ins[m:] if spec.has_pm[j] else None,
                         self.outs[s:], self.outs[c:] if spec.has_cos[j] else None, n,
                         spec.phase0[j], self.accs[4 * j:] if spec.has_acc[j] else None))
        self.bank = core.h.fm_bank(jobs, i16=i16)

    def set_accs(self, values):
        from gpu_util import DEV
        h = np.full(self.accs.numel(), SENT_U, dtype=np.uint32)
        for j, l in enumerate(self.spec.has_acc):
            if l:
                h[4 * j] = values[j]
        self.accs.copy_(self.torch.from_numpy(h.view(np.int32)).to(DEV))

    def upload(self):
        from gpu_util import DEV
        spec = self.spec
        h = np.zeros(self.ins.numel(), dtype=np.int32)
        for j, n in enumerate(spec.ns):
            f, m = self.at_in[j]
            h[f:f + n] = spec.fcw[j].view(np.int32)
            if spec.has_pm[j]:
                h[m:m + n] = spec.pm[j].view(np.int32)
        self.ins.copy_(self.torch.from_numpy(h).to(DEV))
        self.h_ins = h

    def results(self):
        """([(sin, cos or None)], [acc or None]) after checking that the
        inputs, the sentinels, the place of an absent cosine and the words of
        jobs without a d_acc are as they were"""
        self.torch.cuda.synchronize()
        spec = self.spec
        assert np.array_equal(self.ins.cpu().numpy(), self.h_ins)
        o = self.outs.cpu().numpy()
        a = self.accs.cpu().numpy().view(np.uint32)
        written = np.zeros(o.size, dtype=bool)
        got, accs = [], []
        for j, n in enumerate(spec.ns):
            s, c = self.at_out[j]
            assert s % self.W == j % self.W and c % self.W == (3 * j + 1) % self.W
            written[s:s + n] = True
            sin, cos = o[s:s + n].copy(), None
            if spec.has_cos[j]:
                written[c:c + n] = True
                cos = o[c:c + n].copy()
            got.append((sin, cos))
            accs.append(int(a[4 * j]) if spec.has_acc[j] else None)
            if not spec.has_acc[j]:
                assert a[4 * j] == SENT_U, j
            assert (a[4 * j + 1:4 * j + 4] == SENT_U).all(), j
        assert (o[~written] == self.sent).all()
        return got, accs


def expected_of(core, spec, starts=None):
    """per job (sin, cos or None, acc after the run) as int32; starts: the
    words in front of the run, the presets by default"""
    out = []
    quarter = np.uint32(1 << (core.pw - 2))
    for j, n in enumerate(spec.ns):
        acc0 = (spec.preset[j] if starts is None else starts[j]) if spec.has_acc[j] else 0
        p, final = expected(spec.fcw[j], spec.pm[j], spec.phase0[j], acc0)
        ws = core.oracle(p)
        wc = None
        if spec.has_cos[j]:
            with np.errstate(over="ignore"):
                wc = core.oracle(p + quarter)
        if not spec.has_acc[j]:
            final = None
        elif n == 0:
            final = acc0
        out.append((ws, wc, final))
    return out


def assert_equals(got, accs, wanted, tag, i16=False):
    t = np.int16 if i16 else np.int32
    for j, ((gs, gc), a, (ws, wc, wa)) in enumerate(zip(got, accs, wanted)):
        assert np.array_equal(gs, np.asarray(ws).astype(t)), (tag, j, gs.size)
        assert (gc is None) == (wc is None), (tag, j)
        if gc is not None:
            assert np.array_equal(gc, np.asarray(wc).astype(t)), (tag, j, gs.size)
        assert a == wa, (tag, j, gs.size)


def single_calls(torch, core, spec, i16):
    """one cordic_table_fm / cordic_quad_fm (16) call per job on copies of the
    same data"""
    from gpu_util import DEV, dev_i32
    work = torch.zeros(max(16, ca.fm_workspace(max(spec.ns + [1]))), dtype=torch.uint8,
                       device=DEV)
    dt = torch.int16 if i16 else torch.int32
    out = []
    for j, n in enumerate(spec.ns):
        f = dev_i32(spec.fcw[j]) if n else None
        m = dev_i32(spec.pm[j]) if spec.has_pm[j] and n else None
        s = torch.zeros(max(n, 1), dtype=dt, device=DEV)
        c = torch.zeros(max(n, 1), dtype=dt, device=DEV) if spec.has_cos[j] else None
        acc = None
        if spec.has_acc[j]:
            acc = dev_i32(np.array([spec.preset[j]] * 4, dtype=np.uint32))
        core.h.fm(f, s, c, pm=m, n=n, phase0=spec.phase0[j], acc=acc, work=work)
        torch.cuda.synchronize()
        out.append((s.cpu().numpy()[:n], None if c is None else c.cpu().numpy()[:n],
                    None if acc is None else int(acc.cpu().numpy().view(np.uint32)[0])))
    return out


@functools.lru_cache(maxsize=None)
def ragged_spec():
    """every length of LENGTHS twice, with another pattern and another
    (pm, cos, acc) combination the second time"""
    spec = Spec(LENGTHS + LENGTHS, 100)
    ns = spec.ns
    assert 0 < sum(spec.has_acc) < len(ns) and 0 < sum(spec.has_pm) < len(ns)
    assert 0 < sum(spec.has_cos) < len(ns)
    assert set(spec.kind) == set(PATTERNS)
    for n in LENGTHS:
        a, b = [j for j in range(len(ns)) if ns[j] == n]
        assert spec.kind[a] != spec.kind[b]
        assert (spec.has_pm[a], spec.has_cos[a], spec.has_acc[a]) \
            != (spec.has_pm[b], spec.has_cos[b], spec.has_acc[b])
    for j in range(len(ns)):
        if spec.has_acc[j]:
            assert spec.phase0[j] + spec.preset[j] > M32     # the sum wraps
    return spec


def clear_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def check_ragged(core):
    import torch
    spec = ragged_spec()
    wanted = expected_of(core, spec)
    queues = core.h.queue_info
    for i16 in ((False, True) if core.ow <= 16 else (False,)):
        d = DeviceBank(torch, core, spec, i16)
        if i16:     # every offset 0 .. 7 of a short array, 0 .. 3 of a word array
            assert {s % 8 for s, _ in d.at_out} == set(range(8))
        else:
            assert {s % 4 for s, _ in d.at_out} == set(range(4))
        info = d.bank.info()
        assert info["samples"] == spec.samples()
        t = info["tile"] // TILE
        assert info["tile"] == t * TILE and t >= 1 and t & (t - 1) == 0
        assert info["spans"] == spec.spans(t)
        d.bank.run()
        got, accs = d.results()
        assert_equals(got, accs, wanted, (core.pw, core.ow, i16), i16)
        assert_equals(got, accs, single_calls(torch, core, spec, i16),
                      (core.pw, core.ow, i16, "single calls"), i16)
        d.bank.close()
    assert core.h.queue_info == queues      # no tile queue was taken


@pytest.mark.gpu
@pytest.mark.parametrize("kind,iw,ow,pw", TABLES)
def test_gpu_ragged_table_bank_equals_the_oracle_and_the_single_calls(
        kind, iw, ow, pw, monkeypatch):
    clear_knobs(monkeypatch)
    core = TableCore(kind, iw, ow, pw)
    check_ragged(core)
    core.h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", QUADS)
def test_gpu_ragged_quad_bank_equals_the_oracle_and_the_single_calls(name, monkeypatch):
    clear_knobs(monkeypatch)
    core = QuadCore(name)
    check_ragged(core)
    core.h.close()


KNOB_LENGTHS = [9 * 4096, 4097, 5, 0, 3 * 4096 + 7, 4096, 2 * 4096 + 1, 4095]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["lds", "l2"])
def test_gpu_forced_tiles_grid_caps_and_span_caps_give_the_same_bits(layout, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    core = TableCore(ca.QTR, -1, 16, 17) if layout == "lds" \
        else TableCore(ca.QTR, -1, 24, 18)
    # (modes 1 .. 4: a copy in LDS; 0: gathered from L2)
    assert (core.h.lds_mode != 0) == (layout == "lds")
    spec = Spec(KNOB_LENGTHS, 300)
    wanted = expected_of(core, spec)

    def run(tag, tiles=None, cap=MAX_SPANS):
        for i16 in ((False, True) if core.ow <= 16 else (False,)):
            d = DeviceBank(torch, core, spec, i16)
            info = d.bank.info()
            if tiles is not None:
                assert info["tile"] == tiles * TILE
            assert info["spans"] == spec.spans(info["tile"] // TILE, cap)
            d.bank.run()
            got, accs = d.results()
            assert_equals(got, accs, wanted, (layout, tag, i16), i16)
            d.bank.close()
        return info

    run("default")
    for t in (1, 2, 4):
        monkeypatch.setenv("CORDIC_FMOB_TILES", str(t))
        run("tiles %d" % t, t)
    monkeypatch.setenv("CORDIC_FMOB_TILES", "1")
    for cap in (1, 2, 3):       # one block walks spans of many jobs back to back
        monkeypatch.setenv("CORDIC_FMOB_MAX_BLOCKS", str(cap))
        assert run("max blocks %d" % cap, 1)["spans"] == 21 >= 7 * cap
    monkeypatch.delenv("CORDIC_FMOB_MAX_BLOCKS")
    monkeypatch.setenv("CORDIC_FMOB_MAX_SPANS", "3")
    assert spans_of(9 * 4096, 1, 3) == 3            # 9 tiles: spans of 4
    assert spans_of(3 * 4096 + 7, 1, 3) == 2        # 4 tiles: spans of 2
    info = run("max spans 3", 1, 3)
    assert info["spans"] == 21 - 6 - 2 < spec.spans(1)
    monkeypatch.setenv("CORDIC_FMOB_MAX_BLOCKS", "2")
    run("max spans 3 on 2 blocks", 1, 3)
    core.h.close()


ROUNDS = 3
CONT_LENGTHS = [1, 4095, 4097, 3 * 4096 + 7, 0, 5, 2 * 4096]


def continuation(core, phase0):
    """(spec, per round the spec's words, per round the oracle's values)"""
    spec = Spec(CONT_LENGTHS, 41, with_acc=True, phase0=phase0)
    rounds, wanted = [], []
    starts = list(spec.preset)
    for r in range(ROUNDS):
        spec.renew(50 + r)
        rounds.append((spec.fcw, spec.pm))
        w = expected_of(core, spec, starts)     # phase0 is added by every run
        wanted.append(w)
        starts = [q[2] for q in w]
    if phase0 == 0:     # one long computation per job from the preset word
        for j, n in enumerate(spec.ns):
            cat = lambda k: None if rounds[0][k][j] is None else \
                np.concatenate([rounds[r][k][j] for r in range(ROUNDS)])
            p, final = expected(cat(0), cat(1), 0, spec.preset[j])
            ws = core.oracle(p)
            for r in range(ROUNDS):
                assert np.array_equal(wanted[r][j][0], ws[r * n:(r + 1) * n])
            assert wanted[-1][j][2] == final
    else:               # ... and with phase0 added three times
        for j, n in enumerate(spec.ns):
            total = sum(int(rounds[r][0][j].sum(dtype=np.uint64)) for r in range(ROUNDS))
            # (an empty job runs nothing: its word stays as it is)
            assert wanted[-1][j][2] == (spec.preset[j] + (ROUNDS * phase0 + total
                                                          if n else 0)) & M32
    return spec, rounds, wanted


@pytest.mark.gpu
@pytest.mark.parametrize("phase0", [0, 0x9e3779b1])
@pytest.mark.parametrize("which", ["qtr16", "quad"])
def test_gpu_three_runs_on_new_words_continue_every_job(which, phase0, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    core = QuadCore("rtl_quadtbl") if which == "quad" else TableCore(ca.QTR, -1, 16, 17)
    spec, rounds, wanted = continuation(core, phase0)
    for i16 in (False, True):
        d = DeviceBank(torch, core, spec, i16)
        for r in range(ROUNDS):
            spec.fcw, spec.pm = rounds[r]
            d.upload()
            d.outs.fill_(d.sent)
            d.bank.run()
            got, accs = d.results()
            assert_equals(got, accs, wanted[r], (which, phase0, r, i16), i16)
        d.bank.close()
    core.h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["qtr16", "quad"])
def test_gpu_a_captured_run_replayed_three_times_continues_three_times(which, monkeypatch):
    """one stream; once outside the capture first, on a bank with words of its
    own.  The graph is two kernel nodes with one edge between them."""
    import torch
    clear_knobs(monkeypatch)
    core = QuadCore("rtl_quadtbl") if which == "quad" else TableCore(ca.QTR, -1, 16, 17)
    spec, rounds, wanted = continuation(core, 0)
    spec.fcw, spec.pm = rounds[0]
    warm = DeviceBank(torch, core, spec)
    warm.bank.run()
    torch.cuda.synchronize()
    warm.bank.close()
    d = DeviceBank(torch, core, spec)
    queues = core.h.queue_info

    hip = _hip()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipGraphExecDestroy.argtypes = [C.c_void_p]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    h = C.c_void_p(stream.cuda_stream)
    assert hip.hipStreamBeginCapture(h, 2) == 0      # hipStreamCaptureModeRelaxed
    graph = C.c_void_p()
    try:
        d.bank.run(stream=stream.cuda_stream)
    finally:
        rc = hip.hipStreamEndCapture(h, C.byref(graph))
    assert rc == 0 and graph.value
    try:
        assert (d.outs == d.sent).all().item()       # captured, not run
        assert core.h.queue_info == queues           # no queue slot was taken
        cnt = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(cnt)) == 0
        assert cnt.value == 2
        nodes = (C.c_void_p * 2)()
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(cnt)) == 0
        for i in range(2):
            t = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
            assert t.value == 0                      # hipGraphNodeTypeKernel
        edges = C.c_size_t(0)
        assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0
        assert edges.value == 1                      # two nodes, one chain
        ex = C.c_void_p()
        assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
        try:
            for r in range(ROUNDS):
                spec.fcw, spec.pm = rounds[r]
                d.upload()
                d.outs.fill_(d.sent)
                torch.cuda.synchronize()
                assert hip.hipGraphLaunch(ex, h) == 0
                stream.synchronize()
                got, accs = d.results()
                assert_equals(got, accs, wanted[r], (which, r))
        finally:
            hip.hipGraphExecDestroy(ex)
    finally:
        hip.hipGraphDestroy(graph)
    d.bank.close()
    core.h.close()


@pytest.mark.gpu
def test_gpu_empty_banks_run_and_write_nothing(monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    for core in (TableCore(ca.QTR, -1, 16, 17), QuadCore("rtl_quadtbl")):
        for lengths in ([], [0, 0, 0]):
            for i16 in (False, True):
                spec = Spec(lengths, 71, with_acc=True)
                d = DeviceBank(torch, core, spec, i16)
                info = d.bank.info()
                assert (info["samples"], info["spans"]) == (0, 0)
                assert info["tile"] == TILE
                d.bank.run()
                got, accs = d.results()
                assert accs == spec.preset[:len(lengths)]
                assert (d.outs == d.sent).all().item()
                d.bank.close()
        # a zero-length job's pointers are not looked at
        b = core.h.fm_bank([(3, 5, 7, 9, 0, 0, 15)])
        b.run()
        torch.cuda.synchronize()
        b.close()
        core.h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
def test_gpu_create_refuses_overlaps_and_bad_jobs_with_nothing_written(i16, monkeypatch):
    import torch
    from gpu_util import DEV
    clear_knobs(monkeypatch)
    n = 64
    dt, sent = (torch.int16, S16) if i16 else (torch.int32, S32)
    ins = torch.arange(4 * n, dtype=torch.int32, device=DEV)
    outs = torch.full((6 * n,), sent, dtype=dt, device=DEV)
    accs = torch.full((8,), S32, dtype=torch.int32, device=DEV)
    f0, m0, f1, m1 = (ins[k * n:] for k in range(4))
    s0, c0, s1, c1 = (outs[k * n:] for k in range(4))
    a0, a1 = accs, accs[4:]
    as_out = lambda t, k: t.view(dt)[k:]       # element k of an input, as an output

    def job(f=f0, m=m0, s=s0, c=c0, acc=a0):
        return (f, m, s, c, n, 0, acc)

    def other(f=f1, m=m1, s=s1, c=c1, acc=a1):
        return (f, m, s, c, n, 0, acc)

    for core in (ca.Table(ca.QTR, -1, 16, 17), ca.Quad(-1, 13, 2, 18)):
        def refused(*jobs, status=ca.ERR_ARGS, core=core, i16=i16):
            with pytest.raises(ca.CordicError) as e:
                core.fm_bank(list(jobs), i16=i16)
            assert e.value.status == status

        odd = lambda t: t.data_ptr() + (1 if i16 else 2)
        refused(job(), other(s=outs[n - 1:]))               # output over output
        refused(job(c=outs[n - 1:]))                        # ... of the same job
        refused(job(), other(c=outs[2 * n - 1:], s=outs[4 * n:]))
        refused(job(), other(s=as_out(ins, n - 1)))         # output over another's input
        refused(job(), other(c=as_out(ins, 1)))
        refused(job(s=as_out(ins, 3 * n)), other())         # ... over the other's d_pm
        refused(job(s=as_out(ins, n)))                      # ... over its own d_pm
        refused(job(), other(acc=a0))                       # a shared d_acc
        refused(job(), other(acc=outs[n - 2:].view(torch.int32)))   # d_acc in an output
        refused(job(acc=outs[n:].view(torch.int32)))
        refused(job(acc=ins[5:]))                           # ... inside an input array
        refused(job(f=f0.data_ptr() + 2))                   # off the grids
        refused(job(m=m0.data_ptr() + 2))
        refused(job(s=odd(s0)))
        refused(job(c=odd(c0)))
        refused(job(acc=a0.data_ptr() + 2))
        refused(job(f=None))                                # a NULL that is needed
        refused(job(s=None))
        L = ca.lib()
        create = getattr(L, ("cordic_table_fmbank_create" if isinstance(core, ca.Table)
                             else "cordic_quad_fmbank_create") + ("16" if i16 else ""))
        arr = (ca._native._CFmOscJob * 1)()
        for k, v in zip(FIELDS[:5], (f0, m0, s0, c0, a0)):
            setattr(arr[0], k, v.data_ptr())
        arr[0].n = n
        h = C.c_void_p(0x5a5a)
        for field, value in (("reserved", 1), ("n", (1 << 60) + 1)):
            setattr(arr[0], field, value)
            assert create(core._h, 1, arr, C.byref(h)) == ca.ERR_ARGS
            setattr(arr[0], field, 0 if field == "reserved" else n)
        assert create(core._h, 1 << 28, arr, C.byref(h)) == ca.ERR_ARGS   # unread
        assert create(None, 1, arr, C.byref(h)) == ca.ERR_ARGS
        assert create(core._h, 1, None, C.byref(h)) == ca.ERR_ARGS
        assert create(core._h, 1, arr, None) == ca.ERR_ARGS
        assert create(core._h, 0, None, None) == ca.ERR_ARGS
        assert h.value == 0x5a5a                            # no handle was made
        torch.cuda.synchronize()
        assert (outs == sent).all().item() and (accs == S32).all().item()
        assert torch.equal(ins, torch.arange(4 * n, dtype=torch.int32, device=DEV))
        # inputs may alias each other, within a job and between jobs; d_pm, d_cos
        # and d_acc may be NULL
        b = core.fm_bank([job(m=f0), other(f=f0, m=None, c=None, acc=None)], i16=i16)
        accs.zero_()
        b.run()
        torch.cuda.synchronize()
        hh = outs.cpu().numpy()
        assert (hh[3 * n:] == sent).all() and (hh[:3 * n] != sent).any()
        b.close()
        outs.fill_(sent)
        accs.fill_(S32)
        core.close()


@pytest.mark.gpu
def test_gpu_create_refuses_the_wrong_container_and_tables_over_64_kib(monkeypatch):
    import torch
    from gpu_util import DEV
    clear_knobs(monkeypatch)
    n = 64
    f = torch.zeros(n, dtype=torch.int32, device=DEV)
    s16 = torch.full((n,), S16, dtype=torch.int16, device=DEV)
    s32 = torch.full((n,), S32, dtype=torch.int32, device=DEV)
    L = ca.lib()
    h = C.c_void_p(0x5a5a)
    # a 16-bit create on OW > 16: behind the NULL checks, also for an empty bank
    for core in (ca.Table(ca.QTR, -1, 24, 17), ca.Quad(ow=24, pw=32)):
        for jobs in ([(f, None, s16, None, n, 0, None)], []):
            with pytest.raises(ca.CordicError) as e:
                core.fm_bank(jobs, i16=True)
            assert e.value.status == ca.ERR_CONTAINER
        create = getattr(L, "cordic_table_fmbank_create16" if isinstance(core, ca.Table)
                         else "cordic_quad_fmbank_create16")
        assert create(core._h, 1, None, C.byref(h)) == ca.ERR_ARGS
        assert create(core._h, 0, None, None) == ca.ERR_ARGS
        core.close()
    # A quadratic core whose tables exceed 64 KiB is refused as cordic_quad_fm
    # refuses it.  No configuration that cordic_quad_config_init or _init_core
    # accepts has such tables (the largest has 1024 entries of 16 bytes), so
    # the refusal is checked wherever one turns up and its absence is stated.
    big, most = None, 0
    for ow in range(8, 33):
        for xtra in (1, 2, 3, 4, 6):
            for kw in (dict(ow=ow, xtra=xtra, pw=32), dict(core=(32, ow, xtra)),
                       dict(core=(24, ow, xtra))):
                try:
                    q = ca.Quad(device=False, **kw)
                except ca.CordicError:
                    continue
                most = max(most, q.entries * 16)
                if q.entries * 16 > 64 * 1024 and big is None:
                    big = kw
    if big is None:
        assert 0 < most <= 64 * 1024
    else:
        big = ca.Quad(**big)
        work = torch.zeros(max(16, ca.fm_workspace(n)), dtype=torch.uint8, device=DEV)
        with pytest.raises(ca.CordicError) as e:
            big.fm(f, s32, None, n=n, work=work)
        assert e.value.status == ca.ERR_UNSUPPORTED
        with pytest.raises(ca.CordicError) as e:
            big.fm_bank([(f, None, s32, None, n, 0, None)])
        assert e.value.status == ca.ERR_UNSUPPORTED
        big.close()
    torch.cuda.synchronize()
    assert (s16 == S16).all().item() and (s32 == S32).all().item()
    assert h.value == 0x5a5a


@pytest.mark.gpu
def test_gpu_create_refuses_two_to_the_32_spans_and_a_captured_legacy_stream(
        monkeypatch):
    """A job has at most 1024 spans however long it is (one huge n gives 1024
    longer ones), so 2^32 spans take 2^22 + 1 jobs of 1024 tiles at T = 1:
    2^32 + 1024 spans (addresses that nothing dereferences: create refuses
    before it uploads)."""
    import torch
    clear_knobs(monkeypatch)
    core = TableCore(ca.QTR, -1, 16, 17)
    L = ca.lib()
    k = (1 << 22) + 1
    n = MAX_SPANS * TILE
    dt = np.dtype([(f, "<u8") for f in FIELDS[:6]] + [("phase0", "<u4"), ("reserved", "<u4")])
    assert dt.itemsize == 56
    jobs = np.zeros(k, dtype=dt)
    at = np.arange(k, dtype=np.uint64) * np.uint64(4 * n)
    jobs["d_fcw"] = np.uint64(1 << 48) + at
    jobs["d_sin"] = np.uint64(2 << 48) + at
    jobs["n"] = n
    h = C.c_void_p(0x5a5a)
    monkeypatch.setenv("CORDIC_FMOB_TILES", "1")
    assert L.cordic_table_fmbank_create(core.h._h, k, jobs.ctypes.data, C.byref(h)) \
        == ca.ERR_ARGS
    assert h.value == 0x5a5a
    # one huge job alone is 1024 spans: a valid bank
    assert L.cordic_table_fmbank_create(core.h._h, 1, jobs.ctypes.data, C.byref(h)) == 0
    spans = C.c_uint32()
    assert L.cordic_fmbank_info(h, None, C.byref(spans), None) == 0
    assert spans.value == 1024
    L.cordic_fmbank_destroy(h)
    h = C.c_void_p(0x5a5a)
    del jobs
    monkeypatch.delenv("CORDIC_FMOB_TILES")

    # blocking uploads: not while the legacy stream is being captured -- which a
    # capture in the global mode on a BLOCKING stream amounts to (torch's own
    # streams are non-blocking: they do not take the legacy stream with them)
    t = torch.zeros(2 * 64, dtype=torch.int32, device="cuda:0")
    one = (ca._native._CFmOscJob * 1)()
    one[0].d_fcw, one[0].d_sin, one[0].n = t.data_ptr(), t[64:].data_ptr(), 64
    hip = _hip()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hs = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(hs)) == 0     # (default flags: blocking)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(hs, 0) == 0     # hipStreamCaptureModeGlobal
    graph = C.c_void_p()
    try:
        rc = L.cordic_table_fmbank_create(core.h._h, 1, one, C.byref(h))
    finally:
        hip.hipStreamEndCapture(hs, C.byref(graph))
        hip.hipGetLastError()
    if graph.value:
        hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(hs)
    print("create under a global capture: status %d" % rc)
    if rc == 0:
        L.cordic_fmbank_destroy(h)
    assert rc == ca.ERR_UNSUPPORTED and h.value == 0x5a5a
    assert (t == 0).all().item()
    spec = Spec([5, 4097], 81)                       # and afterwards all is well
    d = DeviceBank(torch, core, spec)
    d.bank.run()
    got, accs = d.results()
    assert_equals(got, accs, expected_of(core, spec), "after the refusals")
    d.bank.close()
    core.h.close()


@pytest.mark.gpu
def test_gpu_run_from_another_device_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    core = ca.Table(ca.QTR, -1, 16, 17)
    b = core.fm_bank([])
    with torch.cuda.device(1):
        assert ca.lib().cordic_fmbank_run(b._h, None) == ca.ERR_ARGS
    b.close()
    core.close()


@pytest.mark.gpu
def test_gpu_the_example_builds_and_exits_0(tmp_path):
    """examples/fm_tx_bank.c: one FM oscillator bank into the receive half of
    examples/fm_channeliser.c, against the per-channel calls"""
    exe = tmp_path / "fm_tx_bank"
    r = subprocess.run(
        ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
         "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
         "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-o", str(exe),
         os.path.join(ROOT, "examples", "fm_tx_bank.c"),
         "-L", os.path.join(ROOT, "cordic_amd"), "-lcordic_amd", "-L", "/opt/rocm/lib",
         "-lamdhip64", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "cordic_amd"),
         "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "-c", "8", "-l", "4099", "-r", "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "8 channels" in r.stdout and "x 3 rounds" in r.stdout
    assert "0 words differ" in r.stdout
