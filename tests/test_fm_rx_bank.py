"""Receiver banks (cordic_rxbank_*; include/cordic_amd.h): many
cordic_plan_fm_rx jobs of one plan and one converter in two launches.  Every
sample of every output and every d_acc / d_last word is compared with the
oracle and with the per-job single calls; nothing has a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import test_fm_mix as MIX
import test_fm_rx as RX
import test_fm_rx16 as RX16
from test_fm_demod import Padded, last_word
from test_table_fm import words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("CORDIC_FMRXB_PASSES", "CORDIC_FMRXB_MAX_SPANS", "CORDIC_FMRXB_MAX_BLOCKS",
         "CORDIC_FMRX_MAX_BLOCKS")
PASS, HALO, MAX_SPANS = 1024, 4, 4096
# (pair, int16?, fused): the fused pairs of both containers and one pair that
# runs one by one
BANKS = {
    "nat24-cfg3": ("nat24-cfg3", False, 1),
    "cfg2-cfg3": ("cfg2-cfg3", False, 1),
    "nat16-natr2p24": ("nat16-natr2p24", False, 1),
    "cfg1-io16": ("cfg1-io16", True, 1),
    "ww38-cfg3": ("ww38-cfg3", False, 0),
}
# the single call's lengths and 0, about 40 jobs
RAGGED = list(RX.LENGTHS) + [0] + list(RX.LENGTHS[::-1]) + [0, 2 * 1020, 1020, 1021] \
    + [3 * 1020 + 1, 7, 1019, 4 * 1024, 0, 300]


def clear_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def configs(name):
    pair, i16, fused = BANKS[name]
    if i16:
        mcfg, _, ccfg, _, _ = RX16.configs(pair)
    else:
        _, _, _, mcfg, ccfg = RX.cores(pair)
    return pair, i16, fused, mcfg, ccfg


def oracle(name, *a):
    pair, i16, _ = BANKS[name]
    return (RX16.oracle if i16 else RX.oracle)(pair, *a)


def spans_of(lengths, base=1, cap=MAX_SPANS):
    """the host rule: spans of `base` passes less the halo, doubled for a job
    that would have more than `cap`"""
    total = 0
    for n in lengths:
        if not n:
            continue
        uj = base
        while -(-n // (uj * PASS - HALO)) > cap:
            uj *= 2
        total += -(-n // (uj * PASS - HALO))
    return total


class Spec:
    """the jobs of a bank: lengths, which optional pointers each has, its
    element offsets and its phases; renew(r) draws the data of round r"""

    def __init__(self, name, lengths, seed, all_words=False, zero_phases=False):
        self.name, self.ns, self.seed = name, list(lengths), seed
        _, self.i16, _, mcfg, _ = configs(name)
        self.iw = 16 if self.i16 else mcfg.iw
        rng = np.random.default_rng(seed)
        k = len(self.ns)
        self.has_pm = [bool(j % 3) for j in range(k)]
        self.has_acc = [all_words or bool((j + 1) % 4) for j in range(k)]
        self.has_last = [all_words or bool((j + 2) % 5) for j in range(k)]
        self.offs = [[int(v) for v in rng.integers(0, 6, 6)] for _ in range(k)]
        z = zero_phases
        self.phase0 = [0 if z else int(v) for v in rng.integers(0, 1 << 32, k)]
        self.dphase0 = [0 if z else int(v) for v in rng.integers(0, 1 << 32, k)]
        self.acc0 = [int(v) for v in rng.integers(0, 1 << 32, k)]
        self.last0 = [int(v) for v in rng.integers(0, 1 << 32, k)]
        self.renew(0)

    def renew(self, r):
        self.fcw, self.pm, self.x, self.y = [], [], [], []
        for j, n in enumerate(self.ns):
            s = self.seed * 1000 + r * 100 + j
            x, y = MIX.iq(np.random.default_rng(s), n, self.iw)
            self.fcw.append(words("random", n, s + 1))
            self.pm.append(words("random", n, s + 2) if self.has_pm[j] else None)
            self.x.append(x)
            self.y.append(y)

    def expected(self, acc=None, last=None):
        """per job (mag, freq, *d_acc, *d_last afterwards) from the words given
        (None: the presets; a job without a word starts from 0)"""
        out = []
        for j, n in enumerate(self.ns):
            a0 = (self.acc0[j] if acc is None else acc[j]) if self.has_acc[j] else 0
            l0 = (self.last0[j] if last is None else last[j]) if self.has_last[j] else 0
            m, f, fa, fl = oracle(self.name, self.fcw[j], self.pm[j], self.x[j],
                                  self.y[j], self.phase0[j], a0, self.dphase0[j], l0)
            out.append((m, f, (fa if n else a0) if self.has_acc[j] else None,
                        (fl if n else l0) if self.has_last[j] else None))
        return out


class DeviceBank:
    """the arrays of a Spec on the device, every one with guard elements around
    it, and the bank over them"""

    def __init__(self, torch, plan, ccfg, spec):
        from gpu_util import DEV
        self.torch, self.spec, self.plan, self.ccfg = torch, spec, plan, ccfg
        k = len(spec.ns)
        self.words = torch.zeros(8 * max(1, k), dtype=torch.int32, device=DEV)
        self.arr = []
        for j, n in enumerate(spec.ns):
            o = spec.offs[j]
            self.arr.append(dict(
                fcw=Padded(torch, n, o[0]), pm=Padded(torch, n, o[1]),
                x=Padded(torch, n, o[2], spec.i16), y=Padded(torch, n, o[3], spec.i16),
                mag=Padded(torch, n, o[4], spec.i16), freq=Padded(torch, n, o[5], spec.i16)))
        self.upload()
        self.preset()
        self.bank = (ca.RxBank16 if spec.i16 else ca.RxBank)(plan, ccfg, self.jobs())

    def acc(self, j):
        return self.words[8 * j:] if self.spec.has_acc[j] else None

    def last(self, j):
        return self.words[8 * j + 4:] if self.spec.has_last[j] else None

    def jobs(self):
        s = self.spec
        return [(a["fcw"].view, a["pm"].view if s.has_pm[j] else None, a["x"].view,
                 a["y"].view, a["mag"].view, a["freq"].view, s.ns[j], s.phase0[j],
                 self.acc(j), s.dphase0[j], self.last(j))
                for j, a in enumerate(self.arr)]

    def upload(self):
        s, t = self.spec, self.torch
        put = lambda p, v, dt: p.t[p.off:p.off + p.n].copy_(
            t.from_numpy(np.ascontiguousarray(v).astype(dt)).to(p.t.device))
        for j, a in enumerate(self.arr):
            if not s.ns[j]:
                continue
            put(a["fcw"], s.fcw[j].view(np.int32), np.int32)
            if s.has_pm[j]:
                put(a["pm"], s.pm[j].view(np.int32), np.int32)
            put(a["x"], s.x[j], a["x"].np)
            put(a["y"], s.y[j], a["y"].np)

    def preset(self):
        h = np.zeros(self.words.numel(), dtype=np.uint32)
        for j in range(len(self.spec.ns)):
            h[8 * j], h[8 * j + 4] = self.spec.acc0[j], self.spec.last0[j]
        self.words.copy_(self.torch.from_numpy(h.view(np.int32)).to(self.words.device))

    def clear_outputs(self):
        for a in self.arr:
            a["mag"].t.fill_(a["mag"].sent)
            a["freq"].t.fill_(a["freq"].sent)

    def outputs_untouched(self):
        return all(a["mag"].untouched() and a["freq"].untouched() for a in self.arr)

    def results(self):
        """per job (mag, freq, *d_acc, *d_last), after checking the guards, the
        inputs and the words nobody may write"""
        self.torch.cuda.synchronize()
        s = self.spec
        h = self.words.cpu().numpy().view(np.uint32)
        out = []
        for j, a in enumerate(self.arr):
            if s.ns[j]:
                assert np.array_equal(a["fcw"].get(), s.fcw[j].view(np.int32))
                assert np.array_equal(a["x"].get(), s.x[j])
            w = h[8 * j:8 * j + 8]
            assert not w[1:4].any() and not w[5:8].any()
            if not s.has_acc[j]:
                assert w[0] == s.acc0[j]
            if not s.has_last[j]:
                assert w[4] == s.last0[j]
            out.append((a["mag"].get().astype(np.int32), a["freq"].get().astype(np.int32),
                        int(w[0]) if s.has_acc[j] else None,
                        int(w[4]) if s.has_last[j] else None))
        return out


def assert_equals(got, want, tag):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]), (tag, j, "mag")
        assert np.array_equal(g[1], w[1]), (tag, j, "freq")
        assert g[2] == w[2], (tag, j, "d_acc")
        assert g[3] == w[3], (tag, j, "d_last")


def single_calls(torch, plan, ccfg, spec):
    """the same jobs through cordic_plan_fm_rx / _rx16, one call each"""
    from gpu_util import DEV
    out = []
    size = plan.fm_rx16_workspace if spec.i16 else plan.fm_rx_workspace
    call = plan.fm_rx16 if spec.i16 else plan.fm_rx
    for j, n in enumerate(spec.ns):
        o = spec.offs[j]
        i32 = lambda a: a.view(np.int32)
        df = Padded(torch, n, o[0], src=i32(spec.fcw[j]))
        dm = Padded(torch, n, o[1], src=i32(spec.pm[j])) if spec.has_pm[j] else None
        dx = Padded(torch, n, o[2], spec.i16, src=spec.x[j])
        dy = Padded(torch, n, o[3], spec.i16, src=spec.y[j])
        mag, freq = Padded(torch, n, o[4], spec.i16), Padded(torch, n, o[5], spec.i16)
        acc = last_word(torch, spec.acc0[j]) if spec.has_acc[j] else None
        last = last_word(torch, spec.last0[j]) if spec.has_last[j] else None
        work = torch.zeros(max(16, size(ccfg, n)), dtype=torch.uint8, device=DEV)
        call(ccfg, df.view, dx.view, dy.view, mag.view, freq.view, work,
             pm=None if dm is None else dm.view, n=n, phase0=spec.phase0[j], acc=acc,
             dphase0=spec.dphase0[j], last=last)
        torch.cuda.synchronize()
        word = lambda t: None if t is None else int(t.cpu().numpy().view(np.uint32)[0])
        out.append((mag.get().astype(np.int32), freq.get().astype(np.int32), word(acc),
                    word(last)))
    return out


def open_bank(torch, name, spec):
    _, _, _, mcfg, ccfg = configs(name)
    plan = ca.Plan(mcfg)
    return plan, ccfg, DeviceBank(torch, plan, ccfg, spec)


# ---------------------------------------------------------------- no GPU

def test_the_bank_is_declared_exported_bound_and_re_exported():
    text = open(os.path.join(ROOT, "include", "cordic_amd.h")).read()
    from cordic_amd import _native
    for name in ("cordic_rxbank_create", "cordic_rxbank_create16", "cordic_rxbank_run",
                 "cordic_rxbank_info", "cordic_rxbank_destroy"):
        assert name + "(" in text
        getattr(ca.lib(), name)
        assert name in _native.ABI
    assert text.index("cordic_plan_fm_rx16(") < text.index("cordic_rxbank_create(") \
        < text.index("clocked view (streaming shim)")
    assert "RxBank" in ca.__all__ and "RxBank16" in ca.__all__
    assert C.sizeof(_native._CFmRxJob) == 88
    assert ca.lib().cordic_rxbank_info(None, None, None, None, None) == ca.ERR_ARGS
    assert ca.lib().cordic_rxbank_run(None, None) == ca.ERR_ARGS
    ca.lib().cordic_rxbank_destroy(None)


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BANKS))
def test_gpu_a_ragged_bank_equals_the_single_calls_and_the_oracle(name, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    fused = BANKS[name][2]
    spec = Spec(name, RAGGED, 11)
    plan, ccfg, d = open_bank(torch, name, spec)
    info = d.bank.info()
    assert info["samples"] == sum(spec.ns) and info["fused"] == fused
    assert info["tile"] == (1024 if fused else 0)
    assert info["spans"] == (spans_of(spec.ns) if fused else 0)
    d.bank.run()
    got = d.results()
    assert_equals(got, spec.expected(), name)
    assert_equals(got, single_calls(torch, plan, ccfg, spec), name + " single calls")
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [dict(CORDIC_FMRXB_PASSES="1"),
                                   dict(CORDIC_FMRXB_PASSES="2"),
                                   dict(CORDIC_FMRXB_PASSES="4"),
                                   dict(CORDIC_FMRXB_MAX_SPANS="2"),
                                   dict(CORDIC_FMRXB_MAX_BLOCKS="1"),
                                   dict(CORDIC_FMRXB_MAX_BLOCKS="3")])
@pytest.mark.parametrize("name", ["cfg2-cfg3", "cfg1-io16"])
def test_gpu_forced_spans_span_caps_and_grid_caps_give_the_same_bits(name, knobs,
                                                                      monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    lengths = [5 * 1024 + 3, 1020, 1021, 3, 0, 2 * 1020 + 1, 4 * 1016, 4 * 1016 + 1]
    spec = Spec(name, lengths, 23)
    plan, ccfg, d = open_bank(torch, name, spec)
    base = int(knobs.get("CORDIC_FMRXB_PASSES", 1))
    cap = int(knobs.get("CORDIC_FMRXB_MAX_SPANS", MAX_SPANS))
    assert d.bank.info()["spans"] == spans_of(lengths, base, cap)
    if cap == 2:        # one job forced to longer spans
        assert spans_of(lengths, 1, 2) < spans_of(lengths)
    d.bank.run()
    assert_equals(d.results(), spec.expected(), (name, knobs))
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2-cfg3", "cfg1-io16", "ww38-cfg3"])
def test_gpu_three_runs_on_new_data_continue_every_job(name, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    spec = Spec(name, [2049, 1, 1020, 0, 1025, 4], 31, all_words=True, zero_phases=True)
    plan, ccfg, d = open_bank(torch, name, spec)
    acc, last = None, None
    for r in range(3):
        spec.renew(r)
        d.upload()
        d.clear_outputs()
        want = spec.expected(acc, last)
        d.bank.run()
        assert_equals(d.results(), want, (name, r))
        acc, last = [w[2] for w in want], [w[3] for w in want]
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2-cfg3", "ww38-cfg3"])
def test_gpu_a_captured_run_replayed_three_times_continues_three_times(name, monkeypatch):
    """the same inputs every replay: replay r starts from the words replay r - 1
    left.  Fused: two kernel nodes with one edge between them"""
    import torch
    clear_knobs(monkeypatch)
    fused = BANKS[name][2]
    spec = Spec(name, [2049, 3, 1021, 0], 37, all_words=True, zero_phases=True)
    plan, ccfg, d = open_bank(torch, name, spec)
    warm = DeviceBank(torch, plan, ccfg, spec)      # once outside the capture first
    warm.bank.run()
    torch.cuda.synchronize()
    warm.bank.close()

    hip = MIX._hip()
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
        assert d.outputs_untouched()                 # captured, not run
        cnt = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(cnt)) == 0
        if fused:
            assert cnt.value == 2
            nodes = (C.c_void_p * 2)()
            assert hip.hipGraphGetNodes(graph, nodes, C.byref(cnt)) == 0
            for i in range(2):
                t = C.c_int(-1)
                assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
                assert t.value == 0                  # hipGraphNodeTypeKernel
            edges = C.c_size_t(0)
            assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0
            assert edges.value == 1                  # two nodes, one chain
        ex = C.c_void_p()
        assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
        try:
            acc, last = None, None
            for r in range(3):
                d.clear_outputs()
                torch.cuda.synchronize()
                want = spec.expected(acc, last)
                assert hip.hipGraphLaunch(ex, h) == 0
                stream.synchronize()
                assert_equals(d.results(), want, (name, r))
                acc, last = [w[2] for w in want], [w[3] for w in want]
        finally:
            hip.hipGraphExecDestroy(ex)
    finally:
        hip.hipGraphDestroy(graph)
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2-cfg3", "ww38-cfg3"])
def test_gpu_empty_banks_run_and_write_nothing(name, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    for lengths in ([], [0, 0, 0]):
        spec = Spec(name, lengths, 41, all_words=True)
        plan, ccfg, d = open_bank(torch, name, spec)
        info = d.bank.info()
        assert (info["samples"], info["spans"]) == (0, 0)
        assert info["fused"] == BANKS[name][2]
        d.bank.run()
        got = d.results()
        assert [g[2] for g in got] == spec.acc0 and [g[3] for g in got] == spec.last0
        assert d.outputs_untouched()
        d.bank.close()
        # a zero-length job's pointers are not looked at
        b = ca.RxBank(plan, ccfg, [(3, 5, 7, 9, 11, 13, 0, 0, 15, 0, 17)])
        b.run()
        torch.cuda.synchronize()
        b.close()
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2-cfg3", "ww38-cfg3"])
def test_gpu_create_refuses_overlaps_and_bad_jobs_with_nothing_written(name, monkeypatch):
    import torch
    from gpu_util import DEV
    clear_knobs(monkeypatch)
    _, _, _, mcfg, ccfg = configs(name)
    plan = ca.Plan(mcfg)
    n, SENT = 64, 0x5a5a5a5a
    ins = torch.arange(8 * n, dtype=torch.int32, device=DEV)
    outs = torch.full((6 * n,), SENT, dtype=torch.int32, device=DEV)
    wd = torch.full((16,), SENT, dtype=torch.int32, device=DEV)
    f0, m0, x0, y0, f1, m1, x1, y1 = (ins[k * n:] for k in range(8))
    a0, b0, a1, b1 = (outs[k * n:] for k in range(4))
    c0, l0, c1, l1 = wd, wd[4:], wd[8:], wd[12:]

    def job(f=f0, m=m0, x=x0, y=y0, a=a0, b=b0, acc=c0, last=l0):
        return (f, m, x, y, a, b, n, 0, acc, 0, last)

    def other(f=f1, m=m1, x=x1, y=y1, a=a1, b=b1, acc=c1, last=l1):
        return (f, m, x, y, a, b, n, 0, acc, 0, last)

    def refused(*jobs, status=ca.ERR_ARGS, plan=plan, conv=ccfg):
        with pytest.raises(ca.CordicError) as e:
            ca.RxBank(plan, conv, list(jobs))
        assert e.value.status == status

    odd = lambda t: t.data_ptr() + 2
    refused(job(), other(a=outs[n - 1:]))               # output over output
    refused(job(b=outs[n - 1:]))                        # ... of the same job
    refused(job(), other(a=ins[n - 1:]))                # output over another job's input
    refused(job(a=ins[n:]))                             # ... over its own d_pm
    refused(job(), other(acc=c0))                       # a shared d_acc
    refused(job(), other(last=l0))                      # a shared d_last
    refused(job(), other(last=c0))                      # one's d_last, the other's d_acc
    refused(job(last=c0))                               # d_acc is d_last
    refused(job(), other(last=outs[n - 1:]))            # d_last inside another job's d_omag
    refused(job(last=outs[n + 3:]))                     # ... inside its own d_ofreq
    refused(job(last=ins[5:]))                          # ... inside an input array
    refused(job(acc=outs[n:]))
    for k in range(6):                                  # off the 4-byte grid
        a = [f0, m0, x0, y0, a0, b0]
        a[k] = odd(a[k])
        refused(job(*a))
    refused(job(acc=odd(c0)))
    refused(job(last=odd(l0)))
    for k in (0, 2, 3, 4, 5):                           # a NULL pointer that is needed
        a = [f0, m0, x0, y0, a0, b0]
        a[k] = None
        refused(job(*a))
    L = ca.lib()
    arr = (ca._native._CFmRxJob * 1)()
    for k, v in zip(("d_fcw", "d_pm", "d_xval", "d_yval", "d_omag", "d_ofreq", "d_acc",
                     "d_last"), (f0, m0, x0, y0, a0, b0, c0, l0)):
        setattr(arr[0], k, v.data_ptr())
    arr[0].n = n
    h = C.c_void_p(0x5a5a)
    for field, value in (("reserved", 1), ("reserved", 1 << 40), ("n", (1 << 60) + 1)):
        setattr(arr[0], field, value)
        assert L.cordic_rxbank_create(plan._h, ccfg.ref, 1, arr, C.byref(h)) == ca.ERR_ARGS
        setattr(arr[0], field, 0 if field == "reserved" else n)
    create = L.cordic_rxbank_create
    assert create(plan._h, ccfg.ref, 1 << 28, arr, C.byref(h)) == ca.ERR_ARGS
    assert create(None, ccfg.ref, 1, arr, C.byref(h)) == ca.ERR_ARGS
    assert create(plan._h, None, 1, arr, C.byref(h)) == ca.ERR_ARGS
    assert create(plan._h, ccfg.ref, 1, None, C.byref(h)) == ca.ERR_ARGS
    assert create(plan._h, ccfg.ref, 1, arr, None) == ca.ERR_ARGS
    assert create(plan._h, mcfg.ref, 1, arr, C.byref(h)) == ca.ERR_MODE   # a rotator as conv
    assert L.cordic_rxbank_create16(plan._h, ccfg.ref, 1, arr, C.byref(h)) \
        == ca.ERR_CONTAINER
    assert h.value == 0x5a5a                            # no handle was made
    torch.cuda.synchronize()
    assert (outs == SENT).all().item() and (wd == SENT).all().item()
    assert torch.equal(ins, torch.arange(8 * n, dtype=torch.int32, device=DEV))
    # inputs may alias each other, within a job and between jobs; optional ones may go
    b = ca.RxBank(plan, ccfg, [job(y=x0, m=f0), other(f=f0, m=None, x=x0, y=x0, acc=None,
                                                     last=None)])
    wd.zero_()
    b.run()
    torch.cuda.synchronize()
    hh = outs.cpu().numpy()
    assert (hh[4 * n:] == SENT).all() and (hh[:4 * n] != SENT).any()
    b.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_create_refuses_two_to_the_32_spans_and_a_captured_legacy_stream(monkeypatch):
    """2^20 + 1 jobs of 4096 one-pass spans (1020 samples each) are 2^32 + 4096
    spans (addresses that nothing dereferences: create refuses before it uploads)"""
    import torch
    clear_knobs(monkeypatch)
    _, _, _, mcfg, ccfg = configs("cfg2-cfg3")
    plan = ca.Plan(mcfg)
    L = ca.lib()
    k = (1 << 20) + 1
    n = MAX_SPANS * (PASS - HALO)
    fields = ("d_fcw", "d_pm", "d_xval", "d_yval", "d_omag", "d_ofreq", "d_acc", "d_last", "n")
    dt = np.dtype([(f, "<u8") for f in fields] + [("phase0", "<u4"), ("dphase0", "<u4"),
                                                  ("reserved", "<u8")])
    assert dt.itemsize == 88
    jobs = np.zeros(k, dtype=dt)
    at = np.arange(k, dtype=np.uint64) * np.uint64(4 * n)
    for i, f in enumerate(("d_fcw", "d_xval", "d_yval", "d_omag", "d_ofreq")):
        jobs[f] = np.uint64((i + 1) << 48) + at
    jobs["n"] = n
    h = C.c_void_p(0x5a5a)
    monkeypatch.setenv("CORDIC_FMRXB_PASSES", "1")
    assert L.cordic_rxbank_create(plan._h, ccfg.ref, k, jobs.ctypes.data,
                                  C.byref(h)) == ca.ERR_ARGS
    assert h.value == 0x5a5a
    monkeypatch.delenv("CORDIC_FMRXB_PASSES")

    # blocking uploads: not while the legacy stream is being captured (a capture
    # in the global mode on a BLOCKING stream, as tests/test_fm_mix_bank.py)
    t = torch.zeros(8 * 64, dtype=torch.int32, device="cuda:0")
    one = (ca._native._CFmRxJob * 1)()
    for i, f in enumerate(("d_fcw", "d_xval", "d_yval", "d_omag", "d_ofreq")):
        setattr(one[0], f, t[64 * i:].data_ptr())
    one[0].n = 64
    hip = MIX._hip()
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
        rc = L.cordic_rxbank_create(plan._h, ccfg.ref, 1, one, C.byref(h))
    finally:
        hip.hipStreamEndCapture(hs, C.byref(graph))
        hip.hipGetLastError()
    if graph.value:
        hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(hs)
    if rc == 0:
        L.cordic_rxbank_destroy(h)
    assert rc == ca.ERR_UNSUPPORTED and h.value == 0x5a5a
    assert (t == 0).all().item()
    spec = Spec("cfg2-cfg3", [5, 1025], 43)          # and afterwards all is well
    d = DeviceBank(torch, plan, ccfg, spec)
    d.bank.run()
    assert_equals(d.results(), spec.expected(), "after the refusals")
    d.bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_run_from_another_device_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    _, _, _, mcfg, ccfg = configs("cfg2-cfg3")
    plan = ca.Plan(mcfg)
    b = ca.RxBank(plan, ccfg, [])
    with torch.cuda.device(1):
        assert ca.lib().cordic_rxbank_run(b._h, None) == ca.ERR_ARGS
    b.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_the_example_builds_and_exits_0(tmp_path):
    """examples/afc_receiver.c: ONE receiver bank a round, three rounds, against
    one mixer bank into one demodulation bank on arrays of their own"""
    exe = tmp_path / "afc_receiver"
    r = subprocess.run(
        ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
         "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
         "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-o", str(exe),
         os.path.join(ROOT, "examples", "afc_receiver.c"),
         "-L", os.path.join(ROOT, "cordic_amd"), "-lcordic_amd", "-L", "/opt/rocm/lib",
         "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "cordic_amd"),
         "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "256 channels" in r.stdout and "x 3 rounds" in r.stdout
    assert "0 words differ" in r.stdout and "fused, two launches" in r.stdout
