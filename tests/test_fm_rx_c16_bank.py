"""Receiver banks on interleaved int16 I/Q (cordic_rxbank_create_c16 and
cordic_rxbank_create_decim_c16; include/cordic_amd.h): every job's d_iq is a
slice of ONE capture buffer at an odd complex offset.  The bank against the
oracle, against one single call per job and against the *16 bank on split
copies, words included; nothing has a tolerance, and the capture buffer is read
back unchanged after every run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import test_fm_rx_bank as RXB
import test_fm_rx_decim as RXD
from test_fm_demod import Padded, S16, last_word
from test_fm_rx_bank import RAGGED, Spec, assert_equals, clear_knobs, spans_of
from test_fm_rx_c16 import interleave, replay_three_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED, ONE_BY_ONE = "cfg1-io16", "cfg1-ww36"
RXB.BANKS.setdefault(ONE_BY_ONE, (ONE_BY_ONE, True, 0))     # (for Spec: a 16-bit pair)


def expected(spec, k=0, acc=None, last=None):
    """Spec.expected for a bank at R = 2^k: per job (mag, freq, *d_acc, *d_last)"""
    if not k:
        return spec.expected(acc, last)
    P, out = RXD.Pair(spec.name), []
    for j, n in enumerate(spec.ns):
        a0 = (spec.acc0[j] if acc is None else acc[j]) if spec.has_acc[j] else 0
        l0 = (spec.last0[j] if last is None else last[j]) if spec.has_last[j] else 0
        if n:
            m, f, fa, fl = RXD.Want(P, k, spec.fcw[j], spec.pm[j], spec.x[j], spec.y[j],
                                    spec.phase0[j], a0, spec.dphase0[j], l0).prefix(n >> k)
        else:
            m, f, fa, fl = np.zeros(0, np.int32), np.zeros(0, np.int32), a0, l0
        out.append((m, f, fa if spec.has_acc[j] else None, fl if spec.has_last[j] else None))
    return out


class IqBank(RXB.DeviceBank):
    """the jobs of a Spec with their I/Q interleaved in ONE device buffer, job j
    at the odd complex offset self.at[j] with sentinels between the jobs, and the
    interleaved bank over them (k > 0: a decimating one)"""

    def __init__(self, torch, plan, ccfg, spec, k=0, create=True):
        from gpu_util import DEV
        self.torch, self.spec, self.plan, self.ccfg, self.k = torch, spec, plan, ccfg, k
        self.words = torch.zeros(8 * max(1, len(spec.ns)), dtype=torch.int32, device=DEV)
        self.arr, self.at, cur = [], [], 1
        for j, n in enumerate(spec.ns):
            o = spec.offs[j]
            self.at.append(cur)
            cur += n + 1 + (n + 1) % 2              # the next offset is odd again
            self.arr.append(dict(fcw=Padded(torch, n, o[0]), pm=Padded(torch, n, o[1]),
                                 mag=Padded(torch, n >> k, o[4], True),
                                 freq=Padded(torch, n >> k, o[5], True)))
        assert all(a % 2 for a in self.at)
        self.host_iq = np.full(2 * (cur + 8), S16, dtype=np.int16)
        self.iq = torch.empty(self.host_iq.size, dtype=torch.int16, device=DEV)
        self.upload()
        self.preset()
        self.bank = ca.RxBankC16(plan, ccfg, self.jobs(), k or None) if create else None

    def iq_of(self, j):
        return self.iq[2 * self.at[j]:]

    def jobs(self):
        s = self.spec
        return [(a["fcw"].view, a["pm"].view if s.has_pm[j] else None, self.iq_of(j),
                 a["mag"].view, a["freq"].view, s.ns[j], s.phase0[j], self.acc(j),
                 s.dphase0[j], self.last(j)) for j, a in enumerate(self.arr)]

    def upload(self):
        s, t = self.spec, self.torch
        put = lambda p, v: p.t[p.off:p.off + p.n].copy_(
            t.from_numpy(np.ascontiguousarray(v).astype(np.int32)).to(p.t.device))
        for j, a in enumerate(self.arr):
            n = s.ns[j]
            if not n:
                continue
            put(a["fcw"], s.fcw[j].view(np.int32))
            if s.has_pm[j]:
                put(a["pm"], s.pm[j].view(np.int32))
            self.host_iq[2 * self.at[j]:2 * (self.at[j] + n)] = interleave(s.x[j], s.y[j])
        self.iq.copy_(t.from_numpy(self.host_iq).to(self.iq.device))

    def results(self):
        """per job (mag, freq, *d_acc, *d_last), after checking the guards, the
        capture buffer and the words nobody may write"""
        self.torch.cuda.synchronize()
        s = self.spec
        assert np.array_equal(self.iq.cpu().numpy(), self.host_iq)
        h = self.words.cpu().numpy().view(np.uint32)
        out = []
        for j, a in enumerate(self.arr):
            if s.ns[j]:
                assert np.array_equal(a["fcw"].get(), s.fcw[j].view(np.int32))
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

    def single_calls(self):
        """the same jobs through cordic_plan_fm_rx_c16 / _decim_c16, one call each
        on arrays of their own, from the same capture buffer"""
        from gpu_util import DEV
        t, s, k, plan, out = self.torch, self.spec, self.k, self.plan, []
        for j, n in enumerate(s.ns):
            o = s.offs[j]
            mag, freq = Padded(t, n >> k, o[5], True), Padded(t, n >> k, o[4], True)
            acc = last_word(t, s.acc0[j]) if s.has_acc[j] else None
            last = last_word(t, s.last0[j]) if s.has_last[j] else None
            a = self.arr[j]
            size = plan.fm_rx_decim_c16_workspace(self.ccfg, n, k) if k \
                else plan.fm_rx_c16_workspace(self.ccfg, n)
            work = t.zeros(max(16, size), dtype=t.uint8, device=DEV)
            kw = dict(pm=a["pm"].view if s.has_pm[j] else None, n=n, phase0=s.phase0[j],
                      acc=acc, dphase0=s.dphase0[j], last=last)
            if k:
                plan.fm_rx_decim_c16(self.ccfg, k, a["fcw"].view, self.iq_of(j), mag.view,
                                     freq.view, work, **kw)
            else:
                plan.fm_rx_c16(self.ccfg, a["fcw"].view, self.iq_of(j), mag.view, freq.view,
                               work, **kw)
            t.cuda.synchronize()
            word = lambda v: None if v is None else int(v.cpu().numpy().view(np.uint32)[0])
            out.append((mag.get().astype(np.int32), freq.get().astype(np.int32), word(acc),
                        word(last)))
        return out


def open_bank(torch, name, spec, k=0):
    _, _, _, mcfg, ccfg = RXB.configs(name)
    plan = ca.Plan(mcfg)
    return plan, ccfg, IqBank(torch, plan, ccfg, spec, k)


# ---------------------------------------------------------------- the plain bank

@pytest.mark.gpu
def test_gpu_a_ragged_bank_equals_the_single_calls_the_16_bit_bank_and_the_oracle(monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    spec = Spec(FUSED, RAGGED, 11)
    plan, ccfg, d = open_bank(torch, FUSED, spec)
    info = d.bank.info()
    assert info == dict(samples=sum(spec.ns), spans=spans_of(spec.ns), fused=1, tile=1024)
    d.bank.run()
    got = d.results()
    assert_equals(got, expected(spec), "oracle")
    assert_equals(got, d.single_calls(), "single calls")
    twin = RXB.DeviceBank(torch, plan, ccfg, spec)  # cordic_rxbank_create16 on split copies
    assert twin.bank.info() == info
    twin.bank.run()
    assert_equals(got, twin.results(), "the *16 bank")
    twin.bank.close()
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [dict(CORDIC_FMRXB_PASSES="1"),
                                   dict(CORDIC_FMRXB_PASSES="2"),
                                   dict(CORDIC_FMRXB_PASSES="4"),
                                   dict(CORDIC_FMRXB_MAX_SPANS="2"),
                                   dict(CORDIC_FMRXB_MAX_BLOCKS="1"),
                                   dict(CORDIC_FMRXB_MAX_BLOCKS="3")])
def test_gpu_forced_spans_span_caps_and_grid_caps_give_the_same_bits(knobs, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    lengths = [5 * 1024 + 3, 1020, 1021, 3, 0, 2 * 1020 + 1, 4 * 1016, 4 * 1016 + 1]
    spec = Spec(FUSED, lengths, 23)
    plan, ccfg, d = open_bank(torch, FUSED, spec)
    base = int(knobs.get("CORDIC_FMRXB_PASSES", 1))
    cap = int(knobs.get("CORDIC_FMRXB_MAX_SPANS", RXB.MAX_SPANS))
    assert d.bank.info()["spans"] == spans_of(lengths, base, cap)
    d.bank.run()
    assert_equals(d.results(), expected(spec), knobs)
    d.bank.close()
    plan.close()


# ---------------------------------------------------------------- decimating banks

@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3])
def test_gpu_a_decimating_bank_equals_the_oracle_and_the_single_calls(k, monkeypatch):
    """job lengths in decimated samples: one group, the first flush's 1020 +/- one
    group, no samples at all, several passes"""
    import torch
    clear_knobs(monkeypatch)
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    ms = [1, 1019, 1020, 1021, 0, 3, 2049, 257, 0, 64]
    spec = Spec(FUSED, [m << k for m in ms], 100 + k)
    plan, ccfg, d = open_bank(torch, FUSED, spec, k)
    info = d.bank.info()
    assert info["samples"] == sum(spec.ns) and info["fused"] == 1 and info["tile"] == 1024
    halo = max(4, 1 << k)
    assert info["spans"] == sum(-(-n // (1024 - halo)) for n in spec.ns)
    d.bank.run()
    got = d.results()
    assert_equals(got, expected(spec, k), ("oracle", k))
    assert_equals(got, d.single_calls(), ("single calls", k))
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name, k", [(FUSED, 0), (FUSED, 3), (ONE_BY_ONE, 1)])
def test_gpu_three_runs_on_new_data_continue_every_job(name, k, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    ms = [2049, 1, 1020, 0, 1025, 4]
    spec = Spec(name, [m << k for m in ms], 31, all_words=True, zero_phases=True)
    plan, ccfg, d = open_bank(torch, name, spec, k)
    acc, last = None, None
    for r in range(3):
        spec.renew(r)
        d.upload()
        d.clear_outputs()
        want = expected(spec, k, acc, last)
        d.bank.run()
        assert_equals(d.results(), want, (name, k, r))
        acc, last = [w[2] for w in want], [w[3] for w in want]
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 3])
def test_gpu_a_captured_run_replayed_three_times_continues_three_times(k, monkeypatch):
    """the same capture buffer every replay: replay r starts from the words that
    replay r - 1 left.  Two kernel nodes with one edge between them"""
    import torch
    clear_knobs(monkeypatch)
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    spec = Spec(FUSED, [m << k for m in (2049, 3, 1021, 0)], 37, all_words=True,
                zero_phases=True)
    plan, ccfg, d = open_bank(torch, FUSED, spec, k)
    warm = IqBank(torch, plan, ccfg, spec, k)       # once outside the capture first
    warm.bank.run()
    torch.cuda.synchronize()
    warm.bank.close()
    # (replay_three_times compares ONE job's outputs: job 0's; the others below)
    wants, acc, last = [], None, None
    for r in range(3):
        wants.append(expected(spec, k, acc, last))
        acc, last = [w[2] for w in wants[-1]], [w[3] for w in wants[-1]]
    a0 = d.arr[0]
    replay_three_times(torch, lambda s: d.bank.run(stream=s), a0["mag"], a0["freq"], True,
                       np.concatenate([w[0][0] for w in wants]),
                       np.concatenate([w[0][1] for w in wants]), spec.ns[0] >> k, k)
    assert_equals(d.results(), wants[2], ("after three replays", k))
    d.bank.close()
    plan.close()


# ---------------------------------------------------------------- one by one

@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2])
def test_gpu_a_bank_of_the_pair_that_is_not_fused_runs_one_by_one(k, monkeypatch):
    import torch
    clear_knobs(monkeypatch)
    monkeypatch.delenv("CORDIC_FMRXD_FALLBACK", raising=False)
    ms = [1025, 3, 0, 1020, 2049, 64]
    spec = Spec(ONE_BY_ONE, [m << k for m in ms], 53 + k)
    plan, ccfg, d = open_bank(torch, ONE_BY_ONE, spec, k)
    assert plan.fm_rx_c16_info(ccfg) == (0, 0)
    assert d.bank.info() == dict(samples=sum(spec.ns), spans=0, fused=0, tile=0)
    d.bank.run()
    got = d.results()
    assert_equals(got, expected(spec, k), ("oracle", k))
    assert_equals(got, d.single_calls(), ("single calls", k))
    d.bank.close()
    plan.close()


# ---------------------------------------------------------------- create's refusals

@pytest.mark.gpu
@pytest.mark.parametrize("name", [FUSED, ONE_BY_ONE])
def test_gpu_create_refuses_overlaps_and_bad_jobs_with_nothing_written(name, monkeypatch):
    """a job's d_iq is 4 n bytes: an output of ANOTHER job in its second half is
    an overlap, which a 2 n-byte range would miss"""
    import torch
    clear_knobs(monkeypatch)
    n = 1024
    spec = Spec(name, [n, n], 71, all_words=True)
    _, _, _, mcfg, ccfg = RXB.configs(name)
    plan = ca.Plan(mcfg)
    d = IqBank(torch, plan, ccfg, spec, create=False)
    base = d.jobs()
    KEYS = ("fcw", "pm", "iq", "mag", "freq", "n", "phase0", "acc", "dphase0", "last")
    iq0 = d.iq_of(0).data_ptr()
    L = ca.lib()

    def create(k, j, reserved=0, **kw):
        """job j with the fields of kw replaced (addresses or tensors)"""
        from cordic_amd import _native
        arr = (_native._CFmRxJobC16 * 2)()
        for i, jb in enumerate(base):
            f = dict(zip(KEYS, jb))
            if i == j:
                f.update(kw)
            ptr = lambda v: v if isinstance(v, (int, type(None))) else v.data_ptr()
            arr[i].d_fcw, arr[i].d_pm, arr[i].d_iq = ptr(f["fcw"]), ptr(f["pm"]), ptr(f["iq"])
            arr[i].d_omag, arr[i].d_ofreq = ptr(f["mag"]), ptr(f["freq"])
            arr[i].d_acc, arr[i].d_last = ptr(f["acc"]), ptr(f["last"])
            arr[i].n, arr[i].phase0, arr[i].dphase0 = f["n"], f["phase0"], f["dphase0"]
            arr[i].reserved = reserved if i == j else 0
        h = C.c_void_p()
        if k is None:
            rc = L.cordic_rxbank_create_c16(plan._h, ccfg.ref, 2, arr, C.byref(h))
        else:
            rc = L.cordic_rxbank_create_decim_c16(plan._h, ccfg.ref, k, 2, arr, C.byref(h))
        if rc == 0:
            L.cordic_rxbank_destroy(h)
        else:
            assert not h.value
        return rc

    word_at = lambda byte: (iq0 + byte + 3) & ~3
    bad = [dict(mag=iq0), dict(freq=iq0 + 2 * n - 2),       # job 1's outputs in job 0's first half
           dict(mag=iq0 + 2 * n), dict(freq=iq0 + 4 * n - 2),       # ... and in its second half
           dict(last=word_at(2 * n + 8)), dict(acc=word_at(4 * n - 4)), dict(acc=word_at(8)),
           dict(iq=d.iq_of(1).data_ptr() + 2), dict(iq=d.iq_of(1).data_ptr() + 1),
           dict(iq=None), dict(mag=None), dict(mag=base[0][3]), dict(last=base[0][9])]
    for k in (None, 0, 3):
        assert create(k, 1) == 0
        for kw in bad:
            assert create(k, 1, **kw) == ca.ERR_ARGS, (k, sorted(kw))
        assert create(k, 1, reserved=1) == ca.ERR_ARGS
        assert create(k, 0, reserved=1 << 40) == ca.ERR_ARGS
    # one short behind the 4 n bytes is clear (k = 8: 4 shorts, in front of job 1's d_iq)
    assert create(8, 1, mag=iq0 + 4 * n) == 0
    assert create(8, 1, mag=iq0 + 4 * n - 2) == ca.ERR_ARGS
    assert create(3, 1, n=n + 4) == ca.ERR_ARGS             # n % R != 0
    assert create(9, 1) == ca.ERR_ARGS
    assert create(2, 1, n=n + 4) == 0
    torch.cuda.synchronize()
    assert d.outputs_untouched()
    assert np.array_equal(d.iq.cpu().numpy(), d.host_iq)
    # and the same jobs make a bank that runs clean
    d.bank = ca.RxBankC16(plan, ccfg, base)
    d.bank.run()
    assert_equals(d.results(), expected(spec), name)
    d.bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_the_example_builds_and_exits_0(tmp_path):
    """examples/rx_c16.c: one interleaved capture buffer of 256 channels x 1536
    complex samples through ONE decimating bank at k = 3 for three rounds,
    against cordic_plan_fm_rx_decim16 per channel on arrays split on the host"""
    exe = tmp_path / "rx_c16"
    r = subprocess.run(
        ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
         "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
         "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-o", str(exe),
         os.path.join(ROOT, "examples", "rx_c16.c"),
         "-L", os.path.join(ROOT, "cordic_amd"), "-lcordic_amd", "-L", "/opt/rocm/lib",
         "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "cordic_amd"),
         "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "256 channels" in r.stdout and "x 3 rounds" in r.stdout
    assert "0 words differ" in r.stdout and "fused, two launches" in r.stdout
