"""Decimating receiver banks (cordic_rxbank_create_decim, _create_decim16;
include/cordic_amd.h): many cordic_plan_fm_rx_decim jobs of one plan, one
converter and one k in two launches.  A bank's bits must equal those of one
decimating single call per job on the same inputs -- every sample and both
words -- which tests/test_fm_rx_decim.py holds to the oracle."""
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import test_fm_mix as MIX
from test_fm_demod import S32, Padded, last_value, last_word
from test_fm_rx_decim import Pair, zeros
from test_table_fm import words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("CORDIC_FMRXB_MAX_BLOCKS", "CORDIC_FMRXB_PASSES", "CORDIC_FMRXB_MAX_SPANS",
         "CORDIC_FMRXD_MAX_BLOCKS", "CORDIC_FMRXD_FALLBACK")


def job_ms(k):
    """decimated lengths: an empty job, the partial vector, the wave edge, the
    first flush's 1020, a second flush, and a job of many spans"""
    return [0, 1, 5, 257, 1021, 1025, 2049 + (1024 * 16 >> k)]


class Jobs:
    """the host side of a bank: per job tuning words, optional pm, samples,
    optional preset words and a phase0 / dphase0 with high bits"""

    def __init__(self, P, k, ms, seed):
        rng = np.random.default_rng(seed + k)
        self.P, self.k, self.ms = P, k, ms
        self.ns = [m << k for m in ms]
        self.fcw, self.pm, self.acc0, self.last0, self.p0, self.d0 = [], [], [], [], [], []
        for j, n in enumerate(self.ns):
            s = int(rng.integers(0, 1 << 30))
            self.fcw.append(words("random", n, s))
            self.pm.append(words("random", n, s + 1) if j % 2 else None)
            self.acc0.append((int(rng.integers(0, 1 << 32)) | 0x80000000) if j % 3 else None)
            self.last0.append(int(rng.integers(0, 1 << 32)) if j % 4 != 1 else None)
            self.p0.append(int(rng.integers(0, 1 << 32)) | 0x80000000)
            self.d0.append(int(rng.integers(0, 1 << 32)))
        self.new_samples(rng)

    def new_samples(self, rng):
        xy = [MIX.iq(rng, n, self.P.mcfg.iw) for n in self.ns]
        self.x, self.y = [a for a, _ in xy], [b for _, b in xy]


class Device:
    """`jobs` on the device, every array 4 bytes (2 on shorts) off a 16-byte
    boundary; words: the d_acc / d_last values in front of the first run"""

    def __init__(self, torch, jobs):
        self.torch, self.jobs = torch, jobs
        i16, off = jobs.P.i16, 9 if jobs.P.i16 else 5
        i32 = lambda a: None if a is None else a.view(np.int32)
        self.arr = []
        for j, n in enumerate(jobs.ns):
            self.arr.append(dict(
                fcw=Padded(torch, n, 5, src=i32(jobs.fcw[j])),
                pm=None if jobs.pm[j] is None else Padded(torch, n, 5, src=i32(jobs.pm[j])),
                x=Padded(torch, n, off, i16, src=jobs.x[j]),
                y=Padded(torch, n, off, i16, src=jobs.y[j]),
                mag=Padded(torch, jobs.ms[j], off, i16), freq=Padded(torch, jobs.ms[j], off, i16),
                acc=None if jobs.acc0[j] is None else last_word(torch, jobs.acc0[j]),
                last=None if jobs.last0[j] is None else last_word(torch, jobs.last0[j])))

    def load_samples(self):
        from gpu_util import DEV
        for j, a in enumerate(self.arr):
            for key, src in (("x", self.jobs.x[j]), ("y", self.jobs.y[j])):
                p = a[key]
                if p.n:
                    p.t[p.off:p.off + p.n].copy_(
                        self.torch.from_numpy(src.astype(p.np)).to(DEV))

    def tuples(self):
        v = lambda p: None if p is None else p.view
        J = self.jobs
        return [(a["fcw"].view, v(a["pm"]), a["x"].view, a["y"].view, a["mag"].view,
                 a["freq"].view, J.ns[j], J.p0[j], a["acc"], J.d0[j], a["last"])
                for j, a in enumerate(self.arr)]

    def results(self):
        """[(mag, freq, acc, last)] after checking the guards and the inputs"""
        self.torch.cuda.synchronize()
        out = []
        for j, a in enumerate(self.arr):
            assert np.array_equal(a["x"].get(), self.jobs.x[j])
            assert np.array_equal(a["y"].get(), self.jobs.y[j])
            assert np.array_equal(a["fcw"].get(), self.jobs.fcw[j].view(np.int32))
            out.append((a["mag"].get().copy(), a["freq"].get().copy(),
                        None if a["acc"] is None else last_value(a["acc"]),
                        None if a["last"] is None else last_value(a["last"])))
        return out

    def clear_outputs(self):
        for a in self.arr:
            a["mag"].t.fill_(a["mag"].sent)
            a["freq"].t.fill_(a["freq"].sent)


def single_calls(torch, plan, dev, starts):
    """one decimating single call per job on the same inputs, into arrays and
    words of its own; starts: per job (acc, last) in front, or None each"""
    J, out = dev.jobs, []
    P, k = J.P, J.k
    off = 9 if P.i16 else 5
    ws = plan.fm_rx_decim16_workspace if P.i16 else plan.fm_rx_decim_workspace
    fn = plan.fm_rx_decim16 if P.i16 else plan.fm_rx_decim
    work = zeros(torch, ws(P.ccfg, max(J.ns), k))
    for j, (a, n) in enumerate(zip(dev.arr, J.ns)):
        mag, freq = Padded(torch, n >> k, off, P.i16), Padded(torch, n >> k, off, P.i16)
        acc = None if starts[j][0] is None else last_word(torch, starts[j][0])
        last = None if starts[j][1] is None else last_word(torch, starts[j][1])
        fn(P.ccfg, k, a["fcw"].view, a["x"].view, a["y"].view, mag.view, freq.view, work,
           pm=None if a["pm"] is None else a["pm"].view, n=n, phase0=J.p0[j], acc=acc,
           dphase0=J.d0[j], last=last)
        torch.cuda.synchronize()
        out.append((mag.get().copy(), freq.get().copy(),
                    None if acc is None else last_value(acc),
                    None if last is None else last_value(last)))
    return out


def assert_equals(got, wanted, tag):
    for j, (g, w) in enumerate(zip(got, wanted)):
        assert np.array_equal(g[0], w[0]), (tag, j, g[0].size)
        assert np.array_equal(g[1], w[1]), (tag, j, g[1].size)
        assert g[2:] == w[2:], (tag, j)


def bank_of(P, plan, tuples, k):
    return (ca.RxBank16 if P.i16 else ca.RxBank)(plan, P.ccfg, tuples, log2r=k)


@pytest.mark.gpu
@pytest.mark.parametrize("passes", ["3", "2"])
@pytest.mark.parametrize("k", [1, 3, 6])
@pytest.mark.parametrize("pair", ["cfg2-cfg3", "nat24-cfg3", "cfg1-io16"])
def test_gpu_the_bank_equals_one_single_call_per_job_and_continues(pair, k, passes,
                                                                   monkeypatch):
    """jobs cut into several spans with halos; three runs on new samples
    continue every channel three times.  CORDIC_FMRXB_PASSES=3 is no power of
    two, which the knob takes no notice of: the bank then cuts by its own rule
    (one pass a span for a bank this small).  =2 forces spans of two passes
    less the halo, and the span count is checked against that."""
    import torch
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("CORDIC_FMRXB_PASSES", passes)
    P = Pair(pair)
    plan = P.plan()
    jobs = Jobs(P, k, job_ms(k), 70)
    dev = Device(torch, jobs)
    bank = bank_of(P, plan, dev.tuples(), k)
    info = bank.info()
    assert info["samples"] == sum(jobs.ns) and info["fused"] == 1 and info["tile"] == 1024
    halo = max(4, 1 << k)
    if passes == "2":
        per = 2 * 1024 - halo
        assert info["spans"] == sum(-(-n // per) for n in jobs.ns)
        assert max(jobs.ns) > 2 * per       # a span with a neighbour on both sides
    assert info["spans"] > sum(1 for n in jobs.ns if n)     # some job has a halo
    starts = list(zip(jobs.acc0, jobs.last0))
    rng = np.random.default_rng(700 + k)
    for r in range(3):
        want = single_calls(torch, plan, dev, starts)
        dev.clear_outputs()
        bank.run()
        assert_equals(dev.results(), want, "run %d" % r)
        starts = [(w[2], w[3]) for w in want]
        jobs.new_samples(rng)
        dev.load_samples()
    bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_k_0_is_the_receiver_bank(monkeypatch):
    import torch
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("CORDIC_FMRXB_PASSES", "1")
    P = Pair("cfg2-cfg3")
    plan = P.plan()
    jobs = Jobs(P, 0, [0, 5, 1021, 2049], 80)
    got = []
    for log2r in (0, None):
        dev = Device(torch, jobs)
        bank = ca.RxBank(plan, P.ccfg, dev.tuples(), log2r=log2r)
        got.append((bank.info(), dev, bank))
        bank.run()
    assert got[0][0] == got[1][0]
    assert_equals(got[0][1].results(), got[1][1].results(), "k = 0")
    for _, _, bank in got:
        bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["ww38-cfg3", "cfg2-ug_lj"])
def test_gpu_a_bank_of_a_pair_that_is_not_fused_equals_the_single_calls(pair, monkeypatch):
    import torch
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    P = Pair(pair)
    plan = P.plan()
    k = 2
    jobs = Jobs(P, k, [0, 1, 257, 1025], 90)
    dev = Device(torch, jobs)
    bank = bank_of(P, plan, dev.tuples(), k)
    assert bank.info()["fused"] == 0 and bank.info()["spans"] == 0
    want = single_calls(torch, plan, dev, list(zip(jobs.acc0, jobs.last0)))
    bank.run()
    assert_equals(dev.results(), want, pair)
    bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_create_refuses_what_the_decimated_ranges_do_not_allow():
    import torch
    from gpu_util import DEV
    P = Pair("cfg2-cfg3")
    plan = P.plan()
    n, k = 2048, 3
    m = n >> k
    # inputs: fcw, a gap of n words, x, y
    ins = torch.zeros(4 * n, dtype=torch.int32, device=DEV)
    outs = torch.zeros(4 * n, dtype=torch.int32, device=DEV)
    wd = torch.zeros(8, dtype=torch.int32, device=DEV)
    job = lambda mag, freq, n=n, acc=None, last=None: (
        ins, None, ins[2 * n:], ins[3 * n:], mag, freq, n, 0, acc, 0, last)

    def refused(jobs, k=k):
        with pytest.raises(ca.CordicError) as e:
            ca.RxBank(plan, P.ccfg, jobs, log2r=k)
        assert e.value.status == ca.ERR_ARGS

    # two jobs whose outputs are n >> k apart: a bank at k, none at k = 0
    packed = [job(outs, outs[m:]), job(outs[2 * m:], outs[3 * m:])]
    ca.RxBank(plan, P.ccfg, packed, log2r=k).close()
    refused(packed, 0)
    with pytest.raises(ca.CordicError):
        ca.RxBank(plan, P.ccfg, packed)
    refused([job(outs, outs[m - 1:])])                    # one element closer
    refused([job(outs, outs[m:], n - 4)])                 # n % R
    refused([job(outs, outs[m:])], 9)                     # k > 8
    # an output up to an input: clear by its (n >> k) range, not by its n range
    ca.RxBank(plan, P.ccfg, [job(outs, ins[2 * n - m:])], log2r=k).close()
    refused([job(outs, ins[2 * n - m + 1:])])             # its last element on d_xval
    refused([job(outs, outs[m:], last=wd), job(outs[2 * m:], outs[3 * m:], last=wd)])
    refused([job(outs, outs[m:], acc=wd), job(outs[2 * m:], outs[3 * m:], acc=wd)])
    refused([job(outs, outs[m:], acc=wd, last=wd)])
    ca.RxBank(plan, P.ccfg, [job(outs, outs[m:], acc=wd, last=wd[1:]),
                             job(outs[2 * m:], outs[3 * m:], acc=wd[2:], last=wd[3:])],
              log2r=k).close()
    ca.RxBank(plan, P.ccfg, [], log2r=k).close()          # no jobs
    # the converter's checks come in front of k: a rotator is a mode error
    with pytest.raises(ca.CordicError) as e:
        ca.RxBank(plan, P.mcfg, [job(outs, outs[m:])], log2r=9)
    assert e.value.status == ca.ERR_MODE
    plan.close()


@pytest.mark.gpu
def test_gpu_the_example_builds_and_says_that_nothing_differs(tmp_path):
    """examples/ddc_receiver.c: ddc_channeliser.c's 256 int16 channels at k = 3
    as ONE decimating receiver bank, three rounds, against the decimating mixer
    bank into the demodulation bank"""
    exe = tmp_path / "ddc_receiver"
    r = subprocess.run(
        ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
         "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
         "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-o", str(exe),
         os.path.join(ROOT, "examples", "ddc_receiver.c"),
         "-L", os.path.join(ROOT, "cordic_amd"), "-lcordic_amd", "-L", "/opt/rocm/lib",
         "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "cordic_amd"),
         "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "-c", "256", "-l", "1504", "-r", "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "256 channels x 1504 samples x 3 rounds, decimated by 8 to 188" in r.stdout
    assert re.search(r"receiver bank: 385024 samples, \d+ spans of passes of 1024 \(fused, "
                     r"two launches per round\)", r.stdout), r.stdout
    assert "\n0 shorts or words differ from the decimating mixer bank" in r.stdout
