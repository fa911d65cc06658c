"""Decimating FM mixer banks (cordic_mixbank_create_decim, _create_decim16;
include/cordic_amd.h): many cordic_plan_fm_mix_decim jobs of one plan and one k.
Expected values need no tolerance: per job the oracle's tuned samples for
numpy's wrapping running sum, summed as int64 over reshape(-1, R) and shifted
right by k; in addition the bank's bits must equal those of one decimating
single call per job on the same inputs."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
from test_fm_demod import Padded, last_value, last_word
from test_fm_mix_bank import spans_of
from test_fm_mix_decim import core, decimate, tuned, work_buffer
from test_table_fm import expected as phases, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("CORDIC_FMXB_MAX_BLOCKS", "CORDIC_FMXB_PASSES", "CORDIC_FMXB_MAX_SPANS")
# (name, int16 arrays, fused)
PLANS = (("cfg2", False, True), ("nat24", False, True), ("nat16", True, True),
         ("ww38", False, False), ("n9", True, False))
KS = (1, 3, 8)
M32 = 0xffffffff


def job_lengths(k):
    """37 lengths, all multiples of R: empty jobs, jobs of exactly one pass,
    jobs shorter than a pass, and jobs of several spans at one pass per span
    and at most three spans per job (5 * 1024 + R: six passes, three spans of
    two)"""
    R = 1 << k
    ns = [0, R, 1024, 2 * R, 1024 - R, 1024 + R, 0, 2048 + R, 1024, 3 * R, 5 * 1024 + R,
          2048, 1024, 0, 3 * 1024, 1024 + 2 * R, 4096 - R]
    rng = np.random.default_rng(50 + k)
    ns += [int(v) * R for v in rng.integers(1, 1 + 2500 // R, 20)]
    assert len(ns) == 37 and all(n % R == 0 for n in ns)
    return ns


class Jobs:
    """the host side of a bank: per job tuning words, optional pm, samples, an
    optional preset d_acc word and a phase0 whose sum with it wraps"""

    def __init__(self, name, i16, k, seed=60, ns=None):
        cfg = core(name, i16)
        rng = np.random.default_rng(seed + k)
        self.name, self.i16, self.k = name, i16, k
        self.ns = job_lengths(k) if ns is None else list(ns)     # (ns: multiples of R)
        self.fcw, self.pm, self.x, self.y, self.preset, self.phase0 = [], [], [], [], [], []
        for j, n in enumerate(self.ns):
            s = int(rng.integers(0, 1 << 30))
            self.fcw.append(words("random" if j % 5 else "fsk", n, s))
            self.pm.append(words("random", n, s + 1) if j % 2 else None)
            x, y = MIX16.iq16(rng, n, cfg.iw) if i16 else MIX.iq(rng, n, cfg.iw)
            self.x.append(x)
            self.y.append(y)
            self.preset.append((int(rng.integers(0, 1 << 32)) | 0x80000000) if j % 3 else None)
            self.phase0.append(int(rng.integers(0, 1 << 32)) | 0x80000000)

    def expected(self, starts):
        """per job (ox, oy, *d_acc afterwards) for the words in front of the run"""
        out = []
        for j, n in enumerate(self.ns):
            acc0 = 0 if starts[j] is None else starts[j]
            p, final = phases(self.fcw[j], self.pm[j], self.phase0[j], acc0)
            wx, wy = tuned(self.name, self.i16, self.x[j], self.y[j], p)
            out.append((decimate(wx, self.k), decimate(wy, self.k),
                        None if starts[j] is None else (final if n else acc0)))
        return out


@functools.lru_cache(maxsize=None)
def jobs_of(name, i16, k):
    jobs = Jobs(name, i16, k)
    first = jobs.expected(jobs.preset)
    second = jobs.expected([e[2] for e in first])
    return jobs, first, second


class Device:
    """`jobs` on the device: every array 4 bytes (2 for int16) behind a 16-byte
    boundary, outputs of n elements between guards of which n >> k are the
    bank's to write"""

    def __init__(self, torch, jobs):
        self.torch, self.jobs = torch, jobs
        off = 9 if jobs.i16 else 5
        i32 = lambda a: None if a is None else a.view(np.int32)
        self.arr = []
        for j, n in enumerate(jobs.ns):
            self.arr.append(dict(
                fcw=Padded(torch, n, 5, src=i32(jobs.fcw[j])),
                pm=None if jobs.pm[j] is None else Padded(torch, n, 5, src=i32(jobs.pm[j])),
                x=Padded(torch, n, off, i16=jobs.i16, src=jobs.x[j]),
                y=Padded(torch, n, off, i16=jobs.i16, src=jobs.y[j]),
                ox=Padded(torch, n, off, i16=jobs.i16),
                oy=Padded(torch, n, off, i16=jobs.i16),
                acc=None if jobs.preset[j] is None else last_word(torch, jobs.preset[j])))

    def tuples(self):
        v = lambda p: None if p is None else p.view
        return [(a["fcw"].view, v(a["pm"]), a["x"].view, a["y"].view, a["ox"].view,
                 a["oy"].view, n, self.jobs.phase0[j], a["acc"])
                for j, (a, n) in enumerate(zip(self.arr, self.jobs.ns))]

    def results(self):
        """[(ox, oy, acc)] after checking the guards -- everything at or behind
        n >> k of an output among them -- and the inputs"""
        self.torch.cuda.synchronize()
        jobs, k, out = self.jobs, self.jobs.k, []
        for j, (a, n) in enumerate(zip(self.arr, jobs.ns)):
            got = []
            for key in ("ox", "oy"):
                p = a[key]
                h = p.t.cpu().numpy()
                assert (h[:p.off] == p.sent).all() and (h[p.off + (n >> k):] == p.sent).all(), j
                got.append(h[p.off:p.off + (n >> k)].copy())
            assert np.array_equal(a["fcw"].get(), jobs.fcw[j].view(np.int32))
            assert a["pm"] is None or np.array_equal(a["pm"].get(), jobs.pm[j].view(np.int32))
            assert np.array_equal(a["x"].get(), jobs.x[j])
            assert np.array_equal(a["y"].get(), jobs.y[j])
            out.append((got[0], got[1], None if a["acc"] is None else last_value(a["acc"])))
        return out

    def clear_outputs(self):
        for a in self.arr:
            a["ox"].t.fill_(a["ox"].sent)
            a["oy"].t.fill_(a["oy"].sent)


def assert_equals(got, wanted, tag):
    for j, ((gx, gy, ga), (wx, wy, wa)) in enumerate(zip(got, wanted)):
        assert np.array_equal(gx, wx), (tag, j, gx.size)
        assert np.array_equal(gy, wy), (tag, j, gy.size)
        assert ga == wa, (tag, j, gx.size)


def single_calls(torch, plan, dev):
    """one decimating single call per job on the same inputs, into arrays and
    words of its own"""
    jobs, k, out = dev.jobs, dev.jobs.k, []
    off = 9 if jobs.i16 else 5
    work = work_buffer(torch, plan, max(jobs.ns), k, jobs.i16)
    call = plan.fm_mix_decim16 if jobs.i16 else plan.fm_mix_decim
    for j, (a, n) in enumerate(zip(dev.arr, jobs.ns)):
        ox = Padded(torch, n >> k, off, i16=jobs.i16)
        oy = Padded(torch, n >> k, off, i16=jobs.i16)
        acc = None if jobs.preset[j] is None else last_word(torch, jobs.preset[j])
        call(k, a["fcw"].view, a["x"].view, a["y"].view, ox.view, oy.view, work,
             pm=None if a["pm"] is None else a["pm"].view, n=n, phase0=jobs.phase0[j],
             acc=acc)
        torch.cuda.synchronize()
        out.append((ox.get(), oy.get(), None if acc is None else last_value(acc)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,i16,fused", PLANS)
def test_gpu_the_bank_equals_the_single_calls_and_the_oracle_and_continues(
        name, i16, fused, k, monkeypatch):
    import torch
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("CORDIC_FMXB_PASSES", "1")
    monkeypatch.setenv("CORDIC_FMXB_MAX_SPANS", "3")
    plan = ca.Plan(core(name, i16))
    jobs, first, second = jobs_of(name, i16, k)
    dev = Device(torch, jobs)
    Bank = ca.MixBank16 if i16 else ca.MixBank
    bank = Bank(plan, dev.tuples(), log2r=k)
    info = bank.info()
    assert info["samples"] == sum(jobs.ns) and info["fused"] == (1 if fused else 0)
    # the spans of the non-decimating bank of the same jobs
    plain = Bank(plan, dev.tuples())
    assert plain.info() == info
    plain.close()
    if fused:
        assert info["tile"] == 1024
        assert info["spans"] == sum(spans_of(n, 1, 3) for n in jobs.ns)
        assert any(spans_of(n, 1, 3) == 3 and n > 3 * 1024 for n in jobs.ns)
    singles = single_calls(torch, plan, dev)
    assert_equals(singles, first, "single")
    bank.run()
    assert_equals(dev.results(), first, "run 1")
    dev.clear_outputs()
    bank.run()                      # every channel continues from its d_acc
    assert_equals(dev.results(), second, "run 2")
    bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_create_refuses_what_the_decimated_ranges_do_not_allow():
    import torch
    from gpu_util import DEV
    plan = ca.Plan(MIX.both("cfg2")[0])
    n, k = 2048, 3
    m = n >> k
    # inputs: fcw, a gap of n words, x, y
    ins = torch.zeros(4 * n, dtype=torch.int32, device=DEV)
    outs = torch.zeros(4 * n, dtype=torch.int32, device=DEV)
    job = lambda ox, oy, n=n: (ins, None, ins[2 * n:], ins[3 * n:], ox, oy, n, 0, None)

    def refused(jobs, k=k):
        with pytest.raises(ca.CordicError) as e:
            ca.MixBank(plan, jobs, log2r=k)
        assert e.value.status == ca.ERR_ARGS

    # two jobs whose outputs are n >> k apart: a bank at k, none at k = 0
    packed = [job(outs, outs[m:]), job(outs[2 * m:], outs[3 * m:])]
    ca.MixBank(plan, packed, log2r=k).close()
    refused(packed, 0)
    with pytest.raises(ca.CordicError):
        ca.MixBank(plan, packed)
    refused([job(outs, outs[m - 1:])])                    # one element closer
    refused([job(outs, outs[m:], n - 4)])                 # n % R
    refused([job(outs, outs[m:])], 9)                     # k > 8
    ca.MixBank(plan, [job(outs, ins[2 * n - m:])], log2r=k).close()   # up to an input
    refused([job(outs, ins[2 * n - m + 1:])])             # its last element on d_xval
    ca.MixBank(plan, [], log2r=k).close()                 # no jobs
    plan.close()


@pytest.mark.gpu
def test_gpu_the_example_builds_and_says_that_nothing_differs(tmp_path):
    """examples/ddc_channeliser.c: a decimating 16-bit mixer bank (k = 3) into
    a 16-bit demodulation bank at the decimated length, three rounds, against
    per-channel cordic_plan_fm_mix16 calls, a host-side sum and
    cordic_fm_demod16"""
    exe = tmp_path / "ddc_channeliser"
    r = subprocess.run(
        ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
         "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
         "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-o", str(exe),
         os.path.join(ROOT, "examples", "ddc_channeliser.c"),
         "-L", os.path.join(ROOT, "cordic_amd"), "-lcordic_amd", "-L", "/opt/rocm/lib",
         "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "cordic_amd"),
         "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "-c", "256", "-l", "1504", "-r", "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "256 channels x 1504 samples x 3 rounds, decimated by 8 to 188" in r.stdout
    assert re.search(r"mixer bank: 385024 samples, \d+ spans of at most \d+ \(fused, two "
                     r"launches per round\)", r.stdout), r.stdout
    assert "\n0 shorts or words differ from the chain run channel by channel" in r.stdout
