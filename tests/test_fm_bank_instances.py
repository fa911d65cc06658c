"""Every instance of the FM bank kernels against the oracle.  The receiver banks
(fm_rxbank_xydir<LJ, N, IO>, cordic_fm_rx_bank.hip, and its decimating twin) and
the mixer banks (cordic_fm_mix_bank.hip, cordic_fm_mix_bank_decim.hip) are
__global__ instantiations of their own with entry-point tables of their own:
one per stage count of FMX_STAGES (cordic_fm_mix.h), per unit and per form.
Here each one runs a small ragged bank -- one-pass spans, every array off the
16-byte grid between sentinels -- once on the grid the library chooses and once
on two blocks, and every output sample and every d_acc / d_last word is compared
with the oracle; then every k of the decimating banks runs on the named cores.
The helpers are the bank tests' own.  Nothing has a tolerance."""
import contextlib
import os
import re

import numpy as np
import pytest

import cordic_amd as ca
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
import test_fm_mix_bank as MIXB
import test_fm_mix_decim_bank as MIXDB
import test_fm_rx as RX
import test_fm_rx16 as RX16
import test_fm_rx_bank as RXB
import test_fm_rx_c16_bank as C16
import test_fm_rx_decim as RXD
import test_fm_rx_decim_bank as RXDB
from test_table_fm import expected as phases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")
STAGES = (13, 16, 19, 20, 24, 27, 29)
RX_UNITS = ("lj30", "lj29", "io16", "c16")
MIX_UNITS = ("lj30", "lj29", "io16")
FORMS = ("plain", "decim")
RX_CASES = [(u, n, f) for u in RX_UNITS for n in STAGES for f in FORMS]
MIX_CASES = [(u, n, f) for u in MIX_UNITS for n in STAGES for f in FORMS]
KNOBS = tuple(sorted(set(RXB.KNOBS) | set(RXDB.KNOBS) | set(MIXB.KNOBS)))
PASS = 1024
# plain banks at one pass a span: a receiver's span is 1020 samples.  An empty
# job, a partial vector, one span exactly, a second span of one sample, and a
# job of four spans (front_sum at d.idx >= 2, a span with two neighbours)
RX_LENGTHS = [0, 1, 5, 1019, 1020, 1021, 2 * 1020 + 1, 3 * 1020 + 7]
# (a mixer's span is 1024: one pass exactly as well)
MIX_LENGTHS = RX_LENGTHS + [1024]
K, DECIM_MS = 3, [0, 1, 5, 257, 1021, 2049]        # decimated lengths
SWEEP_MS = [0, 1, 5, 257, 1021, 1025]
TOP = 0x80000000


def case_id(v):
    return str(v)


# ---------------------------------------------------------------- the cores

def unit_core(unit, n):
    """(rotator's cli arguments, WW, the converter's name, int16 arrays?)"""
    if unit == "lj29":
        return (ca.P2R, 32, 32, 2, 32, n), 35, "cfg3", False
    if unit == "lj30":
        return (ca.P2R, 31, 31, 2, 32, n), 34, "cfg3", False
    return (ca.P2R, 16, 16, 15, 32, n), 32, "io16", True


@contextlib.contextmanager
def registered(unit, n):
    """the instance's core under a name of its own in the helpers' dicts, for
    the mixer helpers (MIX.CORES / MIX16.CORES16) and the receiver's (RX.PAIRS /
    RX16.PAIRS, RXB.BANKS)"""
    args, ww, conv, i16 = unit_core(unit, n)
    name = "bank_%s_%d" % (unit, n)
    cores, pairs = (MIX16.CORES16, RX16.PAIRS) if i16 else (MIX.CORES, RX.PAIRS)
    cores[name] = (args, 0)
    pairs[name] = (name, conv, 1)
    RXB.BANKS[name] = (name, i16, 1)
    try:
        cfg = ca.Config.from_cli(*args)
        assert cfg.ww == ww and cfg.nlive == n and cfg.pw == 32
        yield name, i16
    finally:
        del cores[name], pairs[name], RXB.BANKS[name]


def set_knobs(monkeypatch, **knobs):
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def rx_spans(ns, k=0):
    """the host rule at one pass a span: 1024 less the halo of max(4, 2^k)"""
    if not k:
        return RXB.spans_of(ns)
    per = PASS - max(4, 1 << k)
    return sum(-(-n // per) for n in ns)


# ---------------------------------------------------------------- receiver banks

def rx_spec(name, i16, lengths, seed):
    """RXB.Spec with every array off the 16-byte grid and the top bit of phase0
    and of both preset words set"""
    spec = RXB.Spec(name, lengths, seed)
    for j in range(len(spec.ns)):
        # words: 1 .. 3 elements off; shorts: 1 .. 7
        spec.offs[j] = [1 + (j + a) % 3 for a in range(2)] \
            + [1 + (j + a) % (7 if i16 else 3) for a in range(2, 6)]
        spec.phase0[j] |= TOP
        spec.acc0[j] |= TOP
        spec.last0[j] |= TOP
    assert 0 < sum(spec.has_pm) < len(spec.ns) and 0 < sum(spec.has_acc) < len(spec.ns) \
        and 0 < sum(spec.has_last) < len(spec.ns)
    return spec


def rx_spec_results(d):
    """DeviceBank.results (IqBank.results) and the inputs it does not read back"""
    got = d.results()
    s = d.spec
    for j, a in enumerate(d.arr):
        if not s.ns[j]:
            continue
        if s.has_pm[j]:
            assert np.array_equal(a["pm"].get(), s.pm[j].view(np.int32)), j
        if "y" in a:
            assert np.array_equal(a["y"].get(), s.y[j]), j
    return got


def rx_jobs_want(jobs):
    """RXDB.Jobs against the composed oracle: per job (mag, freq, *d_acc, *d_last)"""
    out = []
    for j, m in enumerate(jobs.ms):
        a0, l0 = jobs.acc0[j] or 0, jobs.last0[j] or 0
        if m:
            mag, freq, fa, fl = RXD.Want(jobs.P, jobs.k, jobs.fcw[j], jobs.pm[j], jobs.x[j],
                                         jobs.y[j], jobs.p0[j], a0, jobs.d0[j], l0).prefix(m)
        else:
            mag, freq, fa, fl = np.zeros(0, np.int32), np.zeros(0, np.int32), a0, l0
        out.append((mag, freq, None if jobs.acc0[j] is None else fa,
                    None if jobs.last0[j] is None else fl))
    return out


def rx_jobs_results(dev):
    got = dev.results()
    for j, a in enumerate(dev.arr):
        if a["pm"] is not None:
            assert np.array_equal(a["pm"].get(), dev.jobs.pm[j].view(np.int32)), j
    return got


def check_info(info, samples, spans):
    assert info == dict(samples=samples, spans=spans, fused=1, tile=PASS)


def on_both_grids(plan, knob, monkeypatch, twice, make, check):
    """make() opens a bank (its .bank) on fresh arrays and freshly preset words,
    check(d, cap) runs it and compares: on the grid the library chooses and,
    where `twice`, again with `knob` = 2.  The knob is read at every run; that
    it is the name the launcher reads is pinned with the matrix below (info()
    does not show the grid).  The plan and every bank are closed here, whatever
    check raises."""
    with contextlib.closing(plan):
        for cap in (None, "2") if twice else (None,):
            if cap:
                monkeypatch.setenv(knob, cap)
            d = make()
            with contextlib.closing(d.bank):
                check(d, cap)


def run_rx_plain(torch, name, i16, c16, lengths, seed, monkeypatch, twice=True):
    spec = rx_spec(name, i16, lengths, seed)
    want = C16.expected(spec)
    _, _, _, mcfg, ccfg = RXB.configs(name)
    plan = ca.Plan(mcfg)

    def check(d, cap):
        check_info(d.bank.info(), sum(spec.ns), rx_spans(spec.ns))
        d.bank.run()
        RXB.assert_equals(rx_spec_results(d), want, (name, cap))
    on_both_grids(plan, "CORDIC_FMRXB_MAX_BLOCKS", monkeypatch, twice,
                  lambda: (C16.IqBank if c16 else RXB.DeviceBank)(torch, plan, ccfg, spec),
                  check)


def run_rx_decim(torch, name, i16, c16, k, ms, seed, monkeypatch, twice=True):
    """the decimating bank of `ms` decimated samples per job; the number of
    spans of the longest job"""
    ns = [m << k for m in ms]
    if c16:
        spec = rx_spec(name, True, ns, seed)
        want = C16.expected(spec, k)
        _, _, _, mcfg, ccfg = RXB.configs(name)
        plan = ca.Plan(mcfg)
        make = lambda: C16.IqBank(torch, plan, ccfg, spec, k)
        read, equal = rx_spec_results, RXB.assert_equals
    else:
        P = RXD.Pair(name)
        assert P.i16 == i16
        jobs = RXDB.Jobs(P, k, ms, seed)
        assert any(v is None for v in jobs.pm) and any(v is not None for v in jobs.pm)
        assert all(p & TOP for p in jobs.p0) and all(a & TOP for a in jobs.acc0 if a is not None)
        jobs.last0 = [None if v is None else v | TOP for v in jobs.last0]
        want = rx_jobs_want(jobs)
        plan = P.plan()

        def make():
            dev = RXDB.Device(torch, jobs)
            dev.bank = RXDB.bank_of(P, plan, dev.tuples(), k)
            return dev
        read, equal = rx_jobs_results, RXDB.assert_equals

    def check(d, cap):
        check_info(d.bank.info(), sum(ns), rx_spans(ns, k))
        d.bank.run()
        equal(read(d), want, (name, k, cap))
    on_both_grids(plan, "CORDIC_FMRXB_MAX_BLOCKS", monkeypatch, twice, make, check)
    return rx_spans([max(ns)], k)


# ---------------------------------------------------------------- mixer banks

def run_mix_plain(torch, name, i16, lengths, seed, monkeypatch):
    cfg = MIXDB.core(name, i16)
    if i16:
        spec = MIX16.Spec16(seed, lengths)
        tuned, Dev = MIX16.want16, MIX16.DeviceBank16
    else:
        k = len(lengths)
        spec = MIXB.Spec(lengths, cfg.iw, seed, with_acc=False, with_pm=False)
        spec.has_pm, spec.has_acc = [bool(j % 2) for j in range(k)], [bool(j % 3) for j in range(k)]
        spec.renew(seed + 1)
        tuned, Dev = MIX.want, MIXB.DeviceBank
    assert all(p & TOP for p in spec.phase0) and all(p & TOP for p in spec.preset)
    assert 0 < sum(spec.has_pm) < len(spec.ns) and 0 < sum(spec.has_acc) < len(spec.ns)
    want = []
    for j, n in enumerate(spec.ns):
        acc0 = spec.preset[j] if spec.has_acc[j] else 0
        p, final = phases(spec.fcw[j], spec.pm[j], spec.phase0[j], acc0)
        wx, wy = tuned(name, spec.x[j], spec.y[j], p)
        want.append((wx, wy, None if not spec.has_acc[j] else final if n else acc0))
    plan = ca.Plan(cfg)

    def check(d, cap):
        check_info(d.bank.info(), sum(spec.ns), sum(MIXB.spans_of(n, 1) for n in spec.ns))
        d.bank.run()
        got, accs = d.results()
        MIXB.assert_equals(got, accs, want, (name, cap))
    on_both_grids(plan, "CORDIC_FMXB_MAX_BLOCKS", monkeypatch, True,
                  lambda: Dev(torch, plan, spec), check)


def run_mix_decim(torch, name, i16, k, ms, seed, monkeypatch, twice=True):
    ns = [m << k for m in ms]
    jobs = MIXDB.Jobs(name, i16, k, seed, ns=ns)
    assert any(v is None for v in jobs.pm) and any(v is None for v in jobs.preset)
    assert all(p & TOP for p in jobs.phase0)
    want = jobs.expected(jobs.preset)       # 64-bit sums, floored
    plan = ca.Plan(MIXDB.core(name, i16))

    def make():
        dev = MIXDB.Device(torch, jobs)
        dev.bank = (ca.MixBank16 if i16 else ca.MixBank)(plan, dev.tuples(), log2r=k)
        return dev

    def check(dev, cap):
        check_info(dev.bank.info(), sum(ns), sum(MIXB.spans_of(n, 1) for n in ns))
        dev.bank.run()
        MIXDB.assert_equals(dev.results(), want, (name, k, cap))
    on_both_grids(plan, "CORDIC_FMXB_MAX_BLOCKS", monkeypatch, twice, make, check)
    return MIXB.spans_of(max(ns), 1)


# ---------------------------------------------------------------- no GPU

def params_of(test):
    marks = [m for m in test.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "unit,stages,form"
    return list(marks[0].args[1])


def test_the_matrix_is_the_stage_list_times_the_unit_lists_of_the_sources():
    """a stage count or a container added to the sources without a row here
    fails: FMX_STAGES and fmx::with_unit (cordic_fm_mix.h), CORDIC_FMRX_UNITS
    (cordic_fm_rx_unit.h)"""
    mix_h = open(os.path.join(CSRC, "cordic_fm_mix.h")).read()
    unit_h = open(os.path.join(CSRC, "cordic_fm_rx_unit.h")).read()
    m = re.search(r"^#define\s+FMX_STAGES\(X\)(.*)$", mix_h, re.M)
    stages = [int(v) for v in re.findall(r"X\((\d+)\)", m.group(1))]
    assert re.sub(r"X\(\d+\)|\s", "", m.group(1)) == ""
    assert stages == list(STAGES) == list(MIX.INSTANCES)
    m = re.search(r"^#define\s+CORDIC_FMRX_UNITS\(X\)\s*\\\n(.*)$", unit_h, re.M)
    rx_units = re.findall(r"X\((\w+),\s*(\d+),\s*([\w:]+)\)", m.group(1))
    assert re.sub(r"X\(\w+,\s*\d+,\s*[\w:]+\)|\s", "", m.group(1)) == ""
    assert [u[0] for u in rx_units] == list(RX_UNITS)
    body = re.search(r"bool with_unit\(Unit u, F &&f\)\s*\{(.*?)\n\}", mix_h, re.S).group(1)
    cases = re.findall(r"case kUnit(\w+):\s*return f\(std::integral_constant<int, (\d+)>\{\}, "
                       r"(\w+)\{\}\);", body)
    assert len(cases) == body.count("case ")
    assert [c[0].lower() for c in cases] == list(MIX_UNITS)
    # the same <LJ, container> under the same suffix in both lists
    of = {sfx: (lj, io.split("::")[-1]) for sfx, lj, io in rx_units}
    for sfx, lj, io in cases:
        assert of[sfx.lower()] == (lj, io)
    # the cores below are the units': WW 35 is LJ 29, shorts at WW < 35
    for unit in RX_UNITS:
        _, ww, _, i16 = unit_core(unit, 16)
        assert 64 - ww >= int(of[unit][0]) and (ww == 35) == (of[unit][0] == "29")
        assert i16 == (of[unit][1] != "Io32")
    # the grid caps of the second runs are the names the two launchers read
    # (at every run), and the helpers' knob lists clear them
    for src, knob, knobs in (("cordic_fm_rx_bank.hip", "CORDIC_FMRXB_MAX_BLOCKS", RXB.KNOBS),
                             ("cordic_fm_mix_bank.hip", "CORDIC_FMXB_MAX_BLOCKS", MIXB.KNOBS)):
        text = open(os.path.join(CSRC, src)).read()
        assert re.search(r'span_grids\([^;]*"%s"' % knob, text), knob
        assert knob in knobs and knob in KNOBS
    rx = params_of(test_gpu_every_receiver_bank_instance_equals_the_oracle)
    mix = params_of(test_gpu_every_mixer_bank_instance_equals_the_oracle)
    assert len(rx) == len(set(rx)) == 56 and len(mix) == len(set(mix)) == 42
    assert set(rx) == {(u[0], n, f) for u in rx_units for n in stages for f in FORMS}
    assert set(mix) == {(c[0].lower(), n, f) for c in cases for n in stages for f in FORMS}


def test_the_job_lengths_are_the_edges_of_a_one_pass_span():
    assert sum(MIX_LENGTHS) < 10000 and sum(DECIM_MS) << K < 30000
    assert [RXB.spans_of([n]) for n in RX_LENGTHS] == [0, 1, 1, 1, 1, 2, 3, 4]
    assert max(MIXB.spans_of(n, 1) for n in MIX_LENGTHS) == 3
    assert rx_spans([2049 << K], K) >= 3 and MIXB.spans_of(2049 << K, 1) >= 3
    for k in range(1, 9):                   # the sweeps' largest job
        assert rx_spans([SWEEP_MS[-1] << k], k) >= 2
    assert rx_spans([SWEEP_MS[-1] << 8], 8) == -(-(1025 << 8) // 768) >= 3
    assert sum(SWEEP_MS) << 8 < 600000


# ---------------------------------------------------------------- GPU: every instance

@pytest.mark.gpu
@pytest.mark.parametrize("unit,stages,form", RX_CASES, ids=case_id)
def test_gpu_every_receiver_bank_instance_equals_the_oracle(unit, stages, form, monkeypatch):
    """fm_rxbank_xydir<LJ, N, IO> and its decimating twin (k = 3) for every N
    of every unit: the bank's own grid, then two blocks walking the spans of
    several jobs in sequence"""
    import torch
    set_knobs(monkeypatch, CORDIC_FMRXB_PASSES="1")
    c16 = unit == "c16"
    with registered(unit, stages) as (name, i16):
        seed = 300 + stages
        if form == "plain":
            run_rx_plain(torch, name, i16, c16, RX_LENGTHS, seed, monkeypatch)
        else:
            run_rx_decim(torch, name, i16, c16, K, DECIM_MS, seed, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("unit,stages,form", MIX_CASES, ids=case_id)
def test_gpu_every_mixer_bank_instance_equals_the_oracle(unit, stages, form, monkeypatch):
    """fm_mixbank_xydir<LJ, N, IO> and fm_mixbank_decim_xydir (k = 3) for every
    N of every unit, as the receivers above"""
    import torch
    set_knobs(monkeypatch, CORDIC_FMXB_PASSES="1")
    with registered(unit, stages) as (name, i16):
        seed = 500 + stages
        if form == "plain":
            run_mix_plain(torch, name, i16, MIX_LENGTHS, seed, monkeypatch)
        else:
            run_mix_decim(torch, name, i16, K, DECIM_MS, seed, monkeypatch)


# ---------------------------------------------------------------- GPU: every k

@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 9))
@pytest.mark.parametrize("bank", ["cfg2-cfg3", "cfg1-io16", "cfg1-io16 c16"])
def test_gpu_every_k_of_the_receiver_banks_equals_the_oracle(bank, k, monkeypatch):
    """the halo of a span is max(4, 2^k) input samples: one lane up to k = 2,
    two at k = 3, all of wave 0 at k = 8, where it lies between two neighbours"""
    import torch
    set_knobs(monkeypatch, CORDIC_FMRXB_PASSES="1")
    name, c16 = bank.split()[0], bank.endswith("c16")
    most = run_rx_decim(torch, name, name in RX16.PAIRS, c16, k, SWEEP_MS, 700 + k,
                        monkeypatch, twice=False)
    assert most >= (3 if k == 8 else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 9))
@pytest.mark.parametrize("name,i16", [("cfg2", False), ("nat16", True)])
def test_gpu_every_k_of_the_mixer_banks_equals_the_oracle(name, i16, k, monkeypatch):
    import torch
    set_knobs(monkeypatch, CORDIC_FMXB_PASSES="1")
    most = run_mix_decim(torch, name, i16, k, SWEEP_MS, 800, monkeypatch, twice=False)
    assert most >= (3 if k >= 2 else 2)
