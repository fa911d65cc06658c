"""FM mixer banks on interleaved int16 I/Q, in and out
(cordic_mixbank_create_c16, cordic_mixbank_create_decim_c16;
include/cordic_amd.h): every output short and every d_acc word against the
single *_c16 calls and against the oracle on (iq[0::2], iq[1::2]).  Nothing has
a tolerance.  Every job's iq and oiq lie 1, 2 or 3 complex samples off the
16-byte grid, the two at different offsets, between sentinels; the inputs are
read back unchanged after every run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cordic_amd as ca
import test_fm_mix as MIX
import test_fm_mix16 as MIX16
import test_fm_mix_decim as MIXD
from test_fm_demod import Padded, last_value, last_word
from test_fm_mix_c16 import data, interleave, run, want
from test_fm_rx_c16 import replay_three_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED, ONE_BY_ONE = "cfg1", "n9"
KNOBS = MIX16.KNOBS + ("CORDIC_FMX_MAX_BLOCKS", "CORDIC_FMXD_FALLBACK")
SENT_W = 0x5a5a5a5a


def clear(monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)


class Spec:
    """jobs of `ms` << k complex samples: some without d_pm, some without d_acc"""

    def __init__(self, name, ms, k, seed, all_acc=False):
        rng = np.random.default_rng(seed)
        self.name, self.k, self.ns = name, k, [m << k for m in ms]
        J = len(self.ns)
        self.has_pm = [bool(j % 3) for j in range(J)]
        self.has_acc = [all_acc or bool((j + 1) % 4) for j in range(J)]
        self.phase0 = [int(v) for v in rng.integers(0, 1 << 32, J)]
        self.acc0 = [int(v) | 0x80000000 for v in rng.integers(0, 1 << 32, J)]
        self.renew(seed)

    def renew(self, seed):
        self.fcw, self.pm, self.x, self.y = [], [], [], []
        for j, n in enumerate(self.ns):
            f, p, x, y = data(self.name, n, 1000 * seed + 10 * j, self.has_pm[j])
            self.fcw.append(f); self.pm.append(p); self.x.append(x); self.y.append(y)

    def expected(self, acc=None, phase0=None):
        """the oracle's (ox, oy, *d_acc or None) per job; acc: the words in front
        (None: the presets)"""
        out = []
        for j, n in enumerate(self.ns):
            a0 = (self.acc0[j] if acc is None else acc[j]) if self.has_acc[j] else 0
            p0 = self.phase0[j] if phase0 is None else phase0
            if n:
                wx, wy, final = want(self.name, self.k, self.fcw[j], self.pm[j], self.x[j],
                                     self.y[j], p0, a0)
            else:
                wx, wy, final = np.zeros(0, np.int16), np.zeros(0, np.int16), a0
            out.append((wx, wy, final if self.has_acc[j] else None))
        return out


class IqBank:
    """the jobs of a Spec on the device -- job j's iq 1 + j % 3 complex samples off
    the grid, its oiq 1 + (j + 1) % 3 -- and the interleaved bank over them"""

    def __init__(self, torch, plan, spec, create=True):
        from gpu_util import DEV
        self.torch, self.plan, self.spec = torch, plan, spec
        J = max(1, len(spec.ns))
        self.words = torch.full((4 * J,), SENT_W, dtype=torch.int32, device=DEV)
        self.arr = []
        for j, n in enumerate(spec.ns):
            c = 1 + j % 3
            self.arr.append(dict(fcw=Padded(torch, n, 1 + j % 4), pm=Padded(torch, n, 3),
                                 iq=Padded(torch, 2 * n, 2 * c, True),
                                 oiq=Padded(torch, 2 * (n >> spec.k), 2 * (1 + c % 3), True)))
        self.upload()
        self.preset()
        self.bank = ca.MixBankC16(plan, self.jobs(), spec.k) if create else None

    def acc(self, j):
        return self.words[4 * j:] if self.spec.has_acc[j] else None

    def preset(self):
        h = np.full(self.words.numel(), SENT_W, dtype=np.uint32)
        for j in range(len(self.spec.ns)):
            h[4 * j] = self.spec.acc0[j]
        self.words.copy_(self.torch.from_numpy(h.view(np.int32)).to(self.words.device))

    def jobs(self):
        s = self.spec
        return [(a["fcw"].view, a["pm"].view if s.has_pm[j] else None, a["iq"].view,
                 a["oiq"].view, s.ns[j], s.phase0[j], self.acc(j))
                for j, a in enumerate(self.arr)]

    def upload(self):
        s, t = self.spec, self.torch
        def put(p, v, dt):
            if p.n:
                p.t[p.off:p.off + p.n].copy_(
                    t.from_numpy(np.ascontiguousarray(v).astype(dt)).to(p.t.device))
        for j, a in enumerate(self.arr):
            put(a["fcw"], s.fcw[j].view(np.int32), np.int32)
            if s.has_pm[j]:
                put(a["pm"], s.pm[j].view(np.int32), np.int32)
            put(a["iq"], interleave(s.x[j], s.y[j]), np.int16)

    def clear_outputs(self):
        for a in self.arr:
            a["oiq"].t.fill_(a["oiq"].sent)

    def outputs_untouched(self):
        return all(a["oiq"].untouched() for a in self.arr)

    def results(self):
        """per job (ox, oy, *d_acc or None), after checking the sentinels, the
        inputs and the words nobody may write"""
        self.torch.cuda.synchronize()
        s = self.spec
        h = self.words.cpu().numpy().view(np.uint32)
        out = []
        for j, a in enumerate(self.arr):
            assert np.array_equal(a["fcw"].get(), s.fcw[j].view(np.int32))
            assert np.array_equal(a["iq"].get(), interleave(s.x[j], s.y[j]))
            if s.has_pm[j]:
                assert np.array_equal(a["pm"].get(), s.pm[j].view(np.int32))
            else:
                assert a["pm"].untouched()
            w = h[4 * j:4 * j + 4]
            assert (w[1:] == SENT_W).all()
            if not s.has_acc[j]:
                assert w[0] == s.acc0[j]
            got = a["oiq"].get()
            out.append((got[0::2].copy(), got[1::2].copy(),
                        int(w[0]) if s.has_acc[j] else None))
        return out

    def single_calls(self):
        """the same jobs through cordic_plan_fm_mix_c16 / _decim_c16, one call each
        on buffers of their own"""
        t, s, out = self.torch, self.spec, []
        for j, n in enumerate(s.ns):
            acc = last_word(t, s.acc0[j]) if s.has_acc[j] else None
            if n:
                gx, gy = run(t, self.plan, s.k or None, s.fcw[j], s.pm[j], s.x[j], s.y[j],
                             s.phase0[j], acc, c=1 + (j + 1) % 3)
            else:
                gx, gy = np.zeros(0, np.int16), np.zeros(0, np.int16)
            out.append((gx, gy, None if acc is None else last_value(acc)))
        return out


def assert_equals(got, wanted, tag):
    assert len(got) == len(wanted)
    for j, ((gx, gy, ga), (wx, wy, wa)) in enumerate(zip(got, wanted)):
        assert np.array_equal(gx, wx) and np.array_equal(gy, wy), (tag, j, gx.size)
        assert ga == wa, (tag, j, gx.size)


def twin_info(torch, plan, spec):
    """cordic_mixbank_info of the *16 bank over split arrays of the same lengths"""
    from gpu_util import DEV
    z = lambda n, dt: torch.zeros(max(1, n), dtype=dt, device=DEV)
    jobs = [(z(n, torch.int32), None, z(n, torch.int16), z(n, torch.int16),
             z(n >> spec.k, torch.int16), z(n >> spec.k, torch.int16), n, 0, None)
            for n in spec.ns]
    bank = ca.MixBank16(plan, jobs, spec.k or None)
    info = bank.info()
    bank.close()
    return info


# ---------------------------------------------------------------- ragged banks

@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("name", [FUSED, ONE_BY_ONE])
def test_gpu_a_ragged_bank_run_twice_equals_the_single_calls_and_the_oracle(name, k,
                                                                            monkeypatch):
    import torch
    clear(monkeypatch)
    plan = ca.Plan(MIXD.core(name, True))
    spec = Spec(name, MIX16.BANK_LENGTHS, k, 11 + k)
    assert 0 in spec.ns and 0 < sum(spec.has_pm) < len(spec.ns) > sum(spec.has_acc) > 0
    d = IqBank(torch, plan, spec)
    info = d.bank.info()
    fused = name == FUSED
    assert info["samples"] == sum(spec.ns) and info["fused"] == fused
    assert info == twin_info(torch, plan, spec)         # samples, spans, fused, tile
    if fused:
        p = info["tile"] // 1024
        assert info["tile"] == p * 1024 and p >= 1 and p & (p - 1) == 0
        assert info["spans"] == sum(MIX16.spans_of(n, p) for n in spec.ns)
    else:
        assert (info["tile"], info["spans"]) == (0, 0)
    acc = None
    for r in range(2):              # the second, on new data, continues every d_acc
        if r:
            spec.renew(500 + k)
            d.upload()
            d.clear_outputs()
        wanted = spec.expected(acc)
        d.bank.run()
        got = d.results()
        assert_equals(got, wanted, (name, k, r, "oracle"))
        if r == 0:
            assert_equals(got, d.single_calls(), (name, k, "single calls"))
        acc = [w[2] for w in wanted]
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [dict(CORDIC_FMXB_PASSES="1"),
                                   dict(CORDIC_FMXB_PASSES="1", CORDIC_FMXB_MAX_SPANS="2"),
                                   dict(CORDIC_FMXB_MAX_BLOCKS="2")])
@pytest.mark.parametrize("k", [0, 3])
def test_gpu_forced_spans_span_caps_and_grid_caps_give_the_same_bits(k, knobs, monkeypatch):
    import torch
    clear(monkeypatch)
    for key, v in knobs.items():
        monkeypatch.setenv(key, v)
    plan = ca.Plan(MIXD.core(FUSED, True))
    ms = [5 * 1024 + 7, 1, 9001, 1024, 0, 2049]
    if k:
        ms = [641, 1, 1126, 128, 0, 257]        # (<< 3: 5128, 8, 9008, 1024, 0, 2056)
    spec = Spec(FUSED, ms, k, 23)
    d = IqBank(torch, plan, spec)
    info = d.bank.info()
    assert info["fused"] == 1
    if "CORDIC_FMXB_PASSES" in knobs:
        cap = int(knobs.get("CORDIC_FMXB_MAX_SPANS", 4096))
        assert info["tile"] == 1024
        assert info["spans"] == sum(MIX16.spans_of(n, 1, cap) for n in spec.ns)
    d.bank.run()
    assert_equals(d.results(), spec.expected(), (k, knobs))
    d.bank.close()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stages", MIX.INSTANCES)
def test_gpu_every_instance_of_the_two_bank_kernels_equals_the_oracle(stages, monkeypatch):
    """fm_mixbank_xydir<30, N, IoC16io> (k = 0) and fm_mixbank_decim_xydir<30, N,
    IoC16io> (k = 3) for all 7 N: 16-bit ports with 15 extra bits (WW 32), jobs of
    2049 and 1024 samples"""
    import torch
    clear(monkeypatch)
    name = "mixbc16_%d" % stages
    MIX16.CORES16[name] = ((ca.P2R, 16, 16, 15, 32, stages), 0)
    try:
        cfg = MIXD.core(name, True)
        assert cfg.ww == 32 and cfg.nlive == stages
        plan = ca.Plan(cfg)
        assert plan.fm_mix_c16_info() == (1, 1024)
        for k in (0, 3):
            # (k = 3: whole groups of 8 -- 2056 and 1024)
            spec = Spec(name, [257, 128] if k else [2049, 1024], k, 600 + stages, all_acc=True)
            assert spec.ns == ([2056, 1024] if k else [2049, 1024])
            d = IqBank(torch, plan, spec)
            assert d.bank.info()["fused"] == 1
            d.bank.run()
            assert_equals(d.results(), spec.expected(), (stages, k))
            d.bank.close()
        plan.close()
    finally:
        del MIX16.CORES16[name]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 3])
def test_gpu_a_captured_run_replayed_three_times_continues_three_times(k, monkeypatch):
    """the same capture buffer every replay: replay r starts from the words that
    replay r - 1 left.  Two kernel nodes with one edge between them"""
    import torch
    clear(monkeypatch)
    plan = ca.Plan(MIXD.core(FUSED, True))
    spec = Spec(FUSED, [2049, 3, 1021, 0], k, 37, all_acc=True)
    d = IqBank(torch, plan, spec)
    warm = IqBank(torch, plan, spec)            # once outside the capture first
    warm.bank.run()
    torch.cuda.synchronize()
    warm.bank.close()
    wants, acc = [], None
    for r in range(3):      # (phase0 is added by every run)
        wants.append(spec.expected(acc))
        acc = [w[2] for w in wants[-1]]
    o0 = d.arr[0]["oiq"]
    w0 = np.concatenate([interleave(w[0][0], w[0][1]) for w in wants])
    replay_three_times(torch, lambda s: d.bank.run(stream=s), o0, o0, True, w0, w0,
                       2 * (spec.ns[0] >> k), k)
    assert_equals(d.results(), wants[2], ("after three replays", k))
    d.bank.close()
    plan.close()


# ---------------------------------------------------------------- create's refusals

@pytest.mark.gpu
@pytest.mark.parametrize("name", [FUSED, ONE_BY_ONE])
def test_gpu_create_refuses_overlaps_and_bad_jobs_with_nothing_written(name, monkeypatch):
    """a job's d_iq is 4 n bytes and its d_oiq 4 (n >> k): an output of ANOTHER job
    on the last short of either is an overlap"""
    import torch
    from cordic_amd import _native
    clear(monkeypatch)
    n = 1024
    spec = Spec(name, [n, n], 0, 71, all_acc=True)
    plan = ca.Plan(MIXD.core(name, True))
    d = IqBank(torch, plan, spec, create=False)
    base = d.jobs()
    KEYS = ("fcw", "pm", "iq", "oiq", "n", "phase0", "acc")
    iq0, oiq0 = base[0][2].data_ptr(), base[0][3].data_ptr()
    L = ca.lib()

    def create(k, j, reserved=0, plan_h=None, **kw):
        """job j with the fields of kw replaced (addresses or tensors)"""
        arr = (_native._CFmMixJobC16 * 2)()
        for i, jb in enumerate(base):
            f = dict(zip(KEYS, jb))
            if i == j:
                f.update(kw)
            ptr = lambda v: v if isinstance(v, (int, type(None))) else v.data_ptr()
            arr[i].d_fcw, arr[i].d_pm = ptr(f["fcw"]), ptr(f["pm"])
            arr[i].d_iq, arr[i].d_oiq, arr[i].d_acc = ptr(f["iq"]), ptr(f["oiq"]), ptr(f["acc"])
            arr[i].n, arr[i].phase0 = f["n"], f["phase0"]
            arr[i].reserved = reserved if i == j else 0
        h = C.c_void_p()
        ph = plan._h if plan_h is None else plan_h
        if k is None:
            rc = L.cordic_mixbank_create_c16(ph, 2, arr, C.byref(h))
        else:
            rc = L.cordic_mixbank_create_decim_c16(ph, k, 2, arr, C.byref(h))
        if rc == 0:
            L.cordic_mixbank_destroy(h)
        else:
            assert not h.value
        return rc

    bad = [dict(oiq=iq0), dict(oiq=iq0 + 4 * n - 4),        # job 0's d_iq: first, last short
           dict(oiq=iq0 + 2 * n), dict(acc=iq0 + 2 * n + 8),        # ... its second half
           dict(acc=iq0 + 4 * n - 4), dict(acc=iq0 + 8),
           dict(acc=oiq0), dict(acc=base[0][6]),                    # a shared d_acc
           dict(iq=base[1][2].data_ptr() + 2), dict(oiq=base[1][3].data_ptr() + 2),
           dict(iq=base[1][2].data_ptr() + 1), dict(iq=None), dict(oiq=None),
           dict(oiq=base[1][2]), dict(oiq=base[0][0])]
    for k in (None, 0, 3):
        assert create(k, 1) == 0
        for kw in bad:
            assert create(k, 1, **kw) == ca.ERR_ARGS, (k, sorted(kw))
        assert create(k, 1, reserved=1) == ca.ERR_ARGS
    # job 0's d_oiq is 4 (n >> k) bytes: its last short, and one short behind it
    for k, sh in ((None, 0), (3, 3), (8, 8)):
        end = oiq0 + 4 * (n >> sh)
        assert create(k, 1, oiq=end - 4) == ca.ERR_ARGS, k
        assert create(k, 1, acc=end - 4) == ca.ERR_ARGS, k
        assert create(k, 1, acc=end) == 0, k
    assert create(8, 1, oiq=iq0 + 4 * n) == 0               # tight behind job 0's d_iq
    assert create(3, 1, n=n + 4) == ca.ERR_ARGS             # n % R != 0
    assert create(9, 1) == ca.ERR_ARGS
    assert create(2, 1, n=n + 4) == 0
    wide = ca.Plan(MIX.both("ww38")[0])                     # an int32 plan
    for k in (None, 3):
        assert create(k, 1, plan_h=wide._h) == ca.ERR_CONTAINER
    wide.close()
    torch.cuda.synchronize()
    assert d.outputs_untouched()
    # and the same jobs make a bank that runs clean
    d.bank = ca.MixBankC16(plan, base)
    d.bank.run()
    assert_equals(d.results(), spec.expected(), name)
    d.bank.close()
    plan.close()


@pytest.mark.gpu
def test_gpu_the_example_builds_and_finds_no_difference(tmp_path):
    """examples/ddc_c16.c: one interleaved capture buffer of 256 channels x 1536
    complex samples through ONE decimating mixer bank at k = 3 for three rounds,
    against cordic_plan_fm_mix_decim16 per channel on arrays split on the host"""
    exe = tmp_path / "ddc_c16"
    r = subprocess.run(
        ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
         "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
         "-D__HIP_PLATFORM_AMD__", "-D_GNU_SOURCE", "-o", str(exe),
         os.path.join(ROOT, "examples", "ddc_c16.c"),
         "-L", os.path.join(ROOT, "cordic_amd"), "-lcordic_amd", "-L", "/opt/rocm/lib",
         "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "cordic_amd"),
         "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "256 channels" in r.stdout and "x 3 rounds" in r.stdout
    assert "0 shorts and words differ" in r.stdout and "fused, two launches" in r.stdout
