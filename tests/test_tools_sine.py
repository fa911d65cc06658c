"""tools/cordic_tb on the sine-producing cores: bench/cpp/quadtbl_tb.cpp's
report from device statistics (cordic_quality_sine*) and a device FFT
(cordic_sfdr_*), the full sweep of --all-phases, and the plain tables."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import sine_quality as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB = os.path.join(ROOT, "tools", "cordic_tb")


def run_tb(*args):
    r = subprocess.run([TB] + list(args), capture_output=True, text=True,
                       timeout=300)
    print(r.stdout + r.stderr)
    return r


def three_lines(out):
    return [re.search(p, out).group(0) for p in
            (r"MXERR: [\d.]+ \(.*\)", r"MXVAL: 0x[0-9a-f]{8}",
             r"MNVAL: 0x[0-9a-f]{8}")]


def test_all_phases_is_the_default_grid_up_to_pw_26():
    a = run_tb("-t", "qtbl", "-o", "13", "-p", "18")
    # (in passes of 2^16, so that the sweep is fed in pieces)
    b = run_tb("-t", "qtbl", "-o", "13", "-p", "18", "--all-phases",
               "--lgchunk", "16")
    assert a.returncode == 0 and b.returncode == 0
    assert "SUCCESS!!" in a.stdout and "SUCCESS!!" in b.stdout
    assert three_lines(a.stdout) == three_lines(b.stdout)
    assert "cordic_quad_nco" in b.stdout and "cordic_quad_nco" not in a.stdout
    sa, sb = (float(re.search(r"SFDR = +([\d.]+)", r.stdout).group(1))
              for r in (a, b))
    assert sa == sb


def test_quarter_wave_table_report():
    r = run_tb("-t", "qtr", "-o", "16", "-p", "12")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "SUCCESS!!" in r.stdout
    mx = float(re.search(r"MXERR: ([\d.]+) \(no reference threshold\)",
                         r.stdout).group(1))
    ph = np.arange(1 << 12, dtype=np.uint32)
    out = O.table_lookup(O.QTR, 12, 16, O.table_values(O.QTR, 12, 16), ph)
    want = S.expected(12, 16, ph, out)
    assert abs(mx - want["max_err"]) < 1e-5
    assert "MXVAL: 0x%08x" % want["max_val"] in r.stdout
    assert "MNVAL: 0x%08x" % (want["min_val"] & 0xffffffff) in r.stdout
    assert re.search(r"SFDR = +[\d.]+ dBc", r.stdout)


def test_a_2_to_the_26_point_sweep_now_has_an_sfdr_line():
    """the reference (and this bench before cordic_sfdr) skips the spectrum
    at PW >= 26; the largest case of the suite"""
    r = run_tb("-t", "qtbl", "-o", "16", "-p", "26")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Too many phase bits" not in r.stdout
    assert re.search(r"SFDR = +[\d.]+ dBc", r.stdout)
    assert "SUCCESS!!" in r.stdout
