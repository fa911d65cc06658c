"""CPU-side expected values for the sine cores' acceptance statistics
(bench/cpp/quadtbl_tb.cpp:146-179) and their spectra, from the oracle's
outputs plus numpy.  Used by test_sine_quality.py, test_sfdr.py and
test_tools_sine.py."""
import numpy as np

import oracle_lib as O


def nco_phases(pw, n, phase0, fcw, index0, lead=0):
    """p_i = phase0 + (index0 + i) * fcw (+ lead) mod 2^PW"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(index0 % (1 << 64))
    with np.errstate(over="ignore"):
        p = np.uint64(phase0) + i * np.uint64(fcw) + np.uint64(lead)
    return (p & np.uint64((1 << pw) - 1)).astype(np.uint32)


def sine_err(pw, ow, phase, out):
    """err = |sin(2 pi p / 2^PW) * (2^(OW-1) - 1) - o| per sample, in fp64 as
    the bench computes it (:155-163).  The sine itself is taken in extended
    precision and rounded once: the multiple of 2 pi / 2^PW is then accurate
    to the last place of the double, as the library's sinpi is (plain
    np.sin(p * (2 pi / 2^PW)) loses ~3e-16 * p / 2^PW * 2 pi in the argument,
    which at OW = 24 is 1e-8 output units)."""
    two_pi = np.longdouble(4) * np.arctan2(np.longdouble(1), np.longdouble(0))
    x = phase.astype(np.longdouble) * two_pi / np.longdouble(2 ** pw)
    s = np.sin(x).astype(np.float64)
    return np.abs(s * float((1 << (ow - 1)) - 1) - out.astype(np.float64))


def expected(pw, ow, phase, out):
    e = sine_err(pw, ow, phase, out)
    return dict(err=e, max_err=float(e.max()), max_val=max(0, int(out.max())),
                min_val=min(0, int(out.min())))


def sine_spectrum_input(s):
    """quadtbl_tb.cpp:194-197: outpt[k] = (s[(k + N/4) & (N-1)], s[k])"""
    n = s.size
    k = np.arange(n)
    return s[(k + n // 4) & (n - 1)].astype(np.float64) + 1j * s.astype(np.float64)


def spur(f):
    """|X|^2 of a spectrum -> (master, spur maximum) as cordic_tb.cpp:357-366"""
    p = np.abs(f) ** 2
    return p[1], max(p[0], p[2:].max()) if p.size > 2 else p[0]


class QuadCore:
    def __init__(self, ca, args):
        self.h = ca.Quad(*args)
        self.q = O.quad_cli(*args)
        self.t = O.quad_tables(self.q)
        self.pw, self.ow = self.h.pw, self.h.ow

    def oracle(self, ph):
        return O.quad_lookup(self.q, self.t, ph)

    def quality(self, ca):
        return ca.Quality.for_quad(self.h)


class TableCore:
    def __init__(self, ca, kind, ow, pw):
        self.h = ca.Table(kind, -1, ow, pw)
        self.kind, self.pw, self.ow = kind, self.h.pw, self.h.ow
        self.tbl = O.table_values(kind, self.pw, self.ow)

    def oracle(self, ph):
        return O.table_lookup(self.kind, self.pw, self.ow, self.tbl, ph)

    def quality(self, ca):
        return ca.Quality.for_table(self.h)
