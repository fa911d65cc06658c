"""The C boundary of the data-fed calls on 16-bit sample arrays
(include/cordic_amd.h "16-bit sample containers": cordic_mix16,
cordic_plan_mix16, cordic_plan_p2r16, cordic_job16, cordic_jobset_create16) as
far as it can be checked without a GPU: struct layout, the container rule and
the argument checks, all of which answer before anything is launched."""
import ctypes as C
import os
import subprocess

import cordic_amd as ca
import cordic_amd._native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["d_phase", "phase0", "fcw", "index0", "d_oxval", "d_oyval", "n",
          "d_xval", "d_yval"]


def test_cordic_job16_has_the_layout_of_cordic_job(tmp_path):
    body = ['#include <stddef.h>', '#include <stdio.h>', '#include "cordic_amd.h"',
            'int main(void) {']
    for s in ("cordic_job", "cordic_job16"):
        body.append('printf("%s size %%zu\\n", sizeof(%s));' % (s, s))
        for f in FIELDS:
            body.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    body.append('return 0; }')
    src = tmp_path / "layout16.c"
    src.write_text("\n".join(body) + "\n")
    exe = tmp_path / "layout16"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout
    got = {}
    for ln in out.splitlines():
        a, b, c = ln.split()
        got[(a, b)] = int(c)
    assert got[("cordic_job16", "size")] == got[("cordic_job", "size")]
    assert C.sizeof(N._CJob16) == got[("cordic_job16", "size")]
    for f in FIELDS:
        assert got[("cordic_job16", f)] == got[("cordic_job", f)], f
        assert getattr(N._CJob16, f).offset == got[("cordic_job16", f)], f


def test_the_pointers_of_cordic_job16_are_16_bit_ones(tmp_path):
    """a caller's int16_t / uint16_t arrays go in without a cast (and int32_t
    ones do not: -Werror=incompatible-pointer-types)"""
    ok = ('#include "cordic_amd.h"\n'
          'int main(void) { int16_t a[4] = {0}; uint16_t p[4] = {0}; cordic_job16 j;\n'
          'j.d_phase = p; j.phase0 = 0; j.fcw = 0; j.index0 = 0; j.d_oxval = a;\n'
          'j.d_oyval = a; j.n = 4; j.d_xval = a; j.d_yval = a; return (int)j.n - 4; }\n')
    bad = ok.replace("int16_t a[4]", "int32_t a[4]")
    for text, want in ((ok, True), (bad, False)):
        src = tmp_path / "p.c"
        src.write_text(text)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic",
                            "-Werror", "-I", os.path.join(ROOT, "include"),
                            "-fsyntax-only", str(src)], capture_output=True, text=True)
        assert (r.returncode == 0) == want, r.stderr


def test_container_rule_of_the_mixer_answers_before_any_launch():
    f = ca.lib().cordic_mix16
    for iw, ow in ((17, 16), (16, 17), (17, 17)):
        cfg = ca.Config.from_cli(ca.P2R, iw, ow, 2, 16, 16)
        # (the arrays are never touched: the refusal comes first)
        assert f(cfg.ref, 16, 0, 1, 0, 8, 8, 8, 8, None) == ca.ERR_CONTAINER, (iw, ow)


def test_null_handles_are_refused():
    lib = ca.lib()
    assert lib.cordic_mix16(None, 16, 0, 1, 0, 8, 8, 8, 8, None) == ca.ERR_ARGS
    assert lib.cordic_plan_mix16(None, 16, 0, 1, 0, 8, 8, 8, 8, None) == ca.ERR_ARGS
    assert lib.cordic_plan_p2r16(None, 16, 8, 8, 8, 8, 8, None) == ca.ERR_ARGS
    h = C.c_void_p()
    jobs = (N._CJob16 * 1)()
    assert lib.cordic_jobset_create16(None, ca.JOBS_MIX, 1, jobs, C.byref(h)) == ca.ERR_ARGS
    assert not h.value
