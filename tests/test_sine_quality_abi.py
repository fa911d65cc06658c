"""The C boundary of the sine cores' device statistics and of cordic_sfdr
(include/cordic_amd.h: cordic_quality_create_quad / _table, cordic_quality_sine*,
cordic_sfdr_*) as far as it can be checked without a GPU: exported symbols,
struct layout against the ctypes view, the 16-bit pointer types and the
argument checks that answer before the device is touched."""
import ctypes as C
import os
import subprocess

import cordic_amd as ca
import cordic_amd._native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cordic_quality_create_quad", "cordic_quality_create_table",
         "cordic_quality_sine", "cordic_quality_sine16",
         "cordic_quality_sine_nco", "cordic_quality_sine_nco16",
         "cordic_quality_sine_result", "cordic_sfdr_create",
         "cordic_sfdr_destroy", "cordic_sfdr_load_iq", "cordic_sfdr_load_sine",
         "cordic_sfdr_run", "cordic_sfdr_bins"]
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
       "-I", os.path.join(ROOT, "include")]


def test_the_new_symbols_resolve_and_are_in_the_signature_table():
    L = ca.lib()
    for name in NAMES:
        getattr(L, name)                    # AttributeError: not exported
        assert name in N.ABI, name
    assert L.cordic_abi_version() == 1


def test_result_structs_have_the_headers_layout(tmp_path):
    pairs = [("cordic_sine_quality", N._CSineQuality),
             ("cordic_sfdr_result", N._CSfdrResult)]
    body = ['#include <stddef.h>', '#include <stdio.h>', '#include "cordic_amd.h"',
            'int main(void) {']
    for cname, cls in pairs:
        body.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            body.append('printf("%s %s %%zu\\n", offsetof(%s, %s));'
                        % (cname, f, cname, f))
    body.append('return 0; }')
    src = tmp_path / "layout_sine.c"
    src.write_text("\n".join(body) + "\n")
    exe = tmp_path / "layout_sine"
    r = subprocess.run(GCC + [str(src), "-o", str(exe)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout
    want = {}
    for ln in out.splitlines():
        a, b, c = ln.split()
        want[(a, b)] = int(c)
    for cname, cls in pairs:
        assert C.sizeof(cls) == want[(cname, "size")], cname
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == want[(cname, f)], (cname, f)
    # every field of the header's structs is in the ctypes view: the sizes
    # agree and there is no room for another member
    assert C.sizeof(N._CSineQuality) == 72 and C.sizeof(N._CSfdrResult) == 40


def test_the_pointers_of_the_16_bit_forms_are_16_bit_ones(tmp_path):
    """a caller's int16_t array goes in without a cast (and an int32_t one
    does not: -Werror=incompatible-pointer-types)"""
    ok = ('#include "cordic_amd.h"\n'
          'int main(void) { int16_t a[4] = {0}; uint32_t p[4] = {0};\n'
          'return cordic_quality_sine16(0, 4, p, a, 0)\n'
          '     + cordic_quality_sine_nco16(0, 4, 0u, 1u, 0u, a, 0); }\n')
    bad = ok.replace("int16_t a[4]", "int32_t a[4]")
    for text, want in ((ok, True), (bad, False)):
        src = tmp_path / "p.c"
        src.write_text(text)
        r = subprocess.run(GCC + ["-fsyntax-only", str(src)],
                           capture_output=True, text=True)
        assert (r.returncode == 0) == want, r.stderr


def test_null_handles_and_out_pointers_are_refused():
    L = ca.lib()
    h = C.c_void_p()
    quad = ca.Quad(ow=13, pw=18, device=False)
    tbl = ca.Table(ca.TBL, -1, 12, 10, device=False)
    assert L.cordic_quality_create_quad(None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_quality_create_quad(C.byref(quad.c), None) == ca.ERR_ARGS
    assert L.cordic_quality_create_table(None, C.byref(h)) == ca.ERR_ARGS
    assert L.cordic_quality_create_table(C.byref(tbl.c), None) == ca.ERR_ARGS
    assert not h.value
    # (the arrays are never touched: the refusal comes first)
    assert L.cordic_quality_sine(None, 4, 8, 8, None) == ca.ERR_ARGS
    assert L.cordic_quality_sine16(None, 4, 8, 8, None) == ca.ERR_ARGS
    assert L.cordic_quality_sine_nco(None, 4, 0, 1, 0, 8, None) == ca.ERR_ARGS
    assert L.cordic_quality_sine_nco16(None, 4, 0, 1, 0, 8, None) == ca.ERR_ARGS
    r = N._CSineQuality()
    assert L.cordic_quality_sine_result(None, C.byref(r)) == ca.ERR_ARGS
    s = N._CSfdrResult()
    assert L.cordic_sfdr_load_iq(None, 4, 0, 8, 8, None) == ca.ERR_ARGS
    assert L.cordic_sfdr_load_sine(None, 4, 0, 8, None) == ca.ERR_ARGS
    assert L.cordic_sfdr_run(None, C.byref(s), None) == ca.ERR_ARGS
    assert L.cordic_sfdr_bins(None, 0, 1, 8) == ca.ERR_ARGS
    L.cordic_sfdr_destroy(None)             # a no-op, as the other destroys


def test_sfdr_create_refuses_sizes_outside_1_to_30_before_any_allocation():
    L = ca.lib()
    h = C.c_void_p()
    for lgn in (0, 31, -1, 64):
        assert L.cordic_sfdr_create(lgn, C.byref(h)) == ca.ERR_ARGS, lgn
        assert not h.value
    assert L.cordic_sfdr_create(4, None) == ca.ERR_ARGS
