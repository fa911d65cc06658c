#!/usr/bin/env python3
"""Regenerate tests/golden/checked_in_rtl_vectors.json: what tests/vsim.py
computes when it EXECUTES the reference's checked-in rtl/{cordic,topolar,
seqcordic,seqpolar}.v on the seeded inputs of
tests/test_rtl_vectors.py::test_checked_in_rtl_executed_by_vsim_equals_oracle.
Only data is stored (the cores' IW / WW / PW and their output columns; the
inputs are regenerated from the seed); no Verilog text.

Run:  python tests/golden/make_checked_in_rtl_vectors.py
      (needs the reference tree: REF_RTL of tests/test_rtl_vectors.py)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_rtl_vectors as T  # noqa: E402


def main():
    if not os.path.isdir(T.REF_RTL):
        sys.exit("the reference's rtl/ tree is not mounted")
    out = {}
    for core, mode, cpo in T.CHECKED_IN_CORES:
        params, cols = T.run_checked_in(core, mode, cpo)
        out[core] = {"params": params, "cycles_per_output": cpo, "out": cols}
    path = os.path.join(HERE, "checked_in_rtl_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
