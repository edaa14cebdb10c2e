#!/usr/bin/env python3
"""Record tests/golden/wg_t4_bits.json: the bits of x after 25 iterations of the 4-slice workgroup-resident CG kernel (ELPH_WG_T=4) on 3 right-hand sides of config C, from x0 = 0 and from the non-zero guess of tests/wg_t4_chain_cases.py (SHA-256 of the bytes and a dozen sampled values as hex floats). Run it on the GPU at the commit whose bits are the reference, BEFORE csrc/cg_wg.hip is changed; tests/test_gpu_wg_t4_chain.py compares later builds with it.
usage: python3 tools/record_wg_t4_bits.py [output.json]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["ELPH_WG_T"] = "4"
for k in ("ELPH_NO_WG", "ELPH_WG_NO_DPP", "ELPH_WG_W"):
    os.environ.pop(k, None)

import wg_t4_chain_cases as cases                           # noqa: E402
from elphdynamics_amd import _lib, build, configs          # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "wg_t4_bits.json")
m = configs.make_model("C", tol=1e-5)
assert cases.wg_shape(m, cases.NRHS)[:2] == (1, 4) and cases.wg_shape(m, 1)[:2] == (1, 4), "ELPH_WG_T=4 does not select the 4-slice shape"
_, B = configs.rhs(m, cases.NRHS)
rec = {"config": "C", "ELPH_WG_T": 4, "nrhs": cases.NRHS, "iterations": cases.ITERS, "library_sources": build.library_source_hash(_lib.library_path()),
       "x0_zero": cases.digest(cases.fixed_iterations_from_zero(m, B)),
       "x0_guess": cases.digest(cases.fixed_iterations_from_guess(m, B, cases.guess(m.Ndim, cases.NRHS)))}
assert cases.wg_fallbacks(m) == (0, 0), "a resident launch gave up: these are not the resident kernel's bits"
m.close()
with open(out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec, indent=1))
