#!/usr/bin/env python3
"""Record tests/golden/wg_t4_tail_bits.json: the bits of x after 25 iterations of the 4-slice workgroup-resident CG kernel (ELPH_WG_T=4) on 3 right-hand sides of the 16 x 16 Holstein lattice at 32, 64 and 96 time slices (teams of one, two and three workgroups; tests/wg_t4_tail_cases.py), from x0 = 0 and from the non-zero guess (SHA-256 of the bytes and a dozen sampled values as hex floats). Run it on the GPU at the commit whose bits are the reference, BEFORE csrc/cg_wg.hip is changed; tests/test_gpu_wg_t4_tail.py compares later builds with it.
usage: python3 tools/record_wg_t4_tail_bits.py [output.json]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["ELPH_WG_T"] = "4"
for k in ("ELPH_NO_WG", "ELPH_WG_NO_DPP", "ELPH_WG_W", "ELPH_WG_ALWAYS"):
    os.environ.pop(k, None)

import wg_t4_tail_cases as cases                            # noqa: E402
from elphdynamics_amd import _lib, build, configs          # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "wg_t4_tail_bits.json")
rec = {"lattice": "16 x 16 Holstein, the parameters of config C", "ELPH_WG_T": 4, "nrhs": cases.NRHS, "iterations": cases.ITERS,
       "library_sources": build.library_source_hash(_lib.library_path()), "shapes": {}}
for ltau, shape in cases.SHAPES.items():
    m = cases.model(ltau)
    assert cases.wg_shape(m, cases.NRHS) == shape and cases.wg_shape(m, 1) == shape, (ltau, cases.wg_shape(m, cases.NRHS), cases.wg_shape(m, 1))
    _, B = configs.rhs(m, cases.NRHS)
    rec["shapes"][str(ltau)] = dict(cases.fixed_iteration_digests(m, B, cases.guess(m.Ndim, cases.NRHS)), TWG=list(shape[1:]))
    m.close()
with open(out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec, indent=1))
