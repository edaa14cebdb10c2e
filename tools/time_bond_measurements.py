"""Time of one accumulate_bonds_ (BondBond and BondPairGreens, both time-dependent, every pair of the bond definitions) next to one
measurements.accumulate_ with all five on-site correlations, on the same handle and vectors, at a BASELINE config
(`time_bond_measurements.py [tag] [repetitions]`); n_v = 10.  Both calls synchronise before they return; medians after one warm-up."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from elphdynamics_amd import bond_measurements as bm, configs, greens, measurements as ms, synth
tag = sys.argv[1] if len(sys.argv) > 1 else "C"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
nv = 10
m = configs.make_model(tag, tol=1e-5)
est = greens.EstimateGreensFunction(m, nv=nv)
R = np.stack([synth.randn(900 + i, m.Ndim) for i in range(nv)])
X = np.stack([synth.randn(1900 + i, m.Ndim) for i in range(nv)])
greens.set_vectors_(est, R, X)          # the time of the folds does not depend on what the vectors are: no solve here
td = {"measure": True, "time_dependent": True}
onsite = ms.initialize_measurements_container(m, dict({k: td for k in ms.ONSITE_CORR}, num_random_vectors=nv), "")
bonds = bm.initialize_bond_container(m, dict({k: td for k in bm.BOND_CORR}, num_random_vectors=nv), "")
A, B = [], []
for rep in range(reps + 1):             # the first repetition warms up (allocations, first launches) and is not reported
    t0 = time.perf_counter(); ms.accumulate_(onsite, m, est)
    t1 = time.perf_counter(); bm.accumulate_bonds_(bonds, m, est)
    t2 = time.perf_counter()
    ms.reset_measurements_(onsite, m); bm.reset_bond_measurements_(bonds, m)
    if rep:
        A.append(t1 - t0); B.append(t2 - t1)
npairs = nv * (nv - 1) // 2
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731
print(f"{tag}: n_v = {nv} ({npairs} pairs of vectors), {len(m.bond_definitions)} bond definitions, "
      f"{bonds.intersite_corr['BondBond'].pairs.shape[1]} pairs of bonds; medians of {reps} repetitions (ms): "
      f"measurements.accumulate_ (five on-site correlations) {med(A):.2f} [min {1e3*min(A):.2f}]  "
      f"accumulate_bonds_ (BondBond + BondPairGreens) {med(B):.2f} [min {1e3*min(B):.2f}]")
m.close()
