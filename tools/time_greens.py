"""Time of one measurement's Green's-function work at a BASELINE config: update! (n_v solves), setup! over all pairs with the four arrays to
the host (A), the same launches without the copies, and the device route of measurements.py (B): every pair set up and folded into the
device's accumulators (make_measurements_ without its update_) plus one fetch."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from elphdynamics_amd import configs, greens, measurements as ms, preconditioners as pc, synth
tag = sys.argv[1] if len(sys.argv) > 1 else "C"
nv = 10
m = configs.make_model(tag, tol=1e-5)
P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
est = greens.EstimateGreensFunction(m, nv=nv)
R = np.stack([synth.randn(900 + i, m.Ndim) for i in range(nv)])
info = dict({k: {"measure": True, "time_dependent": True} for k in ms.ONSITE_CORR}, num_random_vectors=nv)
cont = ms.initialize_measurements_container(m, info, "")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
A, B, U = [], [], []
for rep in range(reps + 1):      # the first repetition warms up (allocations, first launches) and is not reported
    t0 = time.perf_counter(); it, res, fl = greens.update_(est, m, P=P, R=R, rng=np.random.default_rng(1)); t1 = time.perf_counter()
    npairs = 0
    for i in range(1, nv):
        for j in range(i + 1, nv + 1):
            greens.setup_(est, i, j); npairs += 1
    t2 = time.perf_counter()
    lib, h = m._lib, m._h
    for i in range(1, nv):
        for j in range(i + 1, nv + 1):
            lib.elph_greens_setup(h, i, j, None, None, None, None)
    t3 = time.perf_counter()
    ms.accumulate_(cont, m, est)
    ms.fetch_(cont, m)
    t4 = time.perf_counter()
    ms.reset_measurements_(cont, m)
    if rep:
        U.append(t1 - t0); A.append(t2 - t1); B.append(t4 - t3)
print(f"{tag}: update! ({nv} solves, KPM, {int(it.max())} its) {1e3*(t1-t0):.2f} ms; setup! x {npairs} pairs: {1e3*(t2-t1):.1f} ms "
      f"({1e3*(t2-t1)/npairs:.3f} ms each, 4 arrays to the host); device only {1e3*(t3-t2):.1f} ms ({1e3*(t3-t2)/npairs:.3f} ms each); "
      f"device route (all pairs folded on the device + one fetch) {1e3*(t4-t3):.1f} ms")
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731
print(f"{tag}: medians of {reps} repetitions (ms): update! {med(U):.2f}  A (setup! x {npairs}, arrays to the host) {med(A):.2f}  "
      f"B (device route + fetch) {med(B):.2f}  [min A {1e3*min(A):.2f}, min B {1e3*min(B):.2f}]")
