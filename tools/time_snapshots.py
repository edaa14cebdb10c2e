"""Time of one elph_snapshots (the density and double-occupancy snapshots of every resident chain from the estimator's vectors, one device
call) next to the host route to the same profiles: elph_greens_get_vectors (both arrays to the host) followed by the numpy sums of
tests/snapshot_reference.py per chain.  Config C (16 x 16, L = 160), n_v = 10 vectors per chain as the decks have it
(`time_snapshots.py [chain counts, default 2,16,64] [repetitions] [n_v]`).  Vectors are set, not solved: only the measurement is timed.
Both sides synchronise before they return; medians after one warm-up, the two sides alternating within a repetition, in one process, on
the same vectors.  The host route is reported in its two parts, the copy (which any host route pays) and the sums.  A call that follows
the host's sums finds the device idle; a measurement loop calls it right after the containers' accumulate_, so the device call is also
timed back to back (3 x repetitions calls in a row after one warm-up).  After the timing the largest difference of the two routes is
printed in units of the bound the tests use (1e-12 of the largest element would be 1.0)."""
import os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))
import snapshot_reference as sref
from elphdynamics_amd import configs, greens, models, snapshots as sn, synth
from elphdynamics_amd._lib import check, dptr
counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
nv = int(sys.argv[3]) if len(sys.argv) > 3 else 10
info = {"Snapshots": {"density": True, "double_occupancy": True}}
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731

for nch in counts:
    m = configs.make_model("C", tol=1e-5)
    N, L = m.Nsites, m.Ltau
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=70 + c) for c in range(nch)])
    models.update_model_chains_(m, X)
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    rng = np.random.default_rng(nch)
    greens.set_vectors_(est, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim)))
    sc = sn.initialize_snapshots_container(m, info, [""] * nch)
    R, MinvR = np.zeros_like(est.R), np.zeros_like(est.MinvR)
    A, B1, B2, A0 = [], [], [], []
    for rep in range(3 * reps + 1):     # back to back
        t0 = time.perf_counter()
        sn.snapshot_arrays_(sc, m, est)
        if rep:
            A0.append(time.perf_counter() - t0)
    for rep in range(reps + 1):         # the first repetition warms up (allocations, first launches) and is not reported
        t0 = time.perf_counter()
        got = sn.snapshot_arrays_(sc, m, est)
        t1 = time.perf_counter()
        check(m._lib.elph_greens_get_vectors(m._h, dptr(R), dptr(MinvR)))
        t2 = time.perf_counter()
        host = [(sref.density(R[c::nch], MinvR[c::nch], N, L), sref.double_occupancy(R[c::nch], MinvR[c::nch], N, L)) for c in range(nch)]
        t3 = time.perf_counter()
        if rep:
            A.append(t1 - t0); B1.append(t2 - t1); B2.append(t3 - t2)
    B = [a + b for a, b in zip(B1, B2)]
    print(f"{nch} chains, n_v = {nv} ({2 * nv * nch * N * L * 8 / 1e6:.1f} MB of vectors): medians of {reps} repetitions (ms): "
          f"elph_snapshots {med(A):.3f} [min {1e3 * min(A):.3f}] (back to back {med(A0):.3f} [min {1e3 * min(A0):.3f}])  host route {med(B):.1f} [min {1e3 * min(B):.1f}] = "
          f"elph_greens_get_vectors {med(B1):.2f} [min {1e3 * min(B1):.2f}] + numpy sums {med(B2):.1f} [min {1e3 * min(B2):.1f}]  "
          f"ratio to the whole route {med(B) / med(A):.0f}, to the copy alone {med(B1) / med(A):.1f}")
    worst = 0.0
    for c in range(nch):
        for name, want in zip(("density", "double_occupancy"), host[c]):
            worst = max(worst, np.abs(got[name][c] - want).max() / np.abs(want).max())
    print(f"{nch} chains: elph_snapshots against the host route: largest difference {worst / 1e-12:.4f} x 1e-12 of the largest element")
    m.close()
