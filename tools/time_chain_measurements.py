"""Time of one chain_measurements.accumulate_ of nchains resident chains next to nchains calls of measurements.accumulate_ on one
configuration (what a lockstep run had to do before: a chain at a time on a single-configuration handle), config C (16 x 16, L = 160),
n_v = 2 vectors per chain, all five on-site correlations time-dependent
(`time_chain_measurements.py [chain counts, default 2,16,64] [repetitions]`).  Vectors are set, not solved: only the measurement is
timed.  Both sides synchronise before they return and take their field from the host; medians after one warm-up, the two sides
alternating within a repetition.  After the timing the last chain of the batch is measured once more on both sides and the largest
difference is printed (relative to max(1, |single|), scalars one by one, a correlation in its max norm): the batch size changes the
tau-DFT kernels chosen.  Also prints the device bytes the chain path holds per chain, computed from the shapes."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from elphdynamics_amd import chain_measurements as cms, configs, greens, measurements as ms, models, synth
counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
nv = 2
td = {"measure": True, "time_dependent": True}
info = dict({k: td for k in ms.ONSITE_CORR}, num_random_vectors=nv)
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731

# the single-configuration side: its own handle, one configuration resident
s = configs.make_model("C", tol=1e-5)
est1 = greens.EstimateGreensFunction(s, nv=nv)
greens.set_vectors_(est1, np.stack([synth.randn(900 + i, s.Ndim) for i in range(nv)]), np.stack([synth.randn(1900 + i, s.Ndim) for i in range(nv)]))
one = ms.initialize_measurements_container(s, info, "")

N, L, ns = s.Nsites, s.Ltau, s.lattice.norbits
nd, ncol, Lo2, Lh = N * L, ns * N, (L + 1) // 2, L // 2 + 1
scratch = 8 * (8 * nd + 4 * L * ncol) + 16 * (2 * Lo2 * N + 6 * Lh * N + 4 * Lh * ncol)      # fields, tables; twisted, plain spectra, Y
fields = 8 * (2 * nd + L * ncol)                                                              # x as it arrives and in layout S, its translation average
acc = 8 * (3 + 9 * ns + int(s.nbonds) + 5 * (L + 1) * (N // ns) * ns * ns)
print(f"C: {N} sites, L = {L}; per chain the chain path holds {scratch} B of estimator scratch + {fields} B of fields and PhononGreens "
      f"table + {acc} B of accumulators = {(scratch + fields + acc) / 2**20:.2f} MiB")

for nch in counts:
    m = configs.make_model("C", tol=1e-5)
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=70 + c) for c in range(nch)])
    models.update_model_chains_(m, X)
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    rng = np.random.default_rng(nch)
    greens.set_vectors_(est, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim)))
    cm = cms.initialize_chain_measurements_container(m, info, [""] * nch)
    A, B = [], []
    for rep in range(reps + 1):         # the first repetition warms up (allocations, first launches) and is not reported
        t0 = time.perf_counter()
        cms.accumulate_(cm, m, est, X)
        t1 = time.perf_counter()
        for c in range(nch):            # a chain at a time: its field into the single-configuration model, one accumulate
            s.x[:] = X[c]
            ms.accumulate_(one, s, est1)
        t2 = time.perf_counter()
        cms.reset_measurements_(cm, m); ms.reset_measurements_(one, s)
        if rep:
            A.append(t1 - t0); B.append(t2 - t1)
    print(f"{nch} chains, n_v = {nv}: medians of {reps} repetitions (ms): one chain_measurements.accumulate_ {med(A):.2f} "
          f"[min {1e3 * min(A):.2f}]  {nch} x measurements.accumulate_ {med(B):.2f} [min {1e3 * min(B):.2f}]  "
          f"ratio {med(B) / med(A):.2f}  per chain {med(A) / nch:.3f} vs {med(B) / nch:.3f}")
    # the numbers of the size that was timed: the last chain on both sides
    c = nch - 1
    greens.set_vectors_(est1, est.R[c::nch], est.MinvR[c::nch])
    s.x[:] = X[c]
    cms.accumulate_(cm, m, est, X); ms.accumulate_(one, s, est1)
    cms.fetch_(cm, m); ms.fetch_(one, s)
    got, want = cm.chains[c], one
    worst = max(np.abs(got.onsite_corr[k].position - want.onsite_corr[k].position).max() / max(1.0, np.abs(want.onsite_corr[k].position).max())
                for k in want.onsite_corr)
    for a, b in [(got.global_meas[k], want.global_meas[k]) for k in want.global_meas] + \
                [(got.onsite_meas[k], want.onsite_meas[k]) for k in want.onsite_meas] + [(got.intersite_meas["el_ke"], want.intersite_meas["el_ke"])]:
        worst = max(worst, float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b))))))
    print(f"{nch} chains: chain {c} against the single-configuration path on the same field and vectors: largest difference {worst:.2e}")
    cms.reset_measurements_(cm, m); ms.reset_measurements_(one, s)
    m.close()
s.close()
