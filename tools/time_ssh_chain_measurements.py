"""Time of one ssh_chain_measurements.accumulate_ (one elph_ssh_meas_chains_accumulate) of nchains resident chains next to nchains calls
of ssh_measurements.accumulate_ (elph_ssh_meas_accumulate) on one configuration (what a lockstep run of an SSH deck had to do before: a
chain at a time on a single-configuration handle), config E (16 x 16, L = 160, N_ph = 512), n_v = 2 vectors per chain, Greens, DenDen,
SpinSpin, PairGreens and PhononGreens (all four pairs of the two phonon types) time-dependent
(`time_ssh_chain_measurements.py [chain counts, default 2,16,64] [repetitions]`).  Vectors are set, not solved: only the measurement is
timed.  Both sides synchronise before they return and take their field from the host; medians after one warm-up, the two sides
alternating within a repetition.  After the timing the last chain of the batch is measured once more on both sides and the largest
difference is printed (relative to max(1, |single|), scalars one by one, a correlation in its max norm): the batch size changes the
tau-DFT kernels chosen.  Also prints the device bytes the chain path holds per chain, computed from the shapes."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from elphdynamics_amd import configs, greens, models, ssh_chain_measurements as scm, ssh_measurements as sm
counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
nv = 2
td = {"measure": True, "time_dependent": True}
info = dict({k: td for k in sm.CREATE_ORDER}, num_random_vectors=nv)
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731

# the single-configuration side: its own handle, one configuration resident
s = configs.make_model("E", tol=1e-5)
est1 = greens.EstimateGreensFunction(s, nv=nv)
rng1 = np.random.default_rng(900)
greens.set_vectors_(est1, rng1.standard_normal((nv, s.Ndim)), rng1.standard_normal((nv, s.Ndim)))
one = sm.initialize_ssh_measurements_container(s, info, "")

N, L, ns, Nph, nph, ndef = s.Nsites, s.Ltau, s.lattice.norbits, int(s.Nph), int(s.nph), int(s.nbonds)
nc, nd, ncol, Lo2, Lh, nP = N // ns, N * L, ns * N, (L + 1) // 2, L // 2 + 1, nph * nph
scratch = 8 * (8 * nd + 4 * L * ncol) + 16 * (2 * Lo2 * N + 6 * Lh * N + 4 * Lh * ncol)      # fields, tables; twisted, plain spectra, Y
fields = 8 * (2 * L * Nph + nP * L * nc) + 16 * (Lh * Nph + nP * Lh * nc)     # x as it arrives and in layout S, the PhononGreens tables; spectra, Y
total = 3 + 3 * ns + 8 * ndef + (L + 1) * nc * (4 * ns * ns + nP)
acc = 8 * 2 * total                                                           # the accumulators and this accumulate's sums
small = 8 * (L * max(2 * ns + 2 + 2 * ndef, 6 * ndef) + 6 * ndef + ns + 1)    # partials, field-only terms, means of mu
print(f"E: {N} sites, L = {L}, {Nph} phonons of {nph} types; per chain the chain path holds {scratch} B of estimator scratch + {fields} B of "
      f"fields, spectra and PhononGreens tables + {acc} B of accumulators + {small} B of partials = "
      f"{(scratch + fields + acc + small) / 2**20:.2f} MiB")

for nch in counts:
    m = configs.make_model("E", tol=1e-5)
    rng = np.random.default_rng(nch)
    X = np.stack([s.x * (1.0 - 0.5 * c / nch) + 0.02 * rng.standard_normal(s.Ndof) for c in range(nch)])
    models.update_model_chains_(m, X)
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    greens.set_vectors_(est, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim)))
    cm = scm.initialize_ssh_chain_measurements_container(m, info, [""] * nch)
    A, B = [], []
    for rep in range(reps + 1):         # the first repetition warms up (allocations, first launches) and is not reported
        t0 = time.perf_counter()
        scm.accumulate_(cm, m, est, X)
        t1 = time.perf_counter()
        for c in range(nch):            # a chain at a time: its field into the single-configuration model, one accumulate
            s.x[:] = X[c]
            sm.accumulate_(one, s, est1)
        t2 = time.perf_counter()
        scm.reset_measurements_(cm, m); sm.reset_measurements_(one, s)
        if rep:
            A.append(t1 - t0); B.append(t2 - t1)
    print(f"{nch} chains, n_v = {nv}: medians of {reps} repetitions (ms): one ssh_chain_measurements.accumulate_ {med(A):.2f} "
          f"[min {1e3 * min(A):.2f}]  {nch} x ssh_measurements.accumulate_ {med(B):.2f} [min {1e3 * min(B):.2f}]  "
          f"ratio {med(B) / med(A):.2f}  per chain {med(A) / nch:.3f} vs {med(B) / nch:.3f}")
    # the numbers of the size that was timed: the last chain on both sides
    c = nch - 1
    greens.set_vectors_(est1, est.R[c::nch], est.MinvR[c::nch])
    s.x[:] = X[c]
    scm.accumulate_(cm, m, est, X); sm.accumulate_(one, s, est1)
    scm.fetch_(cm, m); sm.fetch_(one, s)
    got, want = cm.chains[c], one
    worst = max(np.abs(sm._all_corr(got)[k].position - v.position).max() / max(1.0, np.abs(v.position).max()) for k, v in sm._all_corr(want).items())
    for a, b in [(got.global_meas[k], want.global_meas[k]) for k in want.global_meas] + \
                [(got.onsite_meas[k], want.onsite_meas[k]) for k in want.onsite_meas] + [(got.intersite_meas[k], want.intersite_meas[k]) for k in want.intersite_meas]:
        worst = max(worst, float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b))))))
    print(f"{nch} chains: chain {c} against the single-configuration path on the same field and vectors: largest difference {worst:.2e}")
    scm.reset_measurements_(cm, m); sm.reset_measurements_(one, s)
    m.close()
s.close()
