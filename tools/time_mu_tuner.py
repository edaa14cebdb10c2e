"""Time of one mu_tuner.density_moments (elph_density_moments: <N> and <N^2> of every resident chain from the estimator's vectors) next to
one chain_measurements.accumulate_ on a container that requests no correlation (elph_meas_chains_accumulate: the only other route to the
two numbers, setup! for every pair of vectors), config C (16 x 16, L = 160), n_v = 10 vectors per chain as the decks have it
(`time_mu_tuner.py [chain counts, default 2,16,64] [repetitions] [n_v]`).  Vectors are set, not solved: only the measurement is timed.  Both
sides synchronise before they return; medians after one warm-up, the two sides alternating within a repetition, in one process.  After the
timing the largest difference of the two routes is printed in units of the bound the tests use (2e-12 of the yardstick would be 2.0)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from elphdynamics_amd import chain_measurements as cms, configs, greens, models, mu_tuner as mt, synth
counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
nv = int(sys.argv[3]) if len(sys.argv) > 3 else 10
npairs = nv * (nv - 1) // 2
info = {"num_random_vectors": nv}
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731

for nch in counts:
    m = configs.make_model("C", tol=1e-5)
    N, L = m.Nsites, m.Ltau
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=70 + c) for c in range(nch)])
    models.update_model_chains_(m, X)
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    rng = np.random.default_rng(nch)
    greens.set_vectors_(est, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim)))
    cm = cms.initialize_chain_measurements_container(m, info, [""] * nch)
    A, B = [], []
    for rep in range(reps + 1):         # the first repetition warms up (allocations, first launches) and is not reported
        t0 = time.perf_counter()
        got = mt.density_moments(m, est, nch)
        t1 = time.perf_counter()
        cms.accumulate_(cm, m, est, X)
        t2 = time.perf_counter()
        if rep < reps:
            cms.reset_measurements_(cm, m)
        if rep:
            A.append(t1 - t0); B.append(t2 - t1)
    print(f"{nch} chains, n_v = {nv} ({npairs} pairs, {2 * nv * N * L * 8 / 1e6:.2f} MB of vectors per chain): medians of {reps} repetitions (ms): "
          f"density_moments {med(A):.3f} [min {1e3 * min(A):.3f}]  scalars-only chain_measurements.accumulate_ {med(B):.2f} "
          f"[min {1e3 * min(B):.2f}]  ratio {med(B) / med(A):.1f}")
    # the two routes on the numbers that were timed, in units of 1e-12 of the yardstick (the sums of absolute values, per pair)
    cms.fetch_(cm, m)
    worst = 0.0
    for c in range(nch):
        x, r = np.abs(est.MinvR[c::nch]).reshape(nv, N, L), np.abs(est.R[c::nch]).reshape(nv, N, L)
        Ca = np.einsum("pst,qst->tpq", x, r)
        Ta, Sa = np.einsum("tpp->p", Ca) / L, np.einsum("tpq,tqp->pq", Ca, Ca)
        y1 = y2 = 0.0
        for p in range(nv - 1):
            for q in range(p + 1, nv):
                y1 += N + (Ta[p] + Ta[q]) / 2
                y2 += 4 * (N + Ta[p]) * (N + Ta[q]) + Ta[p] + Ta[q] + (2.0 / L) * Sa[p, q]
        g = cm.chains[c].global_meas
        worst = max(worst, abs(got[0][c] - g["density"].real * N / npairs) / (y1 / npairs), abs(got[1][c] - g["Nsqr"].real / npairs) / (y2 / npairs))
    print(f"{nch} chains: density_moments against the container's density and Nsqr: largest difference {worst / 1e-12:.3f} x 1e-12 of the yardstick")
    m.close()
