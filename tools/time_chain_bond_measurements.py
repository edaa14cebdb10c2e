"""Time of one chain_bond_measurements.accumulate_bonds_ of nchains resident chains next to nchains calls of
bond_measurements.accumulate_bonds_ on one configuration (what a lockstep run had to do before: a chain at a time on a
single-configuration handle), config C (16 x 16, L = 160), the two square bond definitions, all four pairs of BondBond and of
BondPairGreens time-dependent, n_v = 2 vectors per chain
(`time_chain_bond_measurements.py [chain counts, default 2,16,64] [repetitions] [seconds allowed per side and run, default 60]`).
Vectors are set, not solved: only the measurement is timed.  Both sides synchronise before they return; medians after one warm-up, the
two sides alternating within a repetition, each run under its own time limit: a side that exceeds it ends the tool with a message.
After the timing the last chain of the batch is measured once more on both sides and the largest difference is printed (relative to
max(1, max|single|)): the batch size changes the tau-DFT kernels chosen.  Also prints the device bytes the chain path holds per chain,
computed from the shapes."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from elphdynamics_amd import bond_measurements as bm, chain_bond_measurements as cbm, configs, greens, models, synth
counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
limit = float(sys.argv[3]) if len(sys.argv) > 3 else 60.0
nv = 2
td = {"measure": True, "time_dependent": True}
info = {"BondBond": td, "BondPairGreens": td, "num_random_vectors": nv}
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731


def timed(what, fn):
    t0 = time.perf_counter()
    fn()
    dt = time.perf_counter() - t0
    if dt > limit:
        sys.exit(f"{what} took {dt:.1f} s, more than the {limit:.0f} s allowed: stopping")
    return dt


# the single-configuration side: its own handle, one configuration resident
s = configs.make_model("C", tol=1e-5)
est1 = greens.EstimateGreensFunction(s, nv=nv)
greens.set_vectors_(est1, np.stack([synth.randn(900 + i, s.Ndim) for i in range(nv)]), np.stack([synth.randn(1900 + i, s.Ndim) for i in range(nv)]))
one = bm.initialize_bond_container(s, info, "")
assert len(one.bond_definitions) == 2 and all(v.pairs.shape[1] == 4 for v in one.intersite_corr.values())

N, L, ns, nc = s.Nsites, s.Ltau, s.lattice.norbits, s.lattice.ncells
nd, ncol, Lo2, Lh = N * L, ns * N, (L + 1) // 2, L // 2 + 1
ndef, nP = len(one.bond_definitions), sum(v.pairs.shape[1] for v in one.intersite_corr.values())
scratch = 8 * (8 * nd + 4 * L * ncol) + 16 * (2 * Lo2 * N + 6 * Lh * N + 4 * Lh * ncol)      # fields, tables; twisted, plain spectra, Y
buffers = 8 * 6 * ndef * L * nc + 16 * 6 * ndef * Lh * nc + 16 * nP * Lh * nc + 8 * nP * L * nc      # f, nu, Y, B
acc = 8 * sum(v.position.size for v in one.intersite_corr.values())
print(f"C: {N} sites, L = {L}, {ndef} bond definitions, {nP} listed pairs; per chain the chain path holds {scratch} B of estimator scratch + "
      f"{buffers} B of fields, spectra and correlations + {acc} B of accumulators = {(scratch + buffers + acc) / 2**20:.2f} MiB")

for nch in counts:
    m = configs.make_model("C", tol=1e-5)
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=70 + c) for c in range(nch)])
    models.update_model_chains_(m, X)
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    rng = np.random.default_rng(nch)
    greens.set_vectors_(est, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim)))
    cb = cbm.initialize_chain_bond_container(m, info, [""] * nch)
    A, B = [], []

    def chain_at_a_time():
        for c in range(nch):            # the correlations read the vectors alone: one accumulate per chain on the single-configuration handle
            bm.accumulate_bonds_(one, s, est1)

    for rep in range(reps + 1):         # the first repetition warms up (allocations, first launches) and is not reported
        a = timed(f"one chain_bond_measurements.accumulate_bonds_ of {nch} chains", lambda: cbm.accumulate_bonds_(cb, m, est))
        b = timed(f"{nch} x bond_measurements.accumulate_bonds_", chain_at_a_time)
        cbm.reset_bond_measurements_(cb, m); bm.reset_bond_measurements_(one, s)
        if rep:
            A.append(a); B.append(b)
    print(f"{nch} chains, n_v = {nv}: medians of {reps} repetitions (ms): one chain_bond_measurements.accumulate_bonds_ {med(A):.2f} "
          f"[min {1e3 * min(A):.2f}]  {nch} x bond_measurements.accumulate_bonds_ {med(B):.2f} [min {1e3 * min(B):.2f}]  "
          f"ratio {med(B) / med(A):.2f}  per chain {med(A) / nch:.3f} vs {med(B) / nch:.3f}", flush=True)
    # the numbers of the size that was timed: the last chain on both sides
    c = nch - 1
    keep = est1.R.copy(), est1.MinvR.copy()
    greens.set_vectors_(est1, est.R[c::nch], est.MinvR[c::nch])
    cbm.accumulate_bonds_(cb, m, est); bm.accumulate_bonds_(one, s, est1)
    cbm.fetch_bonds_(cb, m); bm.fetch_bonds_(one, s)
    got, want = cb.chains[c].intersite_corr, one.intersite_corr
    worst = max(np.abs(got[k].position - want[k].position).max() / max(1.0, np.abs(want[k].position).max()) for k in want)
    print(f"{nch} chains: chain {c} against the single-configuration path on the same vectors: largest difference {worst:.2e}", flush=True)
    cbm.reset_bond_measurements_(cb, m); bm.reset_bond_measurements_(one, s)
    greens.set_vectors_(est1, *keep)
    m.close()
s.close()
