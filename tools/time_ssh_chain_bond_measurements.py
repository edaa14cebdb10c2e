"""Time of one ssh_chain_bond_measurements.accumulate_ssh_bonds_ (one elph_ssh_bond_chains_accumulate) of nchains resident chains next to
nchains calls of ssh_bond_measurements.accumulate_ssh_bonds_ (elph_ssh_bond_accumulate) on one configuration (what a lockstep run of an
SSH deck had to do before: a chain at a time on a single-configuration handle), config E (16 x 16, L = 160, N_ph = 512, two bond
definitions), n_v = 2 vectors per chain, BondBond, CurrentCurrent and BondPairGreens time-dependent over all four pairs of definitions
(`time_ssh_chain_bond_measurements.py [chain counts, default 2,16,64] [repetitions]`).  Vectors are set, not solved: only the measurement
is timed.  Both sides synchronise before they return and take their field from the host; medians after one warm-up, the two sides
alternating within a repetition.  After the timing the last chain of the batch is measured once more on both sides and the largest
difference is printed (a correlation in its max norm, relative to max(1, max|single|)): the batch size changes the tau-DFT kernels
chosen.  A chain count the library refuses (device memory, a grid limit) is reported with the library's message instead of a time.
Also prints the device bytes the chain path holds per chain, computed from the shapes."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from elphdynamics_amd import _lib, configs, greens, models, ssh_bond_measurements as sb, ssh_chain_bond_measurements as scb
counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
nv = 2
td = {"measure": True, "time_dependent": True}
info = dict({k: td for k in sb.SSH_BOND_CORR}, num_random_vectors=nv)
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731

# the single-configuration side: its own handle, one configuration resident
s = configs.make_model("E", tol=1e-5)
est1 = greens.EstimateGreensFunction(s, nv=nv)
rng1 = np.random.default_rng(900)
greens.set_vectors_(est1, rng1.standard_normal((nv, s.Ndim)), rng1.standard_normal((nv, s.Ndim)))
one = sb.initialize_ssh_bond_container(s, info, "")

N, L, ns, Nph, ndef = s.Nsites, s.Ltau, s.lattice.norbits, int(s.Nph), int(s.nbonds)
nc, nd, ncol, Lo2, Lh, npr = N // ns, N * L, ns * N, (L + 1) // 2, L // 2 + 1, ndef * ndef
scratch = 8 * (8 * nd + 4 * L * ncol) + 16 * (2 * Lo2 * N + 6 * Lh * N + 4 * Lh * ncol)      # fields, tables; twisted, plain spectra, Y
bond = 8 * (6 * ndef * L * nc + 2 * npr * L * nc) + 16 * (6 * ndef * Lh * nc + 2 * npr * Lh * nc)    # BondState: f, B; nu, Y (both correlations)
curr = 8 * (L * Nph + 8 * ndef * L * nc + npr * L * nc + npr * L * 4 + npr * 4) + 16 * (8 * ndef * Lh * nc + npr * Lh * nc)     # xr, f, B, part, dl; nu, Y
acc = 8 * 3 * (L + 1) * nc * npr                                              # [BondBond | BondPairGreens] and [CurrentCurrent]
print(f"E: {N} sites, L = {L}, {Nph} phonons, {ndef} bond definitions; per chain the chain path holds {scratch} B of estimator scratch + {bond} B "
      f"of BondBond / BondPairGreens fields, spectra and tables + {curr} B of CurrentCurrent field, fields, spectra, tables and partials + "
      f"{acc} B of accumulators = {(scratch + bond + curr + acc) / 2**20:.2f} MiB")

for nch in counts:
    m = configs.make_model("E", tol=1e-5)
    rng = np.random.default_rng(nch)
    X = np.stack([s.x * (1.0 - 0.5 * c / nch) + 0.02 * rng.standard_normal(s.Ndof) for c in range(nch)])
    A, B = [], []
    try:
        models.update_model_chains_(m, X)
        est = greens.EstimateGreensFunction(m, nv=nv * nch)
        greens.set_vectors_(est, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim)))
        cb = scb.initialize_ssh_chain_bond_container(m, info, [""] * nch)
        for rep in range(reps + 1):         # the first repetition warms up (allocations, first launches) and is not reported
            t0 = time.perf_counter()
            scb.accumulate_ssh_bonds_(cb, m, est, X)
            t1 = time.perf_counter()
            for c in range(nch):            # a chain at a time: its field into the single-configuration model, one accumulate
                s.x[:] = X[c]
                sb.accumulate_ssh_bonds_(one, s, est1)
            t2 = time.perf_counter()
            scb.reset_ssh_bond_measurements_(cb, m); sb.reset_ssh_bond_measurements_(one, s)
            if rep:
                A.append(t1 - t0); B.append(t2 - t1)
    except _lib.ElphError as e:
        print(f"{nch} chains, n_v = {nv}: refused by the library: {e}")
        m.close()
        continue
    print(f"{nch} chains, n_v = {nv}: medians of {reps} repetitions (ms): one ssh_chain_bond_measurements.accumulate_ssh_bonds_ {med(A):.2f} "
          f"[min {1e3 * min(A):.2f}]  {nch} x ssh_bond_measurements.accumulate_ssh_bonds_ {med(B):.2f} [min {1e3 * min(B):.2f}]  "
          f"ratio {med(B) / med(A):.2f}  per chain {med(A) / nch:.3f} vs {med(B) / nch:.3f}")
    # the numbers of the size that was timed: the last chain on both sides
    c = nch - 1
    greens.set_vectors_(est1, est.R[c::nch], est.MinvR[c::nch])
    s.x[:] = X[c]
    scb.accumulate_ssh_bonds_(cb, m, est, X); sb.accumulate_ssh_bonds_(one, s, est1)
    scb.fetch_ssh_bonds_(cb, m); sb.fetch_ssh_bonds_(one, s)
    worst = {k: np.abs(cb.chains[c].intersite_corr[k].position - v.position).max() / max(1.0, np.abs(v.position).max())
             for k, v in one.intersite_corr.items()}
    print(f"{nch} chains: chain {c} against the single-configuration path on the same field and vectors: largest difference "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    scb.reset_ssh_bond_measurements_(cb, m); sb.reset_ssh_bond_measurements_(one, s)
    m.close()
s.close()
