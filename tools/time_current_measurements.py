"""Time of one elph_current_accumulate (CurrentCurrent of the Holstein model, csrc/currcorr.hip) of 1, 2, 16, 64 resident chains, config C
(16 x 16, L = 160), the two square bond definitions, all four pairs time-dependent, n_v = 10 vectors per chain (45 pairs of vectors)
(`time_current_measurements.py [chain counts, default 1,2,16,64] [repetitions] [n_v] [seconds allowed per run, default 120]`), next to
  - one elph_bond_chains_accumulate that requests BondBond alone over the same four pairs, on the same handle and estimator in the
    same process: an existing path of similar shape (fields, transforms, one inverse transform per listed pair, fold) that also runs the
    estimator's setup! pipeline for every pair of vectors, which CurrentCurrent does not need;
  - the host route: elph_greens_get_vectors (the copy of all vectors) plus the numpy yardstick tests/current_reference.py
    (current_transcript, the np.fft evaluation) for ONE pair of vectors of one chain; a measurement needs 45 of them per chain.
Vectors are set, not solved: only the measurement is timed.  Every call synchronises before it returns; medians after one warm-up, the
two device sides alternating within a repetition, each run under its own time limit: a run that exceeds it ends the tool with a message.
Also prints the device bytes the unit holds per chain, computed from the shapes, and, for the last chain, the largest difference of the
device's sums for its first pair of vectors from the host route's (relative to max(1, max|host|))."""
import os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))
import current_reference as cref
from elphdynamics_amd import chain_bond_measurements as cbm, configs, current_measurements as cm, greens, models, synth
counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1, 2, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
nv = int(sys.argv[3]) if len(sys.argv) > 3 else 10
limit = float(sys.argv[4]) if len(sys.argv) > 4 else 120.0
td = {"measure": True, "time_dependent": True}
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731


def timed(what, fn):
    t0 = time.perf_counter()
    fn()
    dt = time.perf_counter() - t0
    if dt > limit:
        sys.exit(f"{what} took {dt:.1f} s, more than the {limit:.0f} s allowed: stopping")
    return dt


for nch in counts:
    m = configs.make_model("C", tol=1e-5)
    la = m.lattice
    N, L, ns, nc, dims = m.Nsites, m.Ltau, la.norbits, la.ncells, (la.L1, la.L2, la.L3)
    defs = m.bond_definitions
    ndef, Lh = len(defs), L // 2 + 1
    assert ndef == 2 and m.Nbonds == ndef * nc
    if nch > 1:
        models.update_model_chains_(m, np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=70 + c) for c in range(nch)]))
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    rng = np.random.default_rng(nch)
    greens.set_vectors_(est, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim)))
    folders = [""] * nch
    cur = cm.initialize_current_container(m, {"CurrentCurrent": td, "num_random_vectors": nv}, folders if nch > 1 else "")
    bond = cbm.initialize_chain_bond_container(m, {"BondBond": td, "num_random_vectors": nv}, folders)
    corr = cur.chains[0].intersite_corr["CurrentCurrent"]
    nP = corr.pairs.shape[1]
    assert nP == 4 and bond.chains[0].intersite_corr["BondBond"].pairs.shape[1] == 4
    if nch == counts[0]:
        buffers = 8 * 8 * ndef * L * nc + 16 * 8 * ndef * Lh * nc + 16 * nP * Lh * nc + 8 * nP * L * nc + 8 * nP * (L + 1) * 4      # f, nu, Y, B, part + dl
        acc = 2 * 8 * corr.position.size                                                                                       # the accumulator and the call's sum
        print(f"C: {N} sites, L = {L}, {ndef} bond definitions, {nP} listed pairs, n_v = {nv} ({nv * (nv - 1) // 2} pairs of vectors); per chain the "
              f"unit holds {buffers} B of fields, spectra and correlations + {acc} B of sums = {(buffers + acc) / 2**20:.2f} MiB", flush=True)
    A, B = [], []
    for rep in range(reps + 1):         # the first repetition warms up (allocations, first launches) and is not reported
        a = timed(f"one elph_current_accumulate of {nch} chains", lambda: cm.accumulate_current_(cur, m, est))
        b = timed(f"one elph_bond_chains_accumulate (BondBond) of {nch} chains", lambda: cbm.accumulate_bonds_(bond, m, est))
        cm.reset_current_measurements_(cur, m); cbm.reset_bond_measurements_(bond, m)
        if rep:
            A.append(a); B.append(b)
    # the host route: all vectors to the host, then the yardstick for one pair of vectors of the last chain
    c = nch - 1
    Rh, Xh = np.empty((nv * nch, m.Ndim)), np.empty((nv * nch, m.Ndim))
    from elphdynamics_amd._lib import check, dptr
    G = [timed("elph_greens_get_vectors", lambda: check(m._lib.elph_greens_get_vectors(m._h, dptr(Rh), dptr(Xh)))) for _ in range(3)]
    t0 = time.perf_counter()
    host = cref.current_transcript(Rh[c], Xh[c], Rh[nch + c], Xh[nch + c], m.t, L, ns, dims, defs, L + 1, corr.pairs)
    one_pair = time.perf_counter() - t0
    print(f"{nch} chains, n_v = {nv}: medians of {reps} repetitions (ms): elph_current_accumulate {med(A):.2f} [min {1e3 * min(A):.2f}]  "
          f"elph_bond_chains_accumulate (BondBond alone) {med(B):.2f} [min {1e3 * min(B):.2f}]  ratio {med(B) / med(A):.2f}  per chain "
          f"{med(A) / nch:.3f} vs {med(B) / nch:.3f};  host route: elph_greens_get_vectors {med(G):.2f} + numpy yardstick {1e3 * one_pair:.1f} "
          f"per pair of vectors of one chain ({nv * (nv - 1) // 2 * nch} such pairs in all)", flush=True)
    # the device's numbers for that one pair: a two-vector estimator on a single-configuration handle
    s = configs.make_model("C", tol=1e-5)
    est2 = greens.EstimateGreensFunction(s, nv=2)
    greens.set_vectors_(est2, np.stack([Rh[c], Rh[nch + c]]), np.stack([Xh[c], Xh[nch + c]]))
    two = cm.initialize_current_container(s, {"CurrentCurrent": td, "num_random_vectors": 2}, "")
    cm.accumulate_current_(two, s, est2)
    cm.fetch_current_(two, s)
    got = two.chains[0].intersite_corr["CurrentCurrent"].position
    print(f"{nch} chains: the first pair of vectors of chain {c}, device against the host route: largest difference "
          f"{np.abs(got - host).max() / max(1.0, np.abs(host).max()):.2e}", flush=True)
    s.close()
    m.close()
