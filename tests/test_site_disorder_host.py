"""Host side of tests/test_gpu_site_disorder.py (no device): the disorder of tests/site_disorder_cases.py is strong enough, the CPU oracle
is healthy on it, and the comparisons the GPU tests make can see a parameter read at the wrong index.

For every tag of the dynamics list up to a few hundred sites the oracle's HMC update, Langevin step and composed fermion force — the
inputs test_gpu_hmc.check_hmc_update_vs_oracle, test_gpu_langevin.check_langevin_step_vs_oracle and
test_gpu_parity.check_fermion_force_vs_oracle hand to it — are redone with the five parameter arrays rolled by one site and, on
two-orbital lattices, with the two orbitals' values exchanged.  Every quantity those checkers assert has to move by at least 1000
times the bound it is asserted with (the bounds are imported, not restated).  The factor is fixed: a case that misses it is replaced,
not the factor.  The measured factors are printed (pytest -s).
"""
import numpy as np
import pytest

import site_disorder_cases as sdc
from kpm_bounds_reference import host_model
from test_gpu_hmc import UPDATE_BOUNDS, _oracle_update, _randoms
from test_gpu_langevin import STEP_BOUND
from test_gpu_parity import FORCE_BOUND, _oracle_force

TAGS = ["b", "d", "t", "q", "z", "r"]
FACTOR = 1000.0
LANGEVIN_MAXITER = 20000
PARAMS = ("omega", "omega4", "lam", "lam2", "mu")


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _model(tag, variant):
    m = sdc.prepare(tag)(host_model(tag))
    if variant is not None:
        for k, a in variant(m).items():
            getattr(m, k)[:] = a
    return m


def _oracle_model(oracle, m):
    E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
    return oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)


def _run(oracle, tag, variant=None):
    """The oracle's results on the disordered model (variant: a function of the model giving replacement parameter arrays)."""
    from elphdynamics_amd import preconditioners as pc, synth
    out = {}
    # the HMC update of check_hmc_update_vs_oracle: nt = 2, dt = 0.05, tol 1e-6, accelerator mass (1.0, 0.3)
    m = _model(tag, variant)
    fa = pc.FourierAccelerator(m)
    pc.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
    m.solver.tol, m.solver.maxiter = 1e-6, 20000
    nt, dt = 2, 0.05
    acc, x1, v1, info = _oracle_update(oracle, _oracle_model(oracle, m), m, fa, m.x.copy(), np.zeros(m.Ndof), dt, nt, 1, 0.0,
                                       _randoms(m, nt, 500, False, 0.0))
    out.update(hmc_flag=info["flag"], x=x1, v=v1, H0=info["H0"], H1=info["H1"], S=info["S"], K=info["K"])
    # two Heun steps of check_langevin_step_vs_oracle: dt = 0.01, tol 1e-8, accelerator Q (0.7)
    m = _model(tag, variant)
    fa = pc.FourierAccelerator(m)
    pc.update_Q_(fa, m, 0.0, np.inf, 0.7)
    om = _oracle_model(oracle, m)
    x, steps, its = m.x.copy(), [], []
    for step in range(2):
        x_new, it = oracle.langevin_evolve(2, om, x, fa.Q, 0.01, synth.randn(2000 + step, m.Ndof), synth.randn(2100 + step, m.Ndim),
                                           synth.randn(2200 + step, m.Ndim), m.omega, m.omega4, m.lam, m.lam2, m.mu, m.dtau, tol=1e-8,
                                           maxiter=LANGEVIN_MAXITER)
        steps.append(x_new - x)
        its.append(it)
        x = x_new
    out.update(langevin_iters=its, dx1=steps[0], dx2=steps[1])
    # the composed force of check_fermion_force_vs_oracle: tol 1e-11 (_oracle_force asserts the flags of its solves itself)
    m = _model(tag, variant)
    F, X, Sf = _oracle_force(oracle, _oracle_model(oracle, m), m, synth.randn(41, m.Ndim), synth.randn(42, m.Ndim), 1e-11)
    out.update(F=F, Xp=X[0], Xm=X[1])
    return out


# quantity -> (how far apart two results are, the bound the GPU checker asserts it with)
QUANTITIES = {
    "end field": (lambda a, b: rel(a["x"], b["x"]), UPDATE_BOUNDS["x"]),
    "end momentum": (lambda a, b: rel(a["v"], b["v"]), UPDATE_BOUNDS["v"]),
    "H0": (lambda a, b: abs(a["H0"] - b["H0"]) / abs(b["H0"]), UPDATE_BOUNDS["H0"]),
    "H1": (lambda a, b: abs(a["H1"] - b["H1"]) / abs(b["H1"]), UPDATE_BOUNDS["H1"]),
    "S": (lambda a, b: abs(a["S"] - b["S"]) / abs(b["S"]), UPDATE_BOUNDS["S"]),
    "K": (lambda a, b: abs(a["K"] - b["K"]) / abs(b["K"]), UPDATE_BOUNDS["K"]),
    "Langevin step 1": (lambda a, b: rel(a["dx1"], b["dx1"]), STEP_BOUND),
    "Langevin step 2": (lambda a, b: rel(a["dx2"], b["dx2"]), STEP_BOUND),
    "F": (lambda a, b: rel(a["F"], b["F"]), FORCE_BOUND),
    "solution +": (lambda a, b: rel(a["Xp"], b["Xp"]), FORCE_BOUND),
    "solution -": (lambda a, b: rel(a["Xm"], b["Xm"]), FORCE_BOUND),
}


_REFERENCE = {}


def _reference(oracle, tag):
    """_run on the disordered model itself, computed once per tag."""
    if tag not in _REFERENCE:
        _REFERENCE[tag] = _run(oracle, tag)
    return _REFERENCE[tag]


@pytest.mark.parametrize("tag", ["d", "z"])
def test_the_orbitals_differ_by_more_than_the_noise(tag):
    """The two orbitals' means of ω, λ and μ are more than three within-orbital standard deviations (the larger of the two orbitals')
    apart: exchanging the orbitals is not hidden by the site-to-site noise.  The widths of site_disorder_cases put ω and μ at 3.0 in
    the mean (0.3 / 0.1), so a draw meets this or misses it by a little: the seeds of d and z are ones that meet it."""
    m = sdc.prepare(tag)(host_model(tag))
    orb = sdc.orbitals(m)
    assert m.lattice.norbits == 2 and set(orb) == {0, 1}
    for k in ("omega", "lam", "mu"):
        a, b = getattr(m, k)[orb == 0], getattr(m, k)[orb == 1]
        sd = max(a.std(ddof=1), b.std(ddof=1))
        gap = abs(a.mean() - b.mean())
        print(f"site disorder orbitals: tag {tag} {k:5s} means {a.mean():+.4f} {b.mean():+.4f}  gap / std {gap / sd:.2f}")
        assert gap > 3.0 * sd, (tag, k, a.mean(), b.mean(), sd)
    assert np.all(m.omega > 0.0) and np.all(m.omega4 >= 0.0)


def test_the_disorder_is_deterministic_and_leaves_the_field():
    a, b, c = sdc.disorder_(host_model("d")), sdc.disorder_(host_model("d")), host_model("d")
    for k in PARAMS:
        assert np.array_equal(getattr(a, k), getattr(b, k)) and len(np.unique(getattr(a, k))) == a.Nsites
    assert np.array_equal(a.x, c.x)
    one = sdc.disorder_(host_model("b"))
    assert abs(one.omega.mean() - sdc.OMEGA[0]) < 0.1 and abs(one.mu.mean() - sdc.MU[0]) < 0.1
    mus = sdc.chain_mu(a, 3)
    assert mus.shape == (3, a.Nsites) and not np.allclose(mus[0], mus[1]) and not np.allclose(mus[1], mus[2])


@pytest.mark.parametrize("tag", TAGS)
def test_the_oracle_is_healthy_on_the_disordered_model(oracle, tag):
    """Flag 0 of the HMC update and of the force's solves (_oracle_force asserts them).  The oracle's Langevin entry returns no flag:
    a Heun step reports the mean of its two solves' iteration counts, which is held below maxiter / 2 instead — one solve that ran
    out would alone bring the mean to that."""
    r = _reference(oracle, tag)
    assert r["hmc_flag"] == 0 and all(0 < it < LANGEVIN_MAXITER // 2 for it in r["langevin_iters"])
    for k in ("x", "v", "dx1", "dx2", "F", "Xp", "Xm"):
        assert np.all(np.isfinite(r[k])) and np.any(r[k] != 0.0), k
    assert all(np.isfinite(r[k]) for k in ("H0", "H1", "S", "K"))


@pytest.mark.parametrize("tag", TAGS)
def test_an_index_error_moves_every_asserted_quantity(oracle, tag):
    """Parameters rolled by one site / orbitals exchanged: every quantity moves by at least FACTOR times its bound."""
    ref = _reference(oracle, tag)
    variants = [("rolled", sdc.rolled)] + ([("exchanged", sdc.orbitals_exchanged)] if host_model(tag).lattice.norbits == 2 else [])
    low = []
    for name, variant in variants:
        moved = _run(oracle, tag, variant)
        assert moved["hmc_flag"] == 0
        for q, (dist, bound) in QUANTITIES.items():
            factor = dist(moved, ref) / bound
            print(f"site disorder sensitivity: tag {tag:3s} {name:9s} {q:16s} moved {dist(moved, ref):.3e} = {factor:10.3e} x bound {bound:g}")
            if factor < FACTOR:
                low.append((name, q, factor))
    assert not low, low


@pytest.mark.parametrize("tag", TAGS)
def test_the_swap_move_sees_the_bosonic_action(oracle, tag):
    """ΔS_b of the swap the GPU test proposes (site_disorder_cases.swap_columns) is at least 1e-3 |S_b|; the numpy S_b it is formed
    from is the oracle's."""
    m = sdc.prepare(tag)(host_model(tag))
    i, j = sdc.swap_columns(m)
    assert i != j and (m.lattice.norbits == 1 or sdc.orbitals(m)[i] != sdc.orbitals(m)[j])
    Sb = sdc.bosonic_action(m)
    Sb_o = oracle.calc_Sb_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.omega, m.omega4)
    assert abs(Sb - Sb_o) < 1e-12 * abs(Sb_o)
    X = m.x.reshape(m.Nsites, m.Ltau).copy()
    X[[i, j]] = X[[j, i]]
    dS = sdc.swap_delta_Sb(m, i, j)
    assert abs((sdc.bosonic_action(m, X) - Sb) - dS) < 1e-11 * abs(Sb)
    print(f"site disorder swap: tag {tag:3s} columns ({i}, {j})  dS_b = {dS:.6e}  S_b = {Sb:.6e}  ratio {abs(dS) / abs(Sb):.3e}")
    assert dS != 0.0 and abs(dS) >= 1e-3 * abs(Sb)
