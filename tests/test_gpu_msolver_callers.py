"""The callers of the solve on a BiCGStab / GMRES model (-m gpu): the pair solve behind the HMC force and action, the Green's-function
estimator, the HMC update (single chain, chains in lockstep, reject, failed solves), the Langevin step, the special moves and a GMRES deck,
on the smallest models that reach each code path (b, t, e, d).

References.  Tests 1-3 compare with tests/msolver_caller_cases.py / tests/msolver_reference.py (dense numpy restatements): EQUAL iteration
counts — every stage of every case stops with a log-margin >= 1e-2 (tests/test_msolver_callers_host.py) — and x to 1e-10 per solve, the
composed solution of the pair to 1e-10 (1 + KAPPA) with the table's stage-2 sensitivity.  Tests 4, 7 and 8 compare whole trajectories with
the CG route of the same library from the same state and random numbers at tol = 1e-6: both compute the same trajectory up to the solver
tolerance.  Their bounds are measured, not chosen: the CG route's own difference between tol = 1e-6 and tol = 1e-7 on the same inputs
(MEASURED below, taken on an MI355X with the code of this file: _measure_cg_sensitivity), times ALLOW = 10 — the one-sided routes stop on
another residual norm, and one order over the path's own tolerance-sensitivity separates "same trajectory" from "wrong force".

Without a preconditioner the one-sided solvers do not get there on these fields, in the reference's own arithmetic: bare BiCGStab breaks
down or runs out on b, d, e and t at every tolerance tried, bare GMRES(20) stagnates on b (|r|/|b| = 0.12 after 2000 iterations) and needs
700 - 1750 iterations per stage on d and e.  The un-preconditioned HMC cases therefore assert what the reference's ldiv! says about the
first solve of the update (tests/msolver_reference.py's mldiv decides on the CPU): flagged -> the update is killed (flag > 0, rejected, x
restored bit-exactly), converged -> the trajectory comparison as for the preconditioned cases.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from elphdynamics_amd import _lib, configs, greens, hmc, langevin, models, preconditioners as prec, process_input as pi, synth
import msolver_caller_cases as cc
import msolver_reference as ref
import stop_rule_cases as src

pytestmark = pytest.mark.gpu

DECKS = os.path.join(os.path.dirname(__file__), "decks")
SOLVERS = {"cg": ("CG", -1), "bicgstab": ("BiCGStab", -1), "gmres": ("GMRES", 20)}
ALLOW = 10.0             # the bound of a trajectory comparison: ALLOW x the CG route's own difference between tol 1e-6 and 1e-7


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _as(m, solver, tol, maxiter, restart=-1):
    """The model with the solver the constructor keyword would have given it, pushed to the handle as the constructor does."""
    m.solver, m.mul_by_M = models.make_solver(solver, m.Ndim, tol, maxiter, restart)
    m.transposed = False
    m._push_solver()
    return m


def _P(m, n=None):
    cls = prec.LeftRightKPMPreconditioner if m.mul_by_M else prec.SymmetricKPMPreconditioner
    return cls(m, n=min(20, m.Nsites) if n is None else n, buf=0.05, c1=1.0, c2=1.0)


@pytest.fixture(scope="module")
def gpu():
    """(name, nchains) -> (model, LeftRight preconditioner); the expansion's bounds are injected per call from the oracle's Arnoldi run."""
    made = {}

    def get(name, nchains=1):
        if (name, nchains) not in made:
            m = _as(configs.make_model(name), "GMRES", 1e-5, 40, 20)
            if nchains > 1:
                models.update_model_chains_(m, src.chain_fields(ref.host_model(name), nchains))
            made[(name, nchains)] = (m, prec.LeftRightKPMPreconditioner(m))
        return made[(name, nchains)]

    yield get
    for m, _ in made.values():
        m.close()


def _bounds(oracle, name, nchains=1):
    """setup_kwargs that inject the oracle's bounds (one expansion on both sides of the comparison)."""
    if nchains == 1:
        b = ref.setup(oracle, name).bounds
        return dict(e_min=b[0], e_max=b[1])
    bs = [ref.setup(oracle, name, c, nchains).bounds for c in range(nchains)]
    return dict(e_min=[b[0] for b in bs], e_max=[b[1] for b in bs])


# ------------------------------------------------------------------------------------------ 1, 2: the pair solve through the force call

@pytest.mark.parametrize("case", cc.CASES + (cc.BARE_CASE,), ids=cc.case_id)
def test_pair_solve_through_the_force_call(oracle, gpu, case):
    name, solver, restart, use_prec, tol, maxiter, k = case
    S = ref.setup(oracle, name)
    want = cc.pair(S, solver, restart, tol, maxiter, use_prec)
    m, P = gpu(name)
    _as(m, solver, tol, maxiter, restart or -1)
    phi_p, phi_m = cc.phis(S.n)
    Xp, Xm, it, fl = hmc.calc_OinvLambda_phi(m, phi_p, phi_m, P if use_prec else None, setup_kwargs=_bounds(oracle, name))
    if k is None:                                        # the bare BiCGStab case: the reference's answer is the flagged one
        print(f"{cc.case_id(case)}: iters {it} (reference {want['iters']}), flag {fl} (reference {want['flag']})")
        assert (it, fl) == (want["iters"], want["flag"]) == (10, 1) and not Xp.any() and not Xm.any()
        return
    ep, em = _rel(Xp, want["X"][0]), _rel(Xm, want["X"][1])
    print(f"{cc.case_id(case)}: iters {it} (reference {want['iters']} of {want['it']}), flag {fl}, |X+ - ref| {ep:.2e}, |X- - ref| {em:.2e}, "
          f"bound {cc.x_tolerance(k):.2e}")
    assert fl == 0 and want["flag"] == 0 and it == want["iters"]
    assert ep < cc.x_tolerance(k) and em < cc.x_tolerance(k)


@pytest.mark.parametrize("solver,restart,maxiter", (("bicgstab", 0, 5), ("gmres", 4, 4), ("gmres", 20, 20)))
def test_flags_of_a_stage_that_runs_out(oracle, gpu, solver, restart, maxiter):
    """b without a preconditioner and a solver.maxiter stage 1 cannot meet: flag > 0, X₋ zero, iters not halved — the reference's fold."""
    S = ref.setup(oracle, "b")
    want = cc.pair(S, solver, restart, 1e-5, maxiter, False)
    assert want["fl"][0][0] > 0 and want["flag"] > 0                       # (chosen on the CPU)
    assert want["iters"] == want["it"][0][0] + want["it"][1][0] == maxiter + (maxiter if solver == "bicgstab" else 0)
    m, _ = gpu("b")
    _as(m, solver, 1e-5, maxiter, restart or -1)
    Xp, Xm, it, fl = hmc.calc_OinvLambda_phi(m, *cc.phis(S.n))
    print(f"{solver}{restart or ''} maxiter {maxiter}: iters {it}, flag {fl}; reference {want['iters']}, {want['flag']}, stages {want['it']}, {want['fl']}")
    assert fl > 0 and (it, fl) == (want["iters"], want["flag"]) and not Xm.any() and not Xp.any()


# ------------------------------------------------------------------------------------------ 3: the estimator

SEED_R = 4300            # synth.randn seeds of the estimator's explicit noise vectors: SEED_R + v


def _noise(n, nv):
    return np.ascontiguousarray(np.stack([synth.randn(SEED_R + v, n) for v in range(nv)]))


@pytest.mark.parametrize("solver,restart", (("bicgstab", 0), ("gmres", 20)))
@pytest.mark.parametrize("name", ("b", "e", "d"))
def test_estimator_solves_M_x_equal_r(oracle, gpu, name, solver, restart):
    S = ref.setup(oracle, name)
    m, P = gpu(name)
    _as(m, solver, 1e-5, 40, restart or -1)
    est = greens.EstimateGreensFunction(m, 3)
    R = _noise(S.n, est.nv)
    it, res, fl = greens.update_(est, m, P, R=R, setup_kwargs=_bounds(oracle, name))
    for v in range(est.nv):
        margin = ref.solve(solver, S.M, R[v], np.zeros(S.n), 1e-5, 40, 40, restart, S.P("M"))[2]
        xr, itr, resr, flr = ref.mldiv(solver, S.M, R[v], np.zeros(S.n), 1e-5, 40, restart, S.P("M"))
        e = _rel(est.MinvR[v], xr)
        print(f"{name} {solver}{restart or ''} vector {v}: iters {it[v]} (reference {itr}, margin {margin:.3f}), flag {fl[v]}, |x - ref| {e:.2e}")
        assert margin >= ref.MARGIN                                          # (of the input: the reference stops where any summation order does)
        assert (it[v], fl[v]) == (itr, flr) == (itr, 0) and e < 1e-10 and abs(res[v] - resr) < 1e-8
        # x = M⁻¹ r, not (MᵀM)⁻¹ r or (MᵀM)⁻¹ Mᵀ r by CG to another tolerance
        assert _rel(est.MinvR[v], np.linalg.solve(S.M, R[v])) < 1e-3


@pytest.mark.parametrize("name", ("b", "e"))
def test_estimator_two_chains(oracle, gpu, name):
    S = [ref.setup(oracle, name, c, 2) for c in range(2)]
    m, P = gpu(name, 2)
    _as(m, "gmres", 1e-5, 40, 20)
    est = greens.EstimateGreensFunction(m, 4)              # vector v of chain c: row v * 2 + c
    R = _noise(m.Ndim, est.nv)
    it, res, fl = greens.update_(est, m, P, R=R, setup_kwargs=_bounds(oracle, name, 2))
    for r in range(est.nv):
        C = S[r % 2]
        xr, itr, resr, flr = ref.mldiv("gmres", C.M, R[r], np.zeros(C.n), 1e-5, 40, 20, C.P("M"))
        e, cross = _rel(est.MinvR[r], xr), _rel(est.MinvR[r], np.linalg.solve(S[(r + 1) % 2].M, R[r]))
        print(f"{name} row {r} (chain {r % 2}): iters {it[r]} (reference {itr}), |x - ref| {e:.2e}, against the other chain's matrix {cross:.1e}")
        assert (it[r], fl[r]) == (itr, 0) and e < 1e-10 and cross > 1e-3


@pytest.mark.parametrize("solver,restart", (("bicgstab", 0), ("gmres", 20)))
def test_estimator_device_rng_route_equals_explicit_batch(oracle, gpu, solver, restart):
    """elph_greens_update_rng goes through the same solve as the explicit-R route: the same batch gives the same bits of M⁻¹R."""
    m, P = gpu("b")
    _as(m, solver, 1e-5, 40, restart or -1)
    kw = _bounds(oracle, "b")
    seed = 0xE57
    est = greens.EstimateGreensFunction(m, 3)
    est.device_rng_(seed)
    it_d, res_d, fl_d = greens.update_(est, m, P, setup_kwargs=kw)
    est.pull_()
    R_d, X_d = est.R.copy(), est.MinvR.copy()
    batch = synth.randn(synth.batch_seed(seed, 1), est.nv * m.Ndim).reshape(est.nv, m.Ndim)
    # the batch is the one synth names, to the figure of tests/test_gpu_greens_noise.py (the device's log / sincos against numpy's are not the
    # same bits); the explicit route is fed the numbers the device drew, so that the two solves see the same right-hand sides to the bit
    assert np.abs(R_d - batch).max() < 1e-12
    it_e, res_e, fl_e = greens.update_(est, m, P, R=R_d, setup_kwargs=kw)
    assert np.array_equal(it_d, it_e) and np.array_equal(fl_d, fl_e) and np.array_equal(res_d, res_e) and not fl_d.any()
    assert np.array_equal(est.MinvR, X_d) and X_d.any()


# ------------------------------------------------------------------------------------------ 4-8: trajectories against the CG route

def _hmc_model(name, solver, tol, maxiter=20000):
    m = configs.make_model(name, tol=tol, maxiter=maxiter)
    if m.kind == models.SSH:
        m.alpha2[:] = 0.01
        m.omega4 = np.full(m.Nph, 0.02)
        models.update_model_(m)
    else:
        m.omega4[:] = 0.02
    _as(m, *((SOLVERS[solver][0], tol, maxiter, SOLVERS[solver][1])))
    fa = prec.FourierAccelerator(m)
    return m, fa


def _hmc_randoms(m, nt, seed, with_kpm, u):
    return dict(R=synth.randn(seed, m.Ndof), Rp=synth.randn(seed + 1, m.Ndim), Rm=synth.randn(seed + 2, m.Ndim),
                kpm_randn=synth.randn(seed + 3, (nt + 2) * 2 * m.Nsites) if with_kpm else None, u=u)


HMC_NT, HMC_DT, HMC_U = 3, 0.05, 0.5


def _hmc_run(name, nb, with_kpm, solver, tol, u=HMC_U, maxiter=20000):
    """One update from the configuration's own field -> dict(x, v, x0, H0, H1, P_accept, accepted, flag, iters)."""
    m, fa = _hmc_model(name, solver, tol, maxiter)
    prec.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
    H = hmc.HybridMonteCarlo(m, fa, HMC_DT, HMC_NT * HMC_DT, alpha=0.0, Nb=nb)
    x0 = m.x.copy()
    P = _P(m) if with_kpm else None
    acc, its = hmc.update_(m, H, fa, P, randoms=_hmc_randoms(m, HMC_NT, 5100, with_kpm, u))
    out = dict(x=m.x.copy(), v=H.v.copy(), x0=x0, H0=H.H0, H1=H.H1, P_accept=H.P_accept, accepted=acc, flag=H.flag, iters=its)
    m.close()
    return out


def _langevin_run(name, scheme, solver, tol):
    """One preconditioned step -> (displacement, flag, iters)."""
    m, fa = _hmc_model(name, solver, tol)
    prec.update_Q_(fa, m, 0.0, np.inf, 0.7)
    dyn = [langevin.EulerDynamics, langevin.RungeKuttaDynamics, langevin.HeunsDynamics][scheme](m, fa, 0.01)
    x0 = m.x.copy()
    rnd = dict(eta=synth.randn(5200, m.Ndof), g1=synth.randn(5201, m.Ndim), g2=synth.randn(5202, m.Ndim),
               kpm_randn=synth.randn(5203, 4 * m.Nsites))
    it = langevin.evolve_(m, dyn, fa, _P(m), randoms=rnd)
    out = (m.x - x0, dyn.flag, it)
    m.close()
    return out


SPECIAL_MOVES = {"reflect": (hmc.REFLECT, 5, 0), "swap": (hmc.SWAP, 2, 3)}


def _special_run(move, solver, tol, u):
    """One preconditioned special move on b -> dict(accepted, S0, S1, x, flag)."""
    m, fa = _hmc_model("b", solver, tol)
    prec.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
    H = hmc.HybridMonteCarlo(m, fa, 0.05, 0.1)
    kind, ci, cj = SPECIAL_MOVES[move]
    rnd = dict(Rp=synth.randn(5300, m.Ndim), Rm=synth.randn(5301, m.Ndim), kpm_randn=synth.randn(5302, 2 * m.Nsites), u=u)
    acc, S0, S1, it, fl = hmc.special_move_(m, H, kind, ci, cj, P=_P(m), randoms=rnd)
    H.pull_()
    out = dict(accepted=acc, S0=S0, S1=S1, x=m.x.copy(), flag=fl, iters=it)
    m.close()
    return out


HMC_CASES = (("b", 1), ("b", 3), ("d", 1), ("e", 1))
LANGEVIN_CASES = tuple((name, scheme) for name in ("b", "e") for scheme in (0, 1, 2))


def _measure_cg_sensitivity():
    """The CG route at tol = 1e-6 against tol = 1e-7 on the inputs of the trajectory tests -> the dict MEASURED is a print-out of."""
    out = {}
    for name, nb in HMC_CASES:
        for with_kpm in (True, False):
            a, b = _hmc_run(name, nb, with_kpm, "cg", 1e-6), _hmc_run(name, nb, with_kpm, "cg", 1e-7)
            out[f"hmc-{name}-nb{nb}-{'P' if with_kpm else 'bare'}"] = (_rel(a["x"], b["x"]), abs(a["H1"] - b["H1"]))
    for name, scheme in LANGEVIN_CASES:
        a, b = _langevin_run(name, scheme, "cg", 1e-6), _langevin_run(name, scheme, "cg", 1e-7)
        out[f"langevin-{name}-{scheme}"] = (_rel(a[0], b[0]), 0.0)
    return out


# key -> (|Δx| / |x| — Langevin: of the step's displacement —, |ΔH₁| — special moves: |ΔS₁|) between the CG route's tol = 1e-6 and 1e-7
MEASURED = {
    "hmc-b-nb1-P": (2.26e-09, 2.76e-07), "hmc-b-nb1-bare": (1.56e-08, 2.96e-06),
    "hmc-b-nb3-P": (2.26e-09, 2.76e-07), "hmc-b-nb3-bare": (1.57e-08, 2.98e-06),
    "hmc-d-nb1-P": (2.42e-09, 4.09e-08), "hmc-d-nb1-bare": (1.25e-08, 1.72e-06),
    "hmc-e-nb1-P": (1.17e-10, 6.28e-08), "hmc-e-nb1-bare": (7.78e-10, 5.30e-07),
    "langevin-b-0": (1.84e-07, 0.0), "langevin-b-1": (9.65e-08, 0.0), "langevin-b-2": (1.15e-07, 0.0),
    "langevin-e-0": (4.46e-09, 0.0), "langevin-e-1": (4.50e-09, 0.0), "langevin-e-2": (7.98e-09, 0.0),
}


def _first_solve_flags(oracle, name, solver):
    """What the reference's ldiv! says about the first un-preconditioned solve of the update, Mᵀ y = Λϕ₊ = MᵀR₊ at tol² (H₀), on the CPU."""
    S = ref.setup(oracle, name)
    Rp = synth.randn(5101, S.n)
    kind, restart = ("bicgstab", 0) if solver == "bicgstab" else ("gmres", 20)
    return ref.mldiv(kind, S.M.T, S.M.T @ Rp, np.zeros(S.n), 1e-12, 4000, restart, None)[3]


@pytest.mark.parametrize("solver", ("bicgstab", "gmres"))
@pytest.mark.parametrize("with_kpm", (True, False), ids=("P", "bare"))
@pytest.mark.parametrize("name,nb", HMC_CASES)
def test_hmc_update_against_the_cg_route(oracle, name, nb, with_kpm, solver):
    """The CG route's own tol = 1e-6 against 1e-7 on these inputs, measured on an MI355X (MEASURED): |Δx|/|x| 2.3e-9 (b, both Nb), 2.4e-9
    (d), 1.2e-10 (e) with the preconditioner and 1.6e-8, 1.3e-8, 7.8e-10 without; |ΔH₁| 2.8e-7, 4.1e-8, 6.3e-8 and 3.0e-6, 1.7e-6, 5.3e-7.
    The bound is ALLOW = 10 times that.  What the one-sided routes gave against CG at 1e-6 when the bound was set: |Δx|/|x| between 1.6e-10
    and 3.9e-9 preconditioned (|ΔH₁| up to 5.5e-7), 2.9e-8 (d) and 5.2e-9 (e) for the bare GMRES(20) (|ΔH₁| 2.7e-6, 9.5e-7) — the closest
    to its bound is e bare, 5.2e-9 against 7.8e-9."""
    key = f"hmc-{name}-nb{nb}-{'P' if with_kpm else 'bare'}"
    dx, dH = MEASURED[key]
    if not with_kpm and (name == "b" or solver == "bicgstab"):
        # the reference's own first solve does not deliver (see the module docstring): the update is killed
        assert _first_solve_flags(oracle, name, solver) > 0
        r = _hmc_run(name, nb, False, solver, 1e-6, maxiter=4000)
        print(f"{key} {solver}: flag {r['flag']}, accepted {r['accepted']}, P_accept {r['P_accept']}")
        assert r["flag"] > 0 and not r["accepted"] and r["P_accept"] == 0.0 and np.array_equal(r["x"], r["x0"])
        return
    cg, one = _hmc_run(name, nb, with_kpm, "cg", 1e-6), _hmc_run(name, nb, with_kpm, solver, 1e-6)
    ex, eH = _rel(one["x"], cg["x"]), abs(one["H1"] - cg["H1"])
    print(f"{key} {solver}: |Δx|/|x| {ex:.2e} (bound {ALLOW * dx:.2e}), |ΔH1| {eH:.2e} (bound {ALLOW * dH:.2e}), iters {one['iters']} (CG {cg['iters']}), "
          f"P_accept {one['P_accept']:.6f} (CG {cg['P_accept']:.6f}), u {HMC_U}")
    assert cg["flag"] == 0 and one["flag"] == 0
    assert abs(cg["P_accept"] - HMC_U) > ALLOW * dH                          # u is away from the decision by more than the bound
    assert one["accepted"] == cg["accepted"]
    assert ex < ALLOW * dx and eH < ALLOW * dH


@pytest.mark.parametrize("solver", ("bicgstab", "gmres"))
@pytest.mark.parametrize("name,scheme", LANGEVIN_CASES)
def test_langevin_step_against_the_cg_route(name, scheme, solver):
    """One preconditioned step of Euler (0), Runge-Kutta (1), Heun (2); the bound on the displacement is ALLOW x MEASURED."""
    dx = MEASURED[f"langevin-{name}-{scheme}"][0]
    (d_cg, fl_cg, it_cg), (d_one, fl_one, it_one) = _langevin_run(name, scheme, "cg", 1e-6), _langevin_run(name, scheme, solver, 1e-6)
    e = _rel(d_one, d_cg)
    print(f"langevin {name} scheme {scheme} {solver}: displacement differs by {e:.2e} (bound {ALLOW * dx:.2e}), iters {it_one} (CG {it_cg})")
    assert fl_cg == 0 and fl_one == 0 and e < ALLOW * dx


@pytest.mark.parametrize("move", tuple(SPECIAL_MOVES))
def test_special_moves_against_the_cg_route(move):
    """One reflection and one swap move on b with GMRES and the LeftRight preconditioner: the same decisions as the CG route, accepted
    (u = 0) and rejected (u = 1.5); the fields to the bound of the HMC test on b (a move permutes or negates world lines: they are in fact
    the same bits).  The actions as tests/test_gpu_hmc.py's assert_special_actions holds them against its references: S₀ is closed, to
    1e-11; S₁ holds two solves, to 1e-8 (CG's own S₁ does not move at all between tol = 1e-6 and 1e-7 — its error in bᵀx is of second
    order in the residual — so that difference cannot serve as a yardstick here)."""
    from test_gpu_hmc import assert_special_actions
    dx = MEASURED["hmc-b-nb1-P"][0]
    for u in (0.0, 1.5):
        cg, one = _special_run(move, "cg", 1e-6, u), _special_run(move, "gmres", 1e-6, u)
        print(f"{move} u {u}: S1 {one['S1']:.12e} (CG {cg['S1']:.12e}), S0 {one['S0']:.12e} (CG {cg['S0']:.12e}), accepted {one['accepted']}, "
              f"iters {one['iters']} (CG {cg['iters']})")
        assert cg["flag"] == 0 and one["flag"] == 0 and one["accepted"] == cg["accepted"] == (u == 0.0)
        assert_special_actions(one["S0"], one["S1"], cg["S0"], cg["S1"])
        assert _rel(one["x"], cg["x"]) < ALLOW * dx and np.array_equal(one["x"], cg["x"])


def test_reject_restores_x_bit_exactly(oracle):
    r = _hmc_run("b", 1, True, "gmres", 1e-6, u=1.0)
    assert not r["accepted"] and r["flag"] == 0 and 0.0 < r["P_accept"] <= 1.0 and np.array_equal(r["x"], r["x0"])
    r = _hmc_run("e", 1, True, "bicgstab", 1e-6, u=1.5)
    assert not r["accepted"] and r["flag"] == 0 and np.array_equal(r["x"], r["x0"])


# ------------------------------------------------------------------------------------------ 5: chains in lockstep

def _chain_inputs(m, nch, nt, name):
    X0 = src.chain_fields(ref.host_model(name), nch)
    V0 = np.stack([0.3 * synth.randn(950 + c, m.Ndof) for c in range(nch)])
    rnd = dict(R=np.stack([synth.randn(1000 + c, m.Ndof) for c in range(nch)]),
               Rp=np.stack([synth.randn(1100 + c, m.Ndim) for c in range(nch)]),
               Rm=np.stack([synth.randn(1200 + c, m.Ndim) for c in range(nch)]),
               kpm_randn=synth.randn(1300, (nt + 2) * 2 * nch * m.Nsites).reshape(nt + 2, 2, nch, m.Nsites),
               u=np.array([0.0 if c % 2 == 0 else 1.5 for c in range(nch)]))
    return X0, V0, rnd


@pytest.mark.parametrize("name,nch,solver", (("b", 3, "gmres"), ("e", 2, "gmres"), ("b", 3, "bicgstab")))
def test_chains_in_lockstep_equal_single_chain_updates(name, nch, solver):
    from test_gpu_hmc import assert_chain_ends_as_the_single_chain, chain_randoms
    nt, dt = 3, 0.05

    def make(nchains):
        m, fa = _hmc_model(name, solver, 1e-9)
        prec.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
        return m, fa

    m, fa = make(nch)
    X0, V0, rnd = _chain_inputs(m, nch, nt, name)
    H = hmc.HybridMonteCarlo(m, fa, dt=dt, tr=nt * dt, alpha=0.2, Nb=1, nchains=nch)
    H.X[:], H.V[:] = X0, V0
    H.push_()
    acc, its = hmc.update_chains_(m, H, fa, _P(m), randoms=rnd, pull=True)
    assert not H.flags.any() and (its > 0).all()
    Xb, Vb, Eb = H.X.copy(), H.V.copy(), H.energies.copy()
    m.close()
    for c in range(nch):
        m1, fa1 = make(1)
        m1.x[:] = X0[c]
        if m1.kind == models.SSH:
            models.update_model_(m1)
        H1 = hmc.HybridMonteCarlo(m1, fa1, dt=dt, tr=nt * dt, alpha=0.2, Nb=1)
        H1.v[:] = V0[c]
        H1.push_()
        a1, i1 = hmc.update_(m1, H1, fa1, _P(m1), randoms=chain_randoms(rnd, c, True))
        assert_chain_ends_as_the_single_chain(c, a1, i1, m1, H1, acc, its, Xb, Vb, Eb, X0)
        m1.close()
    assert acc[0] and not acc[1]


def test_chain_whose_solve_fails_is_rejected_alone():
    """Chain 1's field makes exp(-Δτ V) span hundreds of orders of magnitude: its preconditioned GMRES solves and their un-preconditioned
    retries run out; chains 0 and 2 end where they end alone."""
    name, nch, nt, dt = "b", 3, 3, 0.05

    def make():
        m, fa = _hmc_model(name, "gmres", 1e-7, maxiter=40)
        prec.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
        return m, fa

    m, fa = make()
    X0 = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=900 + c) for c in range(nch)])
    X0[1] *= 40.0
    rnd = dict(R=np.stack([synth.randn(1000 + c, m.Ndof) for c in range(nch)]),
               Rp=np.stack([synth.randn(1100 + c, m.Ndim) for c in range(nch)]),
               Rm=np.stack([synth.randn(1200 + c, m.Ndim) for c in range(nch)]),
               kpm_randn=synth.randn(1300, (nt + 2) * 2 * nch * m.Nsites).reshape(nt + 2, 2, nch, m.Nsites), u=np.zeros(nch))
    H = hmc.HybridMonteCarlo(m, fa, dt=dt, tr=nt * dt, alpha=0.0, Nb=1, nchains=nch)
    H.X[:] = X0
    H.push_()
    acc, its = hmc.update_chains_(m, H, fa, _P(m), randoms=rnd, pull=True)
    print(f"flags {H.flags}, accepted {acc}, iters {its}")
    assert H.flags[1] > 0 and not acc[1] and H.flags[0] == 0 and H.flags[2] == 0 and acc[0] and acc[2]
    assert np.array_equal(H.X[1], X0[1]) and H.energies[1, 4] == 0.0
    Xb, Vb = H.X.copy(), H.V.copy()
    m.close()
    for c in (0, 2):
        m1, fa1 = make()
        m1.x[:] = X0[c]
        H1 = hmc.HybridMonteCarlo(m1, fa1, dt=dt, tr=nt * dt, alpha=0.0, Nb=1)
        r1 = dict(R=rnd["R"][c], Rp=rnd["Rp"][c], Rm=rnd["Rm"][c], kpm_randn=np.ascontiguousarray(rnd["kpm_randn"][:, :, c, :]), u=0.0)
        a1, i1 = hmc.update_(m1, H1, fa1, _P(m1), randoms=r1)
        assert a1 and np.abs(m1.x - Xb[c]).max() < 1e-6 * np.abs(m1.x).max() and np.abs(H1.v - Vb[c]).max() < 1e-6 * np.abs(H1.v).max()
        m1.close()


# ------------------------------------------------------------------------------------------ 9: the zero-guess start

def _exact_lambda_model(name):
    """The configuration with λ = λ₂ = 0 (Holstein): Λ ≡ 1, so Λϕ± on the device and on the host are the same bits (a shift and a sign) and
    the stage-by-stage route is fed exactly the pair solve's right-hand sides.  Bond phonons have Λ ≡ 1 as they are."""
    m = configs.make_model(name)
    if m.kind == models.HOLSTEIN:
        m.lam[:], m.lam2[:] = 0.0, 0.0
    models.update_model_(m)
    return m


@pytest.mark.parametrize("solver,restart", cc.SOLVERS)
@pytest.mark.parametrize("name,use_prec", (("b", True), ("e", True), ("t", True), ("b", False), ("e", False)), ids=lambda v: {True: "P", False: "bare"}.get(v, v))
def test_zero_guess_start_keeps_every_bit(name, use_prec, solver, restart):
    """calc_OinvLambda_phi (its stages skip the mat-vec on the zero guess) against ldiv_batched_ stage by stage (transposed, then not; X
    zeroed by the caller; the guess is taken as given there: A·0 is computed): identical iterations, flags and bits of x.  The bare runs
    stop at solver.maxiter = 8: flags, zeroed vectors and the fold that is not halved are compared too."""
    m = _exact_lambda_model(name)
    _as(m, solver, 1e-5, 40 if use_prec else 8, restart or -1)
    P = prec.LeftRightKPMPreconditioner(m) if use_prec else None
    kw = dict(b_max=synth.randn(5401, m.Nsites), b_min=synth.randn(5402, m.Nsites)) if use_prec else {}
    phi_p, phi_m = cc.phis(m.Ndim)
    Xp, Xm, it, fl = hmc.calc_OinvLambda_phi(m, phi_p, phi_m, P, setup_kwargs=kw)
    prec.setup_(P, **kw)
    B = np.ascontiguousarray(np.stack([cc.mulLambda(m, phi_p), cc.mulLambda(m, phi_m)]))
    Y, X = np.zeros_like(B), np.zeros_like(B)
    models.transpose_(m)
    it1, _, fl1 = models.ldiv_batched_(Y, m, B, P)
    models.transpose_(m)
    it2, _, fl2 = models.ldiv_batched_(X, m, Y, P)
    want = cc.fold([it1.tolist(), it2.tolist()], [fl1.tolist(), fl2.tolist()])
    if max(fl1[0], fl2[0]) > 0:
        X[1] = 0.0
    print(f"{name} {solver}{restart or ''} {'P' if use_prec else 'bare'}: stages {it1} {it2}, flags {fl1} {fl2}; pair {it}, {fl}")
    assert (it, fl) == want and (fl == 0) == use_prec
    assert np.array_equal(Xp, X[0]) and np.array_equal(Xm, X[1]) and (X[0].any() or not use_prec)
    m.close()


# ------------------------------------------------------------------------------------------ 10: refusals

def test_preconditioner_of_the_wrong_family_is_refused(gpu):
    m, P = gpu("b")
    _as(m, "gmres", 1e-5, 40, 20)
    sym = prec.SymmetricKPMPreconditioner(m, expansion=P)
    fa = prec.FourierAccelerator(m)
    phi = cc.phis(m.Ndim)
    est = greens.EstimateGreensFunction(m, 2)
    with pytest.raises(ValueError):
        hmc.calc_OinvLambda_phi(m, *phi, sym, setup_kwargs=dict(e_min=0.1, e_max=1.9))
    with pytest.raises(ValueError):
        greens.update_(est, m, sym, R=_noise(m.Ndim, 2))
    with pytest.raises(ValueError):
        langevin.evolve_(m, None, fa, sym, randoms={})
    with pytest.raises(ValueError):
        hmc.calc_dSfdx_(np.zeros(m.Ndof), m, *phi, P=sym)
    H = SimpleNamespace(Ndof=m.Ndof, device_rng=False, dt=0.05, Nt=2, Nb=1, alpha=0.0, nchains=1)      # (refused before the library is reached)
    with pytest.raises(ValueError):
        hmc.update_(m, H, fa, sym, randoms={})
    with pytest.raises(ValueError):
        hmc.special_move_(m, H, hmc.REFLECT, 0, P=sym, randoms={})
    # a fixed side cannot serve the callers, which solve with Mt and then with M
    with pytest.raises(ValueError):
        hmc.calc_OinvLambda_phi(m, *phi, prec.LeftKPMPreconditioner(m, expansion=P), setup_kwargs=dict(e_min=0.1, e_max=1.9))
    # a CG model refuses the one-sided ones the same way
    _as(m, "cg", 1e-5, 40)
    for bad in (P, prec.LeftKPMPreconditioner(m, expansion=P)):
        with pytest.raises(ValueError):
            hmc.calc_OinvLambda_phi(m, *phi, bad, setup_kwargs=dict(e_min=0.1, e_max=1.9))
        with pytest.raises(ValueError):
            greens.update_(est, m, bad, R=_noise(m.Ndim, 2))
        with pytest.raises(ValueError):
            langevin.evolve_(m, None, fa, bad, randoms={})
    # ... and still solves
    it, res, fl = greens.update_(est, m, None, R=_noise(m.Ndim, 2))
    assert not fl.any()


def test_one_sided_callers_refuse_a_sharded_handle():
    """The handle as the one rank of a sharded lattice (a slab handle takes the same line of need_ready; no entry point hands one out):
    ELPH_E_STATE naming the solver, from the estimator and from the force call; the CG kind is not refused there; after
    elph_shard_destroy the handle solves again."""
    import ctypes as C
    m = _as(configs.make_model("b"), "gmres", 1e-5, 40, 20)
    est = greens.EstimateGreensFunction(m, 2)
    R = _noise(m.Ndim, 2)
    it, _, fl = greens.update_(est, m, None, R=R)
    X_ok = est.MinvR.copy()
    N = m.Nsites
    gs, key = np.arange(N, dtype=np.int64), (C.c_ubyte * 64)()
    _lib.check(m._lib.elph_shard_create(m._h, 0, 1, 0, N, 0, 0, 0, N, 0, _lib.iptr(gs), C.cast(key, C.c_void_p)))
    for solver, word in (("gmres", "GMRES"), ("bicgstab", "BiCGStab")):
        _as(m, solver, 1e-5, 40, 20 if solver == "gmres" else -1)
        with pytest.raises(Exception, match=word) as info:
            greens.update_(est, m, None, R=R)
        assert "ELPH_E_STATE" in str(info.value)
        with pytest.raises(Exception, match=word) as info:
            hmc.calc_OinvLambda_phi(m, *cc.phis(m.Ndim))
        assert "ELPH_E_STATE" in str(info.value)
    _lib.check(m._lib.elph_shard_destroy(m._h))
    _as(m, "gmres", 1e-5, 40, 20)
    greens.update_(est, m, None, R=R)
    assert np.array_equal(est.MinvR, X_ok)
    m.close()


# ------------------------------------------------------------------------------------------ 11: the deck

@pytest.mark.parametrize("nchains", (1, 2))
def test_gmres_deck_builds_and_runs(nchains):
    sim = pi.process_input_file(os.path.join(DECKS, "holstein_hmc_square_L4_gmres.toml"), nchains=nchains)
    m, P = sim.model, sim.preconditioner
    assert type(P) is prec.LeftRightKPMPreconditioner and isinstance(m.solver, models.GMRES) and m.solver.restart == 20 and m.mul_by_M
    rng = np.random.default_rng(7)
    for dyn in (sim.burnin_dynamics, sim.burnin_dynamics, sim.simulation_dynamics, sim.simulation_dynamics):
        if nchains > 1:
            acc, its = hmc.update_chains_(m, dyn, sim.fa, P, rng=rng)
            print(f"chains: accepted {acc}, iters {its}, flags {dyn.flags}")
            assert not dyn.flags.any() and (its > 0).all()
        else:
            acc, its = hmc.update_(m, dyn, sim.fa, P, rng=rng)
            print(f"accepted {acc}, iters {its}, flag {dyn.flag}")
            assert dyn.flag == 0 and its > 0
    it, res, fl = greens.update_(sim.Gr, m, P, rng=rng)
    print(f"estimator: iters {it}, residuals {res}")
    assert not fl.any() and (it > 0).all() and sim.Gr.nv == 3 * nchains and np.all(res < np.sqrt(m.solver.tol))
    m.close()
