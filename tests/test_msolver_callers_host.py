"""The callers of BiCGStab and GMRES without a device: the case table of tests/msolver_caller_cases.py is held to its own rules (every
stage of every case stops with a log-margin >= ref.MARGIN at the tolerance the table names; the stage-2 sensitivity KAPPA the table names
is what the reference gives), the restated fold of iterations and flags reproduces HMC.jl:851-909 on hand-made inputs, and the deck
reader hands a GMRES deck's solver and preconditioner on.
"""
import os

import numpy as np
import pytest

from elphdynamics_amd import models, preconditioners as prec, process_input as pi
import msolver_caller_cases as cc
import msolver_reference as ref

F64_DOTS = ("sequential", "pairwise", "blas")
DECKS = os.path.join(os.path.dirname(__file__), "decks")


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_every_stage_of_every_case_delivers(oracle, case):
    name, solver, restart, use_prec, tol, maxiter, k = case
    assert tol in ref.TOLS and use_prec
    S = ref.setup(oracle, name)
    counts = set()
    for dot in F64_DOTS:
        row = []
        for b in cc.rhs_pair(S):
            y, it1, res1, fl1 = cc.stage(S, solver, restart, tol, maxiter, b, True, dot=dot)
            i1, m1 = cc.stage_margin(S, solver, restart, tol, maxiter, b, True, dot=dot)
            i2, m2 = cc.stage_margin(S, solver, restart, tol, maxiter, y, False, dot=dot)
            print(f"{cc.case_id(case)} {dot}: stage 1 {i1} iterations, margin {m1:.3f}; stage 2 {i2}, margin {m2:.3f}")
            assert fl1 == 0 and it1 == i1 and 1 <= i1 <= 20 and 1 <= i2 <= 20
            assert min(m1, m2) >= ref.MARGIN
            row += [i1, i2]
        counts.add(tuple(row))
    assert len(counts) == 1                              # the summation order does not move a stop
    p = cc.pair(S, solver, restart, tol, maxiter)
    assert p["flag"] == 0 and p["iters"] == -(-sum(p["it"][0] + p["it"][1]) // 2)
    for s, b in enumerate(cc.rhs_pair(S)):               # the chained solution is O⁻¹ b = (MᵀM)⁻¹ b to the solvers' tolerance
        direct = np.linalg.solve(S.M.T @ S.M, b)
        assert np.linalg.norm(p["X"][s] - direct) < 1e-2 * np.linalg.norm(direct)


@pytest.mark.parametrize("name", ref.MODELS)
def test_stage_two_sensitivity_is_what_the_table_says(oracle, name):
    S = ref.setup(oracle, name)
    for case in cc.CASES:
        if case[0] != name:
            continue
        _, solver, restart, use_prec, tol, maxiter, k = case
        got = cc.kappa(S, solver, restart, tol, maxiter, use_prec)
        print(f"{cc.case_id(case)}: kappa {got:.3f} (table {k}), tolerance of the composed solution {cc.x_tolerance(k):.2e}")
        assert k < 1e3 and k / 2 <= got <= 2 * k


def test_bare_bicgstab_case_is_the_flagged_one(oracle):
    name, solver, restart, use_prec, tol, maxiter, k = cc.BARE_CASE
    assert (name, solver, use_prec, k) == ("t", "bicgstab", False, None) and tol in ref.TOLS
    S = ref.setup(oracle, name)
    for dot in F64_DOTS:
        for b in cc.rhs_pair(S):
            x, it, res, fl = cc.stage(S, solver, restart, tol, maxiter, b, True, False, dot)
            assert (it, fl) == (maxiter, 1) and not x.any() and res > 10 * np.sqrt(tol)
    p = cc.pair(S, solver, restart, tol, maxiter, False)
    assert p["it"] == [[5, 5], [5, 5]] and p["fl"] == [[1, 1], [0, 0]] and (p["iters"], p["flag"]) == (10, 1) and not p["X"].any()
    # ... and no tolerance of the table makes the bare iteration converge on t, even with 400 iterations
    for t in ref.TOLS:
        assert cc.stage(S, solver, restart, t, 400, cc.rhs_pair(S)[0], True, False)[3] > 0


def test_fold_is_the_references():
    """HMC.jl:851-909 on hand-made (iters, flag) of [stage][sign]."""
    # both clean: everything adds up, halved (rounded up)
    assert cc.fold([[5, 6], [7, 9]], [[0, 0], [0, 0]]) == (14, 0)          # cld(27, 2)
    assert cc.fold([[4, 4], [4, 4]], [[0, 0], [0, 0]]) == (8, 0)
    # stage 1 of ϕ₊ flagged: its stage 2 still runs and counts (:869-873), ϕ₋ does not (:888), no halving
    assert cc.fold([[40, 3], [40, 3]], [[1, 0], [0, 0]]) == (80, 1)
    # stage 2 of ϕ₊ flagged
    assert cc.fold([[5, 3], [40, 3]], [[0, 0], [2, 0]]) == (45, 2)
    # both stages of ϕ₊ flagged: the larger flag
    assert cc.fold([[40, 3], [40, 3]], [[1, 0], [2, 0]]) == (80, 2)
    # ϕ₋ flagged (either stage): all four counted, not halved
    assert cc.fold([[5, 40], [7, 9]], [[0, 1], [0, 0]]) == (61, 1)
    assert cc.fold([[5, 6], [7, 40]], [[0, 0], [0, 2]]) == (58, 2)


def test_mulLambda_restatement_is_hmc_pys(oracle):
    from elphdynamics_amd import hmc
    for name in ("b", "e"):
        m = ref.host_model(name)
        Lam, v = np.zeros(m.Ndim), cc.phis(m.Ndim)[0]
        hmc.update_Lambda_(Lam, m)
        out = np.array(v)
        hmc.mulLambda_(out, v, Lam, m)
        assert np.array_equal(Lam, cc.Lambda(m)) and np.array_equal(out, cc.mulLambda(m, v))


# ------------------------------------------------------------------------------------------ the host mirror

class _HostHolstein(models.HolsteinModel):
    def _create(self, *a, **k):
        pass

    def _push_solver(self):
        raise AssertionError("the handle was reached")


def _sided(cls, model):
    P = object.__new__(cls)
    P.model = model
    return P


def test_callers_take_the_preconditioner_of_their_solver():
    from elphdynamics_amd import lattice as lat
    L = lat.Lattice(1, 4, 4, 1)
    cg, gm = _HostHolstein(L, 2.0, 0.1), _HostHolstein(L, 2.0, 0.1, solver="GMRES")
    assert models._caller_prec(None, cg) == models._caller_prec(None, gm) == 0
    assert models._caller_prec(_sided(prec.SymmetricKPMPreconditioner, cg), cg) == 1
    assert models._caller_prec(_sided(prec.LeftRightKPMPreconditioner, gm), gm) == 1
    with pytest.raises(ValueError):
        models._caller_prec(_sided(prec.SymmetricKPMPreconditioner, gm), gm)
    for cls in (prec.LeftKPMPreconditioner, prec.RightKPMPreconditioner, prec.LeftRightKPMPreconditioner):
        with pytest.raises(ValueError):
            models._caller_prec(_sided(cls, cg), cg)
    # the callers solve with Mt and with M in turn: one fixed side cannot serve both
    for cls in (prec.LeftKPMPreconditioner, prec.RightKPMPreconditioner):
        with pytest.raises(ValueError):
            models._caller_prec(_sided(cls, gm), gm)


def test_binding_knows_the_solver_kind_entry_point():
    import ctypes as C
    from elphdynamics_amd import _lib
    res, argtypes = _lib.SIGNATURES["elph_solver_set_kind"]
    assert res is C.c_int and len(argtypes) == 3
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "elph_gpu.h")).read()
    assert "#define ELPH_SOLVER_CG 0" in hdr and "int elph_solver_set_kind(elph_handle h, int solver, int restart);" in hdr
    assert models.SOLVER_CODES == {models.BiCGStab: 1, models.GMRES: 2}


# ------------------------------------------------------------------------------------------ decks

def test_solver_settings_of_the_gmres_deck():
    inp = pi.read_deck(os.path.join(DECKS, "holstein_hmc_square_L4_gmres.toml"))
    assert pi.solver_settings(inp) == ("GMRES", 1e-8, 10000, 20)
    del inp["solver"]["restart"]
    assert pi.solver_settings(inp)[3] == 20                              # the default (ProcessInputFile.jl:227-232)
    inp["solver"]["restart"] = 7
    assert pi.solver_settings(inp)[3] == 7
    cg = pi.read_deck(os.path.join(DECKS, "holstein_hmc_honeycomb_L3.toml"))
    assert pi.solver_settings(cg)[:3] == ("CG", 1e-8, 10000)


def test_deck_chooses_model_solver_and_preconditioner_class(monkeypatch):
    """The builders hand solver.type and restart to the model; initialize_preconditioner follows ProcessInputFile.jl:502-506.  Host logic
    only: the model's _create and the preconditioner's constructor are stubbed."""
    monkeypatch.setattr(models.AbstractModel, "_create", lambda self, *a, **k: None)
    monkeypatch.setattr(prec.SymmetricKPMPreconditioner, "__init__", lambda self, model, **k: setattr(self, "kw", k))
    inp = pi.read_deck(os.path.join(DECKS, "holstein_hmc_square_L4_gmres.toml"))
    m = pi.initialize_model(inp, rng=np.random.default_rng(1))
    assert isinstance(m.solver, models.GMRES) and m.mul_by_M and (m.solver.tol, m.solver.maxiter, m.solver.restart) == (1e-8, 10000, 20)
    assert m.Nsites == 16 and m.Nbonds == 32 and m.Ltau == 12
    P = pi.initialize_preconditioner(inp, m)
    assert type(P) is prec.LeftRightKPMPreconditioner and P.kw == dict(n=12, buf=0.05, c1=1.0, c2=1.0)
    inp["solver"]["type"] = "BiCGStab"
    m = pi.initialize_model(inp, rng=np.random.default_rng(1))
    assert isinstance(m.solver, models.BiCGStab) and m.mul_by_M
    assert type(pi.initialize_preconditioner(inp, m)) is prec.LeftRightKPMPreconditioner
    inp["solver"]["type"] = "cg"
    m = pi.initialize_model(inp, rng=np.random.default_rng(1))
    assert isinstance(m.solver, models.ConjugateGradient) and not m.mul_by_M
    assert type(pi.initialize_preconditioner(inp, m)) is prec.SymmetricKPMPreconditioner
    del inp["solver"]["preconditioner"]
    assert pi.initialize_preconditioner(inp, m) is None
    # a deck of the SSH family
    ssh = pi.read_deck(os.path.join(DECKS, "ssh_langevin_square_L4.toml"))
    ssh["solver"]["type"], ssh["solver"]["restart"] = "GMRES", 6
    ms = pi.initialize_model(ssh, rng=np.random.default_rng(1))
    assert isinstance(ms.solver, models.GMRES) and ms.solver.restart == 6 and ms.mul_by_M
