"""BiCGStab, GMRES and the one-sided KPM preconditioners without a device: tests/msolver_reference.py checks itself against the oracle on
the configurations b, t, e, d, and the host side of the library (constructors, defaults, the solver / preconditioner pairing) is held to
the reference's rules.

What the stop rules control.  BiCGStab tests the TRUE residual |b - A x| / |b| (of its recurrence), so a converged solve has a true residual
below tol.  GMRES with a preconditioner tests the PRECONDITIONED residual |P (b - A x)| / |P b| (IterativeSolvers.jl:485-496, :529); its true
residual is of the order of tol — measured here: between 0.16 tol and 1.8 tol on these inputs — and is held to what ldiv! asks, sqrt(tol)
(Models.jl:100).
"""
import numpy as np
import pytest

from elphdynamics_amd import lattice as lat, models, preconditioners as prec
import msolver_reference as ref

F64_DOTS = ("sequential", "pairwise", "blas")


@pytest.mark.parametrize("name", ref.MODELS)
def test_left_after_right_is_the_symmetric_apply(oracle, name):
    from elphdynamics_amd import synth
    S = ref.setup(oracle, name)
    assert S.K["active"]
    for seed in (5, 6):
        v = np.ascontiguousarray(synth.randn(seed, S.n))
        want = oracle.kpm_apply(S.oP, v)
        got = S.side(False) @ (S.side(True) @ v)
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"{name} seed {seed}: |Left(Right(v)) - kpm_apply(v)| / |.| = {err:.2e}")
        assert err < 1e-12
    # the two sides are each other's transposes (the Right one takes conj(c) and A'^T)
    assert np.linalg.norm(S.side(True) - S.side(False).T) < 1e-12 * np.linalg.norm(S.side(False))


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_preconditioned_cases_deliver(oracle, case):
    name, op, solver, restart, tol, maxiter = case
    assert tol in ref.TOLS
    S = ref.setup(oracle, name)
    A, P = S.A(op), S.P(op)
    runs = {dot: S.solve(case, dot=dot) for dot in F64_DOTS + ("longdouble",)}
    its = {dot: r[1] for dot, r in runs.items()}
    margins = {dot: r[2] for dot, r in runs.items()}
    x = np.asarray(runs["blas"][0], dtype=np.float64)
    res = np.linalg.norm(A @ x - S.b) / np.linalg.norm(S.b)
    pres = np.linalg.norm(P @ (A @ x - S.b)) / np.linalg.norm(P @ S.b)
    spread = max(np.linalg.norm(np.asarray(runs[d][0], dtype=np.float64) - np.asarray(runs["longdouble"][0], dtype=np.float64)) for d in F64_DOTS) / np.linalg.norm(x)
    print(f"{ref.case_id(case)}: iters {its}, margins {margins}, true residual {res:.3e}, preconditioned {pres:.3e}, spread {spread:.1e}")
    assert len(set(its.values())) == 1 and 1 <= its["blas"] <= 20
    assert min(margins.values()) >= ref.MARGIN
    if solver == "bicgstab":
        assert res < tol
    else:
        assert pres < tol * (1 + 1e-6) and res < np.sqrt(tol)
    assert spread < 1e-12
    if restart == 4:
        restarts = ref.gmres(A, S.b, np.zeros(S.n), tol, maxiter, maxiter, restart, P)[3]
        assert restarts >= ref.RESTARTS_MIN[name], restarts


@pytest.mark.parametrize("case", ref.LONG_CASES, ids=ref.case_id)
def test_long_unpreconditioned_gmres(oracle, case):
    name, op, solver, restart, tol, maxiter = case
    S = ref.setup(oracle, name)
    runs = {dot: S.solve(case, prec=False, dot=dot) for dot in F64_DOTS}
    its = {dot: r[1] for dot, r in runs.items()}
    print(f"{ref.case_id(case)}: iters {its}, margins {[r[2] for r in runs.values()]}")
    assert len(set(its.values())) == 1 and 200 <= its["blas"] <= 300
    assert min(r[2] for r in runs.values()) >= ref.MARGIN
    assert max(np.linalg.norm(runs[d][0] - runs["blas"][0]) for d in F64_DOTS) < 1e-12 * np.linalg.norm(runs["blas"][0])


def test_unpreconditioned_bicgstab_is_sensitive_beyond_a_few_iterations(oracle):
    """Why the GPU test of the bare iteration stops at 5: the float64 summation orders agree there, and no longer at 20."""
    S = ref.setup(oracle, "b")
    x5 = [np.asarray(ref.bicgstab(S.M, S.b, np.zeros(S.n), 1e-30, 5, None, dot)[0], dtype=np.float64) for dot in F64_DOTS]
    assert max(np.linalg.norm(a - x5[0]) for a in x5) < 1e-8 * np.linalg.norm(x5[0])


# ------------------------------------------------------------------------------------------ host logic

class _HostHolstein(models.HolsteinModel):
    def _create(self, *a, **k):
        pass

    def _push_solver(self):
        raise AssertionError("the handle was reached")


class _HostSSH(models.SSHModel):
    def _create(self, *a, **k):
        pass


def _sided(cls, model):
    P = object.__new__(cls)
    P.model = model
    return P


def test_solver_defaults_are_the_references():
    g = models.GMRES(1000)
    assert (g.tol, g.maxiter, g.restart) == (1e-4, 1000, 20)
    assert models.GMRES(7).restart == 7 and models.GMRES(7, maxiter=3, restart=2).restart == 2 and models.GMRES(7, maxiter=3).maxiter == 3
    b = models.BiCGStab(50, tol=1e-6, maxiter=12)
    assert (b.tol, b.maxiter) == (1e-6, 12) and models.BiCGStab(50).tol == 1e-4


@pytest.mark.parametrize("cls", (_HostHolstein, _HostSSH))
def test_constructor_keywords_choose_the_solver(cls):
    L = lat.Lattice(1, 4, 4, 1)
    m = cls(L, 2.0, 0.1)
    assert isinstance(m.solver, models.ConjugateGradient) and m.mul_by_M is False and m.transposed is False
    m = cls(L, 2.0, 0.1, tol=1e-6, maxiter=77, solver="GMRES")
    assert isinstance(m.solver, models.GMRES) and m.mul_by_M is True
    assert (m.solver.tol, m.solver.maxiter, m.solver.restart) == (1e-6, 77, 20)
    m = cls(L, 2.0, 0.1, solver="gmres", restart=4)
    assert m.solver.restart == 4
    m = cls(L, 2.0, 0.1, tol=1e-6, maxiter=77, solver="BiCGStab")
    assert isinstance(m.solver, models.BiCGStab) and m.mul_by_M is True and (m.solver.tol, m.solver.maxiter) == (1e-6, 77)
    with pytest.raises(ValueError):
        cls(L, 2.0, 0.1, solver="minres")


def test_solver_and_preconditioner_must_match():
    L = lat.Lattice(1, 4, 4, 1)
    cg, gm = _HostHolstein(L, 2.0, 0.1), _HostHolstein(L, 2.0, 0.1, solver="GMRES")
    x, b = np.zeros(cg.Ndim), np.ones(cg.Ndim)
    for cls in (prec.LeftKPMPreconditioner, prec.RightKPMPreconditioner, prec.LeftRightKPMPreconditioner):
        with pytest.raises(ValueError):
            models.ldiv_(x, cg, b, _sided(cls, cg))
        with pytest.raises(ValueError):
            models.ldiv_batched_(x.reshape(1, -1), cg, b.reshape(1, -1), _sided(cls, cg))
    sym = _sided(prec.SymmetricKPMPreconditioner, gm)
    with pytest.raises(ValueError):
        models.ldiv_(x, gm, b, sym)
    with pytest.raises(ValueError):
        models.solve_(x, gm, b, P=sym)
    # the device solvers pair M with Left and Mt with Right; LeftRight follows model.transposed
    with pytest.raises(ValueError):
        models.ldiv_(x, gm, b, _sided(prec.RightKPMPreconditioner, gm))
    lr = _sided(prec.LeftRightKPMPreconditioner, gm)
    assert lr.side_for(gm) is False and models._use_prec(lr, gm) == 1 and models._use_prec(_sided(prec.LeftKPMPreconditioner, gm), gm) == 1
    models.transpose_(gm)
    assert lr.side_for(gm) is True and models._use_prec(lr, gm) == 1 and models._use_prec(_sided(prec.RightKPMPreconditioner, gm), gm) == 1
    with pytest.raises(ValueError):
        models._use_prec(_sided(prec.LeftKPMPreconditioner, gm), gm)


def test_cut_cycle_difference_is_documented(oracle):
    """solver.maxiter = 5 < restart = 20 without a preconditioner: solve! as written back-substitutes over 20 columns of which 15 were never
    written (0/0: a non-finite x, which ldiv! would pass with flag 0 since NaN > sqrt(tol) is false); the library's rule updates x with the 5
    columns built — the minimiser over the 5-dimensional Krylov space, so the residual does not exceed the initial one."""
    S = ref.setup(oracle, "t")
    x0 = np.zeros(S.n)
    xe, ite, _, _ = ref.gmres(S.M, S.b, x0, 1e-5, 5, 5, 20, as_executed=True)
    xl, itl, _, _ = ref.gmres(S.M, S.b, x0, 1e-5, 5, 5, 20)
    assert ite == itl == 5
    assert not np.all(np.isfinite(xe))
    assert np.all(np.isfinite(xl)) and np.linalg.norm(S.M @ xl - S.b) < np.linalg.norm(S.b)
    # five steps of one long cycle are the same five columns
    x5 = ref.gmres(S.M, S.b, x0, 1e-30, 5, 5, 5)[0]
    assert np.linalg.norm(xl - x5) < 1e-13 * np.linalg.norm(x5)
    # a multiple of restart: the two rules coincide
    a = ref.gmres(S.M, S.b, x0, 1e-30, 8, 8, 4, as_executed=True)[0]
    b = ref.gmres(S.M, S.b, x0, 1e-30, 8, 8, 4)[0]
    assert np.array_equal(a, b)
    # the call maxiter below solver.maxiter does not cut the cycle: iters exceeds it
    assert ref.gmres(S.M, S.b, x0, 1e-30, 5, 40, 20)[1] == 20
