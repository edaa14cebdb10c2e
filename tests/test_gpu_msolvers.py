"""BiCGStab, GMRES and the one-sided KPM preconditioners on the device against tests/msolver_reference.py, on the smallest models that
reach each code path: b (4 x 4, the lane-program family), t (3 x 3 triangular, ragged colours, generic kernels, 72 unknowns), e (bond
phonons), d (honeycomb).  The expansion's bounds are injected on both sides from the oracle's Arnoldi run, so both use one expansion.

Tolerances.  One-sided apply: relative 1e-11, the figure the symmetric apply's GPU tests use.  Preconditioned solves end within 20
iterations: x to relative 1e-10 (the project's parity figure) and EQUAL iteration counts — every case has a log-margin >= 1e-2
(tests/test_msolvers_host.py).  The bare BiCGStab iteration amplifies rounding (O(1) from 20 iterations on), so it is compared after 5
iterations, to 100 x the spread of the float64 summation orders of that same case; the long un-preconditioned GMRES(20) run on t (235
iterations) is stable: equal count and x to 1e-9.  After an un-preconditioned BiCGStab retry of 20 iterations only what decides the outcome
is compared (iters, flag, the zeroed x, a residual above sqrt(tol)), not the residual's digits.
"""
import numpy as np
import pytest

from elphdynamics_amd import configs, models, preconditioners as prec, synth
import msolver_reference as ref
import stop_rule_cases as src

pytestmark = pytest.mark.gpu

F64_DOTS = ("sequential", "pairwise", "blas")


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _as(m, solver, tol, maxiter, restart=-1, transposed=False):
    """The model with the solver of a mul_by_M model (the constructor keyword's effect) and the operator M or Mt."""
    m.solver, m.mul_by_M = models.make_solver(solver, m.Ndim, tol, maxiter, restart)
    m.transposed = bool(transposed)
    return m


@pytest.fixture(scope="module")
def gpu():
    """name -> (model, LeftRight preconditioner set up with the oracle's bounds), made once."""
    made = {}

    def get(oracle, name, nchains=1, bounds=None):
        key = (name, nchains, bounds)
        if key not in made:
            m = configs.make_model(name)
            P = prec.LeftRightKPMPreconditioner(m)
            if nchains > 1:
                models.update_model_chains_(m, src.chain_fields(ref.host_model(name), nchains))
                bs = [ref.setup(oracle, name, c, nchains, bounds).bounds for c in range(nchains)]
                act, _, _ = prec.setup_chains_(P, e_min=[b[0] for b in bs], e_max=[b[1] for b in bs])
                assert act.all()
            else:
                b = ref.setup(oracle, name, bounds=bounds).bounds
                prec.setup_(P, e_min=b[0], e_max=b[1])
                assert P.active
            made[key] = (m, P)
        return made[key]

    yield get
    for m, _ in made.values():
        m.close()


# ------------------------------------------------------------------------------------------ one side of the expansion

@pytest.mark.parametrize("name", ref.MODELS)
def test_one_sided_apply(oracle, gpu, name):
    S = ref.setup(oracle, name)
    m, P = gpu(oracle, name)
    _as(m, "GMRES", 1e-5, 40)
    v = np.ascontiguousarray(synth.randn(5, S.n))
    left, right = prec.LeftKPMPreconditioner(m, expansion=P), prec.RightKPMPreconditioner(m, expansion=P)
    zl, zr, zlr = np.zeros(S.n), np.zeros(S.n), np.zeros(S.n)
    prec.kpm_ldiv_(zl, left, v)
    prec.kpm_ldiv_(zr, right, v)
    el, er = _rel(zl, S.side(False) @ v), _rel(zr, S.side(True) @ v)
    print(f"{name}: Left {el:.2e}, Right {er:.2e}")
    assert el < 1e-11 and er < 1e-11
    # LeftRight is the side model.transposed selects
    prec.kpm_ldiv_(zlr, P, v)
    assert np.array_equal(zlr, zl)
    models.transpose_(m)
    prec.kpm_ldiv_(zlr, P, v)
    assert np.array_equal(zlr, zr)
    models.transpose_(m)
    # Left after Right is the symmetric apply of the same handle
    sym = prec.SymmetricKPMPreconditioner(m, expansion=P)
    zs = np.zeros(S.n)
    prec.kpm_ldiv_(zs, sym, v)
    prec.kpm_ldiv_(zlr, left, zr)
    e = _rel(zlr, zs)
    print(f"{name}: Left(Right(v)) against the symmetric apply {e:.2e}")
    assert e < 1e-11


@pytest.mark.parametrize("name", ("b", "e"))
def test_one_sided_apply_two_chains(oracle, gpu, name):
    m, P = gpu(oracle, name, 2)
    _as(m, "GMRES", 1e-5, 40)
    S = [ref.setup(oracle, name, c, 2) for c in range(2)]
    V = np.ascontiguousarray(np.stack([synth.randn(5 + k, m.Ndim) for k in range(4)]))      # vector k: chain k % 2
    for transposed in (False, True):
        m.transposed = transposed
        Z = np.zeros_like(V)
        prec.kpm_ldiv_(Z, P, V)
        errs = [_rel(Z[k], S[k % 2].side(transposed) @ V[k]) for k in range(4)]
        cross = _rel(Z[1], S[0].side(transposed) @ V[1])
        print(f"{name} transposed {transposed}: {errs}, chain 1's vector against chain 0's expansion {cross:.1e}")
        assert max(errs) < 1e-11 and cross > 1e-6
    m.transposed = False


# ------------------------------------------------------------------------------------------ solve!, preconditioned

@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_solve_preconditioned(oracle, gpu, case):
    name, op, solver, restart, tol, maxiter = case
    S = ref.setup(oracle, name)
    xr, itr, margin = S.solve(case)
    m, P = gpu(oracle, name)
    _as(m, solver, tol, maxiter, restart or -1, op == "MT")
    x = np.zeros(S.n)
    it = models.solve_(x, m, S.b, P=P)
    e = _rel(x, xr)
    print(f"{ref.case_id(case)}: iters {it} (reference {itr}, margin {margin:.3f}), |x - x_ref| / |x_ref| = {e:.2e}")
    assert it == itr and e < 1e-10
    # the keywords of the call override the solver's fields (iszero() defaults, IterativeSolvers.jl:376-382)
    m.solver.tol = 1e-2
    x2 = np.zeros(S.n)
    assert models.solve_(x2, m, S.b, P=P, tol=tol, maxiter=maxiter) == it and np.array_equal(x2, x)
    m.transposed = False


# ------------------------------------------------------------------------------------------ ldiv!, batched

BATCH_SOLVERS = (("bicgstab", 0), ("gmres", 20), ("gmres", 4))


def _batch(S, op):
    X0 = np.ascontiguousarray(np.stack([S[k % len(S)].guess(kind, op) for k, kind in enumerate(src.BATCH)]))
    B = np.ascontiguousarray(np.stack([S[k % len(S)].b for k in range(len(src.BATCH))]))
    return X0, B


@pytest.mark.parametrize("solver,restart", BATCH_SOLVERS)
@pytest.mark.parametrize("op", ("M", "MT"))
@pytest.mark.parametrize("name", ("b", "t"))
def test_ldiv_batched_equals_single_solves(oracle, gpu, name, op, solver, restart):
    S = ref.setup(oracle, name)
    m, P = gpu(oracle, name)
    _as(m, solver, 1e-5, 40, restart or -1, op == "MT")
    X0, B = _batch([S], op)
    X = X0.copy()
    it, res, fl = models.ldiv_batched_(X, m, B, P)
    print(f"{name} {op} {solver}{restart or ''}: iters {it}, residuals {res}")
    assert len(set(it.tolist())) > 1                       # the right-hand sides stop at different iterations
    assert not fl.any() and np.all(res < np.sqrt(1e-5))
    for k, kind in enumerate(src.BATCH):
        x = X0[k].copy()
        it1, res1, fl1 = models.ldiv_(x, m, B[k], P)
        assert (it1, fl1) == (it[k], fl[k]) and res1 == res[k] and np.array_equal(x, X[k]), (k, kind)
        xr, itr, resr, flr = ref.mldiv(solver, S.A(op), S.b, X0[k], 1e-5, 40, restart, S.P(op))
        assert (it1, fl1) == (itr, flr) and _rel(x, xr) < 1e-10 and abs(res1 - resr) < 1e-8
    # the same batch again: identical bits
    X2 = X0.copy()
    it2, res2, fl2 = models.ldiv_batched_(X2, m, B, P)
    assert np.array_equal(X2, X) and np.array_equal(it2, it) and np.array_equal(res2, res)
    m.transposed = False


@pytest.mark.parametrize("solver,restart", (("bicgstab", 0), ("gmres", 20)))
@pytest.mark.parametrize("op", ("M", "MT"))
@pytest.mark.parametrize("name", ("b", "e"))
def test_ldiv_batched_two_chains(oracle, gpu, name, op, solver, restart):
    S = [ref.setup(oracle, name, c, 2) for c in range(2)]
    m, P = gpu(oracle, name, 2)
    _as(m, solver, 1e-5, 40, restart or -1, op == "MT")
    X0, B = _batch(S, op)
    X = X0.copy()
    it, res, fl = models.ldiv_batched_(X, m, B, P)
    print(f"{name} {op} {solver}{restart or ''}, two chains: iters {it}")
    for k in range(len(src.BATCH)):
        C = S[k % 2]
        xr, itr, resr, flr = ref.mldiv(solver, C.A(op), C.b, X0[k], 1e-5, 40, restart, C.P(op))
        assert (it[k], fl[k]) == (itr, flr) and _rel(X[k], xr) < 1e-10 and abs(res[k] - resr) < 1e-8, k
    X2 = X0.copy()
    models.ldiv_batched_(X2, m, B, P)
    assert np.array_equal(X2, X)
    m.transposed = False


@pytest.mark.parametrize("solver,restart", (("bicgstab", 0), ("gmres", 20)))
def test_zero_right_hand_side(oracle, gpu, solver, restart):
    """b = 0, x0 = 0.  GMRES: normb -> 1, eps = 0 < tol: 0 iterations.  BiCGStab: rho = 0 at once, break, return maxiter; the residual is
    0/0 and NaN > sqrt(tol) is false: flag 0 — as the restatement does."""
    S = ref.setup(oracle, "b")
    m, P = gpu(oracle, "b")
    _as(m, solver, 1e-5, 40, restart or -1)
    B = np.ascontiguousarray(np.stack([S.b, np.zeros(S.n), S.b]))
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B, P)
    xr, itr, resr, flr = ref.mldiv(solver, S.M, np.zeros(S.n), np.zeros(S.n), 1e-5, 40, restart, S.P("M"))
    assert itr == (40 if solver == "bicgstab" else 0) and flr == 0
    assert it[1] == itr and fl[1] == 0 and not X[1].any() and (np.isnan(res[1]) if np.isnan(resr) else res[1] == resr)
    assert it[0] == it[2] and np.array_equal(X[0], X[2]) and X[0].any() and fl[0] == 0


# ------------------------------------------------------------------------------------------ flags and the retry

def _check_ldiv(out, want, tol, digits=True):
    """iters, flag and residual_error against mldiv(): a flagged outcome's residual (of order 1) to relative 1e-8; an accepted solve's
    residual is a difference of nearly equal vectors and follows x, which is held to relative 1e-10 — the residual then to 1e-8 of |b|."""
    (x, it, res, fl), (xr, itr, resr, flr) = out, want
    print(f"device (iters, residual, flag) = ({it}, {res:.6e}, {fl}); reference ({itr}, {resr:.6e}, {flr})")
    assert (it, fl) == (itr, flr)
    if fl > 0:
        assert not x.any() and res > np.sqrt(tol) and resr > np.sqrt(tol)
        if digits:
            assert abs(res - resr) <= 1e-8 * resr
    else:
        assert _rel(x, xr) < 1e-10 and abs(res - resr) <= 1e-8


def test_flags_unpreconditioned_bicgstab(oracle, gpu):
    S = ref.setup(oracle, "b")
    m, _ = gpu(oracle, "b")
    for solver_maxiter, call_maxiter, flag in ((5, 0, 1), (40, 5, 2)):      # Models.jl:160 compares solver.maxiter
        _as(m, "BiCGStab", 1e-5, solver_maxiter)
        x = np.zeros(S.n)
        it, res, fl = models.ldiv_(x, m, S.b, maxiter=call_maxiter)
        want = ref.mldiv("bicgstab", S.M, S.b, np.zeros(S.n), 1e-5, solver_maxiter, 0, None, call_maxiter)
        _check_ldiv((x, it, res, fl), want, 1e-5)
        assert fl == flag and it == 5


@pytest.mark.parametrize("name,solver,restart,tol,solver_maxiter", (
    ("t", "gmres", 4, 1e-5, 40), ("t", "gmres", 4, 1e-5, 20), ("b", "gmres", 4, 1e-8, 40), ("b", "bicgstab", 0, 1e-8, 40),
    ("t", "gmres", 20, 1e-5, 40)))
def test_weak_preconditioner_is_retried_without(oracle, gpu, name, solver, restart, tol, solver_maxiter):
    """WEAK_BOUNDS, call maxiter 2: the first four rows run out with a residual above sqrt(tol) and are solved again from zero without the
    expansion within 20 iterations; none of those retries converges on these inputs (tests/msolver_reference.py's mldiv decides: GMRES(4)
    and BiCGStab without the expansion need hundreds of iterations), so the flag of the retry and the zeroed x come back.  GMRES(20) runs
    its whole first cycle whatever the call's maxiter and converges in it: flag 0, no retry."""
    W = ref.setup(oracle, name, bounds=src.WEAK_BOUNDS)
    m, P = gpu(oracle, name, bounds=src.WEAK_BOUNDS)
    _as(m, solver, tol, solver_maxiter, restart or -1)
    want = ref.mldiv(solver, W.M, W.b, np.zeros(W.n), tol, solver_maxiter, restart, W.P("M"), 2)
    first = ref.solve(solver, W.M, W.b, np.zeros(W.n), tol, 2, solver_maxiter, restart, W.P("M"))
    retried = want[1] != first[1]
    assert retried == (restart != 20)
    x = np.zeros(W.n)
    it, res, fl = models.ldiv_(x, m, W.b, P, maxiter=2)
    _check_ldiv((x, it, res, fl), want, tol, digits=solver != "bicgstab")
    if retried:
        assert it == 20 and fl == (1 if solver_maxiter == 20 else 2)
    # in a batch only the flagged right-hand side is retried, alone; its neighbours keep their solves
    if retried and solver == "gmres":
        _as(m, solver, tol, solver_maxiter, restart)
        nearer = np.ascontiguousarray(W.xs("M") * (1.0 + 1e-7 * synth.randn(src.SEED_NEAR, W.n)))
        X = np.ascontiguousarray(np.stack([nearer, np.zeros(W.n), nearer]))
        B = np.ascontiguousarray(np.stack([W.b] * 3))
        itb, resb, flb = models.ldiv_batched_(X, m, B, P, maxiter=2)
        print(f"batch: iters {itb}, flags {flb}, residuals {resb}")
        assert (itb[1], flb[1]) == (it, fl) and not X[1].any() and resb[1] == res
        assert flb[0] == flb[2] == 0 and np.array_equal(X[0], X[2]) and X[0].any()


# ------------------------------------------------------------------------------------------ the bare iterations

@pytest.mark.parametrize("op", ("M", "MT"))
@pytest.mark.parametrize("name", ("b", "t", "e"))
def test_bare_bicgstab_five_iterations(oracle, gpu, name, op):
    S = ref.setup(oracle, name)
    A = S.A(op)
    runs = {d: np.asarray(ref.bicgstab(A, S.b, np.zeros(S.n), 1e-30, 5, None, d)[0], dtype=np.float64) for d in F64_DOTS + ("longdouble",)}
    spread = max(_rel(runs[d], runs["longdouble"]) for d in F64_DOTS)
    m, _ = gpu(oracle, name)
    _as(m, "BiCGStab", 1e-30, 5, transposed=op == "MT")
    x = np.zeros(S.n)
    it = models.solve_(x, m, S.b)
    e = _rel(x, runs["longdouble"])
    print(f"{name} {op}: spread of the float64 variants {spread:.2e}, device against long double {e:.2e}")
    assert it == 5 and e <= 100.0 * spread
    m.transposed = False


@pytest.mark.parametrize("case", ref.LONG_CASES, ids=ref.case_id)
def test_long_unpreconditioned_gmres(oracle, gpu, case):
    name, op, solver, restart, tol, maxiter = case
    S = ref.setup(oracle, name)
    xr, itr, margin = S.solve(case, prec=False)
    m, _ = gpu(oracle, name)
    _as(m, "GMRES", tol, maxiter, restart, op == "MT")
    x = np.zeros(S.n)
    it = models.solve_(x, m, S.b)
    e = _rel(x, xr)
    print(f"{ref.case_id(case)}: iters {it} (reference {itr}, margin {margin:.3f}), |x - x_ref| / |x_ref| = {e:.2e}")
    assert it == itr and e < 1e-9
    m.transposed = False


def test_gmres_cycle_rules(oracle, gpu):
    """The cycle cut at iter == solver.maxiter updates x with the columns it built (the library's rule), and a call maxiter below
    solver.maxiter does not cut the cycle: iters exceeds it (the reference as it executes)."""
    S = ref.setup(oracle, "t")
    m, _ = gpu(oracle, "t")
    x0 = np.zeros(S.n)
    for call_maxiter, solver_maxiter, iters in ((0, 5, 5), (5, 40, 20), (0, 30, 30)):
        _as(m, "GMRES", 1e-30, solver_maxiter, 20)
        xr, itr = ref.gmres(S.M, S.b, x0, 1e-30, call_maxiter or solver_maxiter, solver_maxiter, 20)[:2]
        x = np.zeros(S.n)
        it = models.solve_(x, m, S.b, maxiter=call_maxiter)
        print(f"call maxiter {call_maxiter}, solver.maxiter {solver_maxiter}: iters {it}, |x - x_ref| / |x_ref| = {_rel(x, xr):.2e}")
        assert it == itr == iters and np.all(np.isfinite(x)) and _rel(x, xr) < 1e-10


# ------------------------------------------------------------------------------------------ lifetime

def test_krylov_basis_lifetime(oracle):
    """A model that ran GMRES is closed (the Krylov basis goes with the handle); a fresh model solves again, to the same bits; a larger
    restart and a larger batch on one handle regrow the basis."""
    S = ref.setup(oracle, "t")
    case = ("t", "M", "gmres", 4, 1e-8, 40)
    xs = []
    for _ in range(2):
        m = _as(configs.make_model("t"), "GMRES", 1e-8, 40, 4)
        P = prec.LeftRightKPMPreconditioner(m)
        prec.setup_(P, e_min=S.bounds[0], e_max=S.bounds[1])
        x = np.zeros(S.n)
        it = models.solve_(x, m, S.b, P=P)
        assert it == S.solve(case)[1]
        xs.append(x)
        if len(xs) == 2:
            _as(m, "GMRES", 1e-5, 40, 20)
            B = np.ascontiguousarray(np.stack([S.b] * 5))
            X = np.zeros_like(B)
            itb, _, flb = models.ldiv_batched_(X, m, B, P)
            assert not flb.any() and len(set(itb.tolist())) == 1 and all(np.array_equal(X[0], X[k]) for k in range(5))
            assert _rel(X[0], S.solve(("t", "M", "gmres", 20, 1e-5, 40))[0]) < 1e-10
        m.close()
    assert np.array_equal(xs[0], xs[1])
