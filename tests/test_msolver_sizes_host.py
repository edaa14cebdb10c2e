"""The reference of tests/test_gpu_msolver_sizes.py without a device: the matrix-free operators of tests/msolver_reference.py against the
dense ones on b and t, and every case of tests/msolver_size_cases.py held to what the GPU tests rely on — the launch class the table claims,
a log-margin of at least ref.MARGIN under each float64 summation order (hence equal iteration counts), right-hand sides of a batch that stop at
different iterations, flagged right-hand sides where a case is meant to have them.  Each test prints the spread of x over the three float64
summation orders (the largest relative difference between any two): the GPU bounds are the project's figures where 100 x that spread stays
below them, else 100 x the spread (msolver_size_cases.bound).
"""
import numpy as np
import pytest

from elphdynamics_amd import _lib, synth
import msolver_reference as ref
import msolver_size_cases as sz
import stop_rule_cases as src

F64_DOTS = ("sequential", "pairwise", "blas")


# ------------------------------------------------------------------------------------------ the matrix-free reference against the dense one

@pytest.mark.parametrize("name", ("b", "t"))
def test_matrix_free_operators_equal_the_dense_ones(oracle, name):
    D, F = ref.setup(oracle, name), ref.setup(oracle, name, matrix_free=True)
    assert F.bounds == D.bounds and F.K["active"]
    v = np.ascontiguousarray(synth.randn(5, D.n))
    V = np.ascontiguousarray(np.stack([synth.randn(6 + k, D.n) for k in range(3)], axis=1))
    for op in ("M", "MT"):
        e = sz.rel(F.A(op) @ v, D.A(op) @ v)
        print(f"{name} {op}: matrix-free against dense {e:.2e}")
        assert e < 1e-13
    for transposed in (False, True):
        e = sz.rel(F.side(transposed) @ v, D.side(transposed) @ v)
        eb = sz.rel(ref.side_apply(F.K, F.m.neighbor_table, V, transposed, matrix_free=True), D.side(transposed) @ V)
        print(f"{name} transposed {transposed}: matrix-free side_apply against dense {e:.2e}, a block of 3 vectors {eb:.2e}")
        assert e < 1e-13 and eb < 1e-13


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[0] in ("b", "t")], ids=ref.case_id)
def test_matrix_free_solves_take_the_dense_ones_iterations(oracle, case):
    D, F = ref.setup(oracle, case[0]), ref.setup(oracle, case[0], matrix_free=True)
    for dot in F64_DOTS:
        (xd, itd, _), (xf, itf, _) = D.solve(case, dot=dot), F.solve(case, dot=dot)
        assert itf == itd and sz.rel(xf, xd) < 1e-12, (dot, itf, itd)


def test_the_long_double_variant_stays_dense(oracle):
    F = ref.setup(oracle, "t", matrix_free=True)
    with pytest.raises(AssertionError):
        ref.bicgstab(F.M, F.b, np.zeros(F.n), 1e-5, 5, None, "longdouble")


# ------------------------------------------------------------------------------------------ the table

@pytest.mark.parametrize("tag", tuple(sz.LATTICES))
def test_lattices_reach_their_launch_class(tag):
    m = ref.host_model(tag)
    N, L, waves, cbs, npl, lds = sz.LATTICES[tag]
    assert (m.Nsites, m.Ltau) == (N, L)
    assert sz.launch_shape(m) == (waves, cbs, npl, lds)
    assert (npl > sz.NPL_MAX) == (tag == sz.REFUSED)


def test_the_table_covers_every_class():
    rows = [r for t, r in sz.LATTICES.items() if t != sz.REFUSED]
    assert {r[4] for r in rows} == set(range(1, sz.NPL_MAX + 1)) and {r[5] for r in rows} == {0, 1}
    assert {3, 6, 8, 16} <= {r[2] for r in rows} and {4, 5} & {r[2] for r in rows}
    assert {sz.LATTICES[t][2] for t in sz.SOLVE_TAGS} == {3, 5, 6, 8, 16}
    assert {sz.LATTICES[t][4] for t in sz.TWO_CHAIN_TAGS} == {2, 3}
    for tag, nvec, form in sz.FORM_CASES:            # the forms the library plans for these batches (its planner needs no device)
        N, L = sz.LATTICES[tag][:2]
        assert all(_lib.dft_plan(L, 0, inv, N, nvec)["form"] == _lib.DFT_FORMS[form] for inv in (0, 1)), (tag, nvec, form)


# ------------------------------------------------------------------------------------------ the solves

def _runs(S, case, **kw):
    return {dot: S.solve(case, dot=dot, **kw) for dot in F64_DOTS}


@pytest.mark.parametrize("case", sz.SOLVE_CASES, ids=ref.case_id)
def test_solve_cases_deliver(oracle, case):
    tag, op, solver, restart, tol, maxiter = case
    assert tol in ref.TOLS
    S = ref.setup(oracle, tag, matrix_free=True)
    assert S.K["active"]
    runs = _runs(S, case)
    its, margins = {d: r[1] for d, r in runs.items()}, {d: r[2] for d, r in runs.items()}
    spread = sz.spread([r[0] for r in runs.values()])
    x = runs["blas"][0]
    res = sz.rel(S.A(op) @ x, S.b)
    print(f"{ref.case_id(case)}: iters {its}, margins {margins}, true residual {res:.3e}, spread {spread:.1e}, bound {sz.bound(1e-10, spread):.1e}")
    assert len(set(its.values())) == 1 and 1 <= its["blas"] < maxiter
    assert min(margins.values()) >= ref.MARGIN
    assert res < (tol if solver == "bicgstab" else np.sqrt(tol))
    if restart == 4:
        assert ref.gmres(S.A(op), S.b, np.zeros(S.n), tol, maxiter, maxiter, restart, S.P(op))[3] >= 1


def _batch_guesses(S, op):
    return [S.guess(kind, op) for kind in src.BATCH]


@pytest.mark.parametrize("case", sz.BATCH_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}{c[3] or ''}")
def test_batch_cases_deliver(oracle, case):
    tag, op, solver, restart = case
    S = ref.setup(oracle, tag, matrix_free=True)
    full = (tag, op, solver, restart, sz.BATCH_TOL, sz.SOLVER_MAXITER)
    its, spreads, margins = [], [], []
    for x0 in _batch_guesses(S, op):
        runs = _runs(S, full, x0=x0)
        assert len({r[1] for r in runs.values()}) == 1
        its.append(runs["blas"][1])
        margins.append(min(r[2] for r in runs.values()))
        spreads.append(sz.spread([r[0] for r in runs.values()]))
        out = ref.mldiv(solver, S.A(op), S.b, x0, sz.BATCH_TOL, sz.SOLVER_MAXITER, restart, S.P(op))
        assert out[3] == 0 and out[1] == its[-1]
    print(f"{tag} {op} {solver}{restart or ''}: iters {its}, margins {margins}, spreads {spreads}")
    assert len(set(its)) > 1 and min(margins) >= ref.MARGIN


@pytest.mark.parametrize("case", sz.FLAG_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}{c[3] or ''}")
def test_flag_cases_deliver(oracle, case):
    tag, op, solver, restart = case
    S = ref.setup(oracle, tag, matrix_free=True)
    tol = sz.FLAG_TOL[tag]
    outs, first = [], []
    for x0 in _batch_guesses(S, op):
        outs.append(ref.mldiv(solver, S.A(op), S.b, x0, tol, sz.FLAG_SOLVER_MAXITER, restart, S.P(op), sz.FLAG_CALL_MAXITER))
        x1 = ref.solve(solver, S.A(op), S.b, x0, tol, sz.FLAG_CALL_MAXITER, sz.FLAG_SOLVER_MAXITER, restart, S.P(op))[0]
        first.append(sz.rel(S.A(op) @ x1, S.b))        # what decides the flag of the preconditioned attempt
    flags = [o[3] for o in outs]
    print(f"{tag} {op} {solver}{restart or ''}: iters {[o[1] for o in outs]}, flags {flags}, residuals of the first attempt {first} against "
          f"{np.sqrt(tol):.1e}, final {[o[2] for o in outs]}")
    assert [int(f > 0) for f in flags] == [int(kind != "near") for kind in src.BATCH] and 2 not in flags
    assert min(abs(np.log(r / np.sqrt(tol))) for r in first) >= ref.MARGIN
    for o in outs:
        assert (o[1] == sz.FLAG_SOLVER_MAXITER and not o[0].any()) if o[3] else (o[0].any() and o[1] < sz.FLAG_SOLVER_MAXITER)


@pytest.mark.parametrize("op", ("M", "MT"))
def test_bare_cases_deliver(oracle, op):
    """Five un-preconditioned BiCGStab iterations and one un-preconditioned GMRES(20) cycle on 48 x 48: the spreads behind the GPU bounds."""
    S = ref.setup(oracle, sz.BARE_TAG, matrix_free=True)
    bi = [ref.bicgstab(S.A(op), S.b, np.zeros(S.n), 1e-30, 5, None, d) for d in F64_DOTS]
    gm = [ref.gmres(S.A(op), S.b, np.zeros(S.n), 1e-30, 20, 20, 20, None, d) for d in F64_DOTS]
    print(f"{sz.BARE_TAG} {op}: spread after 5 BiCGStab iterations {sz.spread([r[0] for r in bi]):.1e}, after one GMRES(20) cycle {sz.spread([r[0] for r in gm]):.1e}")
    assert all(r[1] == 5 for r in bi) and all(r[1] == 20 for r in gm)
    assert sz.spread([r[0] for r in bi]) < 1e-8 and sz.spread([r[0] for r in gm]) < 1e-10
