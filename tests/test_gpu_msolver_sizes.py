"""BiCGStab, GMRES and the one-sided KPM apply on the device beyond 320 unknowns, against the matrix-free reference of
tests/msolver_reference.py, on the lattices of tests/msolver_size_cases.py: each reaches one launch class of the route — 3 ... 16 waves in
the solver kernels' workgroup (every scalar of a solve is a sum over them), 64 ... 1024 threads and 1 ... 6 sites per thread in
k_kpm_cheb_side, its bond program in LDS or in memory, every transform form the apply's twisted pair takes, and the refusal beyond six sites
per thread.  Every test asserts the library's own probe (_lib.kpm_side_info, _lib.dft_plan on the handle) for the class it claims, and the
last test of the file asserts that what the file ran covers all of them — it reads what the tests before it recorded and holds for a run
of the whole file.  The expansion's bounds are injected on both sides from the oracle's Arnoldi run, so both use one expansion.

Bounds.  The project's figures: relative 1e-11 for an apply, 1e-10 for the x of a preconditioned solve, with EQUAL iteration counts (every
case has a log-margin >= 1e-2 under each float64 summation order: tests/test_msolver_sizes_host.py).  They stand wherever the reference's own
spread over its three float64 summation orders is at least 100 times smaller, which msolver_size_cases.bound() decides per case from the
spread measured in that test; the host test prints every spread.  Measured there: at most 1.3e-14 over all preconditioned solves, single and
batched (the largest: the far guess under GMRES(20) on 48 x 48), and 6.3e-15 for the bare GMRES(20) cycle — the project's figures stand for
all of them.  The apply sums nothing in an order of its own (spread 0).  ONE case takes 100 x its spread instead, as the bare BiCGStab cases
of tests/test_gpu_msolvers.py do: five un-preconditioned BiCGStab iterations on 48 x 48, spread 3.6e-10 for M and 3.6e-11 for M^T, hence
3.6e-8 and 3.6e-9.  No bound is taken from the device's output.

The scalar transform cannot be reached on a short time axis: every axis of up to 256 slices has a one-tile table, which the twisted pair
prefers to the scalar kernels at every batch size.  Its case is the 4 x 4 lattice on 300 slices (4800 unknowns, 16 waves).
"""
import numpy as np
import pytest

from elphdynamics_amd import _lib, configs, models, preconditioners as prec, synth
import msolver_reference as ref
import msolver_size_cases as sz
import stop_rule_cases as src

pytestmark = pytest.mark.gpu

F64_DOTS = ("sequential", "pairwise", "blas")
# what the tests of this file ran, as the probes reported it: (NPL, TRANSPOSED) of the one-sided kernel, its lds_tables, the waves of the
# solver kernels' workgroup, the forms of the apply's transforms
SEEN = {"npl": set(), "lds": set(), "waves": set(), "forms": set()}


def _as(m, solver, tol, maxiter, restart=-1, transposed=False):
    m.solver, m.mul_by_M = models.make_solver(solver, m.Ndim, tol, maxiter, restart)
    m.transposed = bool(transposed)
    return m


def _probe(m, tag):
    """The probe of a handle, asserted against the table."""
    info = _lib.kpm_side_info(m._h)
    N, L, waves, cbs, npl, lds = sz.LATTICES[tag]
    assert (m.Nsites, m.Ltau) == (N, L)
    assert (info["ms_block"], info["cbs"], info["npl"], info["lds_tables"], info["refused"]) == (64 * waves, cbs, npl, lds, int(npl > sz.NPL_MAX)), info
    return info


def _ran_apply(info, transposed):
    SEEN["npl"].add((info["npl"], bool(transposed)))
    SEEN["lds"].add(info["lds_tables"])


def _ran_solve(info, transposed, prec_=True):
    SEEN["waves"].add(info["ms_block"] // 64)
    if prec_:
        _ran_apply(info, transposed)


@pytest.fixture(scope="module")
def gpu():
    """tag -> (model, LeftRight preconditioner set up with the oracle's bounds, probe), made once per lattice."""
    made = {}

    def get(oracle, tag, nchains=1):
        key = (tag, nchains)
        if key not in made:
            m = configs.make_model(sz.row(tag))
            info = _probe(m, tag)
            P = prec.LeftRightKPMPreconditioner(m)
            if nchains > 1:
                models.update_model_chains_(m, src.chain_fields(ref.host_model(tag), nchains))
                bs = [ref.setup(oracle, tag, c, nchains, matrix_free=True).bounds for c in range(nchains)]
                act, _, _ = prec.setup_chains_(P, e_min=[b[0] for b in bs], e_max=[b[1] for b in bs])
                assert act.all()
            else:
                b = ref.setup(oracle, tag, matrix_free=True).bounds
                prec.setup_(P, e_min=b[0], e_max=b[1])
                assert P.active
            made[key] = (m, P, info)
        return made[key]

    yield get
    for m, _, _ in made.values():
        m.close()


# ------------------------------------------------------------------------------------------ a. one side of the expansion

@pytest.mark.parametrize("tag", sz.APPLY_TAGS)
def test_one_sided_apply(oracle, gpu, tag):
    S = ref.setup(oracle, tag, matrix_free=True)
    m, P, info = gpu(oracle, tag)
    _as(m, "GMRES", 1e-5, 40)
    v = np.ascontiguousarray(synth.randn(5, S.n))
    left, right = prec.LeftKPMPreconditioner(m, expansion=P), prec.RightKPMPreconditioner(m, expansion=P)
    zl, zr, zlr, zs = np.zeros(S.n), np.zeros(S.n), np.zeros(S.n), np.zeros(S.n)
    prec.kpm_ldiv_(zl, left, v)
    prec.kpm_ldiv_(zr, right, v)
    _ran_apply(info, False)
    _ran_apply(info, True)
    el, er = sz.rel(zl, S.side(False) @ v), sz.rel(zr, S.side(True) @ v)
    print(f"{tag} (cbs {info['cbs']}, NPL {info['npl']}, lds_tables {info['lds_tables']}): Left {el:.2e}, Right {er:.2e}")
    assert el < 1e-11 and er < 1e-11
    # Left after Right is the symmetric apply of the same handle (k_kpm_cheb, the patch and register forms: an independent device cross-check)
    sym = prec.SymmetricKPMPreconditioner(m, expansion=P)
    prec.kpm_ldiv_(zs, sym, v)
    prec.kpm_ldiv_(zlr, left, zr)
    e = sz.rel(zlr, zs)
    print(f"{tag}: Left(Right(v)) against the symmetric apply {e:.2e}")
    assert e < 1e-11


@pytest.mark.parametrize("tag", sz.TWO_CHAIN_TAGS)
def test_one_sided_apply_two_chains(oracle, gpu, tag):
    m, P, info = gpu(oracle, tag, 2)
    _as(m, "GMRES", 1e-5, 40)
    S = [ref.setup(oracle, tag, c, 2, matrix_free=True) for c in range(2)]
    V = np.ascontiguousarray(np.stack([synth.randn(5 + k, m.Ndim) for k in range(4)]))      # vector k: chain k % 2
    for transposed in (False, True):
        m.transposed = transposed
        Z = np.zeros_like(V)
        prec.kpm_ldiv_(Z, P, V)
        _ran_apply(info, transposed)
        errs = [sz.rel(Z[k], S[k % 2].side(transposed) @ V[k]) for k in range(4)]
        cross = sz.rel(Z[1], S[0].side(transposed) @ V[1])
        print(f"{tag} transposed {transposed}: {errs}, chain 1's vector against chain 0's expansion {cross:.1e}")
        assert max(errs) < 1e-11 and cross > 1e-6
    m.transposed = False


# ------------------------------------------------------------------------------------------ b. the transform forms on this path

@pytest.mark.parametrize("tag,nvec,form", sz.FORM_CASES)
def test_one_sided_apply_transform_forms(oracle, gpu, tag, nvec, form):
    S = ref.setup(oracle, tag, matrix_free=True)
    m, P, info = gpu(oracle, tag)
    _as(m, "GMRES", 1e-5, 40)
    for inverse in (0, 1):
        assert _lib.dft_plan(m.Ltau, 0, inverse, m.Nsites, nvec, handle=m._h)["form"] == _lib.DFT_FORMS[form]
    V = np.ascontiguousarray(np.stack([synth.randn(20 + k, S.n) for k in range(nvec)]))
    for transposed in (False, True):
        m.transposed = transposed
        Z = np.zeros_like(V)
        prec.kpm_ldiv_(Z, P, V)
        _ran_apply(info, transposed)
        want = ref.side_apply(S.K, S.m.neighbor_table, np.ascontiguousarray(V.T), transposed, matrix_free=True).T
        errs = [sz.rel(Z[k], want[k]) for k in range(nvec)]
        print(f"{tag}, {nvec} vectors ({form}), transposed {transposed}: largest error {max(errs):.2e}")
        assert max(errs) < 1e-11
    SEEN["forms"].add(form)
    m.transposed = False


# ------------------------------------------------------------------------------------------ c. preconditioned solves

@pytest.mark.parametrize("case", sz.SOLVE_CASES, ids=ref.case_id)
def test_solve_preconditioned(oracle, gpu, case):
    tag, op, solver, restart, tol, maxiter = case
    S = ref.setup(oracle, tag, matrix_free=True)
    runs = {d: S.solve(case, dot=d) for d in F64_DOTS}
    xr, itr, margin = runs["blas"]
    spread = sz.spread([r[0] for r in runs.values()])
    m, P, info = gpu(oracle, tag)
    _as(m, solver, tol, maxiter, restart or -1, op == "MT")
    x = np.zeros(S.n)
    it = models.solve_(x, m, S.b, P=P)
    _ran_solve(info, op == "MT")
    e, bound = sz.rel(x, xr), sz.bound(1e-10, spread)
    print(f"{ref.case_id(case)} ({info['ms_block'] // 64} waves, cbs {info['cbs']}, NPL {info['npl']}, lds_tables {info['lds_tables']}): iters {it} "
          f"(reference {itr}, margin {margin:.3f}), |x - x_ref| / |x_ref| = {e:.2e}, bound {bound:.1e} (spread {spread:.1e})")
    assert it == itr and e < bound
    m.transposed = False


# ------------------------------------------------------------------------------------------ d. ldiv!, batched

def _batch(S, op):
    X0 = np.ascontiguousarray(np.stack([S.guess(kind, op) for kind in src.BATCH]))
    B = np.ascontiguousarray(np.stack([S.b] * len(src.BATCH)))
    return X0, B


@pytest.mark.parametrize("case", sz.BATCH_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}{c[3] or ''}")
def test_ldiv_batched_equals_single_solves(oracle, gpu, case):
    tag, op, solver, restart = case
    tol = sz.BATCH_TOL
    S = ref.setup(oracle, tag, matrix_free=True)
    m, P, info = gpu(oracle, tag)
    _as(m, solver, tol, sz.SOLVER_MAXITER, restart or -1, op == "MT")
    X0, B = _batch(S, op)
    X = X0.copy()
    it, res, fl = models.ldiv_batched_(X, m, B, P)
    _ran_solve(info, op == "MT")
    print(f"{tag} {op} {solver}{restart or ''}: iters {it}, residuals {res}")
    assert len(set(it.tolist())) > 1                       # the right-hand sides stop at different iterations
    assert not fl.any() and np.all(res < np.sqrt(tol))
    full = (tag, op, solver, restart, tol, sz.SOLVER_MAXITER)
    for k, kind in enumerate(src.BATCH):
        x = X0[k].copy()
        it1, res1, fl1 = models.ldiv_(x, m, B[k], P)       # one right-hand side in a workspace of six: vstride != nrhs * ndim
        assert (it1, fl1) == (it[k], fl[k]) and res1 == res[k] and np.array_equal(x, X[k]), (k, kind)
        xr, itr, resr, flr = ref.mldiv(solver, S.A(op), S.b, X0[k], tol, sz.SOLVER_MAXITER, restart, S.P(op))
        bound = sz.bound(1e-10, sz.spread([S.solve(full, x0=X0[k], dot=d)[0] for d in F64_DOTS]))
        e = sz.rel(x, xr)
        print(f"   {kind}: iters {it1} (reference {itr}), |x - x_ref| / |x_ref| = {e:.2e}, bound {bound:.1e}, residual {res1:.6e} (reference {resr:.6e})")
        assert (it1, fl1) == (itr, flr) and e < bound and abs(res1 - resr) < 1e-8
    # the same batch again: identical bits
    X2 = X0.copy()
    it2, res2, fl2 = models.ldiv_batched_(X2, m, B, P)
    assert np.array_equal(X2, X) and np.array_equal(it2, it) and np.array_equal(res2, res)
    m.transposed = False


@pytest.mark.parametrize("case", sz.FLAG_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}{c[3] or ''}")
def test_ldiv_batched_flags(oracle, gpu, case):
    """A call maxiter that the zero and the far guesses run out of, as the reference does: they are solved again without the expansion, run out
    again and come back zeroed with flag 1 (k_ms_verdict's residual through the 8- and the 16-wave sum); the near guesses keep their solves.
    After an un-preconditioned BiCGStab retry of 20 iterations only what decides the outcome is compared, not the residual's digits (the
    bare iteration amplifies rounding: tests/test_gpu_msolvers.py)."""
    tag, op, solver, restart = case
    tol = sz.FLAG_TOL[tag]
    S = ref.setup(oracle, tag, matrix_free=True)
    m, P, info = gpu(oracle, tag)
    _as(m, solver, tol, sz.FLAG_SOLVER_MAXITER, restart or -1, op == "MT")
    X0, B = _batch(S, op)
    X = X0.copy()
    it, res, fl = models.ldiv_batched_(X, m, B, P, maxiter=sz.FLAG_CALL_MAXITER)
    _ran_solve(info, op == "MT")
    print(f"{tag} {op} {solver}{restart or ''}: iters {it}, flags {fl}, residuals {res}")
    assert 1 in fl.tolist() and 0 in fl.tolist()
    for k, kind in enumerate(src.BATCH):
        xr, itr, resr, flr = ref.mldiv(solver, S.A(op), S.b, X0[k], tol, sz.FLAG_SOLVER_MAXITER, restart, S.P(op), sz.FLAG_CALL_MAXITER)
        assert (it[k], fl[k]) == (itr, flr), (k, kind)
        if flr:
            assert flr == 1 and not X[k].any() and res[k] > np.sqrt(tol) and resr > np.sqrt(tol)
            if solver != "bicgstab":
                assert abs(res[k] - resr) <= 1e-8 * resr
        else:
            assert sz.rel(X[k], xr) < 1e-10 and abs(res[k] - resr) <= 1e-8
    X2 = X0.copy()
    it2, res2, fl2 = models.ldiv_batched_(X2, m, B, P, maxiter=sz.FLAG_CALL_MAXITER)
    assert np.array_equal(X2, X) and np.array_equal(it2, it) and np.array_equal(fl2, fl) and np.array_equal(res2, res)
    m.transposed = False


# ------------------------------------------------------------------------------------------ e. the bare iterations

@pytest.mark.parametrize("op", ("M", "MT"))
def test_bare_bicgstab_five_iterations(oracle, gpu, op):
    S = ref.setup(oracle, sz.BARE_TAG, matrix_free=True)
    runs = [np.asarray(ref.bicgstab(S.A(op), S.b, np.zeros(S.n), 1e-30, 5, None, d)[0]) for d in F64_DOTS]
    spread = sz.spread(runs)
    m, _, info = gpu(oracle, sz.BARE_TAG)
    _as(m, "BiCGStab", 1e-30, 5, transposed=op == "MT")
    x = np.zeros(S.n)
    it = models.solve_(x, m, S.b)
    _ran_solve(info, op == "MT", prec_=False)
    e = max(sz.rel(x, r) for r in runs)
    print(f"{sz.BARE_TAG} {op}: spread of the float64 variants {spread:.2e}, device against them {e:.2e}")
    assert it == 5 and e <= 100.0 * spread
    m.transposed = False


@pytest.mark.parametrize("op", ("M", "MT"))
def test_bare_gmres_one_cycle(oracle, gpu, op):
    S = ref.setup(oracle, sz.BARE_TAG, matrix_free=True)
    runs = [ref.gmres(S.A(op), S.b, np.zeros(S.n), 1e-30, 20, 20, 20, None, d) for d in F64_DOTS]
    bound = sz.bound(1e-10, sz.spread([r[0] for r in runs]))
    m, _, info = gpu(oracle, sz.BARE_TAG)
    _as(m, "GMRES", 1e-30, 20, 20, op == "MT")
    x = np.zeros(S.n)
    it = models.solve_(x, m, S.b)
    _ran_solve(info, op == "MT", prec_=False)
    e = sz.rel(x, runs[-1][0])
    print(f"{sz.BARE_TAG} {op}: one cycle of GMRES(20), iters {it}, |x - x_ref| / |x_ref| = {e:.2e}, bound {bound:.1e}")
    assert it == runs[-1][1] == 20 and np.all(np.isfinite(x)) and e < bound
    m.transposed = False


# ------------------------------------------------------------------------------------------ f. the refusal

def test_seven_sites_per_thread_are_refused(oracle):
    tag = sz.REFUSED
    S = ref.setup(oracle, tag, matrix_free=True)
    m = configs.make_model(sz.row(tag))
    try:
        info = _probe(m, tag)
        assert info["refused"] == 1 and info["npl"] == sz.NPL_MAX + 1
        P = prec.LeftRightKPMPreconditioner(m)
        prec.setup_(P, e_min=S.bounds[0], e_max=S.bounds[1])
        assert P.active
        v = np.ascontiguousarray(synth.randn(5, S.n))
        z = np.zeros(S.n)
        for solver, restart in (("GMRES", 20), ("BiCGStab", -1)):
            _as(m, solver, 1e-5, 40, restart)
            for transposed in (False, True):
                m.transposed = transposed
                with pytest.raises(_lib.ElphError) as err:
                    prec.kpm_ldiv_(z, P, v)
                assert err.value.code == _lib.ELPH_E_UNSUPPORTED and f"up to {sz.NPL_MAX * info['cbs']} sites" in str(err.value)
                x = np.zeros(S.n)
                with pytest.raises(_lib.ElphError) as err:
                    models.solve_(x, m, S.b, P=P)
                assert err.value.code == _lib.ELPH_E_UNSUPPORTED and f"up to {sz.NPL_MAX * info['cbs']} sites" in str(err.value)
        m.transposed = False
        # without the expansion the handle solves on: one cycle of GMRES(20)
        _as(m, "GMRES", 1e-30, 20, 20)
        runs = [ref.gmres(S.M, S.b, np.zeros(S.n), 1e-30, 20, 20, 20, None, d) for d in F64_DOTS]
        x = np.zeros(S.n)
        it = models.solve_(x, m, S.b)
        e, bound = sz.rel(x, runs[-1][0]), sz.bound(1e-10, sz.spread([r[0] for r in runs]))
        print(f"{tag}: un-preconditioned GMRES(20), iters {it}, |x - x_ref| / |x_ref| = {e:.2e}, bound {bound:.1e}")
        assert it == 20 and e < bound
        # ... and the symmetric apply of that handle works
        zs = np.zeros(S.n)
        prec.kpm_ldiv_(zs, prec.SymmetricKPMPreconditioner(m, expansion=P), v)
        e = sz.rel(zs, oracle.kpm_apply(S.oP, v))
        print(f"{tag}: symmetric apply against the oracle {e:.2e}")
        assert e < 1e-11
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ what the file ran

def test_every_launch_class_ran():
    """Over the tests above (the whole file): every instantiation of k_kpm_cheb_side, both placements of its bond program, the wave counts of the
    solver kernels' workgroup, the four transform forms."""
    assert SEEN["npl"] == {(n, t) for n in range(1, sz.NPL_MAX + 1) for t in (False, True)}, SEEN["npl"]
    assert SEEN["lds"] == {0, 1}
    assert {3, 6, 8, 16} <= SEEN["waves"] and SEEN["waves"] & {4, 5}, SEEN["waves"]
    assert {"SCALAR", "ONE_TILE", "DIRECT"} <= SEEN["forms"] and SEEN["forms"] & {"SPLIT_REG", "SPLIT_LDS"}, SEEN["forms"]
