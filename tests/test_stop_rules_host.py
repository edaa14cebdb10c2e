"""Host side of tests/test_gpu_stop_rules.py (no device): the preconditions of every case of tests/stop_rule_cases.py, on the CPU oracle
alone.  The GPU tests ask for EQUAL iteration counts and for the stopping vector to 1e-10; that is only fair where

  * the three reasons (tolerance, kappa, maxiter) occur as the case designs them;
  * every comparison the solve makes up to its stop — and the sqrt(tol) comparison of ldiv! — has a log-margin of at least 1e-3
    (two summation orders agree on eps to 1e-10 over the first 40 iterations: seven orders below);
  * no stop is later than iteration 40, the retries of flagged right-hand sides included;
  * x_j differs from x_{j-1} and x_{j+1} by more than 1e-4 relative at every kappa and maxiter stop, so that a form returning the
    vector of the neighbouring iteration cannot pass;
  * oracle.cg_solve stops where decide() says and oracle.ldiv returns the (iters, flag) the rule of Models.jl:74-186 gives.

For the 4 x 4 x 20 model (and the 72 unknowns of the 3 x 3 triangular one) the oracle itself is pinned by a dense conjugate-gradient
iteration in numpy.longdouble on the matrix taken column by column from oracle.mulM: same stop, same reason, x to 1e-12.

No case is skipped: one that misses a precondition gets other parameters there, the bounds stay.
The measured margins are printed (pytest -s).
"""
import numpy as np
import pytest

import stop_rule_cases as src

KEYS = list(src.PARAMS)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _flag(res, tol, iters, cmp_maxiter):
    return 0 if res <= np.sqrt(tol) else (1 if iters == cmp_maxiter else 2)


def expected_ldiv(S, U, kind, c, chain, tol, kmax, call, solver_maxiter):
    """(iters, flag, residual, x, margin) of ldiv! by the rule of Models.jl:74-186 from the oracle's solves: a preconditioned solve that
    ends above sqrt(tol) is redone from zero without the expansion (U: the un-preconditioned setup) with 10 x the call maxiter.  margin:
    the smallest log-margin of every decision on the way, the sqrt(tol) comparisons included."""
    x, it, h = S.solve(kind, c, chain, tol, kmax, call)
    j, why, mg = src.decide(S.hist(kind, c, chain), tol, kmax, call)
    assert it == j <= src.LATEST
    res = S.true_residual(x, chain, kind)
    mg = min(mg, abs(np.log(res / np.sqrt(tol))))
    flag = _flag(res, tol, it, call if S.prec else solver_maxiter)
    if flag and S.prec:
        again = "slow" if kind == "slow" else "zero"          # from x = 0, the same right-hand side
        assert 10 * call <= S.HIST or src.decide(U.hist(again, 1.0, chain), tol, kmax, S.HIST)[1] != "maxiter"
        x, it, h = U.solve(again, 1.0, chain, tol, kmax, 10 * call)
        j, why, m2 = src.decide(U.hist(again, 1.0, chain), tol, kmax, min(10 * call, S.HIST))
        assert it == j <= src.LATEST, "the retry of a flagged right-hand side ends beyond the iterations the 1e-10 agreement is stated for"
        res = S.true_residual(x, chain, kind)
        mg = min(mg, m2, abs(np.log(res / np.sqrt(tol))))
        flag = _flag(res, tol, it, solver_maxiter)
    if flag:
        x = np.zeros_like(x)
    return it, flag, res, x, mg


def check_single(oracle, key, chain, single, nchains):
    label, kind, c, tol, kmax, call, solver_mi, reason, flag = single
    S = src.setup(oracle, key[0], key[1], nchains)
    U = src.setup(oracle, key[0], False, nchains)
    h = S.hist(kind, c, chain)
    j, why, mg = src.decide(h, tol, kmax, call)
    assert why == reason, (key, chain, label, j, why)
    assert mg >= src.MARGIN, (key, chain, label, mg)
    assert j <= src.LATEST, (key, chain, label, j)
    if label in ("kappa-at-maxiter", "tol-at-maxiter"):
        assert j == call, (key, label, j, call)
    if label == "call-maxiter":
        assert call != solver_mi
    if label == "slow-kappa":      # just past the kappa screen, on its far side (rr >= 2 y_num: (eps / eps_0)^2 >= 8, with 5 % to spare)
        assert 0.17 * np.sqrt(kmax) <= j < 0.68 * np.sqrt(kmax) and (h[j] / h[0]) ** 2 >= 8.4, (key, j, kmax, h[:j + 1])
    if label == "big-kappa":       # the first iterations pass the kappa screen of cg_stop_test (seq < 0.17 sqrt(kmax)), the stop lies beyond it
        assert 0.17 * np.sqrt(kmax) > 1.0 and j > 0.17 * np.sqrt(kmax) + 1, (key, j, kmax)
    # the oracle stops where the helper says, with the history the helper was given
    x, it, hs = S.solve(kind, c, chain, tol, kmax, call)
    assert it == j and np.array_equal(hs, h[:j + 1]), (key, chain, label, it, j)
    if why != "tol":               # the neighbouring iterates are far away
        for jj in (j - 1, j + 1):
            d = rel(S.iterate(kind, c, chain, jj), x)
            assert d > src.SENSITIVITY, (key, chain, label, jj, d)
    assert np.array_equal(S.iterate(kind, c, chain, j), x)
    # ldiv!: the oracle against the rule, the flag as designed
    ite, fle, rese, xe, mg2 = expected_ldiv(S, U, kind, c, chain, tol, kmax, call, solver_mi)
    xo, ito, reso, flo = S.ldiv(kind, c, chain, tol, kmax, solver_mi, 0 if call == solver_mi else call)
    assert (ito, flo) == (ite, fle), (key, chain, label, ito, flo, ite, fle)
    assert abs(reso - rese) <= 1e-12 * rese and np.array_equal(xo, xe)
    assert mg2 >= src.MARGIN, (key, chain, label, mg2)
    if flag is not None:
        assert flo == flag, (key, chain, label, flo, flag)
    return label, j, why, min(mg, mg2), flo


@pytest.mark.parametrize("key", KEYS, ids=[f"{k[0]}{'-kpm' if k[1] else ''}" for k in KEYS])
def test_every_case_meets_its_preconditions(oracle, key):
    nchains = 2 if key in src.CHAINS else 1
    seen = set()
    for single in src.singles(key):
        for chain in range(nchains if single[0][:2] in ("P-", "F-") else 1):
            label, j, why, mg, fl = check_single(oracle, key, chain, single, nchains)
            print(f"{key[0]}{'-kpm' if key[1] else ''} chain {chain} {label}: stops at {j} by {why}, flag {fl}, log-margin {mg:.3g}")
            seen.add(why)
    assert seen == {"tol", "kappa", "maxiter"}, (key, seen)
    if "P" in src.PARAMS[key]:
        for s in ("P", "F"):
            flags = [check_single(oracle, key, 0, sg, nchains)[4] for sg in src.singles(key) if sg[0].startswith(s + "-")]
            assert (flags == [0, 0, 0]) if s == "P" else (flags[1] == 0 and (key[1] or (flags[0], flags[2]) == (2, 1))), (key, s, flags)


@pytest.mark.parametrize("name", list(src.RETRY))
def test_retry_case_flags_the_far_guesses_only(oracle, name):
    """The four right-hand sides of stop_rule_cases.RETRY: slots 1 and 3 are flagged in the preconditioned pass and come back from the
    retry with flag 0, slots 0 and 2 are not flagged; every decision with its margin, every stop within 40 iterations."""
    tol, call = src.RETRY[name]
    S = src.setup(oracle, name, True, 2, src.WEAK_BOUNDS)
    U = src.setup(oracle, name, False, 2)
    for r, (kind, c) in enumerate(src.RETRY_SLOTS):
        chain = r % 2
        x, it, h = S.solve(kind, c, chain, tol, 1e12, call)
        first = _flag(S.true_residual(x, chain), tol, it, call)
        ite, fle, rese, xe, mg = expected_ldiv(S, U, kind, c, chain, tol, 1e12, call, src.RETRY_SOLVER_MAXITER)
        xo, ito, reso, flo = S.ldiv(kind, c, chain, tol, 1e12, src.RETRY_SOLVER_MAXITER, call)
        print(f"{name} slot {r} ({kind}): first pass {it} iterations, flag {first}; ldiv! returns {ito} iterations, flag {flo}, log-margin {mg:.3g}")
        assert (first != 0) == (r in (1, 3)), (name, r, first)
        assert (ito, flo) == (ite, fle) and flo == 0 and mg >= src.MARGIN, (name, r, ito, flo, ite, fle, mg)
        assert np.array_equal(xo, xe) and (ito > call) == (r in (1, 3))


# ------------------------------------------------------------------------------------------ the oracle itself, 4 x 4 x 20

def _dense_longdouble_cg(A, b, x0, tol, kmax, maxiter):
    """solve! (IterativeSolvers.jl:239-314) on a dense matrix in numpy.longdouble: (x, iters, reason)."""
    ld = np.longdouble
    x, b = x0.astype(ld), b.astype(ld)
    normb = np.sqrt(b @ b)
    r = b - A @ x
    p = r.copy()
    rr = r @ r
    eps0 = np.sqrt(rr) / normb
    K = ld(0)
    for j in range(1, maxiter + 1):
        z = A @ p
        alpha = rr / (p @ z)
        x = x + alpha * p
        r = r - alpha * z
        new = r @ r
        eps = np.sqrt(new) / normb
        K = max(K, (2 * j / np.log(2 * eps0 / eps)) ** 2)
        if eps < tol:
            return x, j, "tol"
        if K > kmax:
            return x, j, "kappa"
        p = r + (new / rr) * p
        rr = new
    return x, maxiter, "maxiter"


@pytest.mark.parametrize("name", ["b", "t"])
def test_oracle_stops_as_a_dense_long_double_iteration_does(oracle, name):
    """4 x 4 x 20 (320 unknowns) and the 3 x 3 triangular lattice with 8 slices (72 unknowns, where a float64 iteration leaves the
    long-double one soonest: the case's maxiter is chosen inside the range in which it has not)."""
    S = src.setup(oracle, name, False, 2 if (name, False) in src.CHAINS else 1)
    n = S.m.Ndim
    eye = np.eye(n)
    M = np.stack([oracle.mulM(S.om[0], np.ascontiguousarray(eye[k])) for k in range(n)], axis=1)
    Mt = np.stack([oracle.mulMT(S.om[0], np.ascontiguousarray(eye[k])) for k in range(n)], axis=1)
    assert np.array_equal(Mt, M.T) or rel(Mt, M.T) < 1e-15          # mulMT is the transpose of mulM, column by column
    Ml = M.astype(np.longdouble)
    A = Ml.T @ Ml
    for s in ("P", "F"):
        tol, kmax, mi, c = src.PARAMS[(name, False)][s]
        for kind in src.KINDS:
            xo, ito, _ = S.solve(kind, c, 0, tol, kmax, mi)
            xd, itd, why = _dense_longdouble_cg(A, S.b, S.guess(kind, c, 0), tol, kmax, mi)
            d = float(np.linalg.norm(xd - xo.astype(np.longdouble)) / np.linalg.norm(xd))
            print(f"set {s} {kind}: dense long double stops at {itd} by {why}, oracle at {ito}; |x - x_dense| / |x_dense| = {d:.2e}")
            assert (itd, why) == (ito, src.DESIGN[s][kind][0])
            assert d < 1e-12
