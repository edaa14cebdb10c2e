"""The cases of the callers of the one-sided solvers (HMC force and action, estimator, Langevin force) and their reference, built on
tests/msolver_reference.py: what calc_O⁻¹Λϕ! computes for a mul_by_M model (HMC.jl:851-909) restated with dense matrices.

    x± = mldiv(M, mldiv(Mᵀ, b±, Right), Left)          b± = Λϕ± (Holstein; mulΛ! restated below) or ϕ± (bond phonons, Λ ≡ 1)

Every stage is ldiv! from a zero guess (ref.mldiv); fold() restates the bookkeeping of iterations and flags.  tests/test_msolver_callers_host.py
holds every stage of every case to a log-margin >= ref.MARGIN at the tolerance written here (so the device stops at the same iteration) and
holds KAPPA, the sensitivity of stage 2 to its right-hand side, to the values written here; tests/test_gpu_msolver_callers.py compares the
device against pair().
"""
import numpy as np

from elphdynamics_amd import models, synth
import msolver_reference as ref

SEED_PHI = (4101, 4102)          # synth.randn seeds of ϕ₊, ϕ₋
SEED_PERTURB = (4201, 4202, 4203)      # ... of the perturbations of stage 1's y that measure KAPPA
PERTURB = 1e-10                  # their relative size: the project's per-solve agreement (tests/test_gpu_msolvers.py)
SOLVERS = (("bicgstab", 0), ("gmres", 20), ("gmres", 4))
SOLVER_MAXITER = ref.SOLVER_MAXITER


def Lambda(m):
    """update_Λ! (HMC.jl:921-941): Λ[i, τ] = exp(-Δτ (λᵢ x + λ₂ᵢ x²) / 2); the identity for bond phonons (:943-946)."""
    if m.kind == models.SSH:
        return np.ones(m.Ndim)
    X = m.x.reshape(m.Nph, m.Ltau)
    return np.exp(-m.dtau * (m.lam[:, None] * X + m.lam2[:, None] * X ** 2) / 2).reshape(-1)


def mulLambda(m, v):
    """mulΛ! (HMC.jl:951-973): (Λv)[τ] = -Λ[τ+1] v[τ+1] for τ < L, (Λv)[L] = Λ[1] v[1]; a copy for bond phonons."""
    if m.kind == models.SSH:
        return np.array(v)
    N, L = m.Nsites, m.Ltau
    u, La = np.asarray(v).reshape(N, L), Lambda(m).reshape(N, L)
    out = np.empty((N, L))
    out[:, :L - 1] = -La[:, 1:] * u[:, 1:]
    out[:, L - 1] = La[:, 0] * u[:, 0]
    return out.reshape(-1)


def phis(n):
    return tuple(np.ascontiguousarray(synth.randn(s, n)) for s in SEED_PHI)


def rhs_pair(S):
    """(b₊, b₋) of a Setup: Λϕ± of its model's field."""
    return tuple(np.ascontiguousarray(mulLambda(S.m, p)) for p in phis(S.n))


def stage(S, solver, restart, tol, maxiter, b, transposed, prec=True, dot="blas"):
    """One ldiv! of calc_O⁻¹Λϕ! from a zero guess -> (x, iters, residual_error, flag)."""
    op = "MT" if transposed else "M"
    return ref.mldiv(solver, S.A(op), b, np.zeros(S.n), tol, maxiter, restart, S.P(op) if prec else None, dot=dot)


def stage_margin(S, solver, restart, tol, maxiter, b, transposed, prec=True, dot="blas"):
    """(iters, log-margin) of the solve inside that ldiv!."""
    op = "MT" if transposed else "M"
    return ref.solve(solver, S.A(op), b, np.zeros(S.n), tol, maxiter, maxiter, restart, S.P(op) if prec else None, dot)[1:3]


def fold(it, fl):
    """(iters, flag) of calc_O⁻¹Λϕ! from it[stage][sign], fl[stage][sign] (sign 0: ϕ₊) as HMC.jl:851-909 folds them: per sign the iterations
    add up and the flags combine by max; ϕ₋ is solved only while the flag is zero; cld(total, 2) when the flag is still zero."""
    iters = it[0][0] + it[1][0]
    flag = max(0, fl[0][0], fl[1][0])
    if flag == 0:
        iters += it[0][1] + it[1][1]
        flag = max(flag, fl[0][1], fl[1][1])
    if flag == 0:
        iters = -(-iters // 2)
    return iters, flag


def pair(S, solver, restart, tol, maxiter, prec=True, bs=None):
    """The chained reference for both signs -> dict(X (2, n), Y (2, n), it, fl ([stage][sign]), iters, flag) — every stage run, as the
    library does; the fold decides what counts."""
    bs = rhs_pair(S) if bs is None else bs
    X, Y, it, fl = np.zeros((2, S.n)), np.zeros((2, S.n)), [[0, 0], [0, 0]], [[0, 0], [0, 0]]
    for s, b in enumerate(bs):
        Y[s], it[0][s], _, fl[0][s] = stage(S, solver, restart, tol, maxiter, b, True, prec)
        X[s], it[1][s], _, fl[1][s] = stage(S, solver, restart, tol, maxiter, Y[s], False, prec)
    iters, flag = fold(it, fl)
    if max(fl[0][0], fl[1][0]) > 0:
        X[1] = 0.0
    return dict(X=X, Y=Y, it=it, fl=fl, iters=iters, flag=flag)


def kappa(S, solver, restart, tol, maxiter, prec=True):
    """How far stage 2's x moves, relative, per relative perturbation of stage 1's y: the maximum over both signs and the seeded
    perturbations of size PERTURB."""
    ref_ = pair(S, solver, restart, tol, maxiter, prec)
    worst = 0.0
    for s in range(2):
        y, x = ref_["Y"][s], ref_["X"][s]
        for seed in SEED_PERTURB:
            u = synth.randn(seed, S.n)
            yp = y + PERTURB * np.linalg.norm(y) * u / np.linalg.norm(u)
            xp = stage(S, solver, restart, tol, maxiter, yp, False, prec)[0]
            worst = max(worst, float(np.linalg.norm(xp - x) / np.linalg.norm(x)) / PERTURB)
    return worst


def x_tolerance(k):
    """The device's composed solution against pair(): each stage agrees to 1e-10 (tests/test_gpu_msolvers.py), and stage 2 carries stage
    1's disagreement through with the factor KAPPA."""
    return 1e-10 * (1.0 + k)


# (config, solver, restart, preconditioned, tol, maxiter, KAPPA).  tol: the first of ref.TOLS at which every stage of both signs has a
# log-margin >= ref.MARGIN under every float64 dot product — 1e-5 serves all of them (the smallest margin is 0.11, GMRES(20) on e);
# KAPPA as kappa() measures it (the host test holds it to within a factor 2, and below 1e3).  It is a property of the matrix and the
# field, not of the solver: stage 2 is M⁻¹ to the tolerance, whoever applies it.
_KAPPA = {"b": 0.41, "t": 0.70, "e": 0.45, "d": 0.62}
CASES = tuple((name, solver, restart, True, 1e-5, SOLVER_MAXITER, _KAPPA[name]) for name in ref.MODELS for solver, restart in SOLVERS)
# The un-preconditioned BiCGStab case, on t.  The bare iteration does not converge there: |r| / |b| stays of order 0.1 - 1 for 400
# iterations at every tolerance of ref.TOLS (tests/test_gpu_msolvers.py compares it after 5 iterations for the same reason), so the
# reference's own answer for this case is the flagged one and that is what the case pins, at solver.maxiter = 5 where the summation order
# cannot move it: stage 1 runs out on both signs (flag 1, y = 0), stage 2 sees a zero right-hand side (maxiter iterations, flag 0),
# iters = 5 + 5 not halved, flag 1, X± = 0.  KAPPA has no meaning there (None).
BARE_CASE = ("t", "bicgstab", 0, False, 1e-5, 5, None)


def by_id(cid):
    return {case_id(c): c for c in CASES + (BARE_CASE,)}[cid]


def case_id(case):
    name, solver, restart, prec, tol, maxiter, _ = case
    return f"{name}-{solver}{restart or ''}-{'P' if prec else 'bare'}-{tol:g}"
