"""Plain numpy restatement of the reference's BiCGStab and GMRES (IterativeSolvers.jl:354-417, :464-584), of the one-sided KPM
preconditioners (KPMPreconditioners.jl:494-600) and of ldiv! for mul_by_M models (Models.jl:74-186) — the reference of
tests/test_msolvers_host.py (CPU: this file checks itself against the oracle) and tests/test_gpu_msolvers.py (GPU).

Setup is dense: M from oracle.mulM on unit vectors of a host model, the Left / Right preconditioners as matrices built from the
oracle's expansion tables.  MatrixFreeSetup (tests/test_msolver_sizes_host.py, tests/test_gpu_msolver_sizes.py: lattices of thousands of
sites) builds no matrix: bicgstab(), gmres() and mldiv() use A and P only through A @ v and P @ v, and take operator objects there — M and
M^T the oracle's mulM / mulMT on a vector, P side_apply(matrix_free=True).  Each solver takes its inner product from
kpm_bounds_reference.DOTS (three float64 summation orders and a sequential long double, the latter with dense operators only); bicgstab()
and gmres() also return the LOG-MARGIN of the solve, the smallest |ln(eps / tol)| over every comparison with the tolerance it made.  Two correct implementations agree on eps far better than a margin of 1e-2, so a case with that
margin stops at the same iteration on both — which is what lets the GPU tests ask for EQUAL iteration counts.

gmres(as_executed=False) is the library's rule; as_executed=True restates solve! literally: the inner loop breaks at
iter == solver_maxiter and update! then back-substitutes over all `restart` columns of H, the ones this cycle never wrote included
(zero in the first cycle: 0/0).  The two coincide whenever the cycle is not cut short.
"""
import numpy as np

from elphdynamics_amd import synth
from kpm_bounds_reference import DOTS, Operator, host_model
import stop_rule_cases as src

SEED_KPM = src.SEED_KPM
MARGIN = 1e-2            # the smallest log-margin a case of the table may have
TOLS = (1e-5, 3e-6, 1e-6, 1e-8)      # a case that falls below MARGIN takes the next of these


def dense_M(orc, om, ndim):
    eye = np.eye(ndim)
    return np.stack([orc.mulM(om, np.ascontiguousarray(eye[k])) for k in range(ndim)], axis=1)


# ------------------------------------------------------------------------------------------ one side of the expansion

def kpm_tables(oP):
    """The oracle's expansion as plain arrays."""
    k = oP._keep
    Lo2 = int(oP.Lo2)
    coff = np.array(k["coff"][:Lo2 + 1])
    ncoef = int(coff[Lo2])
    coeff = k["coeff"][0:2 * ncoef:2] + 1j * k["coeff"][1:2 * ncoef:2]
    return dict(N=int(oP.N), L=int(oP.L), Lo2=Lo2, active=bool(oP.active), order=np.array(k["order"][:Lo2]), coff=coff, coeff=coeff,
                Ebar=np.array(k["Ebar"]), cbar=np.array(k["cbar"]), sbar=np.array(k["sbar"]), lam_avg=float(oP.lam_avg),
                lam_mag=float(oP.lam_mag))


def side_apply(K, table, v, transposed, matrix_free=False):
    """One side of the expansion on v (reference layout, (N L) or (N L, ncols)): the twisted transform (TimeFreqFFTs.jl:37-73), per
    frequency block the Chebyshev series of A' = (A - lam_avg) / lam_mag, A = CBbar diag(Ebar) — Left (transposed False): sum c_n T_n(A'),
    KPMPreconditioners.jl:514-554; Right: sum conj(c_n) T_n(A'^T), :560-600 — the mirror frequencies by conjugation, the inverse transform
    (:112-130).  matrix_free: A' u through Operator.mul / mulT on the (N, ncols) block, bond colour after bond colour, and no N x N matrix."""
    v = np.asarray(v, dtype=np.float64)
    if not K["active"]:
        return v.copy()
    N, L, Lo2 = K["N"], K["L"], K["Lo2"]
    V = v.reshape(N, L, -1)
    t = np.arange(L)
    F = np.exp(-2j * np.pi * np.outer(np.arange(L), t) / L) * np.exp(-1j * np.pi * t / L)[None, :]      # [w, t]
    nu = np.einsum("wt,itc->iwc", F, V)
    op = Operator(table, K["Ebar"], K["cbar"], K["sbar"])
    if matrix_free:
        mul = op.mulT if transposed else op.mul
        Ap = _MatFree(lambda u: (mul(np.ascontiguousarray(u, dtype=np.complex128)) - K["lam_avg"] * u) / K["lam_mag"])
    else:
        A = op.dense()
        if transposed:
            A = A.T
        Ap = (A - K["lam_avg"] * np.eye(N)) / K["lam_mag"]
    out = np.zeros_like(nu)
    for w in range(Lo2):
        order = int(K["order"][w])
        c = K["coeff"][K["coff"][w]:K["coff"][w] + order]
        if transposed:
            c = np.conj(c)
        un = nu[:, w, :]
        acc = c[0] * un
        if order > 1:
            um1, up1, n = None, Ap @ un, 1
            while True:
                n += 1
                um1, un = un, up1
                acc = acc + c[n - 1] * un
                if n == order:
                    break
                up1 = 2.0 * (Ap @ un) - um1
        out[:, L - 1 - w, :] = np.conj(acc)
        out[:, w, :] = acc
    res = np.einsum("wt,iwc->itc", np.conj(F), out).real / L
    return res.reshape(v.shape)


class _MatFree:
    """u -> f(u) behind the @ of a matrix; .T: the operator of ft."""

    matrix_free = True

    def __init__(self, f, ft=None):
        self.f, self.ft = f, ft

    def __matmul__(self, u):
        return self.f(u)

    @property
    def T(self):
        return _MatFree(self.ft, self.f)


def real_operator(f, ft=None):
    """The float64 operator of v -> f(v) (ft: of its transpose) on contiguous vectors, for bicgstab(), gmres() and mldiv()."""
    wrap = lambda g: None if g is None else (lambda u: g(np.ascontiguousarray(u, dtype=np.float64)))      # noqa: E731
    return _MatFree(wrap(f), wrap(ft))


def side_matrix(K, table, transposed):
    n = K["N"] * K["L"]
    return side_apply(K, table, np.eye(n), transposed)


# ------------------------------------------------------------------------------------------ the solvers

def _lm(eps, tol):
    eps = float(eps)
    return abs(np.log(eps / tol)) if eps > 0.0 and np.isfinite(eps) else np.inf


def _cast(dt, *arrs):
    """The arrays in dt; a matrix-free operator passes as it is — it computes in float64 (the oracle's mat-vec), so only with a float64 dt."""
    assert dt is np.float64 or not any(getattr(a, "matrix_free", False) for a in arrs), "the long-double variant is dense-only"
    return [a if a is None or getattr(a, "matrix_free", False) else np.asarray(a, dtype=dt) for a in arrs]


def bicgstab(A, b, x0, tol, maxiter, P=None, dot="blas"):
    """solve!(x, A, b, bicgstab, P; maxiter, tol) (IterativeSolvers.jl:354-417) -> (x, iters, log-margin)."""
    dt, d = DOTS[dot]
    A, b, x, P = _cast(dt, A, b, np.array(x0, dtype=np.float64), P)
    x = x.copy()
    pre = (lambda u: P @ u) if P is not None else (lambda u: u)
    margin = np.inf
    with np.errstate(all="ignore"):
        r = b - A @ x
        rt = r.copy()
        nb = np.sqrt(d(b, b))
        p, v = np.zeros_like(r), np.zeros_like(r)
        alpha, rho1, rho2, omega = dt(0.0), dt(1.0), dt(1.0), dt(1.0)
        for i in range(1, int(maxiter) + 1):
            rho2, rho1 = rho1, d(rt, r)
            if rho1 == 0.0:
                break
            beta = (rho1 / rho2) * (alpha / omega)
            p = r + beta * (p - omega * v)
            ph = pre(p)
            v = A @ ph
            alpha = rho1 / d(rt, v)
            s = r - alpha * v
            eps = np.sqrt(d(s, s)) / nb
            margin = min(margin, _lm(eps, tol))
            if eps < tol:
                return x + alpha * ph, i, margin
            sh = pre(s)
            t = A @ sh
            omega = d(t, s) / d(t, t)
            x = x + (alpha * ph + omega * sh)
            r = s - omega * t
            eps = np.sqrt(d(r, r)) / nb
            margin = min(margin, _lm(eps, tol))
            if eps < tol:
                return x, i, margin
            if omega == 0.0:
                break
    return x, int(maxiter), margin


def _rot(dx, dy):
    """generate_plane_rotation for reals (:579-584): cos, sin of angle(dx + i dy)."""
    th = np.arctan2(dy, dx)
    return np.cos(th), np.sin(th)


def _update(x, k, H, s, V):
    """update!(x, k, H, s, y, V) (:552-570)."""
    y = s.copy()
    for i in range(k - 1, -1, -1):
        y[i] = y[i] / H[i, i]
        for j in range(i - 1, -1, -1):
            y[j] = y[j] - H[j, i] * y[i]
    for j in range(k):
        x = x + y[j] * V[:, j]
    return x


def gmres(A, b, x0, tol, maxiter, solver_maxiter, restart, P=None, dot="blas", as_executed=False):
    """solve!(x, A, b, gmres, M; maxiter, tol) (:464-550) -> (x, iters, log-margin, restarts); see the module docstring for as_executed."""
    dt, d = DOTS[dot]
    A, b, x, P = _cast(dt, A, b, np.array(x0, dtype=np.float64), P)
    x = x.copy()
    n, R = len(b), int(restart)
    pre = (lambda u: P @ u) if P is not None else (lambda u: u)
    H, V = np.zeros((R + 1, R), dtype=dt), np.zeros((n, R + 1), dtype=dt)
    s, cs, sn = np.zeros(R + 1, dtype=dt), np.zeros(R + 1, dtype=dt), np.zeros(R + 1, dtype=dt)
    margin, restarts = np.inf, 0
    with np.errstate(all="ignore"):
        r = pre(b)
        normb = np.sqrt(d(r, r))
        if normb == 0.0:
            normb = dt(1.0)
        r = pre(b - A @ x)
        beta = np.sqrt(d(r, r))
        it = 0
        eps = beta / normb
        margin = min(margin, _lm(eps, tol))
        if eps < tol:
            return x, it, margin, restarts
        while it < maxiter:
            V[:, 0] = r / beta
            s[:] = 0.0
            s[0] = beta
            cols = R
            for i in range(R):
                it += 1
                w = pre(A @ V[:, i])
                for k in range(i + 1):
                    H[k, i] = d(V[:, k], w)
                    w = w - H[k, i] * V[:, k]
                H[i + 1, i] = np.sqrt(d(w, w))
                V[:, i + 1] = w / H[i + 1, i]
                for k in range(i):
                    H[k, i], H[k + 1, i] = cs[k] * H[k, i] + sn[k] * H[k + 1, i], -sn[k] * H[k, i] + cs[k] * H[k + 1, i]
                cs[i], sn[i] = _rot(H[i, i], H[i + 1, i])
                H[i, i], H[i + 1, i] = cs[i] * H[i, i] + sn[i] * H[i + 1, i], -sn[i] * H[i, i] + cs[i] * H[i + 1, i]
                s[i], s[i + 1] = cs[i] * s[i] + sn[i] * s[i + 1], -sn[i] * s[i] + cs[i] * s[i + 1]
                eps = abs(s[i + 1]) / normb
                margin = min(margin, _lm(eps, tol))
                if eps < tol:
                    return _update(x, i + 1, H, s, V), it, margin, restarts
                if it == solver_maxiter:
                    cols = R if as_executed else i + 1
                    break
            x = _update(x, cols, H, s, V)
            restarts += 1
            r = pre(b - A @ x)
            beta = np.sqrt(d(r, r))
            eps = beta / normb
            margin = min(margin, _lm(eps, tol))
            if eps < tol:
                return x, it, margin, restarts
    return x, it, margin, restarts


def solve(solver, A, b, x0, tol, maxiter, solver_maxiter, restart, P=None, dot="blas"):
    """(x, iters, margin) of either solver; maxiter = 0: solver_maxiter."""
    maxiter = maxiter or solver_maxiter
    if solver == "bicgstab":
        return bicgstab(A, b, x0, tol, maxiter, P, dot)
    return gmres(A, b, x0, tol, maxiter, solver_maxiter, restart, P, dot)[:3]


def mldiv(solver, A, b, x0, tol, solver_maxiter, restart, P=None, maxiter=0, dot="blas"):
    """ldiv!(x, model, b[, P]; maxiter) (Models.jl:74-186) -> (x, iters, residual_error, flag)."""
    maxiter = maxiter or solver_maxiter
    A64, b64 = _cast(np.float64, A, b)

    def attempt(x0, P, mi, cmp_maxiter):
        x, it, _ = solve(solver, A, b, x0, tol, mi, solver_maxiter, restart, P, dot)
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            res = float(np.linalg.norm(A64 @ x - b64) / np.linalg.norm(b64))
        flag = 0
        if res > np.sqrt(tol):
            flag = 1 if it == cmp_maxiter else 2
            x = np.zeros_like(x)
        return x, int(it), res, flag

    if P is None:
        return attempt(x0, None, maxiter, solver_maxiter)                # :160 compares solver.maxiter
    out = attempt(x0, P, maxiter, maxiter)                               # :103 compares maxiter
    if out[3] > 0:
        return attempt(np.zeros_like(b64), None, 10 * maxiter, solver_maxiter)      # :129-133
    return out


# ------------------------------------------------------------------------------------------ the oracle's side of a model, computed once

class Setup:
    """One configuration (one chain's field): dense M, right-hand side synth.rhs, the oracle's expansion with Arnoldi bounds from the start
    vectors of default_rng(SEED_KPM + chain) (bounds given: injected), and the dense Left / Right preconditioners."""

    def __init__(self, orc, name, field=None, chain=0, bounds=None):
        self.orc, self.name = orc, name
        self.m = host_model(name)
        self.om = src.oracle_model(orc, self.m, field)
        self.n = self.m.Ndim
        self.M = self._operator()
        self.b = np.ascontiguousarray(synth.rhs(self.n))
        self.oP = orc.make_kpm(self.om, n=20, buf=0.05, c1=1.0, c2=1.0)
        if bounds:
            orc.kpm_setup(self.oP, e_min=bounds[0], e_max=bounds[1])
            self.bounds = tuple(bounds)
        else:
            rng = np.random.default_rng(SEED_KPM + chain)
            self.bounds = orc.kpm_setup(self.oP, b_max=rng.standard_normal(self.m.Nsites), b_min=rng.standard_normal(self.m.Nsites))
        self.K = kpm_tables(self.oP)
        self._side, self._cache = {}, {}

    def _operator(self):
        return dense_M(self.orc, self.om, self.n)

    def A(self, op):
        return self.M.T if op == "MT" else self.M

    def side(self, transposed):
        """The dense Left (False) or Right (True) preconditioner."""
        if transposed not in self._side:
            self._side[transposed] = side_matrix(self.K, self.m.neighbor_table, transposed)
        return self._side[transposed]

    def P(self, op):
        """What LeftRightKPMPreconditioner applies for this operator: Left for M, Right for MT."""
        return self.side(op == "MT")

    def xs(self, op):
        return np.linalg.solve(self.A(op), self.b)

    def guess(self, kind, op, c=1.0):
        """The zero / near / far guesses of stop_rule_cases, rebuilt for M x = b."""
        if kind == "zero":
            return np.zeros(self.n)
        if kind == "near":
            return np.ascontiguousarray(self.xs(op) * (1.0 + 1e-2 * synth.randn(src.SEED_NEAR, self.n)))
        assert kind == "far"
        return np.ascontiguousarray(float(c) * synth.randn(src.SEED_FAR, self.n))

    def solve(self, case, x0=None, prec=True, dot="blas"):
        """(x, iters, margin) of a case of the table from the guess x0 (zero when None)."""
        name, op, solver, restart, tol, maxiter = case
        key = (op, solver, restart, tol, maxiter, prec, dot, None if x0 is None else x0.tobytes())
        if key not in self._cache:
            x0_ = np.zeros(self.n) if x0 is None else x0
            self._cache[key] = solve(solver, self.A(op), self.b, x0_, tol, maxiter, maxiter, restart, self.P(op) if prec else None, dot)
        return self._cache[key]


class MatrixFreeSetup(Setup):
    """The same configuration with no matrix of the size of the problem: M and M^T are the oracle's mulM / mulMT on a vector, the Left / Right
    preconditioners side_apply(matrix_free=True) on a vector or a block of them.  The float64 summation orders only."""

    def _operator(self):
        return real_operator(lambda v: self.orc.mulM(self.om, v), lambda v: self.orc.mulMT(self.om, v))

    def side(self, transposed):
        if transposed not in self._side:
            self._side[transposed] = real_operator(lambda v, t=transposed: side_apply(self.K, self.m.neighbor_table, v, t, matrix_free=True))
        return self._side[transposed]

    def xs(self, op):
        """The solution to a preconditioned residual of 1e-13 (GMRES(20), at most 200 iterations: asserted)."""
        key = ("xs", op)
        if key not in self._cache:
            x, it, _, _ = gmres(self.A(op), self.b, np.zeros(self.n), 1e-13, 200, 200, 20, self.P(op))
            assert it < 200, (self.name, op, it)
            self._cache[key] = x
        return self._cache[key]


_setups = {}


def setup(orc, name, chain=0, nchains=1, bounds=None, matrix_free=False):
    """The Setup of chain `chain` of a model run with nchains chains (fields: stop_rule_cases.chain_fields)."""
    key = (name, chain, nchains, bounds, matrix_free)
    if key not in _setups:
        field = None if nchains == 1 else src.chain_fields(host_model(name), nchains)[chain]
        _setups[key] = (MatrixFreeSetup if matrix_free else Setup)(orc, name, field, chain, bounds)
    return _setups[key]


# ------------------------------------------------------------------------------------------ the cases

MODELS = ("b", "t", "e", "d")
SOLVER_MAXITER = 40      # a multiple of both restarts: the cycle is never cut short, the library's rule and the reference's coincide
# (config, operator, solver, restart, tol, maxiter): preconditioned, zero guess.  tol is one of TOLS with a log-margin >= MARGIN under every
# float64 dot product (the host test asserts it for the value written here): 1e-5, and 1e-8 for GMRES(4), where the solve then crosses two
# or three restarts (13, 15 and 12 iterations on b, e and d; at 1e-5: 8, 9 and 7 — one restart on b and d).  t has 72 unknowns and is done
# after 7 steps even at 1e-8: ONE restart is all GMRES(4) crosses there at any tolerance of TOLS (RESTARTS_MIN).
CASES = tuple((name, op, solver, restart, 1e-8 if restart == 4 else 1e-5, SOLVER_MAXITER)
              for name in MODELS for op in ("M", "MT") for solver, restart in (("bicgstab", 0), ("gmres", 20), ("gmres", 4)))
RESTARTS_MIN = {"b": 2, "e": 2, "d": 2, "t": 1}
# the long un-preconditioned GMRES(20) run on t (72 unknowns): 200 ... 300 iterations
LONG_CASES = (("t", "M", "gmres", 20, 2e-5, 400), ("t", "MT", "gmres", 20, 2e-5, 400))


def case_id(case):
    name, op, solver, restart, tol, maxiter = case
    return f"{name}-{op}-{solver}{restart or ''}-{tol:g}"
