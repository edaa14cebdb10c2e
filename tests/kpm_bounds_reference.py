"""Plain numpy restatement of the eigenvalue bounds of the KPM set-up (arnoldi_eigenvalue_bounds!, KPMPreconditioners.jl:845-942) and of
the eigenvalue problem it hands to LAPACK — the reference of tests/test_kpm_hess_host.py and tests/test_gpu_kpm_bounds.py.

A = CBbar diag(Ebar) on N-vectors: CBbar the checkerboard product of the tau-averaged hoppings, bond after bond in the order of the
handle's table (:387-401), A^-1 v = (CBbar^-1 v) ./ Ebar (:406-420).  The n-step modified Gram-Schmidt Arnoldi recursion runs with FOUR
dot products: float64 summed sequentially, pairwise (np.sum) and by BLAS (np.dot), and np.longdouble summed sequentially.  The long-double
run is the reference value; the SPREAD — the largest |float64 variant - long double| — measures what the summation order alone does to
the result, and sets the tolerance of a comparison with any other correct float64 implementation.

Nothing here needs a device: host_model() builds the configurations of elphdynamics_amd.configs without creating a handle.
"""
import numpy as np
import scipy.linalg

from elphdynamics_amd import configs, lattice as lat, models, synth

EPS = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------------------ models without a handle

class _HostHolstein(models.HolsteinModel):
    def _create(self, *a, **k):
        pass


class _HostSSH(models.SSHModel):
    def _create(self, *a, **k):
        pass


# configurations of single test files, written like the rows of configs.CONFIGS and registered here by their case modules
# (tests/msolver_size_cases.py): host_model() knows them by tag; on the device configs.make_model() takes the row itself
LOCAL_CONFIGS = {}


def config_row(tag):
    return configs.CONFIGS[tag] if tag in configs.CONFIGS else LOCAL_CONFIGS[tag]


def host_model(tag, t_stddev=0.0, seed=synth.SEED_FIELDS):
    """configs.make_model(tag) up to, and without, the device handle: the same lattice, bond table, hoppings and field."""
    kind, norb, Ls, bonds, beta, dtau = config_row(tag)
    L1, L2 = Ls if isinstance(Ls, tuple) else (Ls, Ls if Ls > 1 else 1)
    lattice = lat.Lattice(norb, L1, L2, 1)
    if kind == "holstein":
        m = _HostHolstein(lattice, beta, dtau)
        rng = np.random.default_rng(seed + 991)
        for (o1, o2, d) in bonds:
            m.assign_t_(1.0, o1, o2, d, stddev=t_stddev, rng=rng)
        m.assign_omega_(1.0)
        m.assign_lambda_(1.0)
        m.assign_mu_(0.0)
        m.initialize_model_()
        m.x[:] = synth.phonon_field(m.Nph, m.Ltau, beta, dtau, omega=1.0, lam=1.0, seed=seed)
    else:
        m = _HostSSH(lattice, beta, dtau)
        for (o1, o2, d) in bonds:
            m.assign_hopping_(1.0, 0.1, 0.0, 0.1, o1, o2, d, name="xyz"[d.index(1)])
        m.initialize_model_()
        m.x[:] = 0.25 * synth.phonon_field(m.Nph, m.Ltau, beta, dtau, omega=0.1, lam=0.0, seed=seed)
    return m


def chain_fields(m, nchains, seed=5100, base=0.6):
    """Chains with visibly different spectra (different seeds AND different roughness), as test_kpm_preconditioner_per_chain builds them.
    base: the roughness of chain 0 of a Holstein model — the smoother the field, the more the top Ritz value of a 20-step recursion depends
    on the summation order (at base = 0.6 the float64 variants of this reference disagree by up to 1e-3 on the honeycomb lattice, at 1.1 by
    less than 2e-6): the full-depth cases take base = 1.1, where a 2e-5 comparison means something."""
    if m.kind == models.SSH:
        return np.stack([m.x * (0.4 + 1.2 * c / nchains) * (1.0 + 0.3 * synth.randn(seed + c, m.Ndof)) for c in range(nchains)])
    return np.stack([(base + 0.25 * c) * synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=seed + c) for c in range(nchains)])


def averaged_inputs(m, x):
    """update_A! for the field x of one chain (KPMPreconditioners.jl:332-349 Holstein, :355-381 bond phonons): (Ebar[N], cbar[nb], sbar[nb]),
    the hoppings in the order of m.neighbor_table."""
    L = m.Ltau
    if m.kind == models.HOLSTEIN:
        xs = np.asarray(x, dtype=np.float64).reshape(m.Nsites, L)
        with np.errstate(over="ignore", under="ignore"):
            E = np.exp(-m.dtau * (m.lam[:, None] * xs + m.lam2[:, None] * xs * xs - m.mu[:, None]))
        return E.mean(axis=1), np.array(m.cosht, dtype=np.float64), np.array(m.sinht, dtype=np.float64)
    xs = np.asarray(x, dtype=np.float64).reshape(m.Nph, L)
    t_ph = m.t[m.phonon_to_bond - 1]
    a = m.dtau * (t_ph[:, None] - (m.alpha[:, None] * xs + np.sign(xs) * m.alpha2[:, None] * xs * xs))
    cb = m.checkerboard_perm[m.phonon_to_bond - 1] - 1
    cbar, sbar = np.cosh(m.dtau * m.t_bare_cb), np.sinh(m.dtau * m.t_bare_cb)
    cbar[cb], sbar[cb] = np.cosh(a).mean(axis=1), np.sinh(a).mean(axis=1)
    return np.exp(m.dtau * m.mu), cbar, sbar


# ------------------------------------------------------------------------------------------ the operator

def colour_runs(table):
    """The bond table (1-based, (nb, 2)) cut into maximal runs of site-disjoint bonds.  The bonds of a run commute and touch different
    entries, so applying a run at once is the sequential product over its bonds, entry for entry."""
    runs, start, seen = [], 0, set()
    for b, (i, j) in enumerate(np.asarray(table)):
        if i in seen or j in seen:
            runs.append((start, b))
            start, seen = b, set()
        seen.update((int(i), int(j)))
    if len(table):
        runs.append((start, len(table)))
    return runs


class Operator:
    """v -> A v, v -> A^T v and v -> A^-1 v in the dtype of v: an N-vector, or an (N, ncols) block of them."""

    def __init__(self, table, Ebar, cbar, sbar):
        self.table = np.asarray(table, dtype=np.int64).reshape(-1, 2) - 1
        self.Ebar, self.cbar, self.sbar = Ebar, cbar, sbar
        self.runs = colour_runs(self.table + 1)
        self.N = len(Ebar)

    def _cb(self, y, inverse, backwards=None):
        """The checkerboard product on y in place, run after run (backwards: from the last run to the first; the default: as the inverse
        needs it); inverse: every bond factor inverted."""
        dt = y.dtype.type
        col = (-1,) + (1,) * (y.ndim - 1)
        backwards = inverse if backwards is None else backwards
        for (lo, hi) in (reversed(self.runs) if backwards else self.runs):
            i, j = self.table[lo:hi, 0], self.table[lo:hi, 1]
            c, s = self.cbar[lo:hi].astype(dt).reshape(col), self.sbar[lo:hi].astype(dt).reshape(col)
            if inverse:
                s = -s
            t1, t2 = y[i], y[j]
            y[i] = c * t1 + s * t2
            y[j] = c * t2 + s * t1
        return y

    def _E(self, v):
        return self.Ebar.astype(v.dtype).reshape((-1,) + (1,) * (v.ndim - 1))

    def mul(self, v):
        return self._cb(self._E(v) * v, False)

    def mulT(self, v):
        """A^T v = diag(Ebar) CBbar^T v: every bond factor is symmetric, so CBbar^T is the product in the opposite order."""
        return self._E(v) * self._cb(v.copy(), False, backwards=True)

    def div(self, v):
        return self._cb(v.copy(), True) / self._E(v)

    def dense(self, inverse=False):
        eye = np.eye(self.N)
        f = self.div if inverse else self.mul
        return np.stack([f(eye[:, k].copy()) for k in range(self.N)], axis=1)


# ------------------------------------------------------------------------------------------ Arnoldi

def _dot_seq(a, b):
    return np.cumsum(a * b)[-1]            # cumsum adds in index order, in the dtype of its argument


DOTS = {
    "sequential": (np.float64, _dot_seq),
    "pairwise": (np.float64, lambda a, b: np.sum(a * b)),
    "blas": (np.float64, lambda a, b: np.dot(a, b)),
    "longdouble": (np.longdouble, _dot_seq),
}


def arnoldi_hessenberg(apply, b0, n, dot, dtype):
    """The recursion of :859-886: the leading l x l block of h, l = n or the step at which the 1e-12 breakdown rule stopped it."""
    N = len(b0)
    n = max(1, min(n, N))                                          # :136
    b = np.asarray(b0, dtype=dtype).copy()
    with np.errstate(all="ignore"):
        b = b / np.sqrt(dot(b, b))
        Q = np.zeros((N, n + 1), dtype=dtype)
        h = np.zeros((n + 1, n), dtype=dtype)
        Q[:, 0] = b
        l = n
        for k in range(n):
            v = apply(b)
            for j in range(k + 1):
                h[j, k] = dot(Q[:, j], v)
                v = v - h[j, k] * Q[:, j]
            h[k + 1, k] = np.sqrt(dot(v, v))
            if h[k + 1, k] > 1e-12:
                b = v / h[k + 1, k]
                Q[:, k + 1] = b
            else:
                l = k + 1
                break
    return h[:l, :l]


def max_real(h):
    """maximum(real, eigvals!(h')) of :890-895, +inf for a non-finite h."""
    h = np.asarray(h)
    if not np.all(np.isfinite(h)):
        return np.inf
    if h.dtype == np.longdouble and h.shape[0] > 1:
        return float(hessenberg_top(h)["value"])
    return float(np.max(np.linalg.eigvals(np.asarray(h, dtype=np.float64)).real))


def bounds(table, Ebar, cbar, sbar, b_max, b_min, n):
    """(e_min, e_max) of one chain.  Returns a dict: "e_min", "e_max" the long-double values, "variants" {name: (e_min, e_max)},
    "spread" (of e_min, of e_max), and for N <= n "dense" = (e_min, e_max) from the dense spectra of A^-1 and A."""
    op = Operator(table, np.asarray(Ebar, dtype=np.float64), np.asarray(cbar, dtype=np.float64), np.asarray(sbar, dtype=np.float64))
    out = {"variants": {}}
    for name, (dtype, dot) in DOTS.items():
        e_max = max_real(arnoldi_hessenberg(op.mul, b_max, n, dot, dtype))
        r = max_real(arnoldi_hessenberg(op.div, b_min, n, dot, dtype))
        out["variants"][name] = ((1.0 / r) if np.isfinite(r) else -np.inf, e_max)
    ref = out["variants"]["longdouble"]
    out["e_min"], out["e_max"] = ref
    with np.errstate(invalid="ignore"):
        out["spread"] = tuple(max(abs(v[k] - ref[k]) if np.isfinite(ref[k]) else 0.0 for v in out["variants"].values()) for k in (0, 1))
    if op.N <= n and np.all(np.isfinite(Ebar)):
        out["dense"] = (1.0 / float(np.max(np.linalg.eigvals(op.dense(True)).real)), float(np.max(np.linalg.eigvals(op.dense(False)).real)))
    return out


def tolerance(spread, value):
    """What two correct float64 implementations of the recursion may differ by: 32 x the spread of the summation orders, and never less
    than 64 eps |value| (the rounding of the operator itself)."""
    return max(32.0 * spread, 64.0 * EPS * abs(value))


# ------------------------------------------------------------------------------------------ the small eigenvalue problem

def hessenberg_top(H):
    """The eigenvalue of H with the largest real part: {"value": its real part, "kappa": its condition number |y||x| / |y^H x| from the left
    and right eigenvectors, "norm": the Frobenius norm of H, "complex": whether it is one of a complex pair}.  LAPACK's eigenpair is refined
    by the two-sided Rayleigh quotient y^H H x / y^H x in long double, whose error is of second order in the eigenvectors' errors."""
    H = np.asarray(H)
    H64 = np.asarray(H, dtype=np.float64)
    norm = float(np.sqrt(np.sum((H64 / np.max(np.abs(H64))) ** 2)) * np.max(np.abs(H64))) if np.any(H64) else 0.0
    if H.shape[0] == 1:
        return {"value": float(H[0, 0]), "kappa": 1.0, "norm": norm, "complex": False}
    w, vl, vr = scipy.linalg.eig(H64, left=True, right=True)
    k = int(np.argmax(w.real))
    x, y = vr[:, k].astype(np.clongdouble), vl[:, k].astype(np.clongdouble)
    Hl = H.astype(np.longdouble)
    scale = np.max(np.abs(Hl))
    lam = (np.conj(y) @ ((Hl / scale) @ x)) / (np.conj(y) @ x) * scale
    kappa = float(np.linalg.norm(vl[:, k]) * np.linalg.norm(vr[:, k]) / abs(np.vdot(vl[:, k], vr[:, k])))
    return {"value": lam.real, "kappa": kappa, "norm": norm, "complex": bool(abs(w[k].imag) > 1e-8 * abs(w[k]))}


def qr_bound(n, norm, kappa):
    """|computed - exact| of a backward-stable QR iteration: its backward error 32 n eps |H|_F times the first-order sensitivity kappa."""
    return 32.0 * n * EPS * norm * kappa


def hessenberg_cases():
    """[(name, H)] of the QR-stage tests, in one fixed order."""
    cases = [("n1", np.array([[-2.5]])),
             ("real_pair", np.array([[1.0, 2.0], [0.5, -1.0]])),
             ("complex_pair", np.array([[1.0, -2.0], [3.0, 0.5]])),
             ("cyclic3", np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))]
    rng = np.random.default_rng(2024)
    cases.append(("triangular7", np.triu(rng.standard_normal((7, 7)), 1) + np.diag(np.arange(7.0) - 2.5)))
    blocks = np.zeros((12, 12))
    blocks[:] = np.triu(rng.standard_normal((12, 12)), -1)
    blocks[3, 2] = blocks[7, 6] = 0.0                                # blocks of 3, 4 and 5 rows
    cases.append(("blocks12", blocks))
    cases.append(("toeplitz64", 2.0 * np.eye(64) - np.eye(64, k=1) - np.eye(64, k=-1)))
    for n, seed in RANDOM_SEEDS:
        cases.append((f"random{n}_s{seed}", np.triu(np.random.default_rng(seed).standard_normal((n, n)), -1)))
    m = host_model("C")
    X = chain_fields(m, 3)
    Ebar, cbar, sbar = averaged_inputs(m, X[1])
    op = Operator(m.neighbor_table, Ebar, cbar, sbar)
    rs = np.random.default_rng(11)
    cases.append(("arnoldi_A", arnoldi_hessenberg(op.mul, rs.standard_normal(m.Nsites), 20, _dot_seq, np.float64)))
    cases.append(("arnoldi_Ainv", arnoldi_hessenberg(op.div, rs.standard_normal(m.Nsites), 20, _dot_seq, np.float64)))
    base = np.triu(np.random.default_rng(SCALED_SEED).standard_normal((20, 20)), -1)
    cases.append(("scaled_base", base))
    cases.append(("scaled_up", base * 2.0 ** 300))
    cases.append(("scaled_down", base * 2.0 ** -300))
    return cases


# random Hessenberg matrices (n, seed), seeds chosen for a condition number of the top eigenvalue <= 1e3 (3.9, 7.9, 15 and 380: the host test
# asserts it); (20, 8) has a dominant complex pair
RANDOM_SEEDS = ((20, 1), (20, 8), (33, 1), (64, 1))
SCALED_SEED = 7
