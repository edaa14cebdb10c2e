"""The stop rules of solve! and the vector a solve stops with — the cases, held once, for tests/test_stop_rules_host.py (CPU: the
oracle alone) and tests/test_gpu_stop_rules.py (GPU: every CG form against the oracle).

solve! (IterativeSolvers.jl:198-219, :281-302) ends an iteration j >= 1 when
    eps_j = |r_j| / |b| < tol,   or   K_j = max_{i <= j} (2 i / ln(2 eps_0 / eps_i))^2 > kmax,   or   j = maxiter,
and ldiv! (Models.jl:74-186) keeps the vector it ended with whenever the true residual is at most sqrt(tol).  decide() restates the
rule in numpy on a residual history of the oracle and adds the LOG-MARGIN of the decision: the smallest |ln(eps_i / tol)| and
|ln(K_i / kmax)| over every comparison the solve made up to its stop (the ones at j and j - 1 among them; at the stop itself only the
comparison that ended it).  Two implementations that sum in different orders agree on eps to 1e-10 over the first 40 iterations
(header of tests/test_gpu_parity.py); a case whose margin is 1e-3 or more therefore stops at the same iteration, for the same reason,
on every correct implementation — which is what lets the GPU tests ask for EQUAL iteration counts.

Right-hand side and guesses of a model (all from synth.randn): b = M^T randn(SEED_RHS), one vector per model, and three guesses
    zero:  x0 = 0
    near:  x0 = xs (1 + 1e-2 randn(11)), xs the oracle's solution to 1e-13 (of the chain the right-hand side belongs to)
    far:   x0 = c randn(12)
With two chains, chain 0 carries the model's own field and chain 1 the field of chain_fields().

PARAMS[(model, preconditioned)] holds the parameter sets of a model, chosen on the oracle's histories of these very inputs; the host test asserts
every property below for every entry (and for both chains where GPU tests run the model with two), so an entry that does not
deliver is an error there, not a silent gap.
  "P": (tol, kmax, maxiter, c)  near stops by tolerance, zero by kappa, far at maxiter; all three residuals <= sqrt(tol): flags 0
  "F": (tol, kmax, maxiter, c)  near: flag 0; zero: kappa with a residual above sqrt(tol): flag 2; far: maxiter = solver.maxiter: flag 1
  "big": (tol, kmax, maxiter[, kind])  zero guess, kappa stop beyond 0.17 sqrt(kmax) iterations: the first iterations pass the kappa
                                screen of cg_stop_test (and of the copies in cg_wg.hip / pcg_wg.hip), the later ones run the reference's
                                arithmetic.  Preconditioned, K_j of b = M^T randn stays below 35, where the screen never engages:
                                C and C80 take the "slow" right-hand side, whose residual grows at first, for it
  "slow": (tol, kmax, maxiter)  the right-hand side Setup.rhs("slow"), zero guess: the residual grows at first and the kappa stop falls on
                                the first iteration the kappa screen no longer covers, 0.17 sqrt(kmax) <= j < 0.68 sqrt(kmax), with
                                (eps_j / eps_0)^2 >= 8 — a screen four times too wide would skip the deciding term
The coincidence cases are derived from these (singles()): kappa at exactly j = maxiter, tolerance at exactly j = maxiter, and a call
maxiter different from solver.maxiter that runs out with a large residual (flag 2: Models.jl:160 compares solver.maxiter).
The slab form accepts x0 = 0 only: its reasons come from "Z" = (label, tol, kmax, maxiter, reason) on the zero guess, the two
coincidences at j = maxiter among them.  Every model takes the guess seeds (SEED_NEAR, SEED_FAR): none needed another draw.
"""
import numpy as np

from elphdynamics_amd import configs, models, synth
from kpm_bounds_reference import host_model as _host_config_model

MARGIN = 1e-3            # the smallest log-margin a case may have
SENSITIVITY = 1e-4       # x_j differs from x_{j-1} and x_{j+1} by more than this (relative) at every kappa and maxiter stop
LATEST = 40              # no stop later than this: the 1e-10 agreement of two summation orders is stated for 40 iterations
SEED_NEAR, SEED_FAR = 11, 12
SEED_KPM = 11            # numpy.random.default_rng(SEED_KPM): the Arnoldi start vectors of the expansion's bounds
WEAK_BOUNDS = (0.5, 1.9)  # deliberately poor bounds: a weak preconditioner (test_kpm_fallback_to_unpreconditioned)
KINDS = ("zero", "near", "far")

# the 16 x 16 lattice with 80 time slices (test_gpu_parity._holstein_16x16_ltau80): the smallest model on which both resident kernels exist
_C80 = dict(beta=8.0, dtau=0.1, seed=21)

MODEL_NAMES = ("b", "y", "e", "C", "E", "i", "t", "k", "t12", "k40", "l22", "C80")


class _HostHolstein(models.HolsteinModel):
    """A Holstein model without a device handle."""

    def _create(self, *a, **k):
        pass


def _holstein_16x16_ltau80(cls):
    from elphdynamics_amd import lattice as lat
    m = cls(lat.Lattice(1, 16, 16, 1), _C80["beta"], _C80["dtau"], tol=1e-5, maxiter=10000)
    m.assign_t_(1.0, 1, 1, (1, 0, 0)); m.assign_t_(1.0, 1, 1, (0, 1, 0))
    m.assign_omega_(1.0); m.assign_lambda_(1.0); m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, _C80["beta"], _C80["dtau"], omega=1.0, lam=1.0, seed=_C80["seed"])
    assert m.Ltau == 80
    return m


def host_model(name):
    """The model without a device handle: the same lattice, tables and field as gpu_model(name)."""
    return _holstein_16x16_ltau80(_HostHolstein) if name == "C80" else _host_config_model(name)


def gpu_model(name):
    m = _holstein_16x16_ltau80(models.HolsteinModel) if name == "C80" else configs.make_model(name)
    if name == "C80":
        models.update_model_(m)
    return m


def chain_fields(m, nchains=2):
    """(nchains, Ndof): chain 0 is the model's own field; the others differ visibly (another seed / rescaled and roughened bonds)."""
    rows = [np.array(m.x)]
    for c in range(1, nchains):
        if m.kind == models.SSH:
            rows.append(m.x * (0.55 + 0.3 * c) * (1.0 + 0.2 * synth.randn(8000 + c, m.Ndof)))
        else:
            rows.append(synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=8000 + c))
    return np.ascontiguousarray(np.stack(rows))


def ssh_tables(m, x):
    """cosh / sinh of dtau (t - alpha x - sign(x) alpha2 x^2) per (bond, tau) in checkerboard order (SSHModels.jl:510-562), on the host."""
    X = np.asarray(x, dtype=np.float64).reshape(m.Nph, m.Ltau)
    t_ph = m.t[m.phonon_to_bond - 1]
    a = m.dtau * (t_ph[:, None] - (m.alpha[:, None] * X + np.sign(X) * m.alpha2[:, None] * X * X))
    cb = m.checkerboard_perm[m.phonon_to_bond - 1] - 1
    c = np.repeat(np.cosh(m.dtau * m.t_bare_cb)[:, None], m.Ltau, axis=1)
    s = np.repeat(np.sinh(m.dtau * m.t_bare_cb)[:, None], m.Ltau, axis=1)
    c[cb], s[cb] = np.cosh(a), np.sinh(a)
    return np.ascontiguousarray(c), np.ascontiguousarray(s)


def oracle_model(orc, m, x=None):
    """The oracle's model of field x (the model's own when None), from host arrays alone."""
    x = np.ascontiguousarray(m.x if x is None else x, dtype=np.float64)
    if m.kind == models.HOLSTEIN:
        E = orc.update_model_holstein(m.Nsites, m.Ltau, m.dtau, x, m.lam, m.lam2, m.mu)
        return orc.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)
    c, s = ssh_tables(m, x)
    return orc.make_model(1, m.Nsites, m.Ltau, m.neighbor_table, c.reshape(-1), s.reshape(-1), np.exp(m.dtau * m.mu))


# ------------------------------------------------------------------------------------------ the rule

def kappa_terms(hist):
    """K_j, j = 0 .. len(hist) - 1, the running maximum of (2 j / ln(2 eps_0 / eps_j))^2 (K_0 = 0)."""
    h = np.asarray(hist, dtype=np.float64)
    j = np.arange(len(h), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (2.0 * j / np.log(2.0 * h[0] / h)) ** 2
    v[0] = 0.0
    return np.maximum.accumulate(np.where(np.isnan(v), 0.0, v))      # (@fastmath max: NaN never wins)


def decide(hist, tol, kmax, maxiter):
    """(stopping iteration, reason, log-margin) of solve! on the residual history eps_0 .. eps_n (n >= the stop).
    reason: "tol", "kappa" or "maxiter"; a stop by tolerance or kappa AT j = maxiter keeps its reason."""
    h = np.asarray(hist, dtype=np.float64)
    K = kappa_terms(h)
    margin = np.inf

    def lm(a, b):
        return abs(np.log(a / b)) if a > 0.0 else np.inf

    for j in range(1, int(maxiter) + 1):
        assert j < len(h), "the history is shorter than the solve"
        if h[j] < tol:
            return j, "tol", min(margin, lm(h[j], tol))
        if K[j] > kmax:
            return j, "kappa", min(margin, lm(K[j], kmax))
        margin = min(margin, lm(h[j], tol), lm(K[j], kmax))
    return int(maxiter), "maxiter", margin


# ------------------------------------------------------------------------------------------ the oracle's side of a model, computed once

class Setup:
    """Everything the oracle knows about one (model, preconditioned?, chains): models, expansions, right-hand side, guesses, and
    cached histories / solves.  bounds: (e_min, e_max) injected into every chain's expansion; None: EXPLICIT_BOUNDS of the model, else
    Arnoldi bounds from the start vectors of default_rng(SEED_KPM + chain)."""

    HIST = 48

    def __init__(self, orc, name, prec=False, nchains=1, bounds=None):
        self.orc, self.name, self.prec, self.nchains = orc, name, prec, nchains
        bounds = bounds or EXPLICIT_BOUNDS.get(name)
        self.m = host_model(name)
        self.fields = chain_fields(self.m, nchains)
        self.om = [oracle_model(orc, self.m, self.fields[c]) for c in range(nchains)]
        self.b = np.ascontiguousarray(orc.mulMT(self.om[0], synth.rhs(self.m.Ndim)))
        self.oP, self.bounds = [None] * nchains, []
        if prec:
            for c in range(nchains):
                oP = orc.make_kpm(self.om[c], n=20, buf=0.05, c1=1.0, c2=1.0)
                if bounds:
                    orc.kpm_setup(oP, e_min=bounds[0], e_max=bounds[1])
                    self.bounds.append(tuple(bounds))
                else:
                    rng = np.random.default_rng(SEED_KPM + c)
                    self.bounds.append(orc.kpm_setup(oP, b_max=rng.standard_normal(self.m.Nsites), b_min=rng.standard_normal(self.m.Nsites)))
                self.oP[c] = oP
        self._xs, self._cache = {}, {}

    def xs(self, chain=0):
        if chain not in self._xs:
            x, it = self.orc.cg_solve(self.om[chain], self.b, tol=1e-13, maxiter=50000)
            assert it < 50000
            self._xs[chain] = x
        return self._xs[chain]

    def rhs(self, kind="zero", chain=0):
        """The right-hand side of a kind: b, except "slow" — the solution xs scaled to |b|, rich in the low modes of M^T M, from which the
        residual GROWS over the first iterations (eps_1 > 2.83 eps_0: the far side of cg_stop_test's screen)."""
        if kind != "slow":
            return self.b
        xs = self.xs(chain)
        return np.ascontiguousarray(xs * (np.linalg.norm(self.b) / np.linalg.norm(xs)))

    def guess(self, kind, c=1.0, chain=0):
        n = self.m.Ndim
        s_near, s_far = SEED_NEAR, SEED_FAR
        if kind in ("zero", "slow"):
            return np.zeros(n)
        if kind == "near":
            return np.ascontiguousarray(self.xs(chain) * (1.0 + 1e-2 * synth.randn(s_near, n)))
        assert kind == "far"
        return np.ascontiguousarray(float(c) * synth.randn(s_far, n))

    def _memo(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    def hist(self, kind, c=1.0, chain=0):
        """eps_0 .. eps_HIST of the rule-free iteration (tol = 1e-30, kmax = 1e300)."""
        return self._memo(("h", kind, c, chain), lambda: self.orc.cg_solve(
            self.om[chain], self.rhs(kind, chain), x0=self.guess(kind, c, chain), tol=1e-30, maxiter=self.HIST, kmax=1e300, P=self.oP[chain], history=True)[2])

    def iterate(self, kind, c, chain, j):
        """x_j of the rule-free iteration."""
        return self._memo(("x", kind, c, chain, j), lambda: self.orc.cg_solve(
            self.om[chain], self.rhs(kind, chain), x0=self.guess(kind, c, chain), tol=1e-30, maxiter=j, kmax=1e300, P=self.oP[chain])[0])

    def solve(self, kind, c, chain, tol, kmax, maxiter):
        """(x, iters, history) of oracle.cg_solve under the rule."""
        return self._memo(("s", kind, c, chain, tol, kmax, maxiter), lambda: self.orc.cg_solve(
            self.om[chain], self.rhs(kind, chain), x0=self.guess(kind, c, chain), tol=tol, maxiter=maxiter, kmax=kmax, P=self.oP[chain], history=True))

    def ldiv(self, kind, c, chain, tol, kmax, solver_maxiter, maxiter=0):
        """(x, iters, residual_error, flag) of oracle.ldiv."""
        return self._memo(("l", kind, c, chain, tol, kmax, solver_maxiter, maxiter), lambda: self.orc.ldiv(
            self.om[chain], self.rhs(kind, chain), P=self.oP[chain], maxiter=maxiter, solver_tol=tol, solver_maxiter=solver_maxiter, kmax=kmax,
            x0=self.guess(kind, c, chain)))

    def true_residual(self, x, chain=0, kind="zero"):
        b = self.rhs(kind, chain)
        return float(np.linalg.norm(self.orc.mulMTM(self.om[chain], np.ascontiguousarray(x)) - b) / np.linalg.norm(b))


_setups = {}


def setup(orc, name, prec=False, nchains=1, bounds=None):
    key = (name, prec, nchains, bounds)
    if key not in _setups:
        _setups[key] = Setup(orc, name, prec, nchains, bounds)
    return _setups[key]


# ------------------------------------------------------------------------------------------ the matrix

# (model, preconditioned) -> the parameter sets (module docstring).  CHAINS: the models the GPU tests run with two chains; their sets hold
# on both chains.
PARAMS = {
    ("b", False): {"P": (0.032, 48.8, 19, 10.0), "F": (0.0032, 48.8, 19, 300.0), "big": (1e-12, 109.0, 45), "co": (13, 1, 16)},
    ("y", False): {"P": (0.056, 48.8, 19, 30.0), "F": (0.0018, 48.8, 19, 300.0), "big": (1e-12, 100.0, 45), "co": (13, 1, 16)},
    ("e", False): {"P": (0.056, 48.8, 19, 30.0), "F": (0.0056, 48.8, 19, 300.0), "big": (1e-12, 100.0, 45), "co": (11, 1, 16)},
    ("C", False): {"P": (0.032, 41.6, 19, 10.0), "F": (0.0056, 23.9, 13, 300.0), "big": (1e-12, 109.0, 45), "co": (12, 1, 10),
                   "slow": (1e-12, 8.0, 45)},
    ("E", False): {"P": (0.032, 48.8, 19, 30.0), "F": (0.001, 48.8, 19, 300.0), "big": (1e-12, 109.0, 45), "co": (14, 1, 16)},
    # t, 72 unknowns: from iteration 15 on the float64 iteration itself is 1e-7 away from a long-double one, hence maxiter = 12; K_j never
    # exceeds 33, so no kmax with 0.17 sqrt(kmax) > 1 stops it (and k_cg_ap of kernels.hip has no screen): no "big" case
    ("t", False): {"P": (0.1, 29.6, 12, 30.0), "F": (0.018, 29.6, 12, 300.0), "co": (7, 1, 9)},
    ("k", False): {"P": (0.032, 30.3, 18, 30.0), "F": (0.00056, 30.3, 18, 300.0), "big": (1e-12, 44.2, 45), "co": (11, 1, 15)},
    ("t12", False): {"P": (0.056, 52.8, 19, 10.0), "F": (0.0032, 52.8, 19, 300.0), "big": (1e-12, 100.0, 45), "co": (13, 1, 16)},
    # the slab form starts from x0 = 0 only
    # (K_j stays below 35 on both right-hand sides of this model: no kmax engages the kappa side of the screen, 0.17 sqrt(kmax) > 1)
    ("i", False): {"Z": (("Z-tol", 1e-2, 1e12, 40, "tol"), ("Z-kappa", 1e-12, 20.0, 40, "kappa"), ("Z-maxiter", 1e-12, 1e12, 15, "maxiter"),
                         ("kappa-at-maxiter", 1e-12, 20.0, 13, "kappa"), ("tol-at-maxiter", 1e-2, 1e12, 12, "tol"))},
    # KPM-preconditioned: the three guesses converge at one rate, so their kappa histories nearly coincide and the stops come early.  In
    # set F the kappa stop of the zero guess falls ON maxiter where nothing else separates it from the far guess; ldiv! retries both
    # flagged right-hand sides without the expansion either way (Models.jl:129-133), so what comes back is the retry's outcome.
    ("b", True): {"P": (1.3e-04, 0.903, 4, 1.0), "F": (1.16e-05, 0.903, 4, 300.0), "co": (3, 3, 0)},
    ("C", True): {"P": (5.6e-05, 12.1, 19, 100.0), "F": (0.00926, 2.19, 2, 300.0), "co": (18, 10, 0), "big": (1e-12, 90.0, 45, "slow")},
    ("C80", True): {"P": (0.00032, 3.43, 9, 30.0), "F": (0.00429, 1.39, 2, 300.0), "co": (8, 4, 0), "big": (1e-12, 100.0, 45, "slow")},
    ("l22", True): {"P": (1.65e-04, 1.55, 7, 300.0), "F": (4.17e-05, 1.09, 4, 300.0), "co": (6, 3, 0)},
    ("k40", True): {"P": (3.2e-05, 1.63, 8, 300.0), "F": (4.49e-05, 1.1, 4, 300.0), "co": (7, 4, 0)},
}
# The bounds of a model's expansion: Arnoldi bounds from the start vectors of default_rng(SEED_KPM) unless listed.  With Arnoldi bounds
# b, l22 and k40 leave no set P whose kappa stop is early enough for x_j to differ from its neighbours by 1e-4 (b, l22: the only ones
# stop at iterations 11 and 14, where the iterates differ by 1e-6), or none at all (k40: the kappa history of the far guess overtakes
# the zero guess's within one iteration, at every kmax); with the explicit bounds of WEAK_BOUNDS they do.
EXPLICIT_BOUNDS = {"b": WEAK_BOUNDS, "l22": WEAK_BOUNDS, "k40": WEAK_BOUNDS}
CHAINS = (("b", False), ("e", False), ("C", False))

# The retry of flagged right-hand sides inside a preconditioned batch (ldiv_core): two chains, the expansion with WEAK_BOUNDS, four
# right-hand sides (kind, c) — right-hand side r on chain r % 2 — solved with solver (tol, kmax = 1e12, maxiter = 10000) and the call
# maxiter given: the far guesses (slots 1 and 3, chain 1) run out with a residual above sqrt(tol) and are solved again from zero without
# the expansion within 10 x the call maxiter; slots 0 and 2 (chain 0) keep their preconditioned solutions.  model -> (tol, call maxiter)
RETRY_SLOTS = (("near", 1.0), ("far", 300.0), ("zero", 1.0), ("far", 30.0))
RETRY = {"b": (0.024, 2), "C": (0.056, 2)}
RETRY_SOLVER_MAXITER = 10000
DESIGN = {"P": {"near": ("tol", 0), "zero": ("kappa", 0), "far": ("maxiter", 0)},
          "F": {"near": ("tol", 0), "zero": ("kappa", 2), "far": ("maxiter", 1)}}

# the order of a batch: an early tolerance stop in slot 0 and another in the last slot; with two chains (right-hand side r on chain
# r % 2) every kind meets both chains
BATCH = ("near", "zero", "far", "far", "zero", "near")


def singles(key):
    """The single right-hand sides of a model: [(label, kind, c, tol, kmax, call maxiter, solver.maxiter, reason, flag or None)].
    flag None: the flag is whatever the oracle's ldiv gives (asserted equal on the GPU); a number: designed, asserted on the host."""
    p = PARAMS[key]
    out = []
    if "P" in p:
        for s in ("P", "F"):
            tol, kmax, mi, c = p[s]
            for kind in KINDS:
                out.append((f"{s}-{kind}", kind, c, tol, kmax, mi, mi, DESIGN[s][kind][0], None if key[1] else DESIGN[s][kind][1]))
        jk, jt, short = p["co"]              # the stops of the zero and the near guess under set P; a call maxiter short of set F's
        tol, kmax, mi, c = p["P"]
        out.append(("kappa-at-maxiter", "zero", c, tol, kmax, jk, jk, "kappa", None))
        out.append(("tol-at-maxiter", "near", c, tol, kmax, jt, jt, "tol", 0))
        if not key[1]:
            tol, kmax, mi, c = p["F"]
            out.append(("call-maxiter", "far", c, tol, kmax, short, mi, "maxiter", 2))
    for label, tol, kmax, mi, reason in p.get("Z", ()):
        out.append((label, "zero", 1.0, tol, kmax, mi, mi, reason, None))
    if "big" in p:
        tol, kmax, mi, kind = (tuple(p["big"]) + ("zero",))[:4]
        out.append(("big-kappa", kind, 1.0, tol, kmax, mi, mi, "kappa", None))
    if "slow" in p:
        tol, kmax, mi = p["slow"]
        out.append(("slow-kappa", "slow", 1.0, tol, kmax, mi, mi, "kappa", None))
    return out
