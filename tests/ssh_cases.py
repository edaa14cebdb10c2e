"""The shape and parameter matrix of the bond-phonon (SSH) tests — held once, for tests/test_oracle_ssh_shapes.py (CPU: oracle
vs the dense restatement of ssh_reference.py) and tests/test_gpu_ssh_shapes.py (GPU: device vs oracle and dense restatement).

SHAPES: name -> (orbitals, (L1, L2, L3), bond definitions [(o1, o2, displacement, has_phonon, name, mean t)], Ltau).

Size rule, written once: a case is DENSE when N * Ltau <= DENSE_LIMIT.  Dense cases are compared with the numpy.linalg
restatement as well (on the CPU: all of them, and only them); the others are compared with the oracle alone.

Which kernel family a case reaches (csrc/lattice_shape.cpp: plan_lane_program; csrc/cg_wg.hip: elph_wg_usable) — family() below:
the lane-program kernels (k_mul_fast<NPL,WHICH,SSH>, k_force_ssh<NPL>, k_cg_*<NPL,...>) take a lattice of at most 6 colours and
NPL = ceil(N / 64) <= 8 sites per lane; anything else the generic LDS kernels.  The matrix reaches every instantiated NPL:
  NPL 1: the small cases        NPL 2: sq12x6, sq8x16      NPL 3: sq12, tri12       NPL 4: hc10
  NPL 5: hc12                   NPL 6: sq18                NPL 7: hc14              NPL 8: sq22, hc16
(four-colour programs: square, honeycomb, chains, cu3x2x2, the partial models; six-colour programs: the even triangular lattices
and the five ragged colours of sq5, sq7 and cu4x4x2), and the generic family through the odd triangular lattices (tri3: nine
colours, tri5: eight) and two sizes beyond 512 sites (sq26, hc18: next to e24 of configs.py, several wavefronts per slice).
tests/test_oracle_ssh_shapes.py asserts this coverage from family().

Time axes: the lattices of NPL >= 4 carry Ltau = 6 ... 10 instead of the decks' 20 ... 160 so that the GPU module stays a
small fraction of the suite (these are the shrunk ones: hc10, hc12, hc14, hc16, hc18, sq18, sq22, sq26); no family was dropped.
"""
import numpy as np

from elphdynamics_amd import synth

DTAU = 0.05                  # examples/ssh_hmc_square.toml
DENSE_LIMIT = 2000           # N * Ltau up to which the dense numpy restatement is formed

_X, _Y, _Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def _sq(px=True, py=True, ty=1.0):
    return [(1, 1, _X, px, "x", 1.0), (1, 1, _Y, py, "y", ty)]


def _hc(flags=(True, True, True)):
    return [(1, 2, (0, 0, 0), flags[0], "a", 1.0), (1, 2, (-1, 0, 0), flags[1], "b", 1.0), (1, 2, (0, -1, 0), flags[2], "c", 1.0)]


_TRI = [(1, 1, _X, True, "x", 1.0), (1, 1, _Y, True, "y", 1.0), (1, 1, (1, -1, 0), True, "d", 1.0)]
_CHAIN = [(1, 1, _X, True, "x", 1.0)]
_CUBIC = [(1, 1, _X, True, "x", 1.0), (1, 1, _Y, True, "y", 1.0), (1, 1, _Z, True, "z", 1.0)]

SHAPES = {
    # honeycomb, all three definitions with a phonon: three colours
    "hc3": (2, (3, 3, 1), _hc(), 8),
    "hc6x4": (2, (6, 4, 1), _hc(), 12),
    "hc10": (2, (10, 10, 1), _hc(), 8),             # N = 200
    "hc12": (2, (12, 12, 1), _hc(), 10),            # N = 288
    "hc14": (2, (14, 14, 1), _hc(), 6),             # N = 392
    "hc16": (2, (16, 16, 1), _hc(), 6),             # N = 512: the largest single-wave lattice
    "hc18": (2, (18, 18, 1), _hc(), 6),             # N = 648: generic family, two wavefronts per slice
    # triangular: six colours for even L, nine ragged ones for odd L
    "tri4": (1, (4, 4, 1), _TRI, 10),
    "tri12": (1, (12, 12, 1), _TRI, 8),
    "tri3": (1, (3, 3, 1), _TRI, 6),
    "tri5": (1, (5, 5, 1), _TRI, 6),
    # square: odd (ragged colours), rectangular (the y bonds of sq12x6 carry a NEGATIVE bare hopping), the missing NPL counts
    "sq5": (1, (5, 5, 1), _sq(), 8),
    "sq7": (1, (7, 7, 1), _sq(), 6),
    "sq12x6": (1, (12, 6, 1), _sq(ty=-1.0), 10),
    "sq8x16": (1, (8, 16, 1), _sq(), 8),
    "sq12": (1, (12, 12, 1), _sq(), 6),
    "sq18": (1, (18, 18, 1), _sq(), 6),             # N = 324
    "sq22": (1, (22, 22, 1), _sq(), 6),             # N = 484
    "sq26": (1, (26, 26, 1), _sq(), 6),             # N = 676: generic family, beyond e24
    # chains: two sites (the wrap bond coincides: ONE bond) and a ring
    "ch2": (1, (2, 1, 1), _CHAIN, 8),
    "ch12": (1, (12, 1, 1), _CHAIN, 12),
    # cubic
    "cu3x2x2": (1, (3, 2, 2), _CUBIC, 8),
    "cu4x4x2": (1, (4, 4, 2), _CUBIC, 6),
    # partial models: bare bonds among phonon bonds (Nph < Nbonds, phonon_to_bond not the identity)
    "psq6": (1, (6, 6, 1), _sq(py=False)[::-1], 10),      # phonons on the x bonds only; the bare y bonds come first in the deck
    "phc4": (2, (4, 4, 1), _hc((False, True, False)), 8),      # a phonon on the second of the three definitions
    # time axes: one slice, two, a prime, 161 (divisible by neither 2, 4 nor 8)
    "sq4_Lt1": (1, (4, 4, 1), _sq(), 1),
    "hc3_Lt2": (2, (3, 3, 1), _hc(), 2),
    "tri4_Lt7": (1, (4, 4, 1), _TRI, 7),
    "ch12_Lt161": (1, (12, 1, 1), _CHAIN, 161),
    "sq6x4_Lt161": (1, (6, 4, 1), _sq(), 161),
}

ALL = list(SHAPES)
T_STD, ALPHA_MEAN, ALPHA_STD, OMEGA_MEAN = 0.05, 0.1, 0.02, 0.5

# one case per lattice family for the checks repeated on the generic kernels of a lattice that has lane-program kernels
BOTH_FAMILIES = ["hc6x4", "tri4", "sq12x6", "ch12", "cu4x4x2", "psq6"]
RESIDENT = ["hc6x4", "tri4", "psq6"]                 # honeycomb, even triangular, partial square
DYNAMICS = ["hc6x4", "tri4", "psq6", "cu4x4x2"]      # one HMC update and one Langevin step


def _nsites(name):
    norb, (L1, L2, L3), _, _ = SHAPES[name]
    return norb * L1 * L2 * L3


def is_dense(name):
    return _nsites(name) * SHAPES[name][3] <= DENSE_LIMIT


DENSE = [n for n in ALL if is_dense(n)]


def seed_of(name):
    return 7000 + ALL.index(name)


class Case:
    """The numbers of one case, drawn from numpy.random.default_rng(seed_of(name)).

    t (per raw bond) and alpha (per phonon) follow the ORDER in which SSHModel.initialize_model_ draws its disorder widths
    (per definition: t, then alpha when the definition carries a phonon; SSHModels.jl:381-411), so that a model built with
    t_std / alpha_std from a generator of the same seed holds these very arrays.  alpha2 (both signs), omega, omega4 (per phonon)
    and mu (per site) are drawn afterwards and written over the model's."""

    def __init__(self, name, tab):
        self.name, self.tab = name, tab
        self.norb, self.Ls, self.definitions, self.Ltau = SHAPES[name]
        self.dtau, self.beta, self.seed = DTAU, SHAPES[name][3] * DTAU, seed_of(name)
        self.N, self.Nph, self.Nbonds = tab.N, tab.Nph, tab.Nbonds
        rng = np.random.default_rng(self.seed)
        t, alpha = [], []
        for d, n in zip(self.definitions, tab.per_definition):
            mean = d[5]
            t += list(np.sign(mean) * (abs(mean) + T_STD * rng.standard_normal(n)))
            if d[3]:
                alpha += list(ALPHA_MEAN + ALPHA_STD * rng.standard_normal(n))
        self.t, self.alpha = np.array(t), np.array(alpha)
        self.alpha2 = 0.03 * rng.standard_normal(self.Nph)
        self.omega = OMEGA_MEAN + 0.05 * rng.standard_normal(self.Nph)
        self.omega4 = 0.05 * np.abs(rng.standard_normal(self.Nph))
        self.mu = 0.1 * rng.standard_normal(self.N)
        x = synth.phonon_field(self.Nph, self.Ltau, self.beta, self.dtau, omega=OMEGA_MEAN, lam=0.0, seed=self.seed)
        x = x - x.mean()                                         # both signs on every case, the one-phonon chain included
        # the regime the reference allows (SSHModels.jl:537-539 warns beyond |t'- t| < |t|): shrink x until the coupling term is
        # at most half the smallest bare hopping (for a factor s <= 1, |alpha s x + alpha2 s^2 x^2| <= s (|alpha x| + |alpha2| x^2))
        X = x.reshape(self.Nph, self.Ltau)
        worst = np.max(np.abs(self.alpha)[:, None] * np.abs(X) + np.abs(self.alpha2)[:, None] * X ** 2)
        x = x * min(1.0, 0.5 * np.min(np.abs(self.t)) / worst)
        self.x = np.ascontiguousarray(x)
        X = self.x.reshape(self.Nph, self.Ltau)
        shift = self.alpha[:, None] * X + np.sign(X) * self.alpha2[:, None] * X ** 2
        assert np.max(np.abs(shift)) < 0.8 * np.min(np.abs(self.t)), name
        assert X.min() < 0.0 < X.max(), name
        assert self.Nph == 1 or ((self.alpha2 < 0).any() and (self.alpha2 > 0).any()), name      # (ch2 has one phonon)
        assert ((self.alpha2[:, None] * X) > 0).any() and ((self.alpha2[:, None] * X) < 0).any(), name      # sign(x) alpha2 of both signs

    def vector(self, k, n=None):
        """Deterministic N(0,1) vectors of this case (k-th stream)."""
        return synth.randn(self.seed * 100 + k, self.N * self.Ltau if n is None else n)


def host_view(case, x=None):
    """What the oracle helpers of the GPU tests (_ssh_oracle_bits, _ssh_oracle_force) read from a model, filled from the numpy
    formula on the host arrays (ssh_reference.hopping_tables) instead of the device's own tables."""
    import types
    import ssh_reference as ref
    tab = case.tab
    x = case.x if x is None else np.ascontiguousarray(x)
    c, s = ref.hopping_tables(tab, case.t, case.alpha, case.alpha2, x, case.Ltau, case.dtau)
    return types.SimpleNamespace(Nsites=case.N, Ltau=case.Ltau, dtau=case.dtau, Nbonds=case.Nbonds, Nph=case.Nph, Ndof=case.Nph * case.Ltau,
                                 Ndim=case.N * case.Ltau, neighbor_table=tab.table, checkerboard_perm=tab.cb_perm,
                                 phonon_to_bond=tab.phonon_to_bond, cosht=np.ascontiguousarray(c), sinht=np.ascontiguousarray(s),
                                 expDtauMu=np.exp(case.dtau * case.mu), alpha=case.alpha, alpha2=case.alpha2, x=x)


def oracle_model(oracle, hv):
    """The oracle's model from a host view; the tables are copies (the oracle's updates write into them)."""
    return oracle.make_model(1, hv.Nsites, hv.Ltau, hv.neighbor_table, hv.cosht.reshape(-1).copy(), hv.sinht.reshape(-1).copy(), hv.expDtauMu.copy())


def family(tab):
    """'lane' or 'generic': the rule of build_lane_program (at most 6 colours, at most 8 sites per lane, every colour within the
    lanes' passes), restated so that the tests can say which kernels a case is meant to reach."""
    npl = (tab.N + 63) // 64
    if tab.ncolours > 6 or npl > 8:
        return "generic", npl
    if np.bincount(tab.colours).max() > 64 * ((npl + 1) // 2):
        return "generic", npl
    return "lane", npl


_cache = {}


def make_case(name):
    """(Case, ssh_reference.Tables) of a named shape; the integer tables are cached per session."""
    import ssh_reference as ref
    if name not in _cache:
        norb, (L1, L2, L3), defs, _ = SHAPES[name]
        _cache[name] = ref.Tables(norb, L1, L2, L3, [(d[0], d[1], d[2], d[3]) for d in defs])
    return Case(name, _cache[name])
