"""CPU test of lattice recognition: what elph_create recognises in a bond table (lattice_shape.cpp: elph_recognise_lattice), through the
device-free probe elph_bench_lattice_shape.  The tables are built as models.py builds them; the expected vectors were recorded on the
recogniser this probe was introduced against."""
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (the repository root on sys.path)
from elphdynamics_amd import _lib, configs, synth
from elphdynamics_amd import lattice as lat


# lattices no recogniser knows: simple cubic, and the three-orbital Lieb lattice (a corner site and the two edge sites of a square cell)
CUBIC_BONDS = [(1, 1, (1, 0, 0)), (1, 1, (0, 1, 0)), (1, 1, (0, 0, 1))]
LIEB_BONDS = [(1, 2, (0, 0, 0)), (1, 3, (0, 0, 0)), (2, 1, (1, 0, 0)), (3, 1, (0, 1, 0))]


@functools.lru_cache(maxsize=None)
def tables(kind, norb, Ls, bonds_key, dtau, t_stddev):
    """(nsites, table, cosht, sinht) of a lattice, as HolsteinModel / SSHModel.initialize_model_ build them (configs.make_model's disorder)."""
    bonds = {"sq": lat.SQUARE_BONDS, "hc": lat.HONEYCOMB_BONDS, "tri": lat.TRIANGULAR_BONDS, "cubic": CUBIC_BONDS, "lieb": LIEB_BONDS,
             "none": []}[bonds_key]
    L1, L2, L3 = (Ls + (1,))[:3] if isinstance(Ls, tuple) else (Ls, Ls if Ls > 1 else 1, 1)
    la = lat.Lattice(norb, L1, L2, L3)
    if not bonds:
        return la.nsites, np.zeros((0, 2), dtype=np.int64), np.zeros(0), np.zeros(0)
    raw = np.concatenate([la.calc_neighbor_table(o1, o2, d) for (o1, o2, d) in bonds], axis=0)
    if kind == "ssh":
        return la.nsites, lat.initialize_checkerboard(raw)["table"], None, None
    t = []
    rng = np.random.default_rng(synth.SEED_FIELDS + 991)      # one generator for all bond definitions, as in make_model
    for (o1, o2, d) in bonds:
        n = la.calc_neighbor_table(o1, o2, d).shape[0]
        tn = np.full(n, 1.0)
        if t_stddev:
            tn = tn + t_stddev * rng.standard_normal(n)
        t.append(tn)
    cb = lat.initialize_checkerboard(raw, np.concatenate(t), dtau)
    return la.nsites, cb["table"], cb["cosht"], cb["sinht"]


def bonds_key(bonds):
    return {id(lat.SQUARE_BONDS): "sq", id(lat.HONEYCOMB_BONDS): "hc", id(lat.TRIANGULAR_BONDS): "tri"}.get(id(bonds), "none")


def probe(kind, norb, Ls, bkey, dtau=0.1, t_stddev=0.0, shuffle=False):
    n, tab, c, s = tables(kind, norb, Ls, bkey, dtau, t_stddev)
    if shuffle:
        p = np.random.default_rng(7).permutation(tab.shape[0])
        tab, c, s = tab[p], c[p], s[p]
    v = _lib.lattice_shape(0 if kind == "holstein" else 1, n, tab, c, s)
    return tuple(v[k] for k in _lib.LATTICE_SHAPE_SLOTS)


# every configuration tag; periodic rectangles of the shapes a sharded solve's ring-closed slabs take (16 or 12 columns x a few rows);
# hopping disorder where the patch shape depends on it; a table out of checkerboard order
CASES = {tag: (k, norb, Ls, bonds_key(b), dtau, 0.0, False) for tag, (k, norb, Ls, b, beta, dtau) in configs.CONFIGS.items()}
CASES.update({f"ring_sq{a}x{b}": ("holstein", 1, (a, b), "sq", 0.1, 0.0, False) for a, b in ((16, 4), (16, 6), (16, 8), (16, 10), (32, 4))})
CASES.update({f"ring_hc{a}x{b}": ("holstein", 2, (a, b), "hc", 0.1, 0.0, False) for a, b in ((12, 2), (12, 4), (12, 6), (16, 4))})
CASES.update({f"disorder_sq{L}": ("holstein", 1, L, "sq", 0.1, 0.1, False) for L in (8, 16, 20, 28, 30, 32)})
CASES["disorder_hc12"] = ("holstein", 2, 12, "hc", 0.1, 0.1, False)
CASES["shuffled_sq16"] = ("holstein", 1, 16, "sq", 0.1, 0.0, True)
# look-alikes: cubic 4 x 4 x 4 has 3N bonds in 6 colours, the counts of the 8 x 8 triangular lattice (also out of checkerboard order);
# 4 x 4 x 2 has 5 colours; three orbitals per cell.  None of them is a lattice the register forms know: the generic kernels run.
CASES["cubic4x4x4"] = ("holstein", 1, (4, 4, 4), "cubic", 0.1, 0.0, False)
CASES["shuffled_cubic4x4x4"] = ("holstein", 1, (4, 4, 4), "cubic", 0.1, 0.0, True)
CASES["cubic4x4x2"] = ("holstein", 1, (4, 4, 2), "cubic", 0.1, 0.0, False)
CASES["lieb4x4"] = ("holstein", 3, (4, 4), "lieb", 0.1, 0.0, False)
NOT_RECOGNISED = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0)      # kind NONE: one wavefront, uniform hopping, no bond map

# (slots: _lib.LATTICE_SHAPE_SLOTS)
EXPECTED = {
    'A': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    'B': (8, 8, 1, 0, 0, 0, 0, 0, 0, 0, 1, 4, 4, 0, 1, 1),
    'C': (16, 16, 2, 0, 0, 0, 0, 0, 0, 0, 1, 8, 8, 0, 1, 1),
    'D': (0, 0, 0, 12, 12, 1, 0, 0, 0, 0, 1, 0, 0, 8, 1, 0),
    'E': (16, 16, 2, 0, 0, 0, 0, 0, 0, 0, 1, 8, 8, 0, 0, 1),
    'G': (0, 0, 0, 0, 0, 0, 1, 32, 4, 4, 1, 0, 0, 0, 1, 2),
    'G40': (0, 0, 0, 0, 0, 0, 1, 32, 4, 4, 1, 0, 0, 0, 1, 2),
    'H18': (0, 0, 0, 18, 18, 0, 2, 18, 3, 2, 1, 0, 0, 0, 1, 0),
    'H27': (0, 0, 0, 27, 27, 0, 2, 27, 3, 3, 2, 0, 0, 0, 1, 0),
    'K': (0, 0, 0, 0, 0, 0, 1, 24, 2, 6, 1, 0, 0, 0, 1, 2),
    'L26': (0, 0, 0, 0, 0, 0, 1, 26, 2, 2, 3, 0, 0, 0, 1, 2),
    'L36': (0, 0, 0, 0, 0, 0, 1, 36, 4, 6, 1, 0, 0, 0, 1, 2),
    'L40': (0, 0, 0, 0, 0, 0, 1, 40, 4, 4, 2, 0, 0, 0, 1, 2),
    'Q': (14, 14, 0, 0, 0, 0, 0, 0, 0, 0, 1, 7, 7, 0, 1, 1),
    'R': (8, 16, 0, 0, 0, 0, 0, 0, 0, 0, 1, 4, 8, 0, 1, 0),
    'S': (12, 12, 0, 0, 0, 0, 0, 0, 0, 0, 1, 6, 6, 0, 1, 1),
    'T': (0, 0, 0, 0, 0, 0, 3, 16, 2, 2, 1, 8, 8, 0, 1, 0),
    'W': (0, 0, 0, 12, 8, 0, 0, 0, 0, 0, 1, 0, 0, 4, 1, 0),
    'X24': (0, 0, 0, 24, 24, 0, 2, 24, 3, 3, 1, 0, 0, 0, 1, 0),
    'X32': (0, 0, 0, 0, 0, 0, 1, 32, 4, 4, 1, 0, 0, 0, 1, 2),
    'XT24': (0, 0, 0, 0, 0, 0, 3, 24, 2, 6, 1, 0, 0, 0, 1, 0),
    'Y': (0, 0, 0, 16, 16, 0, 0, 0, 0, 0, 1, 0, 0, 8, 1, 0),
    'b': (4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 0, 1, 1),
    'd': (0, 0, 0, 3, 3, 0, 0, 0, 0, 0, 1, 0, 0, 2, 1, 0),
    'disorder_hc12': (0, 0, 0, 12, 12, 1, 0, 0, 0, 0, 1, 0, 0, 8, 0, 0),
    'disorder_sq16': (16, 16, 2, 0, 0, 0, 0, 0, 0, 0, 1, 8, 8, 0, 0, 1),
    'disorder_sq20': (0, 0, 0, 0, 0, 0, 1, 20, 2, 4, 1, 0, 0, 0, 0, 2),
    'disorder_sq28': (0, 0, 0, 0, 0, 0, 1, 28, 2, 2, 4, 0, 0, 0, 0, 2),
    'disorder_sq30': (0, 0, 0, 0, 0, 0, 1, 30, 2, 2, 4, 0, 0, 0, 0, 2),
    'disorder_sq32': (0, 0, 0, 0, 0, 0, 1, 32, 2, 2, 4, 0, 0, 0, 0, 2),
    'disorder_sq8': (8, 8, 1, 0, 0, 0, 0, 0, 0, 0, 1, 4, 4, 0, 0, 1),
    'e': (4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 0, 0, 1),
    'e12': (12, 12, 0, 0, 0, 0, 0, 0, 0, 0, 1, 6, 6, 0, 0, 1),
    'e20': (0, 0, 0, 0, 0, 0, 1, 20, 2, 4, 1, 0, 0, 0, 0, 2),
    'e24': (0, 0, 0, 0, 0, 0, 1, 24, 2, 6, 1, 0, 0, 0, 0, 2),
    'e8': (8, 8, 1, 0, 0, 0, 0, 0, 0, 0, 1, 4, 4, 0, 0, 1),
    'g': (0, 0, 0, 0, 0, 0, 1, 24, 2, 6, 1, 0, 0, 0, 1, 2),
    'h': (0, 0, 0, 18, 18, 0, 2, 18, 3, 2, 1, 0, 0, 0, 1, 0),
    'h20': (0, 0, 0, 20, 20, 0, 2, 20, 4, 2, 1, 0, 0, 0, 1, 0),
    'h21': (0, 0, 0, 21, 21, 0, 2, 21, 3, 3, 1, 0, 0, 0, 1, 0),
    'h22': (0, 0, 0, 22, 22, 0, 2, 22, 2, 2, 2, 0, 0, 0, 1, 0),
    'h24': (0, 0, 0, 24, 24, 0, 2, 24, 3, 3, 1, 0, 0, 0, 1, 0),
    'h30': (0, 0, 0, 30, 30, 0, 2, 30, 3, 3, 2, 0, 0, 0, 1, 0),
    'i': (0, 0, 0, 0, 0, 0, 1, 18, 2, 6, 1, 0, 0, 0, 1, 2),
    'j': (0, 0, 0, 0, 0, 0, 1, 28, 4, 4, 1, 0, 0, 0, 1, 2),
    'k': (0, 0, 0, 0, 0, 0, 1, 20, 2, 4, 1, 0, 0, 0, 1, 2),
    'k40': (0, 0, 0, 0, 0, 0, 1, 20, 2, 4, 1, 0, 0, 0, 1, 2),
    'l': (4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 0, 1, 1),
    'l22': (0, 0, 0, 0, 0, 0, 1, 22, 2, 2, 2, 0, 0, 0, 1, 2),
    'l26': (0, 0, 0, 0, 0, 0, 1, 26, 2, 2, 3, 0, 0, 0, 1, 2),
    'l30': (0, 0, 0, 0, 0, 0, 1, 30, 2, 10, 1, 0, 0, 0, 1, 2),
    'l34': (0, 0, 0, 0, 0, 0, 1, 34, 2, 2, 5, 0, 0, 0, 1, 2),
    'l36': (0, 0, 0, 0, 0, 0, 1, 36, 4, 6, 1, 0, 0, 0, 1, 2),
    'l40': (0, 0, 0, 0, 0, 0, 1, 40, 4, 4, 2, 0, 0, 0, 1, 2),
    'l48': (0, 0, 0, 0, 0, 0, 1, 48, 4, 4, 3, 0, 0, 0, 1, 2),
    'l64': (0, 0, 0, 0, 0, 0, 1, 64, 4, 4, 4, 0, 0, 0, 1, 2),
    'l800': (4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 0, 1, 1),
    'q': (10, 10, 0, 0, 0, 0, 0, 0, 0, 0, 1, 5, 5, 0, 1, 1),
    'r': (12, 6, 0, 0, 0, 0, 0, 0, 0, 0, 1, 6, 3, 0, 1, 0),
    'ring_hc12x2': (0, 0, 0, 12, 2, 0, 0, 0, 0, 0, 1, 0, 0, 2, 1, 0),
    'ring_hc12x4': (0, 0, 0, 12, 4, 0, 0, 0, 0, 0, 1, 0, 0, 2, 1, 0),
    'ring_hc12x6': (0, 0, 0, 12, 6, 0, 0, 0, 0, 0, 1, 0, 0, 4, 1, 0),
    'ring_hc16x4': (0, 0, 0, 16, 4, 0, 0, 0, 0, 0, 1, 0, 0, 2, 1, 0),
    'ring_sq16x10': (16, 10, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8, 5, 0, 1, 0),
    'ring_sq16x4': (16, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8, 2, 0, 1, 0),
    'ring_sq16x6': (16, 6, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8, 3, 0, 1, 0),
    'ring_sq16x8': (16, 8, 0, 0, 0, 0, 0, 0, 0, 0, 1, 8, 4, 0, 1, 0),
    'ring_sq32x4': (32, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 16, 2, 0, 1, 0),
    's': (6, 6, 0, 0, 0, 0, 0, 0, 0, 0, 1, 3, 3, 0, 1, 1),
    'shuffled_sq16': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    't': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    't12': (0, 0, 0, 0, 0, 0, 3, 12, 2, 2, 1, 6, 6, 0, 1, 0),
    't20': (0, 0, 0, 0, 0, 0, 3, 20, 2, 4, 1, 0, 0, 0, 1, 0),
    't24': (0, 0, 0, 0, 0, 0, 3, 24, 2, 6, 1, 0, 0, 0, 1, 0),
    't32': (0, 0, 0, 0, 0, 0, 3, 32, 4, 4, 1, 0, 0, 0, 1, 0),
    't6': (0, 0, 0, 0, 0, 0, 3, 6, 2, 2, 1, 3, 3, 0, 1, 0),
    'u': (0, 0, 0, 0, 0, 0, 3, 4, 2, 2, 1, 2, 2, 0, 1, 0),
    'w': (0, 0, 0, 6, 4, 0, 0, 0, 0, 0, 1, 0, 0, 2, 1, 0),
    'y': (0, 0, 0, 6, 6, 0, 0, 0, 0, 0, 1, 0, 0, 2, 1, 0),
    'z': (0, 0, 0, 10, 10, 0, 0, 0, 0, 0, 1, 0, 0, 4, 1, 0),
}
EXPECTED.update({case: NOT_RECOGNISED for case in ("cubic4x4x4", "shuffled_cubic4x4x4", "cubic4x4x2", "lieb4x4")})
EXPECTED_NO_MW = {      # where ELPH_PG_MW=0 changes the result
    'H27': (0, 0, 0, 27, 27, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'L26': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'L40': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'disorder_sq28': (0, 0, 0, 0, 0, 0, 1, 28, 4, 4, 1, 0, 0, 0, 0, 2),
    'disorder_sq30': (0, 0, 0, 0, 0, 0, 1, 30, 2, 10, 1, 0, 0, 0, 0, 2),
    'disorder_sq32': (0, 0, 0, 0, 0, 0, 1, 32, 4, 4, 1, 0, 0, 0, 0, 2),
    'h22': (0, 0, 0, 22, 22, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'h30': (0, 0, 0, 30, 30, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'l22': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'l26': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'l34': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'l40': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'l48': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
    'l64': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
}


def test_cubic_look_alike_has_the_triangular_counts():
    """The cubic 4 x 4 x 4 table really reaches match_triangular: 3N bonds, 6 colours, N = 8 x 8 (4 x 4 x 2: 5 colours)."""
    n, tab, c, s = tables("holstein", 1, (4, 4, 4), "cubic", 0.1, 0.0)
    assert n == 64 and tab.shape[0] == 3 * n
    la = lat.Lattice(1, 4, 4, 4)
    raw = np.concatenate([la.calc_neighbor_table(o1, o2, d) for (o1, o2, d) in CUBIC_BONDS], axis=0)
    assert lat.initialize_checkerboard(raw)["ncolours"] == 6
    la = lat.Lattice(1, 4, 4, 2)
    raw = np.concatenate([la.calc_neighbor_table(o1, o2, d) for (o1, o2, d) in CUBIC_BONDS], axis=0)
    assert lat.initialize_checkerboard(raw)["ncolours"] == 5


@pytest.mark.parametrize("case", sorted(CASES))
def test_lattice_shape(case, monkeypatch):
    monkeypatch.delenv("ELPH_PG_MW", raising=False)
    assert probe(*CASES[case]) == EXPECTED[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_lattice_shape_one_wavefront(case, monkeypatch):
    """ELPH_PG_MW=0: patch shapes of one wavefront per slice only (read at recognition)."""
    monkeypatch.setenv("ELPH_PG_MW", "0")
    assert probe(*CASES[case]) == EXPECTED_NO_MW.get(case, EXPECTED[case])
