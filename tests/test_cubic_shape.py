"""CPU test of the simple-cubic lattice recognition (lattice_shape.cpp: match_cubic in elph_recognise_lattice) through the device-free probe
elph_bench_lattice_shape, and of the 2 x 2 x 2 patch layout (pgrid_dev.h: pgrid::Cu) restated in numpy against the bond table.

Recognised: the Holstein model with one (cosh, sinh) for every bond on L x L x L, L = 6, 8, 10, 12 — patch kind 4, reported as side L, PX = PY = 2
and 1, 1, 2, 4 wavefronts per slice; L = 10 and 12 need several wavefronts and are unrecognised with ELPH_PG_MW=0.  Everything else about
a cubic table — smaller and larger cubes, boxes with unequal or odd extents, a table out of checkerboard order, hopping disorder, bond
phonons — keeps the kernels of an unrecognised lattice."""
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (the repository root on sys.path)
import cubic_cases as cc
from elphdynamics_amd import _lib

NOT_RECOGNISED = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0)      # kind NONE: one wavefront, uniform hopping, no bond map


@functools.lru_cache(maxsize=None)
def tables(dims, kind="holstein", t_stddev=0.0):
    return cc.tables(dims, kind, t_stddev)


def probe(dims, kind="holstein", t_stddev=0.0, shuffle=False):
    n, tab, c, s = tables(dims, kind, t_stddev)
    if shuffle:
        p = np.random.default_rng(7).permutation(tab.shape[0])
        tab, c, s = tab[p], c[p], s[p]
    v = _lib.lattice_shape(0 if kind == "holstein" else 1, n, tab, c, s)
    return tuple(v[k] for k in _lib.LATTICE_SHAPE_SLOTS)


def expected(L, nw):
    # (slots: _lib.LATTICE_SHAPE_SLOTS) patch kind 4, side L, 2 x 2 (x 2) sites per thread, nw wavefronts, uniform hopping, no bond map
    return (0, 0, 0, 0, 0, 0, 4, L, 2, 2, nw, 0, 0, 0, 1, 0)


@pytest.mark.parametrize("L", cc.SIDES)
def test_cube_is_recognised(L, monkeypatch):
    monkeypatch.delenv("ELPH_PG_MW", raising=False)
    assert probe((L, L, L)) == expected(L, cc.NW[L])


@pytest.mark.parametrize("L", cc.SIDES)
def test_cube_one_wavefront(L, monkeypatch):
    """ELPH_PG_MW=0: patch shapes of one wavefront per slice only."""
    monkeypatch.setenv("ELPH_PG_MW", "0")
    assert probe((L, L, L)) == (expected(L, 1) if cc.NW[L] == 1 else NOT_RECOGNISED)


@pytest.mark.parametrize("case,args", [
    ("4x4x4", dict(dims=(4, 4, 4))),
    ("14x14x14", dict(dims=(14, 14, 14))),
    ("6x6x4", dict(dims=(6, 6, 4))),
    ("6x8x10", dict(dims=(6, 8, 10))),
    ("5x6x6", dict(dims=(5, 6, 6))),
    ("shuffled_6x6x6", dict(dims=(6, 6, 6), shuffle=True)),
    ("disorder_6x6x6", dict(dims=(6, 6, 6), t_stddev=0.1)),
    ("ssh_6x6x6", dict(dims=(6, 6, 6), kind="ssh")),
])
def test_not_recognised(case, args, monkeypatch):
    monkeypatch.delenv("ELPH_PG_MW", raising=False)
    want = NOT_RECOGNISED
    if case.startswith(("disorder", "ssh")):
        want = want[:14] + (0,) + want[15:]      # (no single (cosh, sinh))
    assert probe(**args) == want


@pytest.mark.parametrize("L", cc.SIDES)
def test_patch_layout_against_the_bond_table(L):
    """pgrid::Cu's site map is a permutation of the sites, and the colours of the table are what its sweeps assume: an even colour of direction
    D pairs the registers (q, q ^ (1 << D)) of one patch; an odd colour pairs the high face of a patch with the low face of the patch above."""
    n, tab, c, s = tables((L, L, L))
    site = cc.site_of(L)
    G = L // 2
    assert site.shape == (G ** 3, 8) and np.array_equal(np.sort(site.ravel()), np.arange(n))
    lane_of, reg_of = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    lane_of[site] = np.arange(G ** 3)[:, None]
    reg_of[site] = np.arange(8)[None, :]
    assert tab.shape[0] == 3 * n
    for col in range(6):
        D, odd = col // 2, col % 2
        b = tab[col * (n // 2):(col + 1) * (n // 2)] - 1
        i, j = b[:, 0], b[:, 1]
        assert np.unique(b).size == n                                   # every site once per colour
        assert np.array_equal(reg_of[i] ^ reg_of[j], np.full(n // 2, 1 << D))
        if not odd:
            assert np.array_equal(lane_of[i], lane_of[j])
        else:
            hi = np.where((reg_of[i] >> D) & 1, i, j)                  # the site on the high face; its partner is on the low face above
            lo = np.where((reg_of[i] >> D) & 1, j, i)
            coord = lambda lane: (lane // G ** np.arange(3)[:, None]) % G      # noqa: E731  (X, Y, Z) of the patches
            step = np.zeros((3, 1), dtype=np.int64)
            step[D] = 1
            assert np.array_equal((coord(lane_of[hi]) + step) % G, coord(lane_of[lo]))
