"""CPU test of the INPUTS of the hopping-disorder tests (no device): the disorder that configs.make_model(tag, t_stddev=...) draws must
depend on the bond's direction.  With one fresh generator per bond definition every definition drew the same numbers — t_x(cell) ==
t_y(cell) on a square lattice, three equal bonds at every A site of a honeycomb lattice — and a kernel that takes the pair of another
direction's bond of the same cell passed every test built on such a model.  Here, on the oracle: the definitions' hoppings differ, and
exchanging the hoppings of two definitions moves M v by far more than any tolerance of the parity tests (1e-13 ... 1e-10).

kpm_bounds_reference.host_model restates make_model without a handle; tests/test_gpu_hopping_disorder.py asserts that the two agree."""
import itertools

import numpy as np
import pytest

import conftest  # noqa: F401  (the repository root on sys.path)
from elphdynamics_amd import lattice as lat
from elphdynamics_amd import synth
from kpm_bounds_reference import host_model

TAGS = ["C", "D", "u"]      # square (2 definitions), honeycomb (3), triangular (3)


def definition_slices(m):
    """Where each bond definition's hoppings sit in m.t (the order of the assign_t_ calls)."""
    n = [m.lattice.calc_neighbor_table(o1, o2, d).shape[0] for (o1, o2, d) in m.bond_definitions]
    ends = np.cumsum(n)
    assert ends[-1] == len(m.t)
    return [slice(int(e - k), int(e)) for e, k in zip(ends, n)]


def oracle_model(oracle, m, t):
    """The oracle's model of m's lattice and field with the hoppings t (definition order, as m.t)."""
    raw = np.concatenate([m.lattice.calc_neighbor_table(o1, o2, d) for (o1, o2, d) in m.bond_definitions], axis=0)
    cb = lat.initialize_checkerboard(raw, t, m.dtau)
    E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
    return oracle.make_model(0, m.Nsites, m.Ltau, cb["table"], cb["cosht"], cb["sinht"], E)


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("tag", TAGS)
def test_disorder_differs_between_bond_definitions(tag):
    m = host_model(tag, 0.1)
    sl = definition_slices(m)
    assert len(sl) == len(m.bond_definitions) >= 2
    for a, b in itertools.combinations(sl, 2):
        ta, tb = m.t[a], m.t[b]
        assert ta.shape == tb.shape and not np.array_equal(ta, tb)
        # independent draws of standard deviation 0.1: the difference has standard deviation 0.14 — not a few odd bonds
        assert np.std(ta - tb) > 0.05 and np.count_nonzero(ta != tb) == ta.size
    # the disorder is what was asked for, and the uniform model draws nothing
    assert 0.05 < np.std(m.t) < 0.2 and abs(np.mean(m.t) - 1.0) < 0.05
    assert np.array_equal(host_model(tag).t, np.ones(len(m.t)))


@pytest.mark.parametrize("tag", TAGS)
def test_swapping_two_definitions_hoppings_moves_the_matvec(oracle, tag):
    """The power of the inputs: with the hoppings of two definitions exchanged, the oracle's M v moves by more than 1e-3 relative
    (measured: >= 1.2e-2 for every pair of C, D, u) — ten orders above what the parity tests tolerate."""
    m = host_model(tag, 0.1)
    sl = definition_slices(m)
    v = synth.randn(77, m.Ndim)
    om = oracle_model(oracle, m, m.t)
    Mv = oracle.mulM(om, v)
    # (the restated tables are the model's own)
    om_own = oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht,
                               oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu))
    assert np.array_equal(Mv, oracle.mulM(om_own, v))
    for a, b in itertools.combinations(sl, 2):
        t = m.t.copy()
        t[a], t[b] = m.t[b], m.t[a]
        d = rel(oracle.mulM(oracle_model(oracle, m, t), v), Mv)
        print(f"{tag}: definitions at {a.start}, {b.start} exchanged: |M'v - Mv| / |Mv| = {d:.3e}")
        assert d > 1e-3
