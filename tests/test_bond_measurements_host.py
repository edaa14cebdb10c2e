"""Host side of the bond correlations (elphdynamics_amd/bond_measurements.py) and the tests' own yardstick (tests/bond_reference.py):
none of this needs a device.  Models here never reach initialize_model_'s library call: the container constructor reads host attributes
only.

The direct-sum yardstick is pinned at the end against its second evaluation with np.fft written as translational_average! writes it
(Utilities.jl:49-60), on the small shapes of tests/test_gpu_bond_measurements.py, at 1e-13 * max(1, max|ref|)."""
import os

import numpy as np
import pytest

import bond_reference as bref
from test_measurements_host import host_model

SQUARE = [(1, 1, (1, 0, 0)), (1, 1, (0, 1, 0))]
HONEYCOMB = [(1, 2, (0, 0, 0)), (1, 2, (-1, 0, 0)), (1, 2, (0, -1, 0))]
BOTH_WAYS = [(1, 2, (0, 0, 0)), (2, 1, (1, 0, 0)), (2, 1, (0, 1, 0))]      # bonds 1 -> 2 and 2 -> 1: a == d, a == c and b == d all occur
CHAIN = [(1, 1, (1, 0, 0))]
CUBIC = [(1, 1, (1, 0, 0)), (1, 1, (1, 1, 0)), (1, 1, (1, 0, 1))]
TD = {"measure": True, "time_dependent": True}

# (norbits, (L1, L2, L3), L, bond definitions, [measurements] table): the small shapes of the GPU test
SMALL = {
    "sq4x4": (1, (4, 4, 1), 8, SQUARE, {"BondBond": TD, "BondPairGreens": TD}),
    "hc3x2": (2, (3, 2, 1), 7, HONEYCOMB, {"BondBond": {"measure": True, "time_dependent": False, "pairs": [[3, 1], [1, 2], [2, 2]]},
                                           "BondPairGreens": {"measure": True, "time_dependent": True, "pairs": [[2, 3], [1, 1]]}}),
    "hc3x2_both_ways": (2, (3, 2, 1), 7, BOTH_WAYS, {"BondBond": TD, "BondPairGreens": TD}),
    "chain12": (1, (12, 1, 1), 6, CHAIN, {"BondBond": TD, "BondPairGreens": TD}),
    "cubic3x2x2": (1, (3, 2, 2), 5, CUBIC, {"BondBond": TD, "BondPairGreens": TD}),
}


def test_assign_t_records_the_bond_definitions_in_order():
    m = host_model(ns=2, dims=(3, 2, 1), L=7, bonds=HONEYCOMB)
    assert m.bond_definitions == HONEYCOMB and m.nbonds == 3
    assert all(isinstance(k, int) for d in m.bond_definitions for k in (d[0], d[1]) + d[2])
    assert host_model().bond_definitions == []
    a, b = host_model(bonds=SQUARE), host_model(bonds=SQUARE[::-1])
    assert a.bond_definitions == SQUARE and b.bond_definitions == SQUARE[::-1]          # per model, call order


def test_container_shapes_pairs_and_susceptibility():
    from elphdynamics_amd import bond_measurements as bm
    m = host_model(ns=2, dims=(3, 2, 1), L=7, bonds=HONEYCOMB)
    info = dict(SMALL["hc3x2"][4], num_random_vectors=3)
    c = bm.initialize_bond_container(m, info, "/nowhere")
    assert c.n_rand_vecs == 3 and c.datafolder == "/nowhere" and c.bond_definitions == HONEYCOMB and c._device_of is None
    bb, bp = c.intersite_corr["BondBond"], c.intersite_corr["BondPairGreens"]
    assert bb.position.shape == bb.momentum.shape == (1, 3, 2, 1, 3) and bb.position.dtype == np.complex128 and bb.position.flags["F_CONTIGUOUS"]
    assert bb.pairs.tolist() == [[1, 2, 3], [2, 2, 1]]                                  # listed, sorted
    assert bp.position.shape == (8, 3, 2, 1, 2) and bp.pairs.tolist() == [[1, 2], [1, 3]]
    assert set(c.intersite_susc) == {"BondPairSusc"}
    s = c.intersite_susc["BondPairSusc"]
    assert s.position.shape == s.momentum.shape == (3, 2, 1, 2) and s.pairs is bp.pairs
    # default pairs: all n_def^2, first index slowest
    c = bm.initialize_bond_container(m, {"BondBond": TD}, "")
    assert c.n_rand_vecs == 1 and set(c.intersite_corr) == {"BondBond"} and c.intersite_susc == {}
    assert c.intersite_corr["BondBond"].pairs.tolist() == [[1, 1, 1, 2, 2, 2, 3, 3, 3], [1, 2, 3, 1, 2, 3, 1, 2, 3]]
    assert c.intersite_corr["BondBond"].position.shape == (8, 3, 2, 1, 9)
    # an equal-time BondPairGreens has no susceptibility
    c = bm.initialize_bond_container(m, {"BondPairGreens": {"measure": True, "time_dependent": False}}, "")
    assert c.intersite_corr["BondPairGreens"].position.shape == (1, 3, 2, 1, 9) and c.intersite_susc == {}
    # measure = false and no table: nothing
    for info in ({}, None, {"BondBond": {"measure": False, "time_dependent": True}, "CurrentCurrent": {"measure": False}}):
        c = bm.initialize_bond_container(m, info, "")
        assert c.intersite_corr == {} and c.intersite_susc == {}
    # definitions passed explicitly win over (and stand in for) the recorded ones
    bare = host_model(ns=2, dims=(3, 2, 1), L=7)
    c = bm.initialize_bond_container(bare, {"BondBond": TD}, "", bond_definitions=[[1, 2, [0, 0, 0]], (2, 1, (1, 0, 0))])
    assert c.bond_definitions == [(1, 2, (0, 0, 0)), (2, 1, (1, 0, 0))] and c.intersite_corr["BondBond"].position.shape == (8, 3, 2, 1, 4)
    assert bm.initialize_bond_container(m, {"BondBond": TD}, "", bond_definitions=SQUARE[:1]).intersite_corr["BondBond"].pairs.tolist() == [[1], [1]]


def test_refusals_name_the_request():
    from elphdynamics_amd import bond_measurements as bm, lattice as lat, measurements as ms, models
    assert bm.UnsupportedMeasurement is ms.UnsupportedMeasurement
    bare = host_model()
    for name in ("BondBond", "BondPairGreens"):
        with pytest.raises(ms.UnsupportedMeasurement, match=name + ".*no bond definitions"):
            bm.initialize_bond_container(bare, {name: TD}, "")
        with pytest.raises(ms.UnsupportedMeasurement, match=name):
            bm.initialize_bond_container(bare, {name: TD}, "", bond_definitions=[])
    m = host_model(bonds=SQUARE)
    with pytest.raises(ms.UnsupportedMeasurement, match="CurrentCurrent.*last time slice"):
        bm.initialize_bond_container(m, {"CurrentCurrent": TD}, "")
    ssh = models.SSHModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    with pytest.raises(ms.UnsupportedMeasurement, match="SSH"):
        bm.initialize_bond_container(ssh, {"BondBond": TD}, "", bond_definitions=SQUARE)
    m._nchains = 2
    with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
        bm.initialize_bond_container(m, {"BondBond": TD}, "")
    with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
        bm.accumulate_bonds_(bm.BondContainer(), m, None)
    # the on-site container goes on refusing the inter-site requests: the bond correlations live beside it
    with pytest.raises(ms.UnsupportedMeasurement, match="BondBond"):
        ms.initialize_measurements_container(host_model(bonds=SQUARE), {"BondBond": TD}, "")
    with pytest.raises(RuntimeError, match="no bond correlation"):
        fresh = host_model(bonds=SQUARE)
        bm.fetch_bonds_(bm.initialize_bond_container(fresh, {"BondBond": TD}, ""), fresh)


def test_folders_key_files_process_and_write(tmp_path):
    from elphdynamics_amd import bond_measurements as bm
    m = host_model(ns=2, dims=(3, 2, 2), L=5, bonds=BOTH_WAYS)
    info = {"num_random_vectors": 4, "BondBond": {"measure": True, "time_dependent": False, "pairs": [[3, 2], [1, 3]]}, "BondPairGreens": TD}
    c = bm.initialize_bond_container(m, info, str(tmp_path))
    bm.initialize_bond_folders_(c)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted("%s_%s_f" % (k, s) for k in ("BondBond", "BondPairGreens", "BondPairSusc") for s in ("position", "momentum"))
    # key files: header, 1-based index in memory order, the pair's bonds, displacements last axis first (tau last)
    rows = open(tmp_path / "BondBond_momentum_f" / "BondBond_momentum_key.out").read().splitlines()
    assert rows[0] == "index bond1 bond2 k3 k2 k1 tau" and len(rows) == 1 + 1 * 3 * 2 * 2 * 2
    assert rows[1] == "1 1 3 0 0 0 0" and rows[2] == "2 1 3 0 0 1 0" and rows[4] == "4 1 3 0 1 0 0" and rows[13] == "13 3 2 0 0 0 0"
    rows = open(tmp_path / "BondPairGreens_position_f" / "BondPairGreens_position_key.out").read().splitlines()
    assert rows[0] == "index bond1 bond2 r3 r2 r1 tau" and len(rows) == 1 + 6 * 12 * 9
    assert rows[1] == "1 1 1 0 0 0 0" and rows[2] == "2 1 1 0 0 0 1" and rows[7] == "7 1 1 0 0 1 0" and rows[73] == "73 1 2 0 0 0 0"
    rows = open(tmp_path / "BondPairSusc_position_f" / "BondPairSusc_position_key.out").read().splitlines()
    assert rows[0] == "index bond1 bond2 r3 r2 r1" and len(rows) == 1 + 12 * 9 and rows[2] == "2 1 1 0 0 1" and rows[13] == "13 1 2 0 0 0"
    assert open(tmp_path / "BondPairSusc_momentum_f" / "BondPairSusc_momentum_key.out").readline() == "index bond1 bond2 k3 k2 k1\n"
    # process and write on sums put in by hand (what fetch_bonds_ would have copied from the device)
    rng = np.random.default_rng(3)
    raw = {k: rng.standard_normal(v.position.shape) for k, v in c.intersite_corr.items()}
    for k, v in c.intersite_corr.items():
        v.position[...] = raw[k]
    c._device_of = m
    m._lib = type("L", (), {"elph_bond_fetch": staticmethod(lambda *a: 0), "elph_bond_reset": staticmethod(lambda *a: 0)})()
    m._h = 1
    bm.process_bond_measurements_(c, 5, m)
    V = 5 * 6                                                               # bin_size * binomial(4, 2)
    for k, v in c.intersite_corr.items():
        assert np.abs(v.position - raw[k] / V).max() < 1e-15
        assert np.abs(v.momentum - np.fft.fftn(raw[k], axes=(1, 2, 3)) / V).max() < 1e-14
    s = c.intersite_susc["BondPairSusc"]
    assert np.abs(s.position - bm.simpson(raw["BondPairGreens"] / V, m.dtau)).max() < 1e-14
    assert np.abs(s.momentum - bm.simpson(np.fft.fftn(raw["BondPairGreens"], axes=(1, 2, 3)) / V, m.dtau)).max() < 1e-14
    bm.write_bond_measurements_(c, m, 12)
    lines = open(tmp_path / "BondPairSusc_momentum_f" / "BondPairSusc_momentum_00012.out").read().splitlines()
    assert lines[0] == "index BondPairSusc_momentum_real BondPairSusc_momentum_imag" and len(lines) == 1 + 12 * 9
    flat = s.momentum.reshape(-1, order="F")
    assert lines[5] == "5 %.8f %.8f" % (flat[4].real, flat[4].imag)
    lines = open(tmp_path / "BondBond_position_f" / "BondBond_position_00012.out").read().splitlines()
    assert lines[0] == "index BondBond_position_real BondBond_position_imag" and len(lines) == 1 + 12 * 2
    bm.reset_bond_measurements_(c, m)
    assert all(not v.position.any() and not v.momentum.any() for g in (c.intersite_corr, c.intersite_susc) for v in g.values())


@pytest.mark.parametrize("case", list(SMALL))
def test_direct_sums_match_the_fft_evaluation(case):
    ns, dims, L, defs, table = SMALL[case]
    from elphdynamics_amd import bond_measurements as bm
    m = host_model(ns=ns, dims=dims, L=L, bonds=defs)
    c = bm.initialize_bond_container(m, table, "")
    request = {k: (v.position.shape[0], v.pairs) for k, v in c.intersite_corr.items()}
    assert set(request) == set(bref.CORRS)
    rng = np.random.default_rng(L)
    N = ns * dims[0] * dims[1] * dims[2]
    R, X = rng.standard_normal((3, N * L)), rng.standard_normal((3, N * L))
    a = bref.measure(R, X, L, ns, dims, defs, request)
    b = bref.measure(R, X, L, ns, dims, defs, request, star=bref.star_fft)
    for k in request:
        assert a[k].shape == c.intersite_corr[k].position.shape and np.isfinite(a[k]).all()
        err = np.abs(a[k] - b[k]).max() / max(1.0, np.abs(a[k]).max())
        print(case, k, "direct sums against np.fft: %.2e" % err, "max|ref| %.3g" % np.abs(a[k]).max())
        assert err < 1e-13, (case, k, err)


def test_the_delta_terms_are_taken_and_skipped():
    """The shapes above reach every branch: a == d (BondBond), delta(a, c) and delta(b, d) (BondPairGreens), each true for some listed pair
    and false for another."""
    seen = {"ad": set(), "ac": set(), "bd": set()}
    for ns, dims, L, defs, table in SMALL.values():
        n = len(defs)
        for name, key in (("BondBond", "ad"), ("BondPairGreens", "ac"), ("BondPairGreens", "bd")):
            pairs = table[name].get("pairs") or [[i, j] for i in range(1, n + 1) for j in range(1, n + 1)]
            for n2, n1 in pairs:
                (d, c, _), (b, a, _) = defs[n2 - 1], defs[n1 - 1]
                seen[key].add({"ad": a == d, "ac": a == c, "bd": b == d}[key])
    assert all(v == {True, False} for v in seen.values()), seen
    ns, dims, L, defs, table = SMALL["hc3x2"]
    for name, key in (("BondBond", "ad"),):
        assert not any(defs[n1 - 1][1] == defs[n2 - 1][0] for n2, n1 in table[name]["pairs"])      # honeycomb 1 -> 2 only: a == d never
