"""Host side of the bond correlations of resident chains (elphdynamics_amd/chain_bond_measurements.py): none of this needs a device.  The
models never reach a library call: the container constructor reads host attributes only, and every wrong count is caught before the
library."""
import os

import numpy as np
import pytest

from test_bond_measurements_host import BOTH_WAYS, HONEYCOMB, SMALL, SQUARE, TD
from test_chain_measurements_host import FakeEstimator, NoLibrary, chain_model, tree
from test_measurements_host import host_model


def test_one_bond_container_per_chain_with_the_single_configuration_shapes():
    from elphdynamics_amd import bond_measurements as bm, chain_bond_measurements as cbm
    info = dict(SMALL["hc3x2"][4], num_random_vectors=3)
    m = chain_model(3, ns=2, dims=(3, 2, 1), L=7, bonds=HONEYCOMB)
    cb = cbm.initialize_chain_bond_container(m, info, ["/a", "/b", "/c"])
    assert cb.nchains == 3 and len(cb.chains) == 3 and cb.n_rand_vecs == 3            # num_random_vectors: per chain
    assert cb._device_of is None and cb._device_est is None
    m._nchains = 1
    one = bm.initialize_bond_container(m, info, "/a")
    assert set(one.intersite_corr) == {"BondBond", "BondPairGreens"} and set(one.intersite_susc) == {"BondPairSusc"}
    for k, c in enumerate(cb.chains):
        assert isinstance(c, bm.BondContainer) and c.datafolder == "/" + "abc"[k] and c.n_rand_vecs == 3 and c.bond_definitions == HONEYCOMB
        assert set(c.intersite_corr) == set(one.intersite_corr) and set(c.intersite_susc) == set(one.intersite_susc)
        for grp in ("intersite_corr", "intersite_susc"):
            for name, want in getattr(one, grp).items():
                got = getattr(c, grp)[name]
                assert got.position.shape == got.momentum.shape == want.position.shape
                assert np.array_equal(got.pairs, want.pairs)
        assert c.intersite_susc["BondPairSusc"].pairs is c.intersite_corr["BondPairGreens"].pairs
    # the chains' arrays are their own
    cb.chains[0].intersite_corr["BondBond"].position[...] = 1
    assert not cb.chains[1].intersite_corr["BondBond"].position.any() and not cb.chains[2].intersite_corr["BondBond"].position.any()
    # one chain resident is a lockstep run of one
    cb1 = cbm.initialize_chain_bond_container(m, info, [""])
    assert cb1.nchains == 1 and cb1.chains[0].intersite_corr["BondPairGreens"].position.shape == (8, 3, 2, 1, 2)
    # definitions passed explicitly stand in for the recorded ones, for every chain
    bare = chain_model(2, ns=2, dims=(3, 2, 1), L=7)
    cb2 = cbm.initialize_chain_bond_container(bare, {"BondBond": TD}, ["", ""], bond_definitions=BOTH_WAYS)
    assert all(c.bond_definitions == BOTH_WAYS and c.intersite_corr["BondBond"].position.shape == (8, 3, 2, 1, 9) for c in cb2.chains)
    # nothing requested: empty containers, and accumulate is a no-op that touches no library
    bare._lib, bare._h = NoLibrary(), 1
    none = cbm.initialize_chain_bond_container(bare, {"num_random_vectors": 2}, ["", ""])
    assert all(c.intersite_corr == {} and c.intersite_susc == {} for c in none.chains)
    cbm.accumulate_bonds_(none, bare, FakeEstimator(bare, 4))


def test_refusals_name_the_request():
    from elphdynamics_amd import chain_bond_measurements as cbm, chain_measurements as cms, lattice as lat, measurements as ms, models
    assert cbm.UnsupportedMeasurement is ms.UnsupportedMeasurement
    m = chain_model(2, bonds=SQUARE)
    with pytest.raises(ms.UnsupportedMeasurement, match="CurrentCurrent.*last time slice"):
        cbm.initialize_chain_bond_container(m, {"CurrentCurrent": TD, "BondBond": TD}, ["", ""])
    cbm.initialize_chain_bond_container(m, {"CurrentCurrent": {"measure": False}, "BondBond": TD}, ["", ""])
    bare = chain_model(2)
    for name in ("BondBond", "BondPairGreens"):
        with pytest.raises(ms.UnsupportedMeasurement, match=name + ".*no bond definitions"):
            cbm.initialize_chain_bond_container(bare, {name: TD}, ["", ""])
        with pytest.raises(ms.UnsupportedMeasurement, match=name):
            cbm.initialize_chain_bond_container(m, {name: TD}, ["", ""], bond_definitions=[])
    ssh = models.SSHModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    ssh._nchains = 2
    with pytest.raises(ms.UnsupportedMeasurement, match="SSH"):
        cbm.initialize_chain_bond_container(ssh, {"BondBond": TD}, ["", ""], bond_definitions=SQUARE)
    for folders in ([""], ["", "", ""]):
        with pytest.raises(ValueError, match="folders"):
            cbm.initialize_chain_bond_container(m, {"BondBond": TD}, folders)
    # the on-site chain container goes on refusing the inter-site requests: the two stand side by side
    for name in ("BondBond", "CurrentCurrent", "BondPairGreens"):
        with pytest.raises(ms.UnsupportedMeasurement, match=name):
            cms.initialize_chain_measurements_container(m, {name: TD}, ["", ""])


def test_wrong_counts_are_caught_before_the_library():
    from elphdynamics_amd import chain_bond_measurements as cbm
    m = chain_model(3, ns=1, dims=(4, 4, 1), L=8, bonds=SQUARE)
    m._lib, m._h = NoLibrary(), 1
    cb = cbm.initialize_chain_bond_container(m, {"num_random_vectors": 3, "BondBond": TD, "BondPairGreens": TD}, ["", "", ""])
    for nv in (3, 6, 10):                                                   # 9 = 3 vectors for each of 3 chains
        with pytest.raises(ValueError, match="vectors"):
            cbm.accumulate_bonds_(cb, m, FakeEstimator(m, nv))
    est = FakeEstimator(m, 9)
    m._nchains = 2                                                          # the chains were dropped or changed since
    with pytest.raises(ValueError, match="3 chains"):
        cbm.accumulate_bonds_(cb, m, est)
    m._nchains = 3
    with pytest.raises(AssertionError, match="the library was called: elph_bond_chains_create"):
        cbm.accumulate_bonds_(cb, m, est)                                   # everything right: only now the library is reached
    assert cb._device_of is None
    with pytest.raises(RuntimeError, match="no bond correlation"):
        cbm.fetch_bonds_(cb, m)


def test_process_and_write_per_chain_on_hand_filled_sums(tmp_path, monkeypatch):
    from elphdynamics_amd import bond_measurements as bm, chain_bond_measurements as cbm
    kw = dict(ns=2, dims=(3, 2, 2), L=5, bonds=BOTH_WAYS)
    info = {"num_random_vectors": 4, "BondBond": {"measure": True, "time_dependent": False, "pairs": [[3, 2], [1, 3]]}, "BondPairGreens": TD}
    folders = [str(tmp_path / ("chain%d" % k)) for k in range(3)] + [str(tmp_path / "single")]
    for f in folders:
        os.mkdir(f)
    m = chain_model(3, **kw)
    cb = cbm.initialize_chain_bond_container(m, info, folders[:3])
    cbm.initialize_bond_folders_(cb)
    rng = np.random.default_rng(23)
    raw = []
    for c in cb.chains:
        for corr in c.intersite_corr.values():
            corr.position[...] = rng.standard_normal(corr.position.shape) * 50
        raw.append({k: v.position.copy() for k, v in c.intersite_corr.items()})
    monkeypatch.setattr(cbm, "fetch_bonds_", lambda cb, model: None)        # the arrays are hand-filled: nothing to fetch
    bin_size = 5
    cbm.process_bond_measurements_(cb, bin_size, m)
    V = bin_size * 6                                                        # binomial(4, 2): 4 vectors per chain, not the estimator's 12
    for c, r in zip(cb.chains, raw):
        for k in r:
            assert np.array_equal(c.intersite_corr[k].position, r[k] / V)
            assert np.array_equal(c.intersite_corr[k].momentum, np.fft.fftn(r[k], axes=(1, 2, 3)) / V)
        assert set(c.intersite_susc) == {"BondPairSusc"}
        assert np.array_equal(c.intersite_susc["BondPairSusc"].position, bm.simpson(r["BondPairGreens"] / V, m.dtau))
        assert np.array_equal(c.intersite_susc["BondPairSusc"].momentum, bm.simpson(np.fft.fftn(r["BondPairGreens"], axes=(1, 2, 3)) / V, m.dtau))
    cbm.write_bond_measurements_(cb, m, 12)
    # the single-configuration run of chain 1's sums: the same files, bit for bit, keys included
    s = host_model(**kw)
    one = bm.initialize_bond_container(s, info, folders[3])
    bm.initialize_bond_folders_(one)
    for k, v in one.intersite_corr.items():
        v.position[...] = raw[1][k]
    bm._process_fetched(one, bin_size, s.dtau)
    bm.write_bond_measurements_(one, s, 12)
    want = tree(folders[3])
    assert len(want) == 2 * 2 * 3                                           # (file + key) x (position, momentum) x (BondBond, BondPairGreens, BondPairSusc)
    assert {os.path.dirname(rel) for rel in want} == {"%s_%s_f" % (k, sp) for k in ("BondBond", "BondPairGreens", "BondPairSusc") for sp in ("position", "momentum")}
    for f in folders[:3]:
        assert tree(f) == want
    for rel in want:
        assert open(os.path.join(folders[1], rel)).read() == open(os.path.join(folders[3], rel)).read(), rel
    lines = open(os.path.join(folders[2], "BondBond_position_f", "BondBond_position_00012.out")).read().splitlines()
    flat = (raw[2]["BondBond"] / V).reshape(-1, order="F")
    assert len(lines) == 1 + 12 * 2 and lines[3] == "3 %.8f %.8f" % (flat[2].real, flat[2].imag)
    cbm.reset_bond_measurements_(cb, m)                                     # no device was ever attached: host arrays only
    for c in cb.chains:
        assert all(not v.position.any() and not v.momentum.any() for g in (c.intersite_corr, c.intersite_susc) for v in g.values())
