"""Host side of the SSH bond correlations of resident chains (elphdynamics_amd/ssh_chain_bond_measurements.py): none of this needs a
device.  The models (tests/test_ssh_bond_measurements_host.build, device=False) never reach a library call: the container constructor
reads host attributes only, and every wrong shape or count is caught before the library."""
import os
from math import comb

import numpy as np
import pytest

import ssh_bond_reference as sbref
from test_ssh_bond_measurements_host import ALL3, CASES, LISTED, TD, build, check_files, yardstick


def chain_model(name, nchains):
    m = build(name)
    m._nchains = nchains
    return m


class FakeEstimator:
    def __init__(self, model, nv):
        self.model, self.nv = model, nv


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def tree(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


def test_one_container_per_chain_with_the_single_configuration_shapes_pairs_and_susceptibility():
    from elphdynamics_amd import ssh_bond_measurements as sb, ssh_chain_bond_measurements as scb
    m = chain_model("hc3", 3)
    info = dict(ALL3, num_random_vectors=3)
    cb = scb.initialize_ssh_chain_bond_container(m, info, ["/a", "/b", "/c"])
    assert cb.nchains == 3 and len(cb.chains) == 3 and cb.n_rand_vecs == 3  # num_random_vectors: per chain
    assert cb._device_of is None and cb._device_est is None
    m._nchains = 1
    one = sb.initialize_ssh_bond_container(m, info, "/a")
    for k, c in enumerate(cb.chains):
        assert isinstance(c, sb.SSHBondContainer) and c.datafolder == "/" + "abc"[k] and c.n_rand_vecs == 3
        assert c.bond_definitions == one.bond_definitions == [(1, 2, (0, 0, 0)), (1, 2, (-1, 0, 0)), (1, 2, (0, -1, 0))]
        assert tuple(c.intersite_corr) == sb.SSH_BOND_CORR
        for name, v in c.intersite_corr.items():                            # default pairs: all n_def^2, first index slowest
            assert v.position.shape == v.momentum.shape == one.intersite_corr[name].position.shape == (9, 3, 3, 1, 9)
            assert v.position.dtype == np.complex128 and v.position.flags["F_CONTIGUOUS"]
            assert v.pairs.tolist() == one.intersite_corr[name].pairs.tolist() == [[1, 1, 1, 2, 2, 2, 3, 3, 3], [1, 2, 3, 1, 2, 3, 1, 2, 3]]
        assert set(c.intersite_susc) == {"BondPairSusc"}                    # CurrentCurrent has no susceptibility
        s = c.intersite_susc["BondPairSusc"]
        assert s.position.shape == s.momentum.shape == (3, 3, 1, 9) and s.pairs is c.intersite_corr["BondPairGreens"].pairs
    # the chains' arrays are their own
    cb.chains[0].intersite_corr["CurrentCurrent"].position[...] = 1
    assert not cb.chains[1].intersite_corr["CurrentCurrent"].position.any()
    # listed pairs, the equal-time requests, per chain
    q = chain_model("hc3x2_listed", 2)
    cb = scb.initialize_ssh_chain_bond_container(q, LISTED, ["", ""])
    assert cb.n_rand_vecs == 1
    for c in cb.chains:
        assert c.intersite_susc == {}
        cc, bb, bp = (c.intersite_corr[k] for k in ("CurrentCurrent", "BondBond", "BondPairGreens"))
        assert cc.position.shape == (1, 3, 2, 1, 3) and cc.pairs.tolist() == [[1, 2, 3], [2, 2, 1]]
        assert bb.position.shape == (8, 3, 2, 1, 2) and bb.pairs.tolist() == [[1, 2], [1, 3]]
        assert bp.position.shape == (1, 3, 2, 1, 1) and bp.pairs.tolist() == [[1], [3]]
    # one chain resident is a lockstep run of one; nothing requested is nothing
    m._nchains = 1
    none = scb.initialize_ssh_chain_bond_container(m, {}, [""])
    assert none.nchains == 1 and none.chains[0].intersite_corr == {} and none.chains[0].intersite_susc == {}


def test_refusals_name_the_request_and_come_before_any_library_call():
    from elphdynamics_amd import lattice as lat, measurements as ms, models, ssh_bond_measurements as sb, ssh_chain_bond_measurements as scb
    from elphdynamics_amd import ssh_chain_measurements as scm
    assert scb.UnsupportedMeasurement is ms.UnsupportedMeasurement
    m = chain_model("psq6", 2)
    m._lib, m._h = NoLibrary(), 1
    for folders in ([""], ["", "", ""]):
        with pytest.raises(ValueError, match="folders.*2 chains"):
            scb.initialize_ssh_chain_bond_container(m, ALL3, folders)
    hol = models.HolsteinModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    hol._nchains = 2
    with pytest.raises(ms.UnsupportedMeasurement, match="Holstein"):
        scb.initialize_ssh_chain_bond_container(hol, {"BondBond": TD}, ["", ""])
    bare = models.SSHModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    bare._nchains = 2
    for name in sbref.CORRS:
        with pytest.raises(ms.UnsupportedMeasurement, match=name + ".*no bond definitions"):
            scb.initialize_ssh_chain_bond_container(bare, {name: TD}, ["", ""])
    scb.initialize_ssh_chain_bond_container(bare, {"BondBond": {"measure": False}}, ["", ""])
    cb = scb.initialize_ssh_chain_bond_container(m, dict(ALL3, num_random_vectors=2), ["", ""])
    hol._lib, hol._h = NoLibrary(), 1
    with pytest.raises(ms.UnsupportedMeasurement, match="Holstein"):        # a container carried over to a Holstein model
        scb.accumulate_ssh_bonds_(cb, hol, FakeEstimator(hol, 4), np.zeros((2, 16)))
    # the single-configuration module keeps refusing the chains, the on-site chain container the three names
    with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
        sb.initialize_ssh_bond_container(m, {"CurrentCurrent": TD}, "")
    for name in sbref.CORRS:
        with pytest.raises(ms.UnsupportedMeasurement, match=name):
            scm.initialize_ssh_chain_measurements_container(m, {name: TD}, ["", ""])


def test_wrong_counts_and_shapes_are_caught_before_the_library():
    from elphdynamics_amd import ssh_chain_bond_measurements as scb
    m = chain_model("tri4_Lt7", 3)
    m._lib, m._h = NoLibrary(), 1
    cb = scb.initialize_ssh_chain_bond_container(m, dict(ALL3, num_random_vectors=3), ["", "", ""])
    X = np.zeros((3, m.Ndof))
    for nv in (3, 6, 10):
        with pytest.raises(ValueError, match="%d vectors.*num_random_vectors = 3 for each of 3 chains" % nv):
            scb.accumulate_ssh_bonds_(cb, m, FakeEstimator(m, nv), X)
    est = FakeEstimator(m, 9)
    for bad in (np.zeros((2, m.Ndof)), np.zeros((3, m.Ndof + 1)), np.zeros(3 * m.Ndof)):
        with pytest.raises(ValueError, match="X has shape"):
            scb.accumulate_ssh_bonds_(cb, m, est, bad)
    m._nchains = 2                                                          # the chains were dropped or changed since
    with pytest.raises(ValueError, match="3 chains, 2 are resident"):
        scb.accumulate_ssh_bonds_(cb, m, est, X)
    m._nchains = 3
    with pytest.raises(RuntimeError, match="no SSH bond correlation"):
        scb.fetch_ssh_bonds_(cb, m)
    scb.reset_ssh_bond_measurements_(cb, m)                                 # no device side yet: host arrays only, no library call
    # with nothing requested nothing is created or launched
    none = scb.initialize_ssh_chain_bond_container(m, {"num_random_vectors": 3}, ["", "", ""])
    scb.accumulate_ssh_bonds_(none, m, est, X)
    assert none._device_of is None


def test_every_chain_gets_the_single_configuration_files_in_its_own_folder(tmp_path):
    from elphdynamics_amd import ssh_bond_measurements as sb, ssh_chain_bond_measurements as scb
    folders = [str(tmp_path / ("chain%d" % k)) for k in range(3)] + [str(tmp_path / "single")]
    for f in folders:
        os.mkdir(f)
    m = chain_model("hc3x2_both_ways", 3)
    info = dict(CASES["hc3x2_both_ways"][1], num_random_vectors=3)
    cb = scb.initialize_ssh_chain_bond_container(m, info, folders[:3])
    scb.initialize_ssh_bond_folders_(cb)
    one = sb.initialize_ssh_bond_container(build("hc3x2_both_ways"), info, folders[3])
    sb.initialize_ssh_bond_folders_(one)
    want = tree(folders[3])
    assert len(want) == 2 * 4                                               # key files of (3 correlations + BondPairSusc) x (position, momentum)
    for f in folders[:3]:
        assert tree(f) == want
        for rel in want:
            assert open(os.path.join(f, rel)).read() == open(os.path.join(folders[3], rel)).read(), rel


def test_process_and_write_of_a_chain_are_the_single_containers(tmp_path, monkeypatch):
    """The same position arrays, put in by hand (what fetch would have copied from the device), give the same numbers and the same files
    as ssh_bond_measurements' single container; a chain's sums are divided by bin_size * binomial(n_rand_vecs, 2), vectors PER CHAIN."""
    from elphdynamics_amd import ssh_bond_measurements as sb, ssh_chain_bond_measurements as scb
    host, R, X, want = yardstick("hc3x2_both_ways")
    nch = 3
    folders = [str(tmp_path / ("chain%d" % k)) for k in range(nch)]
    singles = [str(tmp_path / ("single%d" % k)) for k in range(nch)]
    for f in folders + singles:
        os.mkdir(f)
    m = chain_model("hc3x2_both_ways", nch)
    info = dict(CASES["hc3x2_both_ways"][1], num_random_vectors=4)
    cb = scb.initialize_ssh_chain_bond_container(m, info, folders[:nch])
    scb.initialize_ssh_bond_folders_(cb)
    sums = [{k: (c + 1) * w for k, w in want.items()} for c in range(nch)]  # a chain's own numbers
    for c, s in zip(cb.chains, sums):
        for k, v in c.intersite_corr.items():
            v.position[...] = s[k]
    monkeypatch.setattr(scb, "fetch_ssh_bonds_", lambda cb, model: None)   # the arrays are hand-filled: nothing to fetch
    bin_size = 5
    scb.process_ssh_bond_measurements_(cb, bin_size, m)
    V = bin_size * comb(4, 2)                                               # 4 vectors per chain, not the estimator's 12
    assert V == 30
    scb.write_ssh_bond_measurements_(cb, m, 12)
    single_model = build("hc3x2_both_ways")
    monkeypatch.setattr(sb, "fetch_ssh_bonds_", lambda c, model: None)
    for c, (chain, s) in enumerate(zip(cb.chains, sums)):
        one = sb.initialize_ssh_bond_container(single_model, info, singles[c])
        sb.initialize_ssh_bond_folders_(one)
        for k, v in one.intersite_corr.items():
            v.position[...] = s[k]
        sb.process_ssh_bond_measurements_(one, bin_size, single_model)
        sb.write_ssh_bond_measurements_(one, single_model, 12)
        for grp in ("intersite_corr", "intersite_susc"):
            got, ref = getattr(chain, grp), getattr(one, grp)
            assert set(got) == set(ref)
            for k in ref:
                assert np.array_equal(got[k].position, ref[k].position) and np.array_equal(got[k].momentum, ref[k].momentum), (c, k)
        assert set(chain.intersite_susc) == {"BondPairSusc"}
        for k in s:
            assert np.abs(chain.intersite_corr[k].position - s[k] / V).max() < 1e-15 * max(1.0, np.abs(s[k]).max())
        check_files(folders[c], s, V, m.dtau, 12)
        assert tree(folders[c]) == tree(singles[c]) and len(tree(singles[c])) == 2 * 2 * 4
        for rel in tree(singles[c]):                                        # the same arrays: the same files
            assert open(os.path.join(folders[c], rel)).read() == open(os.path.join(singles[c], rel)).read(), (c, rel)
    scb.reset_ssh_bond_measurements_(cb, m)                                 # no device was ever attached: host arrays only
    for c in cb.chains:
        assert all(not v.position.any() and not v.momentum.any() for g in (c.intersite_corr, c.intersite_susc) for v in g.values())
