"""Host side of the measurements of resident chains (elphdynamics_amd/chain_measurements.py): none of this needs a device.  The models
never reach a library call: the container constructor reads host attributes only, and every wrong shape is caught before the library."""
import os

import numpy as np
import pytest

from test_measurements_host import FULL, host_model


def chain_model(nchains, **kw):
    m = host_model(**kw)
    m._nchains = nchains
    return m


def test_one_container_per_chain_with_the_single_configuration_shapes():
    from elphdynamics_amd import chain_measurements as cms, measurements as ms
    m = chain_model(3, ns=2, dims=(3, 2, 1), L=7)
    cm = cms.initialize_chain_measurements_container(m, FULL, ["/a", "/b", "/c"])
    assert cm.nchains == 3 and len(cm.chains) == 3 and cm.n_rand_vecs == 3            # num_random_vectors: per chain
    m._nchains = 1
    one = ms.initialize_measurements_container(m, FULL, "/a")
    for k, c in enumerate(cm.chains):
        assert isinstance(c, ms.MeasurementsContainer) and c.datafolder == "/" + "abc"[k] and c.n_rand_vecs == 3
        assert set(c.onsite_corr) == set(one.onsite_corr) and set(c.onsite_susc) == set(one.onsite_susc)
        for name in one.onsite_corr:
            assert c.onsite_corr[name].position.shape == one.onsite_corr[name].position.shape
            assert np.array_equal(c.onsite_corr[name].pairs, one.onsite_corr[name].pairs)
        assert all(v.shape == (2,) for v in c.onsite_meas.values()) and set(c.global_meas) == {"density", "Nsqr", "mu"}
    # the chains' arrays are their own
    cm.chains[0].onsite_corr["Greens"].position[...] = 1
    assert not cm.chains[1].onsite_corr["Greens"].position.any()
    # one chain resident is a lockstep run of one
    assert cms.initialize_chain_measurements_container(m, {}, [""]).nchains == 1


def test_refusals_name_the_request():
    from elphdynamics_amd import chain_measurements as cms, lattice as lat, models
    m = chain_model(2)
    for name in ("BondBond", "CurrentCurrent", "BondPairGreens"):
        info = dict(FULL)
        info[name] = {"measure": True, "time_dependent": True}
        with pytest.raises(cms.UnsupportedMeasurement, match=name):
            cms.initialize_chain_measurements_container(m, info, ["", ""])
        info[name] = {"measure": False, "time_dependent": True}
        cms.initialize_chain_measurements_container(m, info, ["", ""])
    for key in ("density", "double_occupancy", "phonon_position"):
        with pytest.raises(cms.UnsupportedMeasurement, match="Snapshots.*" + key):
            cms.initialize_chain_measurements_container(m, {"Snapshots": {key: True}}, ["", ""])
    ssh = models.SSHModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    ssh._nchains = 2
    with pytest.raises(cms.UnsupportedMeasurement, match="SSH"):
        cms.initialize_chain_measurements_container(ssh, FULL, ["", ""])
    for folders in ([""], ["", "", ""]):
        with pytest.raises(ValueError, match="folders"):
            cms.initialize_chain_measurements_container(m, FULL, folders)


class FakeEstimator:
    def __init__(self, model, nv):
        self.model, self.nv = model, nv


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def test_wrong_counts_and_shapes_are_caught_before_the_library():
    from elphdynamics_amd import chain_measurements as cms
    m = chain_model(3, ns=1, dims=(4, 4, 1), L=8)
    m._lib, m._h = NoLibrary(), 1
    cm = cms.initialize_chain_measurements_container(m, FULL, ["", "", ""])
    X = np.zeros((3, m.Ndof))
    with pytest.raises(ValueError, match="9|vectors"):
        cms.accumulate_(cm, m, FakeEstimator(m, 3), X)                      # 3 vectors for 3 chains x 3
    with pytest.raises(ValueError, match="vectors"):
        cms.make_measurements_(cm, m, FakeEstimator(m, 6), X, 1)
    est = FakeEstimator(m, 9)
    for bad in (np.zeros((2, m.Ndof)), np.zeros((3, m.Ndof + 1)), np.zeros(3 * m.Ndof)):
        with pytest.raises(ValueError, match="X has shape"):
            cms.accumulate_(cm, m, est, bad)
    for bad in (np.zeros(m.Nsites), np.zeros((3, m.Nsites - 1)), np.zeros((1, m.Nsites))):
        with pytest.raises(ValueError, match="mu has shape"):
            cms.accumulate_(cm, m, est, X, mu=bad)
        with pytest.raises(ValueError, match="mu has shape"):
            cms.make_measurements_(cm, m, est, X, 1, mu=bad)
    m._nchains = 2                                                          # the chains were dropped or changed since
    with pytest.raises(ValueError, match="3 chains"):
        cms.accumulate_(cm, m, est, X)
    with pytest.raises(RuntimeError, match="nothing has been measured"):
        cms.fetch_(cm, m)


def tree(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


def test_every_chain_gets_the_single_configuration_folder_tree(tmp_path):
    from elphdynamics_amd import chain_measurements as cms, measurements as ms
    info = {"num_random_vectors": 4, "Greens": {"measure": True, "time_dependent": True},
            "PairGreens": {"measure": True, "time_dependent": True, "pairs": [[2, 1], [1, 2]]},
            "DenDen": {"measure": True, "time_dependent": False, "pairs": [[1, 2]]}}
    kw = dict(ns=2, dims=(3, 2, 2), L=5, bonds=[(1, 1, (1, 0, 0)), (1, 2, (1, 1, 0))])
    folders = [str(tmp_path / ("chain%d" % k)) for k in range(3)] + [str(tmp_path / "single")]
    for f in folders:
        os.mkdir(f)
    m = chain_model(3, **kw)
    cm = cms.initialize_chain_measurements_container(m, info, folders[:3])
    cms.initialize_measurement_folders_(cm)
    cms.write_measurements_(cm, m, 4)
    s = host_model(**kw)
    one = ms.initialize_measurements_container(s, info, folders[3])
    ms.initialize_measurement_folders_(one)
    ms.write_measurements_(one, s, 4)
    want = tree(folders[3])
    assert len(want) == 3 + 2 * 2 * 4                                       # scalars; (file + key) x (position, momentum) x (3 correlations + PairSusc)
    for f in folders[:3]:
        assert tree(f) == want
        for rel in want:                                                    # zeros everywhere: the files themselves agree, keys included
            assert open(os.path.join(f, rel)).read() == open(os.path.join(folders[3], rel)).read(), rel


def test_process_divides_by_bin_size_times_the_pairs_of_a_chains_vectors(monkeypatch):
    from elphdynamics_amd import chain_measurements as cms, measurements as ms
    m = chain_model(3, ns=2, dims=(3, 2, 2), L=5, bonds=[(1, 1, (1, 0, 0))])
    info = {"num_random_vectors": 4, "Greens": {"measure": True, "time_dependent": True}, "PairGreens": {"measure": True, "time_dependent": True},
            "DenDen": {"measure": True, "time_dependent": False, "pairs": [[1, 2]]}}
    cm = cms.initialize_chain_measurements_container(m, info, ["", "", ""])
    rng = np.random.default_rng(17)
    raw = []
    for c in cm.chains:
        for k in c.global_meas:
            c.global_meas[k] = complex(rng.standard_normal() * 50)
        for grp in (c.onsite_meas, c.intersite_meas):
            for k in grp:
                grp[k][:] = rng.standard_normal(grp[k].shape) * 50
        for corr in c.onsite_corr.values():
            corr.position[...] = rng.standard_normal(corr.position.shape) * 50
        raw.append((dict(c.global_meas), {k: v.copy() for k, v in c.onsite_meas.items()}, c.intersite_meas["el_ke"].copy(),
                    {k: v.position.copy() for k, v in c.onsite_corr.items()}))
    monkeypatch.setattr(cms, "fetch_", lambda cm, model: None)              # the arrays are hand-filled: nothing to fetch
    bin_size = 5
    cms.process_measurements_(cm, bin_size, m)
    V = bin_size * 6                                                        # binomial(4, 2): 4 vectors per chain, not the estimator's 12
    for c, (g, o, b, corr) in zip(cm.chains, raw):
        assert all(c.global_meas[k] == g[k] / V for k in g)
        assert all(np.array_equal(c.onsite_meas[k], o[k] / V) for k in o) and np.array_equal(c.intersite_meas["el_ke"], b / V)
        for k in corr:
            assert np.array_equal(c.onsite_corr[k].position, corr[k] / V)
            assert np.array_equal(c.onsite_corr[k].momentum, np.fft.fftn(corr[k], axes=(1, 2, 3)) / V)
        assert set(c.onsite_susc) == {"PairSusc"}                           # Simpson's rule over tau of the normalised correlation
        assert np.array_equal(c.onsite_susc["PairSusc"].position, ms.simpson(corr["PairGreens"] / V, m.dtau))
    cms.reset_measurements_(cm, m)                                          # no device was ever attached: host arrays only
    for c in cm.chains:
        assert all(v == 0 for v in c.global_meas.values()) and not any(v.any() for v in c.onsite_meas.values())
        assert not any(k.position.any() or k.momentum.any() for k in c.onsite_corr.values())
