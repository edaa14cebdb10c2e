"""Host side of the SSH measurements of resident chains (elphdynamics_amd/ssh_chain_measurements.py): none of this needs a device.  The
models (tests/ssh_measurement_cases.py, device=False) never reach a library call: the container constructor reads host attributes only,
and every wrong shape or count is caught before the library."""
import os
from math import comb

import numpy as np
import pytest

import ssh_measurement_cases as smc


def chain_model(name, nchains):
    m, table = smc.build_case(name, device=False)
    m._nchains = nchains
    return m, table


class FakeEstimator:
    def __init__(self, model, nv):
        self.model, self.nv = model, nv


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def test_one_container_per_chain_with_the_single_configuration_shapes_and_pairs():
    from elphdynamics_amd import ssh_chain_measurements as scm, ssh_measurements as sm
    m, table = chain_model("hc3", 3)
    info = dict(table, num_random_vectors=3)
    cm = scm.initialize_ssh_chain_measurements_container(m, info, ["/a", "/b", "/c"])
    assert cm.nchains == 3 and len(cm.chains) == 3 and cm.n_rand_vecs == 3  # num_random_vectors: per chain
    m._nchains = 1
    one = sm.initialize_ssh_measurements_container(m, info, "/a")
    for k, c in enumerate(cm.chains):
        assert isinstance(c, sm.SSHMeasurementsContainer) and c.datafolder == "/" + "abc"[k] and c.n_rand_vecs == 3
        for grp in ("onsite_corr", "intersite_corr", "onsite_susc", "intersite_susc"):
            got, want = getattr(c, grp), getattr(one, grp)
            assert set(got) == set(want)
            for name in want:
                assert got[name].position.shape == want[name].position.shape
                assert np.array_equal(got[name].pairs, want[name].pairs)
        assert set(c.intersite_corr) == {"PhononGreens"} and c.intersite_corr["PhononGreens"].pairs.T.tolist() == [[1, 2], [2, 2], [3, 1]]
        assert tuple(c.onsite_meas) == sm.ONSITE_KEYS and all(v.shape == (2,) for v in c.onsite_meas.values())
        assert tuple(c.intersite_meas) == sm.INTERSITE_KEYS and all(v.shape == (int(m.nbonds),) for v in c.intersite_meas.values())
        assert set(c.global_meas) == {"density", "Nsqr", "mu"}
    # the chains' arrays are their own
    cm.chains[0].onsite_corr["Greens"].position[...] = 1
    assert not cm.chains[1].onsite_corr["Greens"].position.any()
    # one chain resident is a lockstep run of one
    assert scm.initialize_ssh_chain_measurements_container(m, {}, [""]).nchains == 1


def test_refusals_name_the_request_and_come_before_any_library_call():
    from elphdynamics_amd import ssh_chain_measurements as scm
    from test_measurements_host import host_model
    m, table = chain_model("hc3", 2)
    m._lib, m._h = NoLibrary(), 1
    for name in ("BondBond", "CurrentCurrent", "BondPairGreens"):
        info = dict(table)
        info[name] = {"measure": True, "time_dependent": True}
        with pytest.raises(scm.UnsupportedMeasurement, match=name):
            scm.initialize_ssh_chain_measurements_container(m, info, ["", ""])
        info[name] = {"measure": False, "time_dependent": True}
        scm.initialize_ssh_chain_measurements_container(m, info, ["", ""])
    for key in ("density", "double_occupancy", "phonon_position"):
        with pytest.raises(scm.UnsupportedMeasurement, match="Snapshots.*" + key):
            scm.initialize_ssh_chain_measurements_container(m, {"Snapshots": {key: True}}, ["", ""])
    for folders in ([""], ["", "", ""]):
        with pytest.raises(ValueError, match="folders"):
            scm.initialize_ssh_chain_measurements_container(m, table, folders)
    hol = host_model()
    hol._nchains = 2
    hol._lib, hol._h = NoLibrary(), 1
    with pytest.raises(scm.UnsupportedMeasurement, match="Holstein"):
        scm.initialize_ssh_chain_measurements_container(hol, {}, ["", ""])
    cm = scm.initialize_ssh_chain_measurements_container(m, dict(table, num_random_vectors=2), ["", ""])
    with pytest.raises(scm.UnsupportedMeasurement, match="Holstein"):       # a container carried over to a Holstein model
        scm.accumulate_(cm, hol, FakeEstimator(hol, 4), np.zeros((2, hol.Ndof)))


def test_wrong_counts_and_shapes_are_caught_before_the_library():
    from elphdynamics_amd import ssh_chain_measurements as scm
    m, table = chain_model("tri4_Lt7", 3)
    m._lib, m._h = NoLibrary(), 1
    cm = scm.initialize_ssh_chain_measurements_container(m, dict(table, num_random_vectors=3), ["", "", ""])
    X = np.zeros((3, m.Ndof))
    with pytest.raises(ValueError, match="vectors"):
        scm.accumulate_(cm, m, FakeEstimator(m, 3), X)                      # 3 vectors for 3 chains x 3
    with pytest.raises(ValueError, match="vectors"):
        scm.make_measurements_(cm, m, FakeEstimator(m, 6), X, 1)
    est = FakeEstimator(m, 9)
    for bad in (np.zeros((2, m.Ndof)), np.zeros((3, m.Ndof + 1)), np.zeros(3 * m.Ndof)):
        with pytest.raises(ValueError, match="X has shape"):
            scm.accumulate_(cm, m, est, bad)
    for bad in (np.zeros(m.Nsites), np.zeros((3, m.Nsites - 1)), np.zeros((1, m.Nsites))):
        with pytest.raises(ValueError, match="mu has shape"):
            scm.accumulate_(cm, m, est, X, mu=bad)
        with pytest.raises(ValueError, match="mu has shape"):
            scm.make_measurements_(cm, m, est, X, 1, mu=bad)
    m._nchains = 2                                                          # the chains were dropped or changed since
    with pytest.raises(ValueError, match="3 chains"):
        scm.accumulate_(cm, m, est, X)
    with pytest.raises(RuntimeError, match="nothing has been measured"):
        scm.fetch_(cm, m)


def tree(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


def test_every_chain_gets_the_single_configuration_files_in_its_own_folder(tmp_path):
    from elphdynamics_amd import ssh_chain_measurements as scm, ssh_measurements as sm
    folders = [str(tmp_path / ("chain%d" % k)) for k in range(3)] + [str(tmp_path / "single")]
    for f in folders:
        os.mkdir(f)
    m, table = chain_model("hc3", 3)
    info = dict(table, num_random_vectors=4)
    cm = scm.initialize_ssh_chain_measurements_container(m, info, folders[:3])
    scm.initialize_measurement_folders_(cm)
    for k, c in enumerate(cm.chains):                                       # a number of its own in every chain's files
        c.global_meas["density"] = complex(k + 1)
    scm.write_measurements_(cm, m, 4)
    s, _ = smc.build_case("hc3", device=False)
    one = sm.initialize_ssh_measurements_container(s, info, folders[3])
    sm.initialize_measurement_folders_(one)
    sm.write_measurements_(one, s, 4)
    want = tree(folders[3])
    # scalars; (file + key) x (position, momentum) x (5 correlations + PairSusc and SpinSusc: DenDen is equal-time)
    assert len(want) == 3 + 2 * 2 * 7
    for k, f in enumerate(folders[:3]):
        assert tree(f) == want
        for rel in want:
            got, ref = open(os.path.join(f, rel)).read(), open(os.path.join(folders[3], rel)).read()
            if rel.startswith("global_measurements_f"):
                assert got == ref.replace("density 0.00000000", "density %.8f" % (k + 1)), rel
            else:
                assert got == ref, rel


def test_process_divides_by_bin_size_times_the_pairs_of_a_chains_vectors(monkeypatch):
    from elphdynamics_amd import ssh_chain_measurements as scm, ssh_measurements as sm
    m, table = chain_model("hc3", 3)
    cm = scm.initialize_ssh_chain_measurements_container(m, dict(table, num_random_vectors=4), ["", "", ""])
    rng = np.random.default_rng(17)
    raw = []
    for c in cm.chains:
        for k in c.global_meas:
            c.global_meas[k] = complex(rng.standard_normal() * 50)
        for grp in (c.onsite_meas, c.intersite_meas):
            for k in grp:
                grp[k][:] = rng.standard_normal(grp[k].shape) * 50
        corr = sm._all_corr(c)
        for v in corr.values():
            v.position[...] = rng.standard_normal(v.position.shape) * 50
        raw.append((dict(c.global_meas), {k: v.copy() for k, v in c.onsite_meas.items()}, {k: v.copy() for k, v in c.intersite_meas.items()},
                    {k: v.position.copy() for k, v in corr.items()}))
    monkeypatch.setattr(scm, "fetch_", lambda cm, model: None)              # the arrays are hand-filled: nothing to fetch
    bin_size = 5
    scm.process_measurements_(cm, bin_size, m)
    V = bin_size * comb(4, 2)                                               # 4 vectors per chain, not the estimator's 12
    assert V == 30
    for c, (g, o, b, corr) in zip(cm.chains, raw):
        assert all(c.global_meas[k] == g[k] / V for k in g)
        assert all(np.array_equal(c.onsite_meas[k], o[k] / V) for k in o) and all(np.array_equal(c.intersite_meas[k], b[k] / V) for k in b)
        got = sm._all_corr(c)
        assert set(got) == set(corr) == set(sm.CREATE_ORDER)
        for k in corr:
            assert np.array_equal(got[k].position, corr[k] / V)
            assert np.array_equal(got[k].momentum, np.fft.fftn(corr[k], axes=(1, 2, 3)) / V)
        assert set(c.onsite_susc) == {"PairSusc", "SpinSusc"}               # DenDen is the equal-time request of this table
        assert np.array_equal(c.onsite_susc["PairSusc"].position, sm.simpson(corr["PairGreens"] / V, m.dtau))
    scm.reset_measurements_(cm, m)                                          # no device was ever attached: host arrays only
    for c in cm.chains:
        assert all(v == 0 for v in c.global_meas.values()) and not any(v.any() for v in c.onsite_meas.values())
        assert not any(v.any() for v in c.intersite_meas.values())
        assert not any(k.position.any() or k.momentum.any() for k in sm._all_corr(c).values())
