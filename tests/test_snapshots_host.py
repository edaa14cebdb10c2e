"""Host side of the snapshot measurements (elphdynamics_amd/snapshots.py): none of this needs a device.  The models never reach a
library call: the container reads host attributes only, the files are written from arrays given by hand, and every wrong count or shape
is caught before the library."""
import os

import numpy as np
import pytest

import snapshot_reference as sref
from test_chain_measurements_host import NoLibrary, chain_model
from test_measurements_host import FULL, host_model
from test_ssh_measurements_host import host_case


def test_split_info_hands_each_container_its_part():
    from elphdynamics_amd import measurements as ms, snapshots as sn
    table = {"density": True, "double_occupancy": False, "phonon_position": True}
    info = dict(FULL, Snapshots=table)
    rest, snap = sn.split_info(info)
    assert snap == table and snap is not table
    assert "Snapshots" not in rest and rest == {k: v for k, v in FULL.items() if k != "Snapshots"}
    assert info["Snapshots"] is table                                       # the caller's table is left as it was
    m = host_model()
    with pytest.raises(ms.UnsupportedMeasurement, match="Snapshots"):
        ms.initialize_measurements_container(m, info, "")
    assert ms.initialize_measurements_container(m, rest, "").n_rand_vecs == 3       # the rest feeds the on-site container
    assert sn.split_info({"num_random_vectors": 2}) == ({"num_random_vectors": 2}, {})
    assert sn.split_info(None) == ({}, {})


def test_container_lists_the_requested_names_in_the_references_order():
    from elphdynamics_amd import snapshots as sn
    m = host_model()
    everything = {"Snapshots": {"phonon_position": True, "double_occupancy": True, "density": True}}      # the deck's order is not the files'
    sc = sn.initialize_snapshots_container(m, everything, "/data")
    assert sc.snapshots == ["density", "double_occupancy", "phonon_position"] == list(sref.NAMES)
    assert sc.datafolders == ["/data"] and sc.nchains == 1
    sc = sn.initialize_snapshots_container(m, {"Snapshots": {"phonon_position": True, "density": False, "double_occupancy": True}}, ["/data"])
    assert sc.snapshots == ["double_occupancy", "phonon_position"]
    for info in (FULL, {}, None, {"Snapshots": {}}, {"Snapshots": {"density": 1, "momentum": False, "phonon_position": "true"}}):
        assert sn.initialize_snapshots_container(m, info, "").snapshots == []            # false entries, and what is not `true`, are ignored
    with pytest.raises(sn.UnsupportedMeasurement, match="Snapshots.*momentum"):
        sn.initialize_snapshots_container(m, {"Snapshots": {"density": True, "momentum": True}}, "")
    # resident chains: one folder each; the SSH model is served alike
    m3 = chain_model(3)
    sc = sn.initialize_snapshots_container(m3, everything, ["/a", "/b", "/c"])
    assert sc.nchains == 3 and sc.datafolders == ["/a", "/b", "/c"] and len(sc.snapshots) == 3
    for folders in ("/a", ["/a"], ["/a", "/b"], ["/a", "/b", "/c", "/d"]):
        with pytest.raises(ValueError, match="data folders for the 3 chains resident in the model"):
            sn.initialize_snapshots_container(m3, everything, folders)
    with pytest.raises(ValueError, match="2 data folders for the 1 chains"):
        sn.initialize_snapshots_container(m, everything, ["/a", "/b"])
    ssh = host_case("hc3")
    assert sn.initialize_snapshots_container(ssh, everything, "/s").snapshots == list(sref.NAMES)


def tree(d):
    return sorted(os.path.relpath(os.path.join(r, x), d) for r, ds, fs in os.walk(d) for x in ds + fs)


def test_folders_are_made_in_every_chains_folder(tmp_path):
    from elphdynamics_amd import snapshots as sn
    folders = [str(tmp_path / ("chain%d" % c)) for c in range(2)]
    for f in folders:
        os.mkdir(f)
    sc = sn.initialize_snapshots_container(chain_model(2), {"Snapshots": {"density": True, "phonon_position": True}}, folders)
    sn.initialize_snapshot_folders_(sc)
    for f in folders:
        assert tree(f) == ["density_snapshots_f", "phonon_position_snapshots_f"]
    with pytest.raises(FileExistsError):                                    # mkdir, as the reference: a second run does not write over a first
        sn.initialize_snapshot_folders_(sc)
    one = str(tmp_path / "single")
    os.mkdir(one)
    sc = sn.initialize_snapshots_container(host_model(), {"Snapshots": {"double_occupancy": True}}, one)
    sn.initialize_snapshot_folders_(sc)
    assert tree(one) == ["double_occupancy_snapshots_f"]
    none = sn.initialize_snapshots_container(host_model(), FULL, one)
    sn.initialize_snapshot_folders_(none)
    sn.write_snapshots_(none, {}, 1)
    assert tree(one) == ["double_occupancy_snapshots_f"]


def test_files_byte_for_byte(tmp_path):
    from elphdynamics_amd import snapshots as sn
    folders = [str(tmp_path / ("chain%d" % c)) for c in range(2)]
    for f in folders:
        os.mkdir(f)
    sc = sn.initialize_snapshots_container(chain_model(2), {"Snapshots": {k: True for k in sref.NAMES}}, folders)
    sn.initialize_snapshot_folders_(sc)
    arrays = {"density": np.array([[1.0, 0.123456789, -4e-9], [2.5, 1e-9, 12345.678901234]]),
              "double_occupancy": np.array([[0.25, -0.5, 1.0 / 3.0], [0.0, 2.0 / 3.0, -1e-10]]),
              "phonon_position": np.array([[-1.5, 0.000000004], [3.0, -0.000000006]])}
    sn.write_snapshots_(sc, arrays, 3)
    sn.write_snapshots_(sc, {k: v[::-1] for k, v in arrays.items()}, 123456)
    want = {("density", 0): "density\n1.00000000\n0.12345679\n-0.00000000\n",
            ("density", 1): "density\n2.50000000\n0.00000000\n12345.67890123\n",
            ("double_occupancy", 0): "double_occupancy\n0.25000000\n-0.50000000\n0.33333333\n",
            ("double_occupancy", 1): "double_occupancy\n0.00000000\n0.66666667\n-0.00000000\n",
            ("phonon_position", 0): "phonon_position\n-1.50000000\n0.00000000\n",
            ("phonon_position", 1): "phonon_position\n3.00000000\n-0.00000001\n"}
    for c, f in enumerate(folders):
        assert tree(f) == sorted([n + "_snapshots_f" for n in sref.NAMES]
                                 + [os.path.join(n + "_snapshots_f", "%s_snapshot_%s.out" % (n, num)) for n in sref.NAMES for num in ("000003", "123456")])
        for name in sref.NAMES:
            read = lambda num: open(os.path.join(f, name + "_snapshots_f", "%s_snapshot_%s.out" % (name, num)), "rb").read()  # noqa: E731
            assert read("000003") == want[(name, c)].encode(), (c, name)
            assert read("123456") == want[(name, 1 - c)].encode(), (c, name)         # the other chain's rows went into this folder
    # one configuration: a folder given as a string, rows of length one
    one = str(tmp_path / "single")
    os.mkdir(one)
    sc = sn.initialize_snapshots_container(host_model(), {"Snapshots": {"density": True}}, one)
    sn.initialize_snapshot_folders_(sc)
    sn.write_snapshots_(sc, {"density": np.array([[0.5, 1.25]]), "double_occupancy": np.zeros((1, 2))}, 1000000)      # seven digits: %.6d is a minimum
    assert tree(one) == ["density_snapshots_f", os.path.join("density_snapshots_f", "density_snapshot_1000000.out")]
    assert open(os.path.join(one, "density_snapshots_f", "density_snapshot_1000000.out")).read() == "density\n0.50000000\n1.25000000\n"
    with pytest.raises(ValueError, match="density has shape"):
        sn.write_snapshots_(sc, {"density": np.zeros((2, 2))}, 2)
    with pytest.raises(ValueError, match="density has shape"):
        sn.write_snapshots_(sc, {"density": np.zeros(2)}, 2)


class FakeEstimator:
    def __init__(self, model):
        self.model = model


def test_phonon_position_is_the_tau_mean_and_wrong_inputs_are_caught_before_the_library():
    from elphdynamics_amd import snapshots as sn
    m = chain_model(3, ns=2, dims=(3, 2, 1), L=7)
    m._lib, m._h = NoLibrary(), 1
    est = FakeEstimator(m)
    sc = sn.initialize_snapshots_container(m, {"Snapshots": {"phonon_position": True}}, ["", "", ""])
    X = np.random.default_rng(3).standard_normal((3, m.Ndof))
    got = sn.snapshot_arrays_(sc, m, est, X)                                # phonon_position alone makes no library call
    assert list(got) == ["phonon_position"] and got["phonon_position"].shape == (3, m.Nph)
    for c in range(3):
        assert np.abs(got["phonon_position"][c] - sref.phonon_position(X[c], m.Nph, m.Ltau)).max() <= 4 * np.finfo(float).eps * np.abs(X[c]).max()
    for bad in (np.zeros((2, m.Ndof)), np.zeros((3, m.Ndof + 1)), np.zeros(3 * m.Ndof)):
        with pytest.raises(ValueError, match="X has shape"):
            sn.snapshot_arrays_(sc, m, est, bad)
    with pytest.raises(ValueError, match="needs X"):
        sn.snapshot_arrays_(sc, m, est)
    with pytest.raises(ValueError, match="another model"):
        sn.snapshot_arrays_(sc, m, FakeEstimator(host_model()), X)
    m._nchains = 2                                                          # the chains were dropped or changed since
    with pytest.raises(ValueError, match="3 chains, 2 are resident"):
        sn.snapshot_arrays_(sc, m, est, X)
    # one configuration: the model's own field when X is not given, a row or a (1, Ndof) array when it is
    s = host_model(ns=1, dims=(4, 4, 1), L=8)
    s._lib, s._h = NoLibrary(), 1
    s.x[:] = np.random.default_rng(4).standard_normal(s.Ndof)
    one = sn.initialize_snapshots_container(s, {"Snapshots": {"phonon_position": True}}, "")
    a = sn.snapshot_arrays_(one, s, FakeEstimator(s))["phonon_position"]
    assert a.shape == (1, s.Nph) and np.array_equal(a, sn.snapshot_arrays_(one, s, FakeEstimator(s), s.x)["phonon_position"])
    assert np.array_equal(a, sn.snapshot_arrays_(one, s, FakeEstimator(s), s.x[None])["phonon_position"])
    assert np.abs(a[0] - sref.phonon_position(s.x, s.Nph, s.Ltau)).max() <= 4 * np.finfo(float).eps * np.abs(s.x).max()
    # the device snapshots do go to the library, after the checks
    dev = sn.initialize_snapshots_container(s, {"Snapshots": {"density": True}}, "")
    with pytest.raises(AssertionError, match="the library was called: elph_snapshots"):
        sn.snapshot_arrays_(dev, s, FakeEstimator(s))


def test_the_reference_restatement_on_numbers_worked_by_hand():
    """d_n = 1 - MinvR R at one site and one slice: n_v = 3 with d = (2, 3, 5).  density = 2 (2 + 3 + 5) / 3; double occupancy over
    n in {1, 2}, m in {2, 3}: 2*3 + 2*5 + 3*3 + 3*5 = 40 (the n = m = 2 term 3*3 is the reference's), over binomial(3, 2) = 3."""
    R = np.array([[1.0], [1.0], [2.0]])
    MinvR = np.array([[-1.0], [-2.0], [-2.0]])
    assert sref.density(R, MinvR, 1, 1)[0] == 20.0 / 3.0
    assert sref.double_occupancy(R, MinvR, 1, 1)[0] == 40.0 / 3.0
    assert sref.double_occupancy(R[:2], MinvR[:2], 1, 1)[0] == 6.0          # n_v = 2: the one pair, once
    # two slices are averaged, sites stay apart: R viewed as (n_v, N, L)
    R2, M2 = np.ones((2, 4)), -np.array([[1.0, 3.0, 0.0, 0.0], [2.0, 4.0, 1.0, 1.0]])
    assert np.array_equal(sref.density(R2, M2, 2, 2), [2 * (2 + 3 + 4 + 5) / 4.0, 2 * (1 + 2 + 1 + 2) / 4.0])
    assert np.array_equal(sref.double_occupancy(R2, M2, 2, 2), [(2 * 3 + 4 * 5) / 2.0, (1 * 2 + 1 * 2) / 2.0])
    assert np.array_equal(sref.phonon_position(np.array([1.0, 2.0, 3.0, 5.0, 5.0, 5.0]), 2, 3), [2.0, 5.0])


def test_the_four_on_site_containers_still_refuse_snapshots():
    from elphdynamics_amd import chain_measurements as cms, measurements as ms, ssh_chain_measurements as scm, ssh_measurements as sm
    h1, h2 = host_model(), chain_model(2)
    s1, s2 = host_case("hc3"), host_case("hc3")
    s2._nchains = 2
    for key in sref.NAMES:
        info = {"num_random_vectors": 3, "Snapshots": {key: True}}
        with pytest.raises(ms.UnsupportedMeasurement, match="Snapshots.*" + key):
            ms.initialize_measurements_container(h1, info, "")
        with pytest.raises(cms.UnsupportedMeasurement, match="Snapshots.*" + key):
            cms.initialize_chain_measurements_container(h2, info, ["", ""])
        with pytest.raises(sm.UnsupportedMeasurement, match="Snapshots.*" + key):
            sm.initialize_ssh_measurements_container(s1, info, "")
        with pytest.raises(scm.UnsupportedMeasurement, match="Snapshots.*" + key):
            scm.initialize_ssh_chain_measurements_container(s2, info, ["", ""])
