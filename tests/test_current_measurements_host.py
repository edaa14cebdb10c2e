"""Host side of the Holstein model's CurrentCurrent (elphdynamics_amd/current_measurements.py) and the tests' own yardstick
(tests/current_reference.py): none of this needs a device.  Models here never reach initialize_model_'s library call.

The yardstick's two evaluations — the transcript of Measurements.jl:1790-2098 and the direct sums of ssh_bond_reference.current_direct
under the last-slice weight table — are pinned against each other at 1e-13 * max(1, max|ref|), the bound the SSH yardstick's two
evaluations meet, on the cases tests/test_gpu_current_measurements.py runs on the device; and the direct sums with t on ALL slices (the
reading of the reference's comments) are shown to differ from it by more than 1e-6 relative wherever the hopping is not 1, so the
device test can tell the two readings apart."""
import os

import numpy as np
import pytest

import current_reference as cref
from test_bond_measurements_host import BOTH_WAYS, SQUARE, TD
from test_measurements_host import host_model

ET = {"measure": True, "time_dependent": False}
CHAIN2 = [(1, 1, (1, 0, 0)), (1, 1, (-2, 0, 0))]                            # a negative, unreduced r'': the b == c term reduces it mod L

# (norbits, (L1, L2, L3), L, bond definitions, hopping (t, stddev) per definition, the CurrentCurrent entry)
CASES = {
    "hc3x2_disorder": (2, (3, 2, 1), 7, BOTH_WAYS, [(1.0, 0.2), (0.85, 0.2), (0.7, 0.2)], TD),
    "hc3x2_uniform_subset": (2, (3, 2, 1), 7, BOTH_WAYS, [(0.7, 0.0), (-1.3, 0.0), (0.9, 0.0)],
                             {"measure": True, "time_dependent": True, "pairs": [[1, 2], [3, 1], [2, 2], [1, 1]]}),
    "hc3x2_equal_time": (2, (3, 2, 1), 7, BOTH_WAYS, [(1.0, 0.2), (-0.85, 0.2), (0.7, 0.2)], ET),
    "chain12_disorder": (1, (12, 1, 1), 6, CHAIN2, [(1.0, 0.3), (-0.6, 0.3)], TD),
    "chain12_equal_time_subset": (1, (12, 1, 1), 6, CHAIN2, [(1.4, 0.0), (-0.6, 0.0)], {"measure": True, "time_dependent": False, "pairs": [[2, 1], [2, 2]]}),
    "sq4x4_uniform": (1, (4, 4, 1), 8, SQUARE, [(1.2, 0.0), (-0.8, 0.0)], TD),
    "sq4x4_unit": (1, (4, 4, 1), 8, SQUARE, [(1.0, 0.0), (1.0, 0.0)], TD),       # t = 1: the two readings coincide
}
NON_UNIT = [k for k in CASES if k != "sq4x4_unit"]


def assign_hoppings(m, defs, hop, seed):
    rng = np.random.default_rng(seed)
    for (o1, o2, v), (t, sd) in zip(defs, hop):
        m.assign_t_(t, o1, o2, v, stddev=sd, rng=rng)


def host_case(case):
    """A host-only HolsteinModel of CASES[case] with its hoppings assigned (seeded)."""
    from elphdynamics_amd import lattice as lat, models
    ns, dims, L, defs, hop, entry = CASES[case]
    m = models.HolsteinModel(lat.Lattice(ns, *dims), L * 0.1, 0.1)
    assert m.Ltau == L
    assign_hoppings(m, defs, hop, seed=L + sum(dims))
    m._create = lambda *a, **k: None
    m.initialize_model_()
    return m


def pairs_of(entry, n):
    from elphdynamics_amd.measurements import _pairs
    return _pairs(entry, n)


def rough_vectors(m, nv, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nv, m.Ndim)), rng.standard_normal((nv, m.Ndim))


@pytest.mark.parametrize("case", list(CASES))
def test_every_shape_reshapes_and_t_stays_in_definition_order(case):
    ns, dims, L, defs, hop, entry = CASES[case]
    m = host_case(case)
    nc = dims[0] * dims[1] * dims[2]
    assert m.Nbonds == len(defs) * nc == len(m.t) and m.bond_definitions == defs
    for n, (t, sd) in enumerate(hop):                                       # definition n's bonds are t[n nc : (n + 1) nc], sign included
        blk = m.t[n * nc:(n + 1) * nc]
        assert np.all(np.sign(blk) == np.sign(t))
        assert (np.ptp(blk) > 0) == (sd > 0)


@pytest.mark.parametrize("case", list(CASES))
def test_transcript_matches_the_direct_sums(case):
    ns, dims, L, defs, hop, entry = CASES[case]
    m = host_case(case)
    pairs = pairs_of(entry, len(defs))
    L0 = L + 1 if entry["time_dependent"] else 1
    R, X = rough_vectors(m, 3, seed=L)
    a = cref.measure(R, X, m.t, L, ns, dims, defs, L0, pairs)
    b = cref.measure(R, X, m.t, L, ns, dims, defs, L0, pairs, one=cref.current_transcript)
    assert a.shape == b.shape == (L0,) + dims + (pairs.shape[1],) and np.isfinite(a).all() and np.abs(a).max() > 0
    err = np.abs(a - b).max() / max(1.0, np.abs(a).max())
    print(case, "transcript against direct sums: %.2e (max|ref| %.3g), bound 1e-13" % (err, np.abs(a).max()))
    assert err <= 1e-13, (case, err)


@pytest.mark.parametrize("case", NON_UNIT)
def test_the_two_readings_can_be_told_apart(case):
    """t on the last slice alone (what the reference executes) against t on every slice (what its comments describe)."""
    ns, dims, L, defs, hop, entry = CASES[case]
    m = host_case(case)
    pairs = pairs_of(entry, len(defs))
    L0 = L + 1 if entry["time_dependent"] else 1
    R, X = rough_vectors(m, 3, seed=L)
    a = cref.measure(R, X, m.t, L, ns, dims, defs, L0, pairs)
    everywhere = lambda *args: cref.current_direct(*args, everywhere=True)  # noqa: E731
    c = cref.measure(R, X, m.t, L, ns, dims, defs, L0, pairs, one=everywhere)
    diff = np.abs(a - c).max() / max(1.0, np.abs(a).max())
    print(case, "last slice alone against every slice: %.2e relative" % diff)
    assert diff > 1e-6, (case, diff)


def test_with_unit_hopping_the_two_readings_coincide():
    ns, dims, L, defs, hop, entry = CASES["sq4x4_unit"]
    m = host_case("sq4x4_unit")
    pairs = pairs_of(entry, len(defs))
    R, X = rough_vectors(m, 2, seed=1)
    everywhere = lambda *args: cref.current_direct(*args, everywhere=True)  # noqa: E731
    assert np.array_equal(cref.measure(R, X, m.t, L, ns, dims, defs, L + 1, pairs), cref.measure(R, X, m.t, L, ns, dims, defs, L + 1, pairs, one=everywhere))


def test_the_delta_terms_are_taken_and_skipped():
    """Each of a == c, a == d, b == c, b == d is true for some listed pair of the cases and false for another."""
    seen = {k: set() for k in ("ac", "ad", "bc", "bd")}
    for ns, dims, L, defs, hop, entry in CASES.values():
        pairs = pairs_of(entry, len(defs))
        for n2, n1 in pairs.T:
            (d, c, _), (b, a, _) = defs[n2 - 1], defs[n1 - 1]
            for k, v in (("ac", a == c), ("ad", a == d), ("bc", b == c), ("bd", b == d)):
                seen[k].add(v)
    assert all(v == {True, False} for v in seen.values()), seen
    # the listed subset alone reaches every branch both ways too
    ns, dims, L, defs, hop, entry = CASES["hc3x2_uniform_subset"]
    sub = {k: set() for k in seen}
    for n2, n1 in entry["pairs"]:
        (d, c, _), (b, a, _) = defs[n2 - 1], defs[n1 - 1]
        for k, v in (("ac", a == c), ("ad", a == d), ("bc", b == c), ("bd", b == d)):
            sub[k].add(v)
    assert all(v == {True, False} for v in sub.values()), sub


def test_container_shapes_pairs_and_split_info():
    from elphdynamics_amd import current_measurements as cm
    m = host_case("hc3x2_uniform_subset")
    info = {"num_random_vectors": 3, "CurrentCurrent": CASES["hc3x2_uniform_subset"][5], "BondBond": TD, "Greens": TD}
    rest, cur = cm.split_info(info)
    assert rest == {"num_random_vectors": 3, "BondBond": TD, "Greens": TD} and cur == {"num_random_vectors": 3, "CurrentCurrent": info["CurrentCurrent"]}
    assert "CurrentCurrent" in info                                         # the deck's table is left as it was
    assert cm.split_info(None) == ({}, {}) and cm.split_info({"Greens": TD}) == ({"Greens": TD}, {})
    for table in (info, cur):                                               # the whole table or its part: the same container
        c = cm.initialize_current_container(m, table, "/nowhere")
        assert c.nchains == 1 and c.n_rand_vecs == 3 and c.bond_definitions == BOTH_WAYS and c._device_of is None
        one = c.chains[0]
        assert one.datafolder == "/nowhere" and set(one.intersite_corr) == {"CurrentCurrent"}
        cc = one.intersite_corr["CurrentCurrent"]
        assert cc.position.shape == cc.momentum.shape == (8, 3, 2, 1, 4) and cc.position.dtype == np.complex128 and cc.position.flags["F_CONTIGUOUS"]
        assert cc.pairs.tolist() == [[1, 1, 2, 3], [1, 2, 2, 1]]            # listed, sorted
    # default pairs: all n_def^2, first index slowest; equal-time: one slice
    c = cm.initialize_current_container(m, {"CurrentCurrent": ET}, "")
    cc = c.chains[0].intersite_corr["CurrentCurrent"]
    assert c.n_rand_vecs == 1 and cc.position.shape == (1, 3, 2, 1, 9)
    assert cc.pairs.tolist() == [[1, 1, 1, 2, 2, 2, 3, 3, 3], [1, 2, 3, 1, 2, 3, 1, 2, 3]]
    # measure = false and no table: nothing, and nothing to accumulate (no library call)
    for table in ({}, None, {"CurrentCurrent": {"measure": False, "time_dependent": True}}):
        c = cm.initialize_current_container(m, table, "")
        assert c.chains[0].intersite_corr == {}
    # definitions passed explicitly win over (and stand in for) the recorded ones
    bare = host_model(ns=2, dims=(3, 2, 1), L=7)
    c = cm.initialize_current_container(bare, {"CurrentCurrent": TD}, "", bond_definitions=[[1, 2, [0, 0, 0]], (2, 1, (1, 0, 0))])
    assert c.bond_definitions == [(1, 2, (0, 0, 0)), (2, 1, (1, 0, 0))] and c.chains[0].intersite_corr["CurrentCurrent"].position.shape == (8, 3, 2, 1, 4)
    # one container per resident chain, each with its own arrays and folder
    m._nchains = 3
    c = cm.initialize_current_container(m, info, ["a", "b", "c"])
    assert c.nchains == 3 and [ch.datafolder for ch in c.chains] == ["a", "b", "c"] and c.n_rand_vecs == 3
    arrays = [ch.intersite_corr["CurrentCurrent"].position for ch in c.chains]
    assert all(a.shape == (8, 3, 2, 1, 4) for a in arrays) and arrays[0] is not arrays[1]


def test_refusals():
    from elphdynamics_amd import current_measurements as cm, lattice as lat, measurements as ms, models
    assert cm.UnsupportedMeasurement is ms.UnsupportedMeasurement
    ssh = models.SSHModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    with pytest.raises(ms.UnsupportedMeasurement, match="SSH"):
        cm.initialize_current_container(ssh, {"CurrentCurrent": TD}, "", bond_definitions=SQUARE)
    bare = host_model()
    with pytest.raises(ms.UnsupportedMeasurement, match="CurrentCurrent.*no bond definitions"):
        cm.initialize_current_container(bare, {"CurrentCurrent": TD}, "")
    with pytest.raises(ms.UnsupportedMeasurement, match="CurrentCurrent"):
        cm.initialize_current_container(bare, {"CurrentCurrent": TD}, "", bond_definitions=[])
    m = host_model(bonds=SQUARE)
    with pytest.raises(ValueError, match="2 data folders for the 1 chains"):
        cm.initialize_current_container(m, {"CurrentCurrent": TD}, ["a", "b"])
    m._nchains = 2
    with pytest.raises(ValueError, match="1 data folders for the 2 chains"):
        cm.initialize_current_container(m, {"CurrentCurrent": TD}, "a")
    c = cm.initialize_current_container(m, {"CurrentCurrent": TD}, ["a", "b"])
    m._nchains = 1
    with pytest.raises(ValueError, match="made for 2 chains, 1 are resident"):
        cm.accumulate_current_(c, m, None)
    with pytest.raises(RuntimeError, match="no CurrentCurrent"):
        cm.fetch_current_(c, m)


def test_the_three_holstein_containers_keep_refusing_currentcurrent():
    from elphdynamics_amd import bond_measurements as bm, chain_bond_measurements as cbm, measurements as ms
    m = host_model(bonds=SQUARE)
    with pytest.raises(ms.UnsupportedMeasurement, match="CurrentCurrent.*last time slice"):
        bm.initialize_bond_container(m, {"CurrentCurrent": TD}, "")
    with pytest.raises(ms.UnsupportedMeasurement, match="CurrentCurrent.*last time slice"):
        cbm.initialize_chain_bond_container(m, {"CurrentCurrent": TD}, [""])
    with pytest.raises(ms.UnsupportedMeasurement, match="CurrentCurrent"):
        ms.initialize_measurements_container(m, {"CurrentCurrent": TD}, "")
    # ... and split_info's first part passes all three
    from elphdynamics_amd import current_measurements as cm
    rest, cur = cm.split_info({"CurrentCurrent": TD, "BondBond": TD, "num_random_vectors": 2})
    assert set(bm.initialize_bond_container(m, rest, "").intersite_corr) == {"BondBond"}
    assert set(cbm.initialize_chain_bond_container(m, rest, [""]).chains[0].intersite_corr) == {"BondBond"}
    rest.pop("BondBond")
    assert ms.initialize_measurements_container(m, rest, "").n_rand_vecs == 2


def test_folders_key_files_process_write_and_reset(tmp_path):
    from elphdynamics_amd import current_measurements as cm
    m = host_model(ns=2, dims=(3, 2, 2), L=5, bonds=BOTH_WAYS)
    m._nchains = 2
    folders = [str(tmp_path / "run0"), str(tmp_path / "run1")]
    for f in folders:
        os.mkdir(f)
    info = {"num_random_vectors": 4, "CurrentCurrent": {"measure": True, "time_dependent": True, "pairs": [[3, 2], [1, 3]]}}
    c = cm.initialize_current_container(m, info, folders)
    cm.initialize_current_folders_(c)
    for f in folders:
        assert sorted(os.listdir(f)) == ["CurrentCurrent_momentum_f", "CurrentCurrent_position_f"]      # no susceptibility (:157-162)
    rows = open(os.path.join(folders[1], "CurrentCurrent_position_f", "CurrentCurrent_position_key.out")).read().splitlines()
    assert rows[0] == "index bond1 bond2 r3 r2 r1 tau" and len(rows) == 1 + 6 * 12 * 2
    assert rows[1] == "1 1 3 0 0 0 0" and rows[2] == "2 1 3 0 0 0 1" and rows[7] == "7 1 3 0 0 1 0" and rows[73] == "73 3 2 0 0 0 0"
    rows = open(os.path.join(folders[0], "CurrentCurrent_momentum_f", "CurrentCurrent_momentum_key.out")).read().splitlines()
    assert rows[0] == "index bond1 bond2 k3 k2 k1 tau" and len(rows) == 1 + 6 * 12 * 2
    et = cm.initialize_current_container(m, {"CurrentCurrent": {"measure": True, "time_dependent": False, "pairs": [[1, 1]]}},
                                         [str(tmp_path / "e0"), str(tmp_path / "e1")])
    for ch in et.chains:
        os.mkdir(ch.datafolder)
    cm.initialize_current_folders_(et)
    rows = open(tmp_path / "e0" / "CurrentCurrent_momentum_f" / "CurrentCurrent_momentum_key.out").read().splitlines()
    assert rows[0] == "index bond1 bond2 k3 k2 k1 tau" and len(rows) == 1 + 12 and rows[2] == "2 1 1 0 0 1 0"
    # process and write on sums put in by hand (what fetch_current_ would have copied from the device)
    rng = np.random.default_rng(3)
    raw = [rng.standard_normal(ch.intersite_corr["CurrentCurrent"].position.shape) for ch in c.chains]
    for ch, r in zip(c.chains, raw):
        ch.intersite_corr["CurrentCurrent"].position[...] = r
    calls = []
    c._device_of = m
    m._lib = type("L", (), {"elph_current_fetch": staticmethod(lambda *a: calls.append(("fetch", a[1])) or 0),
                            "elph_current_reset": staticmethod(lambda *a: calls.append(("reset",)) or 0)})()
    m._h = 1
    cm.process_current_measurements_(c, 5, m)
    assert calls == [("fetch", 0), ("fetch", 1)]
    V = 5 * 6                                                               # bin_size * binomial(4, 2), the vectors of ONE chain
    for ch, r in zip(c.chains, raw):
        v = ch.intersite_corr["CurrentCurrent"]
        assert np.abs(v.position - r / V).max() < 1e-15
        assert np.abs(v.momentum - np.fft.fftn(r, axes=(1, 2, 3)) / V).max() < 1e-14
    cm.write_current_measurements_(c, m, 12)
    for f, ch in zip(folders, c.chains):
        for space in ("position", "momentum"):
            lines = open(os.path.join(f, "CurrentCurrent_%s_f" % space, "CurrentCurrent_%s_00012.out" % space)).read().splitlines()
            assert lines[0] == "index CurrentCurrent_%s_real CurrentCurrent_%s_imag" % (space, space) and len(lines) == 1 + 6 * 12 * 2
            flat = getattr(ch.intersite_corr["CurrentCurrent"], space).reshape(-1, order="F")
            assert lines[5] == "5 %.8f %.8f" % (flat[4].real, flat[4].imag)
    cm.reset_current_measurements_(c, m)
    assert calls[-1] == ("reset",)
    assert all(not v.position.any() and not v.momentum.any() for ch in c.chains for v in ch.intersite_corr.values())
