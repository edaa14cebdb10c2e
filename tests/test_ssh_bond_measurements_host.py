"""Host side of the SSH model's inter-site correlations (elphdynamics_amd/ssh_bond_measurements.py) and the tests' own yardstick
(tests/ssh_bond_reference.py): none of this needs a device.  Models here never reach initialize_model_'s library call.

The cases are those of tests/test_gpu_ssh_bond_measurements.py.  The two evaluations of CurrentCurrent in the yardstick, the transcript
of the reference's text and the direct sums, are held to 1e-13 * max(1, max|ref|) on every case: a tenth of the bound the device is
held to."""
import functools
import os

import numpy as np
import pytest

import ssh_bond_reference as sbref
import ssh_measurement_cases as smc
from test_bond_measurements_host import BOTH_WAYS

TD = {"measure": True, "time_dependent": True}
ALL3 = {k: TD for k in sbref.CORRS}
BOTH_WAYS_SSH = [(o1, o2, v, True, "abc"[i], 1.0) for i, (o1, o2, v) in enumerate(BOTH_WAYS)]
NEGATIVE = [(1, 1, (-1, 0, 0), True, "x", 1.0), (1, 1, (0, -1, 0), True, "y", 1.0), (1, 1, (-1, -1, 0), False, "d", 0.7)]
LISTED = {"BondBond": {"measure": True, "time_dependent": True, "pairs": [[2, 3], [1, 1]]},
          "CurrentCurrent": {"measure": True, "time_dependent": False, "pairs": [[3, 1], [1, 2], [2, 2]]},     # the equal-time request
          "BondPairGreens": {"measure": True, "time_dependent": False, "pairs": [[1, 3]]}}

# name -> (a case of ssh_measurement_cases, or (orbitals, cells, bond definitions, Ltau) for build_model; the [measurements] table)
CASES = {
    "hc3": ("hc3", ALL3),
    "hc3x2_both_ways": ((2, (3, 2, 1), BOTH_WAYS_SSH, 7), ALL3),           # a == d and b == c on mixed pairs, at non-zero displacements
    "psq6": ("psq6", ALL3),                                                 # the bare bonds (t' = t) come first in the deck
    "sq12x6": ("sq12x6", ALL3),                                             # t' changes sign; non-square cells
    "cubic3x2x2": ("cubic3x2x2", ALL3),                                     # three dimensions, odd L, no bond lost
    "hc3_Lt2": ("hc3_Lt2", ALL3),
    "tri4_Lt7": ("tri4_Lt7", ALL3),
    "hc3x2_listed": ((2, (3, 2, 1), BOTH_WAYS_SSH, 7), LISTED),             # CurrentCurrent equal-time, listed subsets of pairs
    "sq4x3_negative": ((1, (4, 3, 1), NEGATIVE, 6), ALL3),                  # displacements given negative: l = r'' is reduced mod L
}


def build(name, device=False):
    what, _ = CASES[name]
    if isinstance(what, str):
        return smc.build_case(what, device=device)[0]
    norb, dims, defs, L = what
    return smc.build_model(norb, dims, defs, L, seed=9100 + list(CASES).index(name), device=device)


def container_of(name, model, datafolder="", nv=3):
    from elphdynamics_amd import ssh_bond_measurements as sb
    return sb.initialize_ssh_bond_container(model, dict(CASES[name][1], num_random_vectors=nv), datafolder)


def request_of(c):
    return {k: (v.position.shape[0], v.pairs) for k, v in c.intersite_corr.items()}


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """(host model, R, M^-1 R, direct sums of the case's request for n_v = 3): computed once per session, never written to."""
    m = build(name)
    rng = np.random.default_rng(77 + list(CASES).index(name))
    R, X = rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim))
    want = sbref.measure(R, X, m.x, smc.ref_par(m), sbref.definitions(m), request_of(container_of(name, m)))
    for a in (R, X) + tuple(want.values()):
        a.setflags(write=False)
    return m, R, X, want


@pytest.mark.parametrize("case", list(CASES))
def test_transcript_matches_direct_sums(case):
    m, R, X, want = yardstick(case)
    L0, pairs = request_of(container_of(case, m))["CurrentCurrent"]
    a = sbref.measure_current(R, X, m.x, smc.ref_par(m), sbref.definitions(m), L0, pairs, one=sbref.current_transcript)
    b = want["CurrentCurrent"]
    la = m.lattice
    assert a.shape == b.shape == (L0, la.L1, la.L2, la.L3, pairs.shape[1]) and np.isfinite(b).all()
    err = np.abs(a - b).max() / max(1.0, np.abs(b).max())
    print(case, "CurrentCurrent transcript against direct sums: %.2e" % err, "max|ref| %.3g" % np.abs(b).max())
    assert err < 1e-13, (case, err)
    assert np.abs(b).max() > 1e-3                                           # not a comparison of zeros


def test_the_cases_reach_every_branch():
    """Each of a == c, a == d, b == c, b == d is true for some listed CurrentCurrent pair and false for another; the a == d and b == c
    terms land on non-zero displacements; a bare definition, a sign change of t' and a negative displacement occur."""
    seen = {k: set() for k in ("ac", "ad", "bc", "bd")}
    nonzero = {"ad": False, "bc": False}
    for name in CASES:
        m = build(name)
        defs = sbref.definitions(m)
        dims = (m.lattice.L1, m.lattice.L2, m.lattice.L3)
        for n2, n1 in request_of(container_of(name, m))["CurrentCurrent"][1].T:
            (d, c, rpp), (b, a, rp) = defs[n2 - 1], defs[n1 - 1]
            for key, val in (("ac", a == c), ("ad", a == d), ("bc", b == c), ("bd", b == d)):
                seen[key].add(val)
            nonzero["ad"] |= a == d and any((-rp[k]) % dims[k] for k in range(3))
            nonzero["bc"] |= b == c and any(rpp[k] % dims[k] for k in range(3))
    assert all(v == {True, False} for v in seen.values()), seen
    assert all(nonzero.values()), nonzero
    m = build("psq6")
    assert not m.bond_to_phonon[:36].any() and m.bond_to_phonon[36:].all()
    tp = sbref.hopping(build("sq12x6").x, smc.ref_par(build("sq12x6")))
    assert (np.sign(tp).min(axis=1) < np.sign(tp).max(axis=1)).any()       # t' changes sign along tau on some bond
    assert any(k < 0 for d in sbref.definitions(build("sq4x3_negative")) for k in d[2])
    for name in CASES:
        m = build(name)
        assert m.Nbonds == m.nbonds * m.lattice.ncells, name


def test_the_reshape_of_the_hopping_fails_where_a_bond_was_removed():
    import ssh_cases as sc
    norb, dims, defs, L = sc.SHAPES["cu3x2x2"]
    m = smc.build_model(norb, dims, defs, L, seed=5, device=False)
    assert m.Nbonds != m.nbonds * m.lattice.ncells
    rng = np.random.default_rng(0)
    R = rng.standard_normal((2, m.Ndim))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        sbref.measure_current(R, R, m.x, smc.ref_par(m), sbref.definitions(m), 1, np.array([[1], [1]]))


def test_container_shapes_pairs_and_susceptibility():
    from elphdynamics_amd import ssh_bond_measurements as sb
    m = build("hc3")
    c = sb.initialize_ssh_bond_container(m, dict(ALL3, num_random_vectors=3), "/nowhere")
    assert c.n_rand_vecs == 3 and c.datafolder == "/nowhere" and c._device_of is None
    assert c.bond_definitions == [(1, 2, (0, 0, 0)), (1, 2, (-1, 0, 0)), (1, 2, (0, -1, 0))]
    assert tuple(c.intersite_corr) == sb.SSH_BOND_CORR == ("BondBond", "CurrentCurrent", "BondPairGreens")
    for v in c.intersite_corr.values():                                     # default pairs: all n_def^2, first index slowest
        assert v.position.shape == v.momentum.shape == (9, 3, 3, 1, 9) and v.position.dtype == np.complex128 and v.position.flags["F_CONTIGUOUS"]
        assert v.pairs.tolist() == [[1, 1, 1, 2, 2, 2, 3, 3, 3], [1, 2, 3, 1, 2, 3, 1, 2, 3]]
    assert set(c.intersite_susc) == {"BondPairSusc"}                        # CurrentCurrent has no susceptibility
    s = c.intersite_susc["BondPairSusc"]
    assert s.position.shape == s.momentum.shape == (3, 3, 1, 9) and s.pairs is c.intersite_corr["BondPairGreens"].pairs
    # listed pairs are sorted; the equal-time request keeps one slice; an equal-time BondPairGreens has no susceptibility
    q = build("hc3x2_listed")
    c = sb.initialize_ssh_bond_container(q, LISTED, "")
    assert c.n_rand_vecs == 1 and c.intersite_susc == {}
    cc, bb, bp = (c.intersite_corr[k] for k in ("CurrentCurrent", "BondBond", "BondPairGreens"))
    assert cc.position.shape == (1, 3, 2, 1, 3) and cc.pairs.tolist() == [[1, 2, 3], [2, 2, 1]]
    assert bb.position.shape == (8, 3, 2, 1, 2) and bb.pairs.tolist() == [[1, 2], [1, 3]]
    assert bp.position.shape == (1, 3, 2, 1, 1) and bp.pairs.tolist() == [[1], [3]]
    # measure = false and no table: nothing
    for info in ({}, None, {"BondBond": {"measure": False, "time_dependent": True}, "CurrentCurrent": {"measure": False}}):
        c = sb.initialize_ssh_bond_container(m, info, "")
        assert c.intersite_corr == {} and c.intersite_susc == {}
    c = sb.initialize_ssh_bond_container(m, {"CurrentCurrent": TD}, "")
    assert set(c.intersite_corr) == {"CurrentCurrent"} and c.intersite_susc == {}


def test_refusals_name_the_request():
    from elphdynamics_amd import lattice as lat, measurements as ms, models, ssh_bond_measurements as sb, ssh_measurements as sm
    assert sb.UnsupportedMeasurement is ms.UnsupportedMeasurement
    hol = models.HolsteinModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    with pytest.raises(ms.UnsupportedMeasurement, match="Holstein"):
        sb.initialize_ssh_bond_container(hol, {"BondBond": TD}, "")
    with pytest.raises(ms.UnsupportedMeasurement, match="Holstein"):
        sb.accumulate_ssh_bonds_(sb.SSHBondContainer(), hol, None)
    bare = models.SSHModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    for name in sbref.CORRS:
        with pytest.raises(ms.UnsupportedMeasurement, match=name + ".*no bond definitions"):
            sb.initialize_ssh_bond_container(bare, {name: TD}, "")
    sb.initialize_ssh_bond_container(bare, {"BondBond": {"measure": False}}, "")
    m = build("psq6")
    m._nchains = 2
    with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
        sb.initialize_ssh_bond_container(m, {"CurrentCurrent": TD}, "")
    with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
        sb.accumulate_ssh_bonds_(sb.SSHBondContainer(), m, None)
    m._nchains = 1
    # the SSH container goes on refusing the three names, and says where they are measured
    for name in sbref.CORRS:
        with pytest.raises(ms.UnsupportedMeasurement, match=name + ".*initialize_ssh_bond_container"):
            sm.initialize_ssh_measurements_container(m, {name: TD}, "")
    with pytest.raises(RuntimeError, match="no SSH bond correlation"):
        sb.fetch_ssh_bonds_(sb.initialize_ssh_bond_container(m, {"BondBond": TD}, ""), m)
    # the estimator has to hold the vectors the container normalises for
    Gr = type("G", (), {"model": m, "nv": 2})()
    with pytest.raises(ValueError, match="num_random_vectors = 3"):
        sb.accumulate_ssh_bonds_(sb.initialize_ssh_bond_container(m, dict(ALL3, num_random_vectors=3), ""), m, Gr)


def parse(path):
    lines = open(path).read().splitlines()[1:]
    return np.array([float(ln.split()[1]) + 1j * float(ln.split()[2]) for ln in lines])


def check_files(d, want, V, dtau, bin, susc=True):
    """The written files of bin `bin` against the sums `want` divided by V, at 5e-9 absolute (half a unit of the 8 decimals written)."""
    import ssh_measurements_reference as sref
    for k, w in want.items():
        pos = w / V
        for space, arr in (("position", pos), ("momentum", sref.momentum(pos))):
            got = parse(os.path.join(d, "%s_%s_f" % (k, space), "%s_%s_%.5d.out" % (k, space, bin))).reshape(arr.shape, order="F")
            assert np.abs(got.real - arr.real).max() <= 5e-9 and np.abs(got.imag - arr.imag).max() <= 5e-9, (k, space)
            if k == "BondPairGreens" and susc:
                s = sref.simpson(arr, dtau)
                got = parse(os.path.join(d, "BondPairSusc_%s_f" % space, "BondPairSusc_%s_%.5d.out" % (space, bin))).reshape(s.shape, order="F")
                assert np.abs(got.real - s.real).max() <= 5e-9 and np.abs(got.imag - s.imag).max() <= 5e-9, ("BondPairSusc", space)


def test_folders_key_files_process_and_write(tmp_path):
    from elphdynamics_amd import ssh_bond_measurements as sb
    m, R, X, want = yardstick("hc3x2_both_ways")
    c = container_of("hc3x2_both_ways", m, str(tmp_path))
    sb.initialize_ssh_bond_folders_(c)
    assert sorted(os.listdir(tmp_path)) == sorted("%s_%s_f" % (k, s) for k in sbref.CORRS + ("BondPairSusc",) for s in ("position", "momentum"))
    rows = open(tmp_path / "CurrentCurrent_position_f" / "CurrentCurrent_position_key.out").read().splitlines()
    assert rows[0] == "index bond1 bond2 r3 r2 r1 tau" and len(rows) == 1 + 8 * 6 * 9
    assert rows[1] == "1 1 1 0 0 0 0" and rows[2] == "2 1 1 0 0 0 1" and rows[9] == "9 1 1 0 0 1 0" and rows[49] == "49 1 2 0 0 0 0"
    assert open(tmp_path / "CurrentCurrent_momentum_f" / "CurrentCurrent_momentum_key.out").readline() == "index bond1 bond2 k3 k2 k1 tau\n"
    assert open(tmp_path / "BondPairSusc_position_f" / "BondPairSusc_position_key.out").readline() == "index bond1 bond2 r3 r2 r1\n"
    # process and write on the direct sums put in by hand (what fetch_ssh_bonds_ would have copied from the device)
    for k, v in c.intersite_corr.items():
        v.position[...] = want[k]
    c._device_of = m
    m._lib = type("L", (), {"elph_ssh_bond_fetch": staticmethod(lambda *a: 0), "elph_ssh_bond_reset": staticmethod(lambda *a: 0)})()
    m._h = 1
    try:
        sb.process_ssh_bond_measurements_(c, 2, m)
        V = 2 * 3                                                           # bin_size * binomial(3, 2)
        for k, v in c.intersite_corr.items():
            assert np.abs(v.position - want[k] / V).max() < 1e-15 * max(1.0, np.abs(want[k]).max())
        sb.write_ssh_bond_measurements_(c, m, 12)
        check_files(str(tmp_path), want, V, m.dtau, 12)
        lines = open(tmp_path / "CurrentCurrent_momentum_f" / "CurrentCurrent_momentum_00012.out").read().splitlines()
        assert lines[0] == "index CurrentCurrent_momentum_real CurrentCurrent_momentum_imag" and len(lines) == 1 + 8 * 6 * 9
        sb.reset_ssh_bond_measurements_(c, m)
        assert all(not v.position.any() and not v.momentum.any() for g in (c.intersite_corr, c.intersite_susc) for v in g.values())
    finally:
        m._lib, m._h = None, None
