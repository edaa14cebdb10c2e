"""Host side of the SSH measurements (elphdynamics_amd/ssh_measurements.py) and the tests' own yardstick
(tests/ssh_measurements_reference.py): none of this needs a device.  Models here never reach initialize_model_'s library call."""
import os

import numpy as np
import pytest

import ssh_cases as sc
import ssh_measurement_cases as smc
import ssh_measurements_reference as ref


def host_case(name):
    return smc.build_case(name, device=False)[0]


def host_shape(name):
    norb, dims, defs, L = sc.SHAPES[name]
    return smc.build_model(norb, dims, defs, L, seed=3, device=False)


def test_container_keys_shapes_and_pair_defaults():
    from elphdynamics_amd import ssh_measurements as sm
    m = host_case("hc3")
    c = sm.initialize_ssh_measurements_container(m, dict(smc.ALL_TD, num_random_vectors=3), "/nowhere")
    assert c.n_rand_vecs == 3 and c.datafolder == "/nowhere" and c.snapshots == []
    assert set(c.global_meas) == {"density", "Nsqr", "mu"}
    assert tuple(c.onsite_meas) == ("density", "double_occ", "mu") and all(v.shape == (2,) and v.dtype == np.complex128 for v in c.onsite_meas.values())
    assert tuple(c.intersite_meas) == ("x", "x2", "x4", "phonon_pe", "phonon_ke", "elph_energy", "el_ke", "sign_switch")
    assert all(v.shape == (3,) and v.dtype == np.complex128 for v in c.intersite_meas.values())
    assert set(c.onsite_corr) == {"Greens", "DenDen", "SpinSpin", "PairGreens"} and set(c.intersite_corr) == {"PhononGreens"}
    g, p = c.onsite_corr["Greens"], c.intersite_corr["PhononGreens"]
    assert g.position.shape == (9, 3, 3, 1, 4) and g.pairs.tolist() == [[1, 1, 2, 2], [1, 2, 1, 2]] and g.position.flags["F_CONTIGUOUS"]
    assert p.position.shape == p.momentum.shape == (9, 3, 3, 1, 9)                               # nph^2 pairs of phonon types
    assert p.pairs.tolist() == [[1, 1, 1, 2, 2, 2, 3, 3, 3], [1, 2, 3, 1, 2, 3, 1, 2, 3]]
    assert set(c.onsite_susc) == {"PairSusc", "ChargeSusc", "SpinSusc"} and c.intersite_susc == {}
    assert c.onsite_susc["ChargeSusc"].position.shape == (3, 3, 1, 4)
    # explicit lists are sorted; an equal-time correlation has no susceptibility
    c = sm.initialize_ssh_measurements_container(m, smc.HC3_TABLE, "")
    assert c.n_rand_vecs == 1 and c.intersite_corr["PhononGreens"].pairs.tolist() == [[1, 2, 3], [2, 2, 1]]
    assert c.onsite_corr["DenDen"].position.shape == (1, 3, 3, 1, 2) and set(c.onsite_susc) == {"PairSusc", "SpinSusc"}
    # one phonon type among two definitions; no table at all: scalars only
    q = host_case("psq6")
    c = sm.initialize_ssh_measurements_container(q, smc.ALL_TD, "")
    assert c.intersite_corr["PhononGreens"].pairs.tolist() == [[1], [1]] and c.intersite_meas["el_ke"].shape == (2,)
    c0 = sm.initialize_ssh_measurements_container(q, {}, "")
    assert c0.onsite_corr == {} and c0.intersite_corr == {} and c0.onsite_susc == {}


@pytest.mark.parametrize("name", ["BondBond", "CurrentCurrent", "BondPairGreens"])
def test_intersite_correlations_are_refused_by_name(name):
    from elphdynamics_amd import ssh_measurements as sm
    m = host_case("psq6")
    info = dict(smc.ALL_TD)
    info[name] = {"measure": True, "time_dependent": True}
    with pytest.raises(sm.UnsupportedMeasurement, match=name):
        sm.initialize_ssh_measurements_container(m, info, "")
    info[name] = {"measure": False, "time_dependent": True}
    sm.initialize_ssh_measurements_container(m, info, "")


def test_other_out_of_scope_requests_are_refused_by_name():
    from elphdynamics_amd import lattice as lat, models, ssh_measurements as sm
    m = host_case("psq6")
    with pytest.raises(sm.UnsupportedMeasurement, match="BondPairSusc"):
        sm.initialize_ssh_measurements_container(m, {"BondPairGreens": {"measure": True, "time_dependent": True}}, "")
    for key in ("density", "double_occupancy", "phonon_position"):
        with pytest.raises(sm.UnsupportedMeasurement, match="Snapshots.*" + key):
            sm.initialize_ssh_measurements_container(m, {"Snapshots": {key: True}}, "")
        sm.initialize_ssh_measurements_container(m, {"Snapshots": {key: False}}, "")
    hol = models.HolsteinModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    with pytest.raises(sm.UnsupportedMeasurement, match="Holstein"):
        sm.initialize_ssh_measurements_container(hol, smc.ALL_TD, "")
    m._nchains = 2
    with pytest.raises(sm.UnsupportedMeasurement, match="chains"):
        sm.initialize_ssh_measurements_container(m, smc.ALL_TD, "")
    with pytest.raises(sm.UnsupportedMeasurement, match="chains"):
        sm.accumulate_(sm.SSHMeasurementsContainer(), m, None)


@pytest.mark.parametrize("name", ["psq6", "phc4", "hc3"])
def test_bond_to_definition_and_bond_to_phonon(name):
    """SSHModels.jl:386-431: 1-based, 0 = a bare bond; against the tables of tests/ssh_reference.py."""
    m = host_shape(name)
    tab = sc.make_case(name).tab
    per = list(tab.per_definition)
    assert m.nbonds == len(per) and m.bond_to_definition.dtype == m.bond_to_phonon.dtype == np.int64
    assert m.bond_to_definition.tolist() == [d + 1 for d, n in enumerate(per) for _ in range(n)]
    want, nph = [], 0
    for (_, _, _, has_phonon, _, _), n in zip(sc.SHAPES[name][2], per):
        want += list(range(nph * n + 1, (nph + 1) * n + 1)) if has_phonon else [0] * n
        nph += bool(has_phonon)
    assert m.bond_to_phonon.tolist() == want and nph == m.nph
    # inverse of phonon_to_bond where a bond has a phonon
    has = m.bond_to_phonon > 0
    assert has.sum() == m.Nph and np.array_equal(m.phonon_to_bond[m.bond_to_phonon[has] - 1], np.flatnonzero(has) + 1)
    if name == "psq6":
        assert not has[:36].any() and has[36:].all() and m.phonon_to_bond[0] == 37      # bare bonds first: phonon_to_bond is not the identity


def fft_phonon_greens(x, b1, b2, L, L0, nph, dims):
    """translational_average!(x2x1, x_b2, x_b1) as Utilities.jl:49-60 writes it."""
    X = np.asarray(x).reshape((nph,) + tuple(dims[::-1]) + (L,)).transpose(4, 3, 2, 1, 0)       # (L, L1, L2, L3, nph)
    f, g = np.fft.fftn(X[..., b2 - 1]), np.fft.fftn(X[..., b1 - 1])
    gp = np.roll(g, tuple(n - 1 for n in g.shape), axis=(0, 1, 2, 3))[::-1, ::-1, ::-1, ::-1]
    fg = np.fft.ifftn(f * gp / f.size)
    assert np.abs(fg.imag).max() < 1e-13
    return fg.real.reshape(L, -1, order="F")[np.arange(L0) % L]


@pytest.mark.parametrize("name", ["hc3", "tri4_Lt7", "cubic3x2x2"])
def test_reference_phonon_greens_against_fft_form(name):
    m = host_case(name)
    la = m.lattice
    dims = (la.L1, la.L2, la.L3)
    for b1 in range(1, m.nph + 1):
        for b2 in range(1, m.nph + 1):
            for L0 in (1, m.Ltau + 1):
                a = ref.phonon_greens(m.x, b1, b2, m.Ltau, L0, m.nph, dims)
                b = fft_phonon_greens(m.x, b1, b2, m.Ltau, L0, m.nph, dims)
                assert a.shape == b.shape == (L0, la.ncells) and np.abs(a - b).max() < 1e-13 * max(1.0, np.abs(b).max())
    with pytest.raises(ValueError, match="DimensionMismatch"):
        ref.phonon_greens(m.x[:-m.Ltau], 1, 1, m.Ltau, 1, m.nph, dims)


def test_reference_scalars_on_a_constant_case():
    """The restatement on inputs whose sums are known in closed form: M^-1 r = g r^-1 makes every estimate G = g."""
    m = host_case("psq6")
    rng = np.random.default_rng(1)
    R = rng.standard_normal((2, m.Ndim))
    g = 0.3
    want = ref.measure(R, g / R, m.x, smc.ref_par(m), {})
    assert abs(want["glob"]["density"] - 2 * (1 - g)) < 1e-12 and np.allclose(want["onsite"]["double_occ"], (1 - g) ** 2)
    assert np.allclose(want["onsite"]["mu"], m.mu.mean()) and abs(want["glob"]["mu"] - m.mu.mean()) < 1e-15
    X = m.x.reshape(m.Nph, m.Ltau)
    assert np.allclose(want["inter"]["x"], [0.0, X.mean()]) and np.allclose(want["inter"]["x2"], [0.0, (X ** 2).mean()])
    assert np.allclose(want["inter"]["phonon_pe"][1], (m.omega[:, None] ** 2 * X ** 2 / 2).mean()) and want["inter"]["phonon_ke"][0] == 0.0
    assert np.all(want["inter"]["sign_switch"] == 0.0)
    # el_ke of the bare definition: -t h / V with h = -(g r_i / r_j + ...), non-zero; of the phonon definition it differs from the bare-t value
    assert want["inter"]["el_ke"][0] != 0.0 and want["abs"]["inter"]["el_ke"][1] > 0.0


def test_sign_switch_case_switches_some_but_not_all():
    m = host_case("sq12x6")
    rng = np.random.default_rng(2)
    want = ref.measure(rng.standard_normal((2, m.Ndim)), rng.standard_normal((2, m.Ndim)), m.x, smc.ref_par(m), {})
    assert m.t[72:].max() < 0 < m.t[:72].min()                                                   # negative bare hopping on y
    assert np.all(want["inter"]["sign_switch"] > 0.0) and np.all(want["inter"]["sign_switch"] < 1.0)


def parse(path):
    lines = open(path).read().splitlines()[1:]
    return np.array([float(ln.split()[1]) + 1j * float(ln.split()[2]) for ln in lines])


def test_folders_keys_and_files_parse_back(tmp_path):
    from elphdynamics_amd import ssh_measurements as sm
    m = host_case("hc3")
    c = sm.initialize_ssh_measurements_container(m, dict(smc.HC3_TABLE, num_random_vectors=3), str(tmp_path))
    sm.initialize_measurement_folders_(c)
    d = str(tmp_path)
    made = sorted(os.listdir(d))
    want = ["global_measurements_f", "onsite_measurements_f", "intersite_measurements_f"]
    for k in ("Greens", "DenDen", "SpinSpin", "PairGreens", "PhononGreens", "PairSusc", "SpinSusc"):
        want += ["%s_position_f" % k, "%s_momentum_f" % k]
    assert made == sorted(want)
    key = open(os.path.join(d, "PhononGreens_position_f", "PhononGreens_position_key.out")).read().splitlines()
    assert key[0] == "index bond1 bond2 r3 r2 r1 tau" and len(key) == 1 + 9 * 9 * 3
    assert key[1] == "1 1 2 0 0 0 0" and key[2] == "2 1 2 0 0 0 1" and key[10] == "10 1 2 0 0 1 0" and key[-1] == "243 3 1 0 2 2 8"
    key = open(os.path.join(d, "Greens_momentum_f", "Greens_momentum_key.out")).read().splitlines()
    assert key[0] == "index orbit1 orbit2 k3 k2 k1 tau" and key[-1] == "162 2 2 0 2 2 8"
    key = open(os.path.join(d, "SpinSusc_position_f", "SpinSusc_position_key.out")).read().splitlines()
    assert key[0] == "index orbit1 orbit2 r3 r2 r1" and len(key) == 1 + 9
    # fill the container as a fetch would, then process by hand (no device) and write
    rng = np.random.default_rng(4)
    for k in c.global_meas:
        c.global_meas[k] = complex(rng.standard_normal())
    for group in (c.onsite_meas, c.intersite_meas):
        for v in group.values():
            v[:] = rng.standard_normal(v.shape)
    for group in (c.onsite_corr, c.intersite_corr):
        for corr in group.values():
            corr.position[...] = rng.standard_normal(corr.position.shape)
    pos = {k: v.position.copy() for k, v in list(c.onsite_corr.items()) + list(c.intersite_corr.items())}
    scal = {k: v.copy() for k, v in list(c.onsite_meas.items()) + list(c.intersite_meas.items())}
    c._device_of = m
    orig, sm.fetch_ = sm.fetch_, lambda container, model: None
    try:
        sm.process_measurements_(c, 2, m)                                                        # V = 2 * binomial(3, 2) = 6
    finally:
        sm.fetch_ = orig
    sm.write_measurements_(c, m, 7)
    V = 6
    lines = open(os.path.join(d, "intersite_measurements_f", "intersite_measurements_00007.out")).read().splitlines()
    assert lines[0] == "measurement bond value" and [ln.split()[0] for ln in lines[1::3]] == list(sm.INTERSITE_KEYS) and len(lines) == 1 + 8 * 3
    for ln in lines[1:]:
        k, b, v = ln.split()
        assert abs(float(v) - scal[k][int(b) - 1].real / V) <= 5e-9
    lines = open(os.path.join(d, "onsite_measurements_f", "onsite_measurements_00007.out")).read().splitlines()
    assert lines[0] == "measurement orbit value" and [ln.split()[0] for ln in lines[1::2]] == ["density", "double_occ", "mu"]
    assert [ln.split()[0] for ln in open(os.path.join(d, "global_measurements_f", "global_measurements_00007.out"))] == ["density", "Nsqr", "mu"]
    for k, p in pos.items():
        for space, arr in (("position", p / V), ("momentum", ref.momentum(p / V))):
            got = parse(os.path.join(d, "%s_%s_f" % (k, space), "%s_%s_00007.out" % (k, space))).reshape(arr.shape, order="F")
            assert np.abs(got - arr).max() <= 1e-8, (k, space)
    s = ref.simpson(pos["SpinSpin"] / V, m.dtau)
    got = parse(os.path.join(d, "SpinSusc_position_f", "SpinSusc_position_00007.out")).reshape(s.shape, order="F")
    assert np.abs(got - s).max() <= 1e-8
    sm.reset_measurements_(c, None)
    assert not any(np.any(v.position) or np.any(v.momentum) for g in (c.onsite_corr, c.intersite_corr, c.onsite_susc) for v in g.values())
    assert not any(np.any(v) for g in (c.onsite_meas, c.intersite_meas) for v in g.values()) and c.global_meas["Nsqr"] == 0
