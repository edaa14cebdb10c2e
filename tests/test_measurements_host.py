"""Host side of the measurements (elphdynamics_amd/measurements.py) and the tests' own yardstick (tests/measurements_reference.py): none
of this needs a device.  Models here never reach initialize_model_'s library call: the container constructor reads host attributes only.

The direct-sum reference is pinned at the end against a second evaluation of the same definitions with np.fft written as the reference
writes convolve! (GreensFunctions.jl:351-400) and translational_average! (Utilities.jl:49-60)."""
import os

import numpy as np
import pytest

import measurements_reference as ref


def host_model(ns=1, dims=(4, 4, 1), L=8, bonds=(), t=None):
    """A HolsteinModel with its host attributes as initialize_model_ leaves them, without the device."""
    from elphdynamics_amd import lattice as lat, models
    m = models.HolsteinModel(lat.Lattice(ns, *dims), L * 0.1, 0.1)
    assert m.Ltau == L
    for k, (o1, o2, d) in enumerate(bonds):
        m.assign_t_(1.0 if t is None else t[k], o1, o2, d)
    m._create = lambda *a, **k: None
    m.initialize_model_()
    return m


FULL = {"num_random_vectors": 3,
        "Greens": {"measure": True, "time_dependent": True},
        "DenDen": {"measure": True, "time_dependent": False},
        "SpinSpin": {"measure": True, "time_dependent": True, "pairs": [[2, 2], [1, 2]]},
        "PairGreens": {"measure": True, "time_dependent": True, "pairs": [[2, 1]]},
        "PhononGreens": {"measure": False, "time_dependent": True},
        "BondBond": {"measure": False, "time_dependent": False},
        "Snapshots": {"density": False, "double_occupancy": False, "phonon_position": False}}


def test_container_shapes_pairs_and_susceptibilities():
    from elphdynamics_amd import measurements as ms
    m = host_model(ns=2, dims=(3, 2, 1), L=7)
    c = ms.initialize_measurements_container(m, FULL, "/nowhere")
    assert c.n_rand_vecs == 3 and c.datafolder == "/nowhere"
    assert set(c.global_meas) == {"density", "Nsqr", "mu"}
    assert set(c.onsite_meas) == set(ref.ONSITE_KEYS) and all(v.shape == (2,) and v.dtype == np.complex128 for v in c.onsite_meas.values())
    assert c.intersite_meas["el_ke"].shape == (0,)
    assert set(c.onsite_corr) == {"Greens", "DenDen", "SpinSpin", "PairGreens"}                 # PhononGreens: measure = false
    g, d, s, p = (c.onsite_corr[k] for k in ("Greens", "DenDen", "SpinSpin", "PairGreens"))
    assert g.position.shape == g.momentum.shape == (8, 3, 2, 1, 4) and g.position.dtype == np.complex128 and g.position.flags["F_CONTIGUOUS"]
    assert g.pairs.tolist() == [[1, 1, 2, 2], [1, 2, 1, 2]]                                     # default: first orbital slowest
    assert d.position.shape == (1, 3, 2, 1, 4)                                                  # equal-time
    assert s.position.shape == (8, 3, 2, 1, 2) and s.pairs.tolist() == [[1, 2], [2, 2]]         # sorted
    assert p.position.shape == (8, 3, 2, 1, 1) and p.pairs.tolist() == [[2], [1]]
    # susceptibilities only for time-dependent correlations: DenDen is equal-time here
    assert set(c.onsite_susc) == {"PairSusc", "SpinSusc"}
    assert c.onsite_susc["SpinSusc"].position.shape == (3, 2, 1, 2) and c.onsite_susc["SpinSusc"].pairs is s.pairs
    assert c.intersite_corr == {} and c.intersite_susc == {} and c.snapshots == []
    # no table at all: scalars only
    c0 = ms.initialize_measurements_container(m, {}, "")
    assert c0.n_rand_vecs == 1 and c0.onsite_corr == {} and c0.onsite_susc == {}
    assert ms.initialize_measurements_container(host_model(bonds=[(1, 1, (1, 0, 0)), (1, 1, (0, 1, 0))]), {}, "").intersite_meas["el_ke"].shape == (2,)


@pytest.mark.parametrize("name", ["BondBond", "CurrentCurrent", "BondPairGreens"])
def test_intersite_correlations_are_refused_by_name(name):
    from elphdynamics_amd import measurements as ms
    info = dict(FULL)
    info[name] = {"measure": True, "time_dependent": True}
    with pytest.raises(ms.UnsupportedMeasurement, match=name):
        ms.initialize_measurements_container(host_model(), info, "")
    info[name] = {"measure": False, "time_dependent": True}
    ms.initialize_measurements_container(host_model(), info, "")


def test_other_out_of_scope_requests_are_refused_by_name():
    from elphdynamics_amd import lattice as lat, measurements as ms, models
    with pytest.raises(ms.UnsupportedMeasurement, match="BondPairSusc"):
        ms.initialize_measurements_container(host_model(), {"BondPairGreens": {"measure": True, "time_dependent": True}}, "")
    for key in ("density", "double_occupancy", "phonon_position"):
        with pytest.raises(ms.UnsupportedMeasurement, match="Snapshots.*" + key):
            ms.initialize_measurements_container(host_model(), {"Snapshots": {key: True}}, "")
    ssh = models.SSHModel(lat.Lattice(1, 4, 4, 1), 1.0, 0.1)
    with pytest.raises(ms.UnsupportedMeasurement, match="SSH"):
        ms.initialize_measurements_container(ssh, FULL, "")
    m = host_model()
    m._nchains = 2
    with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
        ms.initialize_measurements_container(m, FULL, "")
    # duplicate bonds removed on an axis of two cells: the reference's bond -> definition map does not hold, el_ke says so
    with pytest.raises(ValueError, match="definitions"):
        ms.bond_arrays(host_model(dims=(4, 2, 1), bonds=[(1, 1, (1, 0, 0)), (1, 1, (0, 1, 0))]))


def test_simpson_rule():
    """Exact on cubics for an odd number of points; for an even number Simpson on all but the last interval plus the reference's
    three-point end correction (Utilities.jl:72-74), which is exact on quadratics."""
    from elphdynamics_amd import measurements as ms
    dx = 0.1
    for n in (3, 9, 41):
        t = dx * np.arange(n)
        f = 0.3 - 1.1 * t + 0.7 * t ** 2 + 2.3 * t ** 3
        exact = 0.3 * t[-1] - 1.1 * t[-1] ** 2 / 2 + 0.7 * t[-1] ** 3 / 3 + 2.3 * t[-1] ** 4 / 4
        assert abs(ms.simpson(f, dx) - exact) < 1e-13 * max(1.0, abs(exact))
        assert abs(ref.simpson(f, dx) - exact) < 1e-13 * max(1.0, abs(exact))
    for n in (4, 8, 26):
        t = dx * np.arange(n)
        f = np.cos(1.3 * t) + 0.2 * t ** 3
        want = ms.simpson(f[:-1], dx) + dx * (5 / 12 * f[-1] + 2 / 3 * f[-2] - 1 / 12 * f[-3])
        assert abs(ms.simpson(f, dx) - want) < 1e-15 * n
        q = 0.4 + 0.9 * t - 1.7 * t ** 2
        assert abs(ms.simpson(q, dx) - (0.4 * t[-1] + 0.9 * t[-1] ** 2 / 2 - 1.7 * t[-1] ** 3 / 3)) < 1e-13
    # along the first axis of an array, complex values
    rng = np.random.default_rng(5)
    a = rng.standard_normal((9, 3, 2)) + 1j * rng.standard_normal((9, 3, 2))
    got = ms.simpson(a, dx)
    assert got.shape == (3, 2) and abs(got[1, 1] - ms.simpson(a[:, 1, 1], dx)) < 1e-15
    assert np.abs(got - ref.simpson(a, dx)).max() < 1e-14


def filled_container(tmp, ns=2, dims=(3, 2, 2), L=5, seed=11):
    from elphdynamics_amd import measurements as ms
    m = host_model(ns=ns, dims=dims, L=L, bonds=[(1, 1, (1, 0, 0)), (1, ns, (1, 1, 0))])
    info = {"num_random_vectors": 4, "Greens": {"measure": True, "time_dependent": True},
            "DenDen": {"measure": True, "time_dependent": False, "pairs": [[1, ns]]},
            "PhononGreens": {"measure": True, "time_dependent": True, "pairs": [[ns, ns], [1, 1]]}}
    c = ms.initialize_measurements_container(m, info, str(tmp))
    rng = np.random.default_rng(seed)
    for k in c.global_meas:
        c.global_meas[k] = complex(rng.standard_normal() * 50)
    for grp in (c.onsite_meas, c.intersite_meas):
        for k in grp:
            grp[k][:] = rng.standard_normal(grp[k].shape) * 50
    for corr in c.onsite_corr.values():
        corr.position[...] = rng.standard_normal(corr.position.shape) * 50
    return m, c


def test_momentum_copy_is_the_direct_dft_and_normalisation(tmp_path):
    from elphdynamics_amd import measurements as ms
    m, c = filled_container(tmp_path)
    raw = {k: v.position.copy() for k, v in c.onsite_corr.items()}
    raw_s = {k: v.copy() for k, v in c.onsite_meas.items()}
    raw_g = dict(c.global_meas)
    raw_b = c.intersite_meas["el_ke"].copy()
    ms.fourier_transform_correlations_(c.onsite_corr)
    L1, L2, L3 = 3, 2, 2
    l1, l2, l3 = np.meshgrid(np.arange(L1), np.arange(L2), np.arange(L3), indexing="ij")
    for k, corr in c.onsite_corr.items():
        assert np.array_equal(corr.position, raw[k])
        for (k1, k2, k3) in [(0, 0, 0), (1, 1, 0), (2, 0, 1), (1, 1, 1)]:
            ph = np.exp(-2j * np.pi * (k1 * l1 / L1 + k2 * l2 / L2 + k3 * l3 / L3))
            direct = np.einsum("txyzp,xyz->tp", raw[k], ph)
            assert np.abs(corr.momentum[:, k1, k2, k3, :] - direct).max() < 1e-12 * np.abs(raw[k]).max() * L1 * L2 * L3
        assert np.abs(corr.momentum - ref.momentum(raw[k])).max() == 0
    mom = {k: v.momentum.copy() for k, v in c.onsite_corr.items()}
    bin_size = 7
    ms.normalize_(c, bin_size)
    V = bin_size * 6                                                        # binomial(4, 2)
    for k in raw:
        assert np.array_equal(c.onsite_corr[k].position, raw[k] / V) and np.array_equal(c.onsite_corr[k].momentum, mom[k] / V)
    for k in raw_s:
        assert np.array_equal(c.onsite_meas[k], raw_s[k] / V)
    assert all(c.global_meas[k] == raw_g[k] / V for k in raw_g) and np.array_equal(c.intersite_meas["el_ke"], raw_b / V)
    ms.measure_susceptibilities_(c, m.dtau)
    assert c.onsite_susc == {}                                              # DenDen is equal-time: no susceptibility container at all
    c.n_rand_vecs = 1
    with pytest.raises(ValueError):
        ms.normalize_(c, bin_size)


def read_table(path, header):
    lines = open(path).read().splitlines()
    assert lines[0] == header, (path, lines[0])
    return [ln.split() for ln in lines[1:]]


def test_files_parse_back_and_keys_list_every_index(tmp_path):
    from elphdynamics_amd import measurements as ms
    m = host_model(ns=2, dims=(3, 2, 2), L=5, bonds=[(1, 1, (1, 0, 0)), (1, 2, (1, 1, 0))])
    info = {"num_random_vectors": 4, "Greens": {"measure": True, "time_dependent": True},
            "PairGreens": {"measure": True, "time_dependent": True, "pairs": [[2, 1], [1, 2]]},
            "DenDen": {"measure": True, "time_dependent": False, "pairs": [[1, 2]]}}
    c = ms.initialize_measurements_container(m, info, str(tmp_path))
    rng = np.random.default_rng(3)
    for k in c.global_meas:
        c.global_meas[k] = complex(rng.standard_normal() * 3)
    for grp in (c.onsite_meas, c.intersite_meas):
        for k in grp:
            grp[k][:] = rng.standard_normal(grp[k].shape) * 3
    for corr in c.onsite_corr.values():
        corr.position[...] = rng.standard_normal(corr.position.shape) * 3
    ms.initialize_measurement_folders_(c)
    ms.fourier_transform_correlations_(c.onsite_corr)
    ms.normalize_(c, 2)
    ms.measure_susceptibilities_(c, m.dtau)
    ms.write_measurements_(c, m, 12)
    d = str(tmp_path)
    want_dirs = {"global_measurements_f", "onsite_measurements_f", "intersite_measurements_f"}
    for k in ("Greens", "PairGreens", "DenDen", "PairSusc"):
        want_dirs |= {k + "_position_f", k + "_momentum_f"}
    assert set(os.listdir(d)) == want_dirs
    # scalars: name-keyed lines at 8 decimals
    rows = [ln.split() for ln in open(os.path.join(d, "global_measurements_f", "global_measurements_00012.out")).read().splitlines()]
    assert [r[0] for r in rows] == ["density", "Nsqr", "mu"]
    for name, val in rows:
        assert abs(float(val) - c.global_meas[name].real) <= 5e-9 and len(val.split(".")[1]) == 8
    rows = read_table(os.path.join(d, "onsite_measurements_f", "onsite_measurements_00012.out"), "measurement orbit value")
    assert len(rows) == 9 * 2
    for name, o, val in rows:
        assert abs(float(val) - c.onsite_meas[name][int(o) - 1].real) <= 5e-9
    rows = read_table(os.path.join(d, "intersite_measurements_f", "intersite_measurements_00012.out"), "measurement bond value")
    assert [(r[0], r[1]) for r in rows] == [("el_ke", "1"), ("el_ke", "2")]
    for name, b, val in rows:
        assert abs(float(val) - c.intersite_meas[name][int(b) - 1].real) <= 5e-9
    # arrays: 1-based index in memory order, real and imaginary parts
    for group in (c.onsite_corr, c.onsite_susc):
        for name, corr in group.items():
            for space in ("position", "momentum"):
                arr = getattr(corr, space)
                meas = "%s_%s" % (name, space)
                rows = read_table(os.path.join(d, meas + "_f", meas + "_00012.out"), "index %s_real %s_imag" % (meas, meas))
                assert [int(r[0]) for r in rows] == list(range(1, arr.size + 1))
                got = np.array([float(r[1]) + 1j * float(r[2]) for r in rows]).reshape(arr.shape, order="F")
                assert np.abs(got.real - arr.real).max() <= 5e-9 and np.abs(got.imag - arr.imag).max() <= 5e-9
                # the key: every index once, orbitals of the pair, displacements 0-based, slowest axis first
                letter = "r" if space == "position" else "k"
                tail = " tau" if arr.ndim == 5 else ""
                keys = read_table(os.path.join(d, meas + "_f", meas + "_key.out"), "index orbit1 orbit2 %s3 %s2 %s1%s" % (letter, letter, letter, tail))
                assert [int(r[0]) for r in keys] == list(range(1, arr.size + 1))
                seen = set()
                for r in keys:
                    v = [int(z) for z in r]
                    cidx = tuple(v[3:][::-1])                               # (tau,) l1, l2, l3
                    p = [q for q in range(corr.pairs.shape[1]) if (corr.pairs[0, q], corr.pairs[1, q]) == (v[1], v[2])]
                    assert len(p) == 1
                    full = cidx + (p[0],)
                    assert np.ravel_multi_index(full, arr.shape, order="F") == v[0] - 1
                    seen.add(full)
                assert len(seen) == arr.size
    assert c.onsite_corr["PairGreens"].pairs.tolist() == [[1, 2], [2, 1]]
    # reset: zeros everywhere (no device was ever attached to this container)
    ms.reset_measurements_(c, m)
    assert all(v == 0 for v in c.global_meas.values()) and not any(v.any() for v in c.onsite_meas.values())
    assert not any(k.position.any() or k.momentum.any() for g in (c.onsite_corr, c.onsite_susc) for k in g.values())


def test_bond_arrays_follow_the_definitions_with_bond_dependent_t():
    """model.t stays in definition order, model.neighbor_table is sorted into checkerboard order: row checkerboard_perm[bond] of the
    sorted table is bond `bond` of the definition-ordered list (up to the orientation of the two sites, which el_ke does not see)."""
    from elphdynamics_amd import measurements as ms
    bonds = [(1, 2, (0, 0, 0)), (1, 2, (-1, 0, 0)), (2, 2, (1, 1, 0))]
    m = host_model(ns=2, dims=(4, 3, 1), L=4, bonds=bonds, t=[1.0, 0.7, -0.4])
    rng = np.random.default_rng(8)
    m.t = m.t * (1 + 0.1 * rng.standard_normal(m.t.shape))                  # bond-dependent, after the sort: t is not permuted by it
    sites, t = ms.bond_arrays(m)
    nc = m.lattice.ncells
    assert sites.shape == (3 * nc, 2) and np.array_equal(t, m.t)
    for d, (o1, o2, v) in enumerate(bonds):
        want = m.lattice.calc_neighbor_table(o1, o2, v)
        assert np.array_equal(np.sort(sites[d * nc:(d + 1) * nc], axis=1), np.sort(want, axis=1)), d


# ---- the yardstick itself: direct sums against the reference's own FFT formulation ----------------------------------------------

def fft_tables(r1, x1, r2, x2, L, ns, dims):
    """setup! with convolve! as the reference writes it (GreensFunctions.jl:239-288, :351-400): doubled arrays [2L, ns, L1, L2, L3], fft over
    (tau, cells), a[w, s2, k] * b[-w, s1, -k] / V, inverse fft."""
    nc = dims[0] * dims[1] * dims[2]

    def arr(v, sign):
        f = np.asarray(v).reshape(nc, ns, L).transpose(2, 1, 0).reshape((L, ns) + tuple(dims), order="F")
        return np.concatenate([f, sign * f], axis=0).astype(np.complex128)

    def convolve(a, b):
        fa, fb = np.fft.fftn(a, axes=(0, 2, 3, 4)), np.fft.fftn(b, axes=(0, 2, 3, 4))
        fbn = np.roll(np.flip(fb, axis=(0, 2, 3, 4)), 1, axis=(0, 2, 3, 4))              # b[-w, s1, -k]
        V = 2 * L * nc
        ab = fa[:, :, None] * fbn[:, None, :] / V                                        # [w, s2, s1, k]
        out = np.fft.ifftn(ab, axes=(0, 3, 4, 5))
        assert np.abs(out.imag).max() < 1e-12 * max(1.0, np.abs(out.real).max())
        return out.real.reshape((2 * L, ns, ns, nc), order="F")

    X1, X2, R1, R2 = arr(x1, -1), arr(x2, -1), arr(r1, -1), arr(r2, -1)
    pX1, pX2, pR1, pR2 = arr(x1, 1), arr(x2, 1), arr(r1, 1), arr(r2, 1)
    s2 = np.sqrt(2.0)
    return [convolve((X1 + X2) / s2, (R1 + R2) / s2), convolve(pX1 * pX2, pR1 * pR2), convolve(pX2 * pR2, pX1 * pR1),
            convolve(pX1 * pR2, pX2 * pR1)]


def fft_phonon(x, o1, o2, L, L0, ns, dims):
    """translational_average! (Utilities.jl:49-60): fg = ifft(fft(f) * reverse(circshift(fft(g))) / N)."""
    nc = dims[0] * dims[1] * dims[2]
    X = np.asarray(x).reshape(nc, ns, L).transpose(2, 1, 0)
    f = X[:, o1 - 1, :].reshape((L,) + tuple(dims), order="F").astype(np.complex128)
    g = X[:, o2 - 1, :].reshape((L,) + tuple(dims), order="F").astype(np.complex128)
    ff, fg = np.fft.fftn(f), np.fft.fftn(g)
    gp = np.flip(np.roll(fg, [s - 1 for s in fg.shape], axis=(0, 1, 2, 3)))
    out = np.fft.ifftn(ff * gp / f.size).real.reshape((L, nc), order="F")
    return out[np.arange(L0) % L]


@pytest.mark.parametrize("ns,dims,L", [(1, (4, 3, 1), 6), (2, (3, 2, 1), 5), (1, (3, 2, 2), 4)])
def test_direct_sum_reference_matches_the_fft_formulation(ns, dims, L):
    from elphdynamics_amd import lattice as lat
    rng = np.random.default_rng(sum(dims) + L + ns)
    la = lat.Lattice(ns, *dims)
    N, nc = la.nsites, la.ncells
    R, X = rng.standard_normal((3, N * L)), rng.standard_normal((3, N * L))
    x = rng.standard_normal(N * L)
    defs = [(1, 1, (1, 0, 0)), (1, ns, (1, 1, 0))]
    bonds = []
    for (o1, o2, v) in defs:
        tab = la.calc_neighbor_table(o1, o2, v)
        assert tab.shape[0] == nc
        bonds.append((tab[:, 0], tab[:, 1], 1 + 0.2 * rng.standard_normal(nc)))
    par = dict(L=L, ns=ns, dims=dims, dtau=0.1, omega=1 + 0.1 * rng.standard_normal(N), omega4=0.1 * rng.random(N),
               lam=1 + 0.1 * rng.standard_normal(N), mu=0.1 * rng.standard_normal(N), bonds=bonds)
    allp = np.array([[i, j] for i in range(1, ns + 1) for j in range(1, ns + 1)]).T
    request = {"Greens": (L + 1, allp), "DenDen": (1, allp), "SpinSpin": (L + 1, allp), "PairGreens": (L + 1, allp[:, -1:]),
               "PhononGreens": (L + 1, allp)}
    a = ref.measure(R, X, x, par, request)
    b = ref.measure(R, X, x, par, request, tables=fft_tables, phonon=fft_phonon)
    for name in request:
        assert a["corr"][name].shape == (request[name][0],) + tuple(dims) + (request[name][1].shape[1],)
        assert np.abs(a["corr"][name] - b["corr"][name]).max() < 1e-12 * max(1.0, np.abs(b["corr"][name]).max()), name
    assert abs(a["glob"]["Nsqr"] - b["glob"]["Nsqr"]) < 1e-12 * a["abs"]["glob"]["Nsqr"]
    # independent spot checks of the scalars: literal loops of the reference's text over (orbit, site, tau) for one pair
    r1, x1, r2, x2 = R[0], X[0], R[1], X[1]
    one = ref.measure(R[:2], X[:2], x, par, {})
    dens, docc, ke = np.zeros(ns), np.zeros(ns), np.zeros(ns)
    for o in range(ns):
        for site in range(o, N, ns):
            for tau in range(L):
                i = site * L + tau
                G1, G2 = x1[i] * r1[i], x2[i] * r2[i]
                dens[o] += ((1 - G1) + (1 - G2)) / (nc * L)
                docc[o] += (1 - G1) * (1 - G2) / (nc * L)
                dxx = x[site * L + (tau + 1) % L] - x[i]
                ke[o] += (0.5 / 0.1 - dxx ** 2 / 0.01 / 2) / (nc * L)
    assert np.abs(one["onsite"]["density"] - dens).max() < 1e-12 and np.abs(one["onsite"]["double_occ"] - docc).max() < 1e-12
    assert np.abs(one["onsite"]["phonon_ke"] - ke).max() < 1e-12 * np.abs(ke).max() * 10
    el = 0.0
    s1, s2, t = bonds[1]
    for bnd in range(nc):
        for tau in range(L):
            i, j = (s1[bnd] - 1) * L + tau, (s2[bnd] - 1) * L + tau
            h = -(x1[i] * r1[j] + x1[j] * r1[i] + x2[i] * r2[j] + x2[j] * r2[i])
            el += -t[bnd] * h / (nc * L)
    assert abs(one["el_ke"][1] - el) < 1e-12 * one["abs"]["el_ke"][1]
    assert abs(one["glob"]["density"] - (2 * (N - x1 @ r1 / L) + 2 * (N - x2 @ r2 / L)) / (2 * N)) < 1e-13
