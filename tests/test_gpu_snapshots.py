"""GPU tests of the snapshot measurements (csrc/snapshots.hip through elphdynamics_amd/snapshots.py).

elph_snapshots returns, per resident chain, the density and double-occupancy profiles take_density_snapshot! and
take_double_occupancy_snapshot! write (Measurements.jl:1351-1435).  The reference value is tests/snapshot_reference.py, the reference's
loops over the vectors written out with its own ranges.  Bound: 1e-12 of the largest element of the reference's profile, the bound of the
measurement units.

Vectors go in through greens.set_vectors_ (no solve) except in the end-to-end case.  The shapes are those at which the kernels can go
wrong (snapshots.hip: 64 sites per workgroup, 4 slices per segment of the tau axis): hc3x2 has N = 12, less than one wavefront, and
L = 7, a full segment and a ragged one; sq20x13 has N = 260, four full site blocks and a ragged fifth, and L = 5; sq4x4L40 has ten
full segments.  n_v = 2: the first and the last vector are the only two; n_v = 3: the n = m term of the reference's ranges appears."""
import os

import numpy as np
import pytest

import snapshot_reference as sref
from test_gpu_chain_measurements import chain_inputs
from test_gpu_measurements import HONEYCOMB, SQUARE, build_model, snapshot

pytestmark = pytest.mark.gpu

TOL = 1e-12
DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decks")
# (norbits, (L1, L2, L3), L, bond definitions)
SHAPES = {"hc3x2": (2, (3, 2, 1), 7, HONEYCOMB), "sq20x13": (1, (20, 13, 1), 5, SQUARE), "sq4x4L40": (1, (4, 4, 1), 40, SQUARE)}
ALL = {"Snapshots": {"density": True, "double_occupancy": True, "phonon_position": True}}


def resident(case, nch, nv, seed):
    """A model of SHAPES[case] with nch chains resident (one: the model's own configuration), an estimator holding nv vectors per chain,
    vector v of chain c at row v nch + c, and the chains' fields (nch, Ndof)."""
    from elphdynamics_amd import greens, models
    ns, dims, L, defs = SHAPES[case]
    m = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    X, _, R, MinvR = chain_inputs(m, nch, nv, seed)
    if nch > 1:
        models.update_model_chains_(m, X)
    else:
        X = m.x[None].copy()
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    greens.set_vectors_(est, R, MinvR)
    return m, est, X


def raw(m, nch, density=True, double_occ=True):
    """elph_snapshots straight through the C ABI: (return code, density, double occupancy), an array not asked for is None."""
    from elphdynamics_amd import _lib
    a = np.full((nch, m.Nsites), np.nan) if density else None
    b = np.full((nch, m.Nsites), np.nan) if double_occ else None
    rc = m._lib.elph_snapshots(m._h, nch, _lib.dptr(a) if density else None, _lib.dptr(b) if double_occ else None)
    return rc, a, b


def check_against_reference(m, est, X, nch, got, label):
    """Every requested profile of every chain against the restatement, 1e-12 of its largest element."""
    worst = {}
    for c in range(nch):
        want = sref.snapshots(est.R[c::nch], est.MinvR[c::nch], X[c], m.Nsites, m.Nph, m.Ltau)
        for name, a in got.items():
            assert a.shape == (nch, want[name].size), (label, name, a.shape)
            worst[name] = max(worst.get(name, 0.0), np.abs(a[c] - want[name]).max() / np.abs(want[name]).max())
    print(label, "worst deviation in units of the largest element:", {k: "%.2e" % v for k, v in worst.items()}, "(bound %.1e)" % TOL)
    assert all(v <= TOL for v in worst.values()), (label, worst)


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("nv", [2, 3, 7])
@pytest.mark.parametrize("case", list(SHAPES))
def test_profiles_match_the_references_loops_over_each_chains_own_vectors(case, nv, nch):
    from elphdynamics_amd import snapshots as sn
    m, est, X = resident(case, nch, nv, seed=29)
    try:
        sc = sn.initialize_snapshots_container(m, ALL, [""] * nch)
        got = sn.snapshot_arrays_(sc, m, est, X if nch > 1 else None)
        assert list(got) == list(sref.NAMES)
        check_against_reference(m, est, X, nch, got, "%s, %d chains, n_v = %d:" % (case, nch, nv))
        for name in got:                                                    # the chains' profiles differ: a mix-up of rows cannot pass
            assert all(not np.array_equal(got[name][a], got[name][b]) for a in range(nch) for b in range(a))
    finally:
        m.close()


@pytest.mark.parametrize("nv", [3, 7])
def test_the_density_profile_sums_to_the_density_moments_N(nv):
    """Independent of the restatement: sum_i density[i] = (2 / n_v) sum_n (N - T_n) with T_n = (1/L) sum_{tau, i} MinvR R, and <N> of
    elph_density_moments averages N_p = 2 (N - T_p) over the pairs, in which every vector appears n_v - 1 times: the same number."""
    from elphdynamics_amd import mu_tuner as mt
    nch = 3
    m, est, X = resident("hc3x2", nch, nv, seed=31)
    try:
        rc, dens, _ = raw(m, nch, double_occ=False)
        assert rc == 0
        N, _ = mt.density_moments(m, est, nch)
        for c in range(nch):
            total = dens[c].sum()
            print("n_v = %d, chain %d: sum of the density profile %.15g, N %.15g, relative difference %.2e" % (nv, c, total, N[c], abs(total - N[c]) / abs(N[c])))
            assert abs(total - N[c]) <= TOL * abs(N[c]), (c, total, N[c])
    finally:
        m.close()


def test_an_ssh_handle_is_served_alike():
    """The 4 x 4, L = 8 bond-phonon deck of the SSH tests, two chains: Nph = 32 phonons on 16 sites."""
    from elphdynamics_amd import greens, models, process_input as pi, snapshots as sn
    from test_gpu_ssh_chain_measurements import chain_inputs as ssh_chain_inputs
    nch, nv = 2, 3
    sim = pi.process_input_file(pi.read_deck(os.path.join(DECKS, "ssh_langevin_square_L4.toml")), nchains=nch)
    m = sim.model
    try:
        assert m.kind != 0 and (m.Nsites, m.Ltau, m.Nph) == (16, 8, 32)
        X, _, R, MinvR = ssh_chain_inputs(m, nch, nv, seed=41)
        models.update_model_chains_(m, X)
        est = greens.EstimateGreensFunction(m, nv=nv * nch)
        greens.set_vectors_(est, R, MinvR)
        sc = sn.initialize_snapshots_container(m, ALL, ["", ""])
        got = sn.snapshot_arrays_(sc, m, est, X)
        assert got["phonon_position"].shape == (nch, m.Nph) and got["density"].shape == got["double_occupancy"].shape == (nch, m.Nsites)
        check_against_reference(m, est, X, nch, got, "SSH deck, 2 chains:")
    finally:
        m.close()


def test_repeats_bit_for_bit_chains_do_not_leak_and_a_chain_equals_a_single_configuration():
    from elphdynamics_amd import greens
    nch, nv = 3, 7
    m, est, X = resident("sq4x4L40", nch, nv, seed=9)
    try:
        rc1, d1, o1 = raw(m, nch)
        rc2, d2, o2 = raw(m, nch)
        assert rc1 == rc2 == 0 and np.array_equal(d1, d2) and np.array_equal(o1, o2)
        # one output alone: the same bits, and the array not asked for is not needed
        rc, d, none = raw(m, nch, double_occ=False)
        assert rc == 0 and none is None and np.array_equal(d, d1)
        rc, none, o = raw(m, nch, density=False)
        assert rc == 0 and none is None and np.array_equal(o, o1)
        R0, M0 = est.R.copy(), est.MinvR.copy()
        # chain 1's rows alone change
        _, _, R2, M2 = chain_inputs(m, nch, nv, seed=90)
        Rn, Mn = R0.copy(), M0.copy()
        Rn[1::nch], Mn[1::nch] = R2[1::nch], M2[1::nch]
        greens.set_vectors_(est, Rn, Mn)
        rc, dn, on = raw(m, nch)
        assert rc == 0
        for a, b in ((d1, dn), (o1, on)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and not np.array_equal(a[1], b[1])
        check_against_reference(m, est, X, nch, {"density": dn, "double_occupancy": on}, "after chain 1's rows changed:")
    finally:
        m.close()
    # every chain against a single-configuration handle that holds the chain's vectors: the segments of the tau axis depend on L alone
    ns, dims, L, defs = SHAPES["sq4x4L40"]
    s = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    try:
        one = greens.EstimateGreensFunction(s, nv=nv)
        for c in range(nch):
            greens.set_vectors_(one, R0[c::nch], M0[c::nch])
            rc, d, o = raw(s, 1)
            assert rc == 0 and np.array_equal(d[0], d1[c]) and np.array_equal(o[0], o1[c]), c
    finally:
        s.close()


def test_refusals_leave_the_handle_usable():
    import ctypes as C
    from elphdynamics_amd import _lib, configs, greens, models
    ns, dims, L, defs = SHAPES["hc3x2"]
    m = build_model(ns, dims, L, defs, seed=3)
    try:
        lib = m._lib
        last = lambda: lib.elph_last_error().decode()  # noqa: E731

        def valid(nch, est, X):
            rc, d, o = raw(m, nch)
            assert rc == _lib.ELPH_OK, last()
            check_against_reference(m, est, X, nch, {"density": d, "double_occupancy": o}, "after a refusal, %d chain(s):" % nch)

        assert raw(m, 1)[0] == _lib.ELPH_E_STATE and "elph_greens_create has not been called" in last(), last()       # no estimator
        est = greens.EstimateGreensFunction(m, nv=3)
        assert raw(m, 1)[0] == _lib.ELPH_E_STATE and "no vectors" in last() and "3 vectors" in last(), last()         # an estimator without vectors
        rng = np.random.default_rng(1)
        greens.set_vectors_(est, rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim)))
        X1 = m.x[None].copy()
        valid(1, est, X1)
        for n in (0, 2, 3):                                                 # one configuration is resident
            rc = lib.elph_snapshots(m._h, n, _lib.dptr(np.zeros(3 * m.Nsites)), None)
            assert rc == _lib.ELPH_E_ARG and "%d chains" % n in last() and "1 are resident" in last(), last()
            valid(1, est, X1)
        assert raw(m, 1, density=False, double_occ=False)[0] == _lib.ELPH_E_ARG and "null" in last() and "2" in last(), last()
        valid(1, est, X1)
        # three chains resident, four vectors
        X, _, R, MinvR = chain_inputs(m, 3, 3, seed=5)
        models.update_model_chains_(m, X)
        rc = lib.elph_snapshots(m._h, 1, _lib.dptr(np.zeros(m.Nsites)), None)
        assert rc == _lib.ELPH_E_ARG and "1 chains" in last() and "3 are resident" in last(), last()
        def nine():                                                         # a new estimator drops the scratch; the next call makes it again
            est9 = greens.EstimateGreensFunction(m, nv=9)
            assert raw(m, 3)[0] == _lib.ELPH_E_STATE and "no vectors" in last() and "9 vectors" in last(), last()
            greens.set_vectors_(est9, R, MinvR)
            valid(3, est9, X)
            return est9

        est4 = greens.EstimateGreensFunction(m, nv=4)
        greens.set_vectors_(est4, R[:4], MinvR[:4])
        assert raw(m, 3)[0] == _lib.ELPH_E_STATE and "4 vectors" in last() and "3 resident chains" in last(), last()
        nine()
        est3 = greens.EstimateGreensFunction(m, nv=3)                       # a vector per chain: binomial(1, 2) = 0
        greens.set_vectors_(est3, R[:3], MinvR[:3])
        assert raw(m, 3)[0] == _lib.ELPH_E_STATE and "1 vector per chain" in last(), last()
        est9 = nine()
        # a sharded handle (one rank owning the whole lattice), made as test_gpu_ssh_chain_measurements.py makes one; it stays sharded, so
        # the valid call after this refusal is the first handle's
        s = configs.make_model("e")
        try:
            ests = greens.EstimateGreensFunction(s, nv=2)
            greens.set_vectors_(ests, rng.standard_normal((2, s.Ndim)), rng.standard_normal((2, s.Ndim)))
            assert raw(s, 1)[0] == _lib.ELPH_OK
            key = (C.c_ubyte * 64)()
            assert s._lib.elph_shard_create(s._h, 0, 1, 0, s.Nsites, 0, 0, 0, 0, 0, None, C.cast(key, C.c_void_p)) == _lib.ELPH_OK
            assert raw(s, 1)[0] == _lib.ELPH_E_UNSUPPORTED and "sharded" in s._lib.elph_last_error().decode()
        finally:
            s.close()
        valid(3, est9, X)
        del est4, est3
    finally:
        m.close()


def parse(path, name):
    lines = open(path).read().splitlines()
    assert lines[0] == name
    return np.array([float(v) for v in lines[1:]])


def test_a_deck_in_lockstep_end_to_end(tmp_path):
    """The Holstein deck with two chains in lockstep: update_chains_, greens.update_, the chain container's accumulate_, then
    take_snapshots_ with nmeas = 3.  The files parse back to the arrays within 5e-9 (the rounding of %.8f), and the chain container's sums
    are the bits of a measurement without the snapshot call."""
    from elphdynamics_amd import chain_measurements as cms, greens, hmc, process_input as pi, snapshots as sn
    nch = 2
    deck = pi.read_deck(os.path.join(DECKS, "holstein_hmc_honeycomb_L3.toml"))
    deck["measurements"] = dict(deck["measurements"], Greens={"measure": True, "time_dependent": True}, **ALL)
    sim = pi.process_input_file(deck, nchains=nch)
    H, m = sim.simulation_dynamics, sim.model
    try:
        H.device_rng_(31)
        hmc.update_chains_(m, H, sim.fa, sim.preconditioner, pull=True)
        assert not H.flags.any()
        _, _, fl = greens.update_(sim.Gr, m, sim.preconditioner, rng=np.random.default_rng(2))
        assert not fl.any()
        folders = [str(tmp_path / ("run%d" % c)) for c in range(nch)]
        for f in folders:
            os.mkdir(f)
        rest, _ = sn.split_info(sim.input["measurements"])
        cm = cms.initialize_chain_measurements_container(m, rest, folders)
        sc = sn.initialize_snapshots_container(m, sim.input["measurements"], folders)
        cms.initialize_measurement_folders_(cm)
        sn.initialize_snapshot_folders_(sc)
        # a measurement without the snapshot call
        cms.accumulate_(cm, m, sim.Gr, H.X)
        cms.fetch_(cm, m)
        without = [snapshot(c) for c in cm.chains]
        cms.reset_measurements_(cm, m)
        # the same with it, between the accumulation and the fetch
        cms.accumulate_(cm, m, sim.Gr, H.X)
        wrote = sn.take_snapshots_(sc, m, sim.Gr, 3, X=H.X)
        cms.fetch_(cm, m)
        for c in range(nch):
            got = snapshot(cm.chains[c])
            assert set(got) == set(without[c]) and all(np.array_equal(got[k], without[c][k]) for k in got), c
            assert any(np.any(v != 0) for v in got.values())
        arrays = sn.snapshot_arrays_(sc, m, sim.Gr, H.X)
        assert list(arrays) == list(sref.NAMES) and all(np.array_equal(arrays[k], wrote[k]) for k in arrays)
        check_against_reference(m, sim.Gr, H.X, nch, arrays, "deck, 2 chains:")
        for c, f in enumerate(folders):
            for name in sref.NAMES:
                assert os.listdir(os.path.join(f, name + "_snapshots_f")) == ["%s_snapshot_000003.out" % name]
                back = parse(os.path.join(f, name + "_snapshots_f", "%s_snapshot_000003.out" % name), name)
                assert back.shape == arrays[name][c].shape and np.abs(back - arrays[name][c]).max() <= 5e-9, (c, name)
    finally:
        m.close()
