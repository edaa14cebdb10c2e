"""GPU parity of the measurements of resident chains (csrc/measure.hip through elphdynamics_amd/chain_measurements.py): every
chain's container against the direct-sum restatement tests/measurements_reference.py evaluated on that chain's field, mu row and vectors
[v * nchains + c], with the bounds of tests/test_gpu_measurements.py (its `compare`: 1e-12 on the correlations, 1e-12 of the yardstick on
the reduced scalars).

Vectors go in through greens.set_vectors_ (no solve) unless a test says otherwise.  Three chains with three vectors each: three pairs,
neither count a power of two, so a chain-major / vector-major mix-up cannot pass.  Against the device's single-configuration path
(measurements.accumulate_) the bound is 2e-12 * max(1, |single|): each side meets 1e-12 of the direct sum in the existing suite."""
import copy
import os

import numpy as np
import pytest

import measurements_reference as ref
from test_gpu_measurements import ALL_TD, SHAPES, assert_same_bits_as_single, build_model, compare, parse, ref_par, request_of, snapshot

pytestmark = pytest.mark.gpu

DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decks")


def chain_inputs(m, nch, nv, seed):
    """(X (nch, Ndof) a rough field per chain, mu (nch, Nsites) a distinct row per chain, R, MinvR (nv * nch, Ndim))."""
    from elphdynamics_amd import synth
    rng = np.random.default_rng(seed)
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=seed + 1 + c) for c in range(nch)])
    mu = np.stack([m.mu + 0.05 * (c + 1) + 0.1 * rng.standard_normal(m.Nsites) for c in range(nch)])
    return X, mu, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim))


def lockstep(case, nch, nv, seed, table=None):
    """A model of SHAPES[case] with nch chains resident, its estimator and chain container, and the inputs."""
    from elphdynamics_amd import chain_measurements as cms, greens, models
    ns, dims, L, defs, tab = SHAPES[case]
    m = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    X, mu, R, MinvR = chain_inputs(m, nch, nv, seed)
    models.update_model_chains_(m, X)
    cm = cms.initialize_chain_measurements_container(m, dict(table or tab, num_random_vectors=nv), [""] * nch)
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    greens.set_vectors_(est, R, MinvR)
    return m, defs, cm, est, X, mu


def want_of(m, defs, cm, est, X, mu, c):
    """The direct sums of chain c: its field, its mu row, its vectors."""
    nch = cm.nchains
    return ref.measure(est.R[c::nch], est.MinvR[c::nch], X[c], dict(ref_par(m, defs), mu=mu[c]), request_of(cm.chains[c]))


def add(a, b):
    """The reference sums of two accumulations."""
    out = copy.deepcopy(a)
    for grp in ("glob", "onsite", "corr"):
        for k in out[grp]:
            out[grp][k] = a[grp][k] + b[grp][k]
    out["el_ke"] = a["el_ke"] + b["el_ke"]
    for grp in ("glob", "onsite"):
        for k in out["abs"][grp]:
            out["abs"][grp][k] = a["abs"][grp][k] + b["abs"][grp][k]
    out["abs"]["el_ke"] = a["abs"]["el_ke"] + b["abs"]["el_ke"]
    return out


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", ["sq4x4", "hc3x2", "cubic3x2x2"])
def test_every_chain_matches_the_direct_sums_of_its_own_inputs(case):
    from elphdynamics_amd import chain_measurements as cms
    m, defs, cm, est, X, mu = lockstep(case, 3, 3, seed=41)
    try:
        cms.accumulate_(cm, m, est, X, mu=mu)
        cms.fetch_(cm, m)
        for c in range(3):
            compare(cm.chains[c], want_of(m, defs, cm, est, X, mu, c), label="%s chain %d" % (case, c))
    finally:
        m.close()


def test_two_accumulates_add_up_fetch_does_not_clear_reset_zeroes():
    from elphdynamics_amd import chain_measurements as cms, greens
    m, defs, cm, est, X, mu = lockstep("hc3x2", 3, 3, seed=5)
    try:
        cms.accumulate_(cm, m, est, X, mu=mu)
        first = [want_of(m, defs, cm, est, X, mu, c) for c in range(3)]
        X2, mu2, R2, MinvR2 = chain_inputs(m, 3, 3, seed=77)
        greens.set_vectors_(est, R2, MinvR2)
        cms.accumulate_(cm, m, est, X2, mu=mu2)                             # the tuners moved mu in between: the second sums take the new rows
        cms.fetch_(cm, m)
        for c in range(3):
            compare(cm.chains[c], add(first[c], want_of(m, defs, cm, est, X2, mu2, c)), label="two accumulates, chain %d" % c)
        two = [snapshot(c) for c in cm.chains]
        cms.accumulate_(cm, m, est, X2)                                     # no mu given: the device keeps the rows it has
        cms.fetch_(cm, m)
        for c in range(3):
            assert abs(snapshot(cm.chains[c])["g:mu"][0] - two[c]["g:mu"][0] - 3 * mu2[c].mean()) < 1e-12
        once = [snapshot(c) for c in cm.chains]
        cms.fetch_(cm, m)                                                   # fetch does not clear
        assert all(same_bits(a, snapshot(c)) for a, c in zip(once, cm.chains))
        cms.reset_measurements_(cm, m)
        cms.fetch_(cm, m)
        for c in cm.chains:
            assert all(not v.any() for v in snapshot(c).values())           # exact zeros
    finally:
        m.close()


def test_chains_do_not_leak_into_one_another_and_runs_repeat_bit_for_bit():
    from elphdynamics_amd import chain_measurements as cms, greens
    m, defs, cm, est, X, mu = lockstep("hc3x2", 3, 3, seed=8)
    try:
        cms.accumulate_(cm, m, est, X, mu=mu)
        cms.fetch_(cm, m)
        one = [snapshot(c) for c in cm.chains]
        # the same inputs again: the same bits
        cms.reset_measurements_(cm, m)
        cms.accumulate_(cm, m, est, X)
        cms.fetch_(cm, m)
        assert all(same_bits(a, snapshot(c)) for a, c in zip(one, cm.chains))
        # only chain 1's field and vectors change
        X2, _, R2, MinvR2 = chain_inputs(m, 3, 3, seed=99)
        Xn, Rn, Mn = X.copy(), est.R.copy(), est.MinvR.copy()
        Xn[1], Rn[1::3], Mn[1::3] = X2[1], R2[1::3], MinvR2[1::3]
        greens.set_vectors_(est, Rn, Mn)
        cms.reset_measurements_(cm, m)
        cms.accumulate_(cm, m, est, Xn)
        cms.fetch_(cm, m)
        two = [snapshot(c) for c in cm.chains]
        assert same_bits(one[0], two[0]) and same_bits(one[2], two[2])
        moved = [k for k in one[1] if not np.array_equal(one[1][k], two[1][k])]
        assert set(moved) >= {"g:density", "g:Nsqr", "o:x", "o:elph_energy", "el_ke", "c:Greens", "c:PhononGreens"}, moved
        compare(cm.chains[1], want_of(m, defs, cm, est, Xn, mu, 1), label="chain 1 after its inputs changed")
    finally:
        m.close()


def assert_close_to_single(chain, single, label):
    """|chain path - single-configuration path| <= 2e-12 * max(1, |single|): the scalars one by one, a correlation in its max norm."""
    a, b = snapshot(chain), snapshot(single)
    worst = {}
    for k in b:
        if k.startswith("c:"):
            assert not a[k].imag.any()
            worst[k] = np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max())
        else:
            worst[k] = (np.abs(a[k] - b[k]) / np.maximum(1.0, np.abs(b[k]))).max() if b[k].size else 0.0
    print(label, {k: "%.2e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 2e-12, (label, k, v)


def single_configuration(m2, X, mu, R, MinvR, table, nv):
    """measurements.accumulate_ of one configuration on the handle of m2: the fetched container."""
    from elphdynamics_amd import greens, measurements as ms
    m2.x[:] = X
    m2.mu[:] = mu
    c = ms.initialize_measurements_container(m2, dict(table, num_random_vectors=nv), "")
    est = greens.EstimateGreensFunction(m2, nv=nv)                          # (a new estimator drops the handle's previous container)
    greens.set_vectors_(est, R, MinvR)
    ms.accumulate_(c, m2, est)
    ms.fetch_(c, m2)
    return c


def test_production_shape_against_the_single_configuration_path():
    """16 x 16, L = 160, all five correlations time-dependent: the tau-DFTs take their matrix-core forms and the batch (2 chains) changes
    the kernel chosen.  The reference is the device's single-configuration path on a second handle, same fields and vectors."""
    from elphdynamics_amd import chain_measurements as cms
    m, defs, cm, est, X, mu = lockstep("sq16x16", 2, 2, seed=16)
    ns, dims, L, _, table = SHAPES["sq16x16"]
    m2 = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    try:
        cms.accumulate_(cm, m, est, X, mu=mu)
        cms.fetch_(cm, m)
        for c in range(2):
            single = single_configuration(m2, X[c], mu[c], est.R[c::2], est.MinvR[c::2], table, 2)
            assert_close_to_single(cm.chains[c], single, "16 x 16 x 160, chain %d" % c)
    finally:
        m.close()
        m2.close()


def test_one_chain_resident_agrees_with_the_single_configuration_path():
    from elphdynamics_amd import chain_measurements as cms, greens, measurements as ms
    ns, dims, L, defs, table = SHAPES["sq4x4"]
    m = build_model(ns, dims, L, defs, seed=3)
    try:
        info = dict(table, num_random_vectors=3)
        cm = cms.initialize_chain_measurements_container(m, info, [""])
        c1 = ms.initialize_measurements_container(m, info, "")
        est = greens.EstimateGreensFunction(m, nv=3)
        rng = np.random.default_rng(1)
        greens.set_vectors_(est, rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim)))
        cms.accumulate_(cm, m, est, m.x[None, :])
        ms.accumulate_(c1, m, est)                                          # both containers live on the handle side by side
        cms.fetch_(cm, m)
        ms.fetch_(c1, m)
        assert_same_bits_as_single(snapshot(cm.chains[0]), snapshot(c1), "one chain resident")
        compare(cm.chains[0], ref.measure(est.R, est.MinvR, m.x, ref_par(m, defs), request_of(c1)), label="one chain resident")
    finally:
        m.close()


def test_deck_in_lockstep_measured_end_to_end(tmp_path):
    """process_input_file(deck, nchains = 3) with a [measurements] table, one update of all chains, then make_measurements_ with the device's
    own preconditioned solve on the chains' fields; the written files against the reference at 5e-9 absolute (half a unit of the 8
    decimals written)."""
    from elphdynamics_amd import chain_measurements as cms, hmc, lattice as lat, process_input as pi
    nch = 3
    deck = pi.read_deck(os.path.join(DECKS, "holstein_hmc_honeycomb_L3.toml"))
    info = dict(ALL_TD, num_random_vectors=3)
    info["DenDen"] = {"measure": True, "time_dependent": True, "pairs": [[1, 1], [2, 1]]}
    deck["measurements"] = info
    sim = pi.process_input_file(deck, nchains=nch)
    H, m = sim.simulation_dynamics, sim.model
    try:
        H.device_rng_(31)
        hmc.update_chains_(m, H, sim.fa, sim.preconditioner, pull=True)
        assert not H.flags.any()
        folders = [str(tmp_path / ("run%d" % c)) for c in range(nch)]
        for f in folders:
            os.mkdir(f)
        cm = cms.initialize_chain_measurements_container(m, sim.input["measurements"], folders)
        cms.initialize_measurement_folders_(cm)
        assert sim.Gr.nv == cm.n_rand_vecs * nch
        it, res, fl = cms.make_measurements_(cm, m, sim.Gr, H.X, 1, P=sim.preconditioner, rng=np.random.default_rng(2))
        assert not fl.any() and it.min() > 0                                # the solve raised no flags
        mu = np.tile(m.mu, (nch, 1))
        wants = [want_of(m, lat.HONEYCOMB_BONDS, cm, sim.Gr, H.X, mu, c) for c in range(nch)]
        cms.fetch_(cm, m)
        for c in range(nch):
            compare(cm.chains[c], wants[c], label="deck, chain %d" % c)
        bin_size = 1
        cms.process_measurements_(cm, bin_size, m)
        cms.write_measurements_(cm, m, 3)
        V = bin_size * 3                                                    # binomial(3, 2), the vectors of ONE chain
        susc_of = {"PairGreens": "PairSusc", "DenDen": "ChargeSusc", "SpinSpin": "SpinSusc"}
        for c, (d, want) in enumerate(zip(folders, wants)):
            rows = dict(ln.split() for ln in open(os.path.join(d, "global_measurements_f", "global_measurements_00003.out")).read().splitlines())
            for k in ref.GLOBAL_KEYS:
                assert abs(float(rows[k]) - want["glob"][k] / V) <= 5e-9 + 1e-12 * want["abs"]["glob"][k], (c, k)
            for ln in open(os.path.join(d, "onsite_measurements_f", "onsite_measurements_00003.out")).read().splitlines()[1:]:
                k, o, v = ln.split()
                assert abs(float(v) - want["onsite"][k][int(o) - 1] / V) <= 5e-9, (c, k, o)
            for ln in open(os.path.join(d, "intersite_measurements_f", "intersite_measurements_00003.out")).read().splitlines()[1:]:
                k, b, v = ln.split()
                assert k == "el_ke" and abs(float(v) - want["el_ke"][int(b) - 1] / V) <= 5e-9, (c, b)
            for k, w in want["corr"].items():
                pos = w / V
                for space, arr in (("position", pos), ("momentum", ref.momentum(pos))):
                    got = parse(os.path.join(d, "%s_%s_f" % (k, space), "%s_%s_00003.out" % (k, space))).reshape(arr.shape, order="F")
                    assert np.abs(got.real - arr.real).max() <= 5e-9 and np.abs(got.imag - arr.imag).max() <= 5e-9, (c, k, space)
                    if k in susc_of:
                        s = ref.simpson(arr, m.dtau)
                        name = "%s_%s" % (susc_of[k], space)
                        got = parse(os.path.join(d, name + "_f", name + "_00003.out")).reshape(s.shape, order="F")
                        assert np.abs(got.real - s.real).max() <= 5e-9 and np.abs(got.imag - s.imag).max() <= 5e-9, (c, name)
            assert set(cm.chains[c].onsite_susc) == set(susc_of.values())
    finally:
        m.close()


def raw_create(m, nchains):
    """elph_meas_chains_create with Greens alone requested for one orbital pair, straight through the C ABI."""
    import ctypes as C
    from elphdynamics_amd._lib import dptr
    z = np.zeros(m.Nsites)
    zz = np.zeros(max(nchains, 1) * m.Nsites)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    meas, td, npairs, pr = i32([1, 0, 0, 0, 0]), i32([1, 0, 0, 0, 0]), i32([1, 0, 0, 0, 0]), i32([1, 1])
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    return m._lib.elph_meas_chains_create(m._h, nchains, dptr(z), dptr(z), dptr(z), dptr(zz), 0.1, 0, 0, None, None, ip(meas), ip(td), ip(npairs),
                                          ip(pr))


def test_refusals_from_the_library():
    from elphdynamics_amd import _lib, chain_measurements as cms, configs, greens, models
    m, defs, cm, est, X, mu = lockstep("hc3x2", 3, 3, seed=2)
    try:
        lib = m._lib
        last = lambda: lib.elph_last_error().decode()  # noqa: E731
        # a chain count that is not the resident one
        for n in (0, 2, 4):
            assert raw_create(m, n) == _lib.ELPH_E_ARG and "3 are resident" in last(), last()
        assert lib.elph_meas_chains_accumulate(m._h, _lib.dptr(X)) == _lib.ELPH_E_STATE and "elph_meas_chains_create" in last()
        assert lib.elph_meas_chains_set_mu(m._h, _lib.dptr(mu)) == _lib.ELPH_E_STATE and "elph_meas_chains_create" in last()
        # fetch of chain nchains (and of chain -1)
        cms.accumulate_(cm, m, est, X, mu=mu)
        scal = np.zeros(3 + 9 * 2 + 3)
        for chain in (3, -1):
            assert lib.elph_meas_chains_fetch(m._h, chain, _lib.dptr(scal), None, None, None, None, None) == _lib.ELPH_E_ARG
            assert "outside 0..2" in last(), last()
        assert lib.elph_meas_chains_fetch(m._h, 2, _lib.dptr(scal), None, None, None, None, None) == _lib.ELPH_OK and scal[0] != 0
        # an estimator whose vectors are not a multiple of the chains: 4 vectors, 3 chains (a new estimator drops the container)
        est4 = greens.EstimateGreensFunction(m, nv=4)
        assert raw_create(m, 3) == _lib.ELPH_OK
        assert lib.elph_meas_chains_accumulate(m._h, _lib.dptr(X)) == _lib.ELPH_E_STATE
        assert "4 vectors" in last() and "3 resident chains" in last(), last()
        # accumulate before any vectors
        est6 = greens.EstimateGreensFunction(m, nv=6)
        assert raw_create(m, 3) == _lib.ELPH_OK
        assert lib.elph_meas_chains_accumulate(m._h, _lib.dptr(X)) == _lib.ELPH_E_STATE and "no vectors" in last(), last()
        greens.set_vectors_(est6, np.ones((6, m.Ndim)), np.ones((6, m.Ndim)))
        assert lib.elph_meas_chains_accumulate(m._h, _lib.dptr(X)) == _lib.ELPH_OK
        # update_model_ drops the chains: the container was made for three
        models.update_model_(m)
        assert lib.elph_meas_chains_accumulate(m._h, _lib.dptr(X)) == _lib.ELPH_E_STATE
        assert "3 chains" in last() and "1 are resident" in last(), last()
        assert lib.elph_meas_chains_reset(m._h) == _lib.ELPH_OK             # ... and is still there
        # a new estimator drops the device side; the container notices and makes it again for the new one
        models.update_model_chains_(m, X)
        est9 = greens.EstimateGreensFunction(m, nv=9)
        greens.set_vectors_(est9, est.R, est.MinvR)
        cms.accumulate_(cm, m, est9, X)
        cms.fetch_(cm, m)
        for c in range(3):
            compare(cm.chains[c], want_of(m, defs, cm, est9, X, np.tile(m.mu, (3, 1)), c), label="after a new estimator, chain %d" % c)
        del est4
    finally:
        m.close()
    s = configs.make_model("e")
    try:
        greens.EstimateGreensFunction(s, nv=2)
        assert raw_create(s, 1) == _lib.ELPH_E_UNSUPPORTED and "SSH" in s._lib.elph_last_error().decode()
        with pytest.raises(cms.UnsupportedMeasurement, match="SSH"):
            cms.initialize_chain_measurements_container(s, ALL_TD, [""])
    finally:
        s.close()
