"""GPU parity of the bond correlations of resident chains (csrc/bondcorr.hip through elphdynamics_amd/chain_bond_measurements.py):
every chain's container against the direct-sum restatement tests/bond_reference.py evaluated on that chain's vectors [v * nchains + c],
with the bound of tests/test_gpu_bond_measurements.py (its `compare`: max|got - ref| < 1e-12 * max(1, max|ref|)).

Vectors go in through greens.set_vectors_ (no solve) unless a test says otherwise.  Three chains with three vectors each: three pairs,
neither count a power of two, so a chain-major / vector-major mix-up cannot pass.  Against the device's single-configuration path
(bond_measurements.accumulate_bonds_) the bound is 2e-12 * max(1, max|single|): each side is held to 1e-12 of the direct sums."""
import os

import numpy as np
import pytest

import bond_reference as bref
import measurements_reference as mref
from test_bond_measurements_host import SMALL, SQUARE, TD
from test_gpu_bond_measurements import compare, request_of, snapshot
from test_gpu_measurements import assert_same_bits_as_single, build_model, mulM_still_right, parse

pytestmark = pytest.mark.gpu

DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decks")
NCH = NV = 3


def vectors(m, nch, nv, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim))


def fields(m, nch, seed):
    from elphdynamics_amd import synth
    return np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=seed + 1 + c) for c in range(nch)])


def lockstep(case, seed, table=None, nch=NCH, nv=NV, shape=None):
    """A model of SMALL[case] with nch chains resident, its estimator with nv vectors per chain set, and the chain bond container."""
    from elphdynamics_amd import chain_bond_measurements as cbm, greens, models
    ns, dims, L, defs, tab = shape or SMALL[case]
    m = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    models.update_model_chains_(m, fields(m, nch, seed))
    cb = cbm.initialize_chain_bond_container(m, dict(table or tab, num_random_vectors=nv), [""] * nch)
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    greens.set_vectors_(est, *vectors(m, nch, nv, seed))
    return m, cb, est


def want_of(m, cb, R, MinvR, c):
    """The direct sums of chain c: its vectors."""
    la = m.lattice
    one = cb.chains[c]
    return bref.measure(R[c::cb.nchains], MinvR[c::cb.nchains], m.Ltau, la.norbits, (la.L1, la.L2, la.L3), one.bond_definitions, request_of(one))


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", ["hc3x2", "hc3x2_both_ways", "cubic3x2x2", "chain12"])
def test_every_chain_matches_the_direct_sums_of_its_own_vectors(case):
    from elphdynamics_amd import chain_bond_measurements as cbm
    m, cb, est = lockstep(case, seed=41)
    try:
        cbm.accumulate_bonds_(cb, m, est)
        assert (est.n1, est.n2) == (1, 2)                                   # the estimator's own tables are left alone
        cbm.fetch_bonds_(cb, m)
        for c in range(NCH):
            compare(cb.chains[c], want_of(m, cb, est.R, est.MinvR, c), label="%s chain %d" % (case, c))
    finally:
        m.close()


def test_two_accumulates_add_up_fetch_does_not_clear_reset_zeroes_and_runs_repeat():
    from elphdynamics_amd import chain_bond_measurements as cbm, greens
    m, cb, est = lockstep("hc3x2", seed=5)
    try:
        cbm.accumulate_bonds_(cb, m, est)
        cbm.fetch_bonds_(cb, m)
        one = [snapshot(c) for c in cb.chains]
        first = [want_of(m, cb, est.R, est.MinvR, c) for c in range(NCH)]
        R1, M1 = est.R.copy(), est.MinvR.copy()
        greens.set_vectors_(est, *vectors(m, NCH, NV, seed=77))
        cbm.accumulate_bonds_(cb, m, est)
        cbm.fetch_bonds_(cb, m)
        for c in range(NCH):
            compare(cb.chains[c], add(first[c], want_of(m, cb, est.R, est.MinvR, c)), label="two accumulates, chain %d" % c)
        two = [snapshot(c) for c in cb.chains]
        cbm.fetch_bonds_(cb, m)                                             # fetch does not clear
        assert all(same_bits(a, snapshot(c)) for a, c in zip(two, cb.chains))
        cbm.reset_bond_measurements_(cb, m)
        cbm.fetch_bonds_(cb, m)
        for c in cb.chains:
            assert all(not v.any() for v in snapshot(c).values())           # exact zeros
        greens.set_vectors_(est, R1, M1)                                    # the same inputs again: the same bits
        cbm.accumulate_bonds_(cb, m, est)
        cbm.fetch_bonds_(cb, m)
        assert all(same_bits(a, snapshot(c)) for a, c in zip(one, cb.chains))
    finally:
        m.close()


def test_chains_do_not_leak_into_one_another():
    from elphdynamics_amd import chain_bond_measurements as cbm, greens
    m, cb, est = lockstep("hc3x2_both_ways", seed=8)
    try:
        cbm.accumulate_bonds_(cb, m, est)
        cbm.fetch_bonds_(cb, m)
        one = [snapshot(c) for c in cb.chains]
        # only chain 1's vectors change
        R2, M2 = vectors(m, NCH, NV, seed=99)
        Rn, Mn = est.R.copy(), est.MinvR.copy()
        Rn[1::NCH], Mn[1::NCH] = R2[1::NCH], M2[1::NCH]
        greens.set_vectors_(est, Rn, Mn)
        cbm.reset_bond_measurements_(cb, m)
        cbm.accumulate_bonds_(cb, m, est)
        cbm.fetch_bonds_(cb, m)
        two = [snapshot(c) for c in cb.chains]
        assert same_bits(one[0], two[0]) and same_bits(one[2], two[2])
        assert all(not np.array_equal(one[1][k], two[1][k]) for k in one[1])
        compare(cb.chains[1], want_of(m, cb, Rn, Mn, 1), label="chain 1 after its vectors changed")
    finally:
        m.close()


def test_one_correlation_alone_gives_the_same_bits():
    """A container with BondBond alone, or BondPairGreens alone, transforms only that correlation's fields [k0, k1), here with the chain
    strides: same bits as together."""
    from elphdynamics_amd import chain_bond_measurements as cbm
    m, both, est = lockstep("hc3x2_both_ways", seed=3)
    table = SMALL["hc3x2_both_ways"][4]
    try:
        cbm.accumulate_bonds_(both, m, est)
        cbm.fetch_bonds_(both, m)
        for name in bref.CORRS:
            alone = cbm.initialize_chain_bond_container(m, {name: table[name], "num_random_vectors": NV}, [""] * NCH)
            cbm.accumulate_bonds_(alone, m, est)                            # replaces the handle's chain bond accumulators
            cbm.fetch_bonds_(alone, m)
            for c in range(NCH):
                assert set(alone.chains[c].intersite_corr) == {name}
                assert np.array_equal(alone.chains[c].intersite_corr[name].position, both.chains[c].intersite_corr[name].position), (name, c)
        compare(both.chains[2], want_of(m, both, est.R, est.MinvR, 2), label="both together, chain 2")
    finally:
        m.close()


@pytest.mark.parametrize("order", ["bonds_first", "onsite_first"])
def test_beside_the_onsite_chain_container_in_either_order(order):
    """The two chain containers on one handle and estimator: each one's sums are the bits it gets alone."""
    from elphdynamics_amd import chain_bond_measurements as cbm, chain_measurements as cms
    from test_gpu_measurements import snapshot as onsite_snapshot
    onsite = {"Greens": TD, "SpinSpin": {"measure": True, "time_dependent": False}, "PhononGreens": TD, "num_random_vectors": NV}
    m, cb, est = lockstep("hc3x2", seed=12)
    X = fields(m, NCH, 12)
    try:
        # each alone first
        cm = cms.initialize_chain_measurements_container(m, onsite, [""] * NCH)
        cms.accumulate_(cm, m, est, X)
        cms.fetch_(cm, m)
        onsite_alone = [onsite_snapshot(c) for c in cm.chains]
        cms.reset_measurements_(cm, m)
        cbm.accumulate_bonds_(cb, m, est)
        cbm.fetch_bonds_(cb, m)
        bonds_alone = [snapshot(c) for c in cb.chains]
        cbm.reset_bond_measurements_(cb, m)
        # then interleaved
        if order == "bonds_first":
            cbm.accumulate_bonds_(cb, m, est)
            cms.accumulate_(cm, m, est, X)
        else:
            cms.accumulate_(cm, m, est, X)
            cbm.accumulate_bonds_(cb, m, est)
        cms.fetch_(cm, m)
        cbm.fetch_bonds_(cb, m)
        for c in range(NCH):
            got = onsite_snapshot(cm.chains[c])
            assert all(np.array_equal(got[k], onsite_alone[c][k]) for k in got), (order, c)
            assert same_bits(snapshot(cb.chains[c]), bonds_alone[c]), (order, c)
        compare(cb.chains[1], want_of(m, cb, est.R, est.MinvR, 1), label="beside the on-site container, chain 1")
    finally:
        m.close()


def test_production_shape_against_the_single_configuration_path():
    """16 x 16, L = 160, two chains of two vectors, both correlations time-dependent over all four pairs: the tau-DFTs take their
    matrix-core forms and the batch changes the kernel chosen.  The reference is the device's single-configuration path
    (bond_measurements) on a second handle with the same vectors; the bound 2e-12 * max(1, max|single|), each side being held to 1e-12 of
    the direct sums."""
    from elphdynamics_amd import bond_measurements as bm, chain_bond_measurements as cbm, greens
    shape = (1, (16, 16, 1), 160, SQUARE, {"BondBond": TD, "BondPairGreens": TD})
    m, cb, est = lockstep(None, seed=16, nch=2, nv=2, shape=shape)
    ns, dims, L, defs, table = shape
    m2 = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    try:
        cbm.accumulate_bonds_(cb, m, est)
        cbm.fetch_bonds_(cb, m)
        for c in range(2):
            single = bm.initialize_bond_container(m2, dict(table, num_random_vectors=2), "")
            est2 = greens.EstimateGreensFunction(m2, nv=2)                  # (a new estimator drops the handle's previous accumulators)
            greens.set_vectors_(est2, est.R[c::2], est.MinvR[c::2])
            bm.accumulate_bonds_(single, m2, est2)
            bm.fetch_bonds_(single, m2)
            a, b = snapshot(cb.chains[c]), snapshot(single)
            assert set(a) == set(b) == set(bref.CORRS)
            for k in b:
                assert not a[k].imag.any() and np.abs(b[k]).max() > 0
                worst = np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max())
                print("16 x 16 x 160, chain %d, %s: %.2e (max|single| %.3g), bound 2e-12" % (c, k, worst, np.abs(b[k]).max()))
                assert worst <= 2e-12, (c, k, worst)
    finally:
        m.close()
        m2.close()


def test_one_chain_resident_agrees_with_the_single_configuration_path():
    from elphdynamics_amd import bond_measurements as bm, chain_bond_measurements as cbm, greens
    ns, dims, L, defs, table = SMALL["sq4x4"]
    m = build_model(ns, dims, L, defs, seed=3)
    try:
        info = dict(table, num_random_vectors=3)
        cb = cbm.initialize_chain_bond_container(m, info, [""])
        c1 = bm.initialize_bond_container(m, info, "")
        est = greens.EstimateGreensFunction(m, nv=3)
        greens.set_vectors_(est, *vectors(m, 1, 3, seed=1))
        cbm.accumulate_bonds_(cb, m, est)
        bm.accumulate_bonds_(c1, m, est)                                    # both containers live on the handle side by side
        cbm.fetch_bonds_(cb, m)
        bm.fetch_bonds_(c1, m)
        want = want_of(m, cb, est.R, est.MinvR, 0)
        compare(cb.chains[0], want, label="one chain resident, chain container")
        compare(c1, want, label="one chain resident, single-configuration container")
        assert set(snapshot(c1)) == set(bref.CORRS) and all(np.abs(v).max() > 0 for v in snapshot(c1).values())
        assert_same_bits_as_single(snapshot(cb.chains[0]), snapshot(c1), "one chain resident")
    finally:
        m.close()


def test_deck_in_lockstep_measured_end_to_end(tmp_path):
    """process_input_file(deck, nchains = 3), one update of all chains, the device's own preconditioned solve for all chains' vectors,
    then accumulate; the fetched sums against the direct sums on Gr.R, Gr.MinvR per chain, the written files at 5e-9 absolute (half a
    unit of the 8 decimals written)."""
    from elphdynamics_amd import chain_bond_measurements as cbm, greens, hmc, lattice as lat, process_input as pi
    deck = pi.read_deck(os.path.join(DECKS, "holstein_hmc_honeycomb_L3.toml"))
    deck["measurements"] = {"num_random_vectors": NV, "BondBond": TD,
                            "BondPairGreens": {"measure": True, "time_dependent": True, "pairs": [[2, 1], [1, 1], [1, 2]]}}
    sim = pi.process_input_file(deck, nchains=NCH)
    H, m = sim.simulation_dynamics, sim.model
    try:
        assert m.bond_definitions == lat.HONEYCOMB_BONDS
        H.device_rng_(31)
        hmc.update_chains_(m, H, sim.fa, sim.preconditioner, pull=True)
        assert not H.flags.any()
        folders = [str(tmp_path / ("run%d" % c)) for c in range(NCH)]
        for f in folders:
            os.mkdir(f)
        cb = cbm.initialize_chain_bond_container(m, sim.input["measurements"], folders)
        cbm.initialize_bond_folders_(cb)
        assert sim.Gr.nv == cb.n_rand_vecs * NCH
        it, res, fl = greens.update_(sim.Gr, m, sim.preconditioner, rng=np.random.default_rng(2))
        assert not fl.any() and it.min() > 0                                # the solve raised no flags
        cbm.accumulate_bonds_(cb, m, sim.Gr)
        wants = [want_of(m, cb, sim.Gr.R, sim.Gr.MinvR, c) for c in range(NCH)]
        cbm.fetch_bonds_(cb, m)
        for c in range(NCH):
            compare(cb.chains[c], wants[c], label="deck, chain %d" % c)
        bin_size = 1
        cbm.process_bond_measurements_(cb, bin_size, m)
        cbm.write_bond_measurements_(cb, m, 3)
        V = bin_size * 3                                                    # binomial(3, 2), the vectors of ONE chain
        for c, (d, want) in enumerate(zip(folders, wants)):
            for k, w in want.items():
                pos = w / V
                for space, arr in (("position", pos), ("momentum", mref.momentum(pos))):
                    got = parse(os.path.join(d, "%s_%s_f" % (k, space), "%s_%s_00003.out" % (k, space))).reshape(arr.shape, order="F")
                    assert np.abs(got.real - arr.real).max() <= 5e-9 and np.abs(got.imag - arr.imag).max() <= 5e-9, (c, k, space)
                    if k == "BondPairGreens":
                        s = mref.simpson(arr, m.dtau)
                        got = parse(os.path.join(d, "BondPairSusc_%s_f" % space, "BondPairSusc_%s_00003.out" % space)).reshape(s.shape, order="F")
                        assert np.abs(got.real - s.real).max() <= 5e-9 and np.abs(got.imag - s.imag).max() <= 5e-9, (c, "BondPairSusc", space)
            assert set(cb.chains[c].intersite_susc) == {"BondPairSusc"}
    finally:
        m.close()


def raw_create(m, nchains, defs, pairs=(1, 1), which=0, npairs=1):
    """elph_bond_chains_create with one correlation requested for `npairs` pairs of bonds, straight through the C ABI."""
    import ctypes as C
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    o1, o2, v = i32([d[0] for d in defs]), i32([d[1] for d in defs]), i32([k for d in defs for k in d[2]])
    flag = i32([which == 0, which == 1])
    return m._lib.elph_bond_chains_create(m._h, nchains, len(defs), ip(o1), ip(o2), ip(v), ip(flag), ip(flag), ip(flag * npairs), ip(i32(list(pairs))))


def test_refusals_from_the_library(oracle):
    from elphdynamics_amd import _lib, chain_bond_measurements as cbm, configs, greens, models
    from test_gpu_bond_measurements import raw_create as raw_create_single
    m, cb, est = lockstep("hc3x2", seed=2)
    defs = SMALL["hc3x2"][3]
    try:
        lib = m._lib
        last = lambda: lib.elph_last_error().decode()  # noqa: E731
        # nothing created yet
        for call in (lambda: lib.elph_bond_chains_accumulate(m._h), lambda: lib.elph_bond_chains_reset(m._h),
                     lambda: lib.elph_bond_chains_fetch(m._h, 0, None, None)):
            assert call() == _lib.ELPH_E_STATE and "elph_bond_chains_create" in last(), last()
        # a chain count that is not the resident one
        for n in (0, 2, 4):
            assert raw_create(m, n, defs) == _lib.ELPH_E_ARG and "created for %d chains, 3 are resident" % n in last(), last()
        # the argument and pair checks, naming correlation and index
        assert raw_create(m, 3, defs, pairs=(1, 4), which=1) == _lib.ELPH_E_ARG and "bond 4" in last() and "BondPairGreens" in last(), last()
        assert raw_create(m, 3, defs, pairs=(0, 1)) == _lib.ELPH_E_ARG and "bond 0" in last() and "BondBond" in last(), last()
        assert raw_create(m, 3, [(1, 3, (0, 0, 0))]) == _lib.ELPH_E_ARG and "orbital 3" in last() and "definition 1" in last(), last()
        assert raw_create(m, 3, defs, npairs=0) == _lib.ELPH_E_ARG and "BondBond" in last() and "no pair" in last(), last()
        assert raw_create(m, 3, []) == _lib.ELPH_E_ARG and "0 bond definitions" in last(), last()
        assert lib.elph_bond_chains_accumulate(m._h) == _lib.ELPH_E_STATE and "elph_bond_chains_create" in last()      # every refusal left no state
        # grids beyond 65535 in y or z, refused before anything is allocated: 4 fields x 5462 definitions x 3 chains; 21846 pairs x 3 chains
        many = [(1, 2, (0, 0, 0))] * 5462
        assert raw_create(m, 3, many) == _lib.ELPH_E_UNSUPPORTED and "5462 bond definitions" in last() and "65544" in last(), last()
        assert raw_create(m, 3, defs, pairs=[1, 1] * 21846, npairs=21846) == _lib.ELPH_E_UNSUPPORTED and "21846 listed pairs" in last(), last()
        assert raw_create(m, 3, many[:5461]) == _lib.ELPH_OK                # 65532 slices: allowed (one pair listed)
        # fetch of chain nchains (and of chain -1)
        cbm.accumulate_bonds_(cb, m, est)
        for chain in (3, -1):
            assert lib.elph_bond_chains_fetch(m._h, chain, None, None) == _lib.ELPH_E_ARG and "outside 0..2" in last(), last()
        bb = np.zeros(2 * 6 * 3)
        assert lib.elph_bond_chains_fetch(m._h, 2, _lib.dptr(bb), None) == _lib.ELPH_OK and bb[0] != 0
        # with npairs all zero nothing is launched
        none = cbm.initialize_chain_bond_container(m, {"num_random_vectors": NV}, [""] * NCH)
        cbm.accumulate_bonds_(none, m, est)
        zero = np.zeros(2, dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(_lib.P_int)  # noqa: E731
        one = np.ones(3, dtype=np.int32)
        assert lib.elph_bond_chains_create(m._h, 3, 1, ip(one), ip(one), ip(np.zeros(3, dtype=np.int32)), ip(zero), ip(zero), ip(zero), None) == _lib.ELPH_OK
        assert lib.elph_bond_chains_accumulate(m._h) == _lib.ELPH_OK and lib.elph_bond_chains_fetch(m._h, 1, None, None) == _lib.ELPH_OK
        # an estimator whose vectors are not a multiple of the chains: 4 vectors, 3 chains (a new estimator drops the device side)
        est4 = greens.EstimateGreensFunction(m, nv=4)
        assert lib.elph_bond_chains_accumulate(m._h) == _lib.ELPH_E_STATE and "elph_bond_chains_create" in last()
        assert raw_create(m, 3, defs) == _lib.ELPH_OK
        assert lib.elph_bond_chains_accumulate(m._h) == _lib.ELPH_E_STATE and "4 vectors" in last() and "3 resident chains" in last(), last()
        # accumulate before any vectors
        est6 = greens.EstimateGreensFunction(m, nv=6)
        assert raw_create(m, 3, defs) == _lib.ELPH_OK
        assert lib.elph_bond_chains_accumulate(m._h) == _lib.ELPH_E_STATE and "no vectors" in last(), last()
        greens.set_vectors_(est6, np.ones((6, m.Ndim)), np.ones((6, m.Ndim)))
        assert lib.elph_bond_chains_accumulate(m._h) == _lib.ELPH_OK
        # the single-configuration entry points keep refusing resident chains
        assert raw_create_single(m, defs) == _lib.ELPH_E_UNSUPPORTED and "chains" in last()
        # update_model_ drops the chains: the container was made for three
        models.update_model_(m)
        assert lib.elph_bond_chains_accumulate(m._h) == _lib.ELPH_E_STATE and "3 chains" in last() and "1 are resident" in last(), last()
        assert lib.elph_bond_chains_reset(m._h) == _lib.ELPH_OK             # ... and is still there
        mulM_still_right(oracle, m)
        # a new estimator drops the device side; the container notices and makes it again for the new one
        models.update_model_chains_(m, fields(m, NCH, 2))
        est9 = greens.EstimateGreensFunction(m, nv=9)
        greens.set_vectors_(est9, est.R, est.MinvR)
        cbm.accumulate_bonds_(cb, m, est9)
        cbm.fetch_bonds_(cb, m)
        for c in range(NCH):
            compare(cb.chains[c], want_of(m, cb, est.R, est.MinvR, c), label="after a new estimator, chain %d" % c)
        del est4
    finally:
        m.close()
    s = configs.make_model("e")
    try:
        greens.EstimateGreensFunction(s, nv=2)
        assert raw_create(s, 1, SQUARE) == _lib.ELPH_E_UNSUPPORTED and "SSH" in s._lib.elph_last_error().decode()
        with pytest.raises(cbm.UnsupportedMeasurement, match="SSH"):
            cbm.initialize_chain_bond_container(s, {"BondBond": TD}, [""], bond_definitions=SQUARE)
        mulM_still_right(oracle, s)
    finally:
        s.close()
