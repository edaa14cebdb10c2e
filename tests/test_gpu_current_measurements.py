"""GPU parity of the Holstein model's CurrentCurrent (csrc/currcorr.hip through elphdynamics_amd/current_measurements.py) against the
direct sums of tests/current_reference.py (ssh_bond_reference.current_direct under the last-slice weight table), which
tests/test_current_measurements_host.py pins against the transcript of Measurements.jl:1790-2098 and shows to differ from the other
reading (t on every slice) by more than 1e-6 on every case with non-unit hopping.

Bound on every entry: |got - ref| <= 1e-12 * max(1, max|ref|), the bound DESIGN holds the SSH CurrentCurrent kernels to.  Vectors go in
through greens.set_vectors_ (no solve) with n_v = 3 per chain, rough and seeded; the hoppings come from assign_t_ with stddev > 0
(seeded) or uniform with t != 1 and a negative sign in one definition (CASES of the host test).  Chains: 2 and 3 resident.

Not asserted, because they cannot be reached at test size: the refusals of grids beyond 65535 in y or z (8 n_def nchains slices,
npairs nchains transforms) and of a lattice whose frequency slice does not fit the LDS.  Not asserted either: the refusal of a slab
handle, which is the library's own and cannot be reached from outside (the sharded handle, refused by the same check, is driven)."""
import ctypes as C
import os

import numpy as np
import pytest

import current_reference as cref
from test_bond_measurements_host import BOTH_WAYS, SQUARE, TD
from test_current_measurements_host import CASES, assign_hoppings
from test_gpu_measurements import mulM_still_right, parse

pytestmark = pytest.mark.gpu

NV = 3


def device_case(case, nchains=1, seed=0):
    """A HolsteinModel of CASES[case] on the device, with nchains chains resident when nchains > 1."""
    from elphdynamics_amd import lattice as lat, models, synth
    ns, dims, L, defs, hop, entry = CASES[case]
    rng = np.random.default_rng(seed + L)
    m = models.HolsteinModel(lat.Lattice(ns, *dims), L * 0.1, 0.1, tol=1e-13, maxiter=20000)
    assert m.Ltau == L
    assign_hoppings(m, defs, hop, seed=L + sum(dims))
    N = m.Nsites
    m.omega[:] = 1.0 + 0.1 * rng.standard_normal(N)
    m.lam[:] = 1.0 + 0.1 * rng.standard_normal(N)
    m.mu[:] = 0.1 * rng.standard_normal(N)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=seed + 3)
    if nchains > 1:
        models.update_model_chains_(m, fields(m, nchains, seed))
    else:
        models.update_model_(m)
    nc = dims[0] * dims[1] * dims[2]
    assert m.Nbonds == len(defs) * nc                                       # the reference's reshape of t holds
    return m


def fields(m, nch, seed):
    from elphdynamics_amd import synth
    return np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=seed + 1 + c) for c in range(nch)])


def vectors(m, nch, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((NV * nch, m.Ndim)), rng.standard_normal((NV * nch, m.Ndim))


def setup(case, nchains=1, seed=0, entry=None):
    """Model, container, estimator with its vectors set."""
    from elphdynamics_amd import current_measurements as cm, greens
    m = device_case(case, nchains, seed)
    info = {"num_random_vectors": NV, "CurrentCurrent": entry or CASES[case][5]}
    c = cm.initialize_current_container(m, info, [""] * nchains if nchains > 1 else "")
    est = greens.EstimateGreensFunction(m, nv=NV * nchains)
    greens.set_vectors_(est, *vectors(m, nchains, seed + 11))
    return m, c, est


def want_of(m, c, R, MinvR, chain):
    """The direct sums of chain `chain`: its vectors [v * nchains + chain]."""
    la = m.lattice
    corr = c.chains[chain].intersite_corr["CurrentCurrent"]
    return cref.measure(R[chain::c.nchains], MinvR[chain::c.nchains], m.t, m.Ltau, la.norbits, (la.L1, la.L2, la.L3), c.bond_definitions,
                        corr.position.shape[0], corr.pairs)


def device_tables(m):
    """The estimator's four device tables (elph_greens_dev_arrays) copied to the host as they are."""
    arrs, cnt = (C.c_void_p * 4)(), C.c_int64()
    assert m._lib.elph_greens_dev_arrays(m._h, arrs, C.byref(cnt)) == 0
    hip = C.CDLL("libamdhip64.so")
    out = []
    for k in range(4):
        buf = np.empty(2 * cnt.value)
        assert hip.hipMemcpy(buf.ctypes.data_as(C.c_void_p), C.c_void_p(arrs[k]), C.c_size_t(16 * cnt.value), 2) == 0
        out.append(buf)
    return list(arrs), out


def snapshot(c):
    return [ch.intersite_corr["CurrentCurrent"].position.copy() for ch in c.chains]


def compare(c, chain, want, scale=1.0, label=""):
    got = c.chains[chain].intersite_corr["CurrentCurrent"].position
    w = scale * want
    assert got.shape == w.shape and np.abs(w).max() > 0
    assert not got.imag.any()                                               # exact zeros
    worst = np.abs(got.real - w).max() / max(1.0, np.abs(w).max())
    print(label, "CurrentCurrent: %.2e (max|ref| %.3g), bound 1e-12" % (worst, np.abs(w).max()))
    assert worst <= 1e-12, (label, worst)


@pytest.mark.parametrize("case", list(CASES))
def test_accumulator_matches_the_direct_sums(case):
    """One configuration: every entry within the bound; two runs give the same bits; twice accumulated is exactly twice; reset zeroes;
    Gr.n1, Gr.n2 and the estimator's device tables are left as they were."""
    from elphdynamics_amd import current_measurements as cm, greens
    m, c, est = setup(case, seed=4)
    try:
        greens.setup_(est, 1, 3)
        where, tables = device_tables(m)
        assert all(t.any() for t in tables)
        want = want_of(m, c, est.R, est.MinvR, 0)
        cm.accumulate_current_(c, m, est)
        assert (est.n1, est.n2) == (1, 3)                                   # not the last pair's: setup! never ran
        cm.fetch_current_(c, m)
        compare(c, 0, want, label=case)
        one = snapshot(c)[0]
        cm.accumulate_current_(c, m, est)                                   # a second accumulation without reset: exactly twice one
        cm.fetch_current_(c, m)
        assert np.array_equal(snapshot(c)[0], 2 * one)
        compare(c, 0, want, scale=2.0, label=case + " x2")
        cm.fetch_current_(c, m)                                             # fetch does not clear
        assert np.array_equal(snapshot(c)[0], 2 * one)
        cm.reset_current_measurements_(c, m)
        cm.fetch_current_(c, m)
        assert not snapshot(c)[0].any()                                     # reset: exact zeros
        cm.accumulate_current_(c, m, est)
        cm.fetch_current_(c, m)
        assert np.array_equal(snapshot(c)[0], one)                          # the same inputs again: the same bits
        # the estimator's device tables, read back with no setup_ in between: the same allocations holding the same bits
        where_now, tables_now = device_tables(m)
        assert where_now == where and all(np.array_equal(a, b) for a, b in zip(tables, tables_now))
    finally:
        m.close()


@pytest.mark.parametrize("case, nch", [("hc3x2_disorder", 3), ("hc3x2_uniform_subset", 2), ("chain12_disorder", 2), ("sq4x4_uniform", 3),
                                       ("chain12_equal_time_subset", 3)])
def test_every_chain_equals_a_single_configuration_handle_bit_for_bit(case, nch):
    from elphdynamics_amd import current_measurements as cm, greens
    m, c, est = setup(case, nchains=nch, seed=21)
    m1 = device_case(case, 1, seed=21)
    try:
        cm.accumulate_current_(c, m, est)
        assert (est.n1, est.n2) == (1, 2)
        cm.fetch_current_(c, m)
        chains = snapshot(c)
        for ch in range(nch):
            compare(c, ch, want_of(m, c, est.R, est.MinvR, ch), label="%s, %d chains, chain %d" % (case, nch, ch))
            single = cm.initialize_current_container(m1, {"num_random_vectors": NV, "CurrentCurrent": CASES[case][5]}, "")
            est1 = greens.EstimateGreensFunction(m1, nv=NV)                 # (a new estimator drops the handle's previous accumulators)
            greens.set_vectors_(est1, est.R[ch::nch], est.MinvR[ch::nch])
            cm.accumulate_current_(single, m1, est1)
            cm.fetch_current_(single, m1)
            assert np.abs(chains[ch]).max() > 0 and np.array_equal(chains[ch], snapshot(single)[0]), (case, ch)
        # two runs: the same bits
        cm.reset_current_measurements_(c, m)
        cm.accumulate_current_(c, m, est)
        cm.fetch_current_(c, m)
        assert all(np.array_equal(a, b) for a, b in zip(chains, snapshot(c)))
    finally:
        m.close()
        m1.close()


def test_chains_do_not_leak_into_one_another():
    from elphdynamics_amd import current_measurements as cm, greens
    nch = 3
    m, c, est = setup("hc3x2_disorder", nchains=nch, seed=8)
    try:
        cm.accumulate_current_(c, m, est)
        cm.fetch_current_(c, m)
        one = snapshot(c)
        R2, M2 = vectors(m, nch, seed=99)                                   # only chain 1's vectors change
        Rn, Mn = est.R.copy(), est.MinvR.copy()
        Rn[1::nch], Mn[1::nch] = R2[1::nch], M2[1::nch]
        greens.set_vectors_(est, Rn, Mn)
        cm.reset_current_measurements_(c, m)
        cm.accumulate_current_(c, m, est)
        cm.fetch_current_(c, m)
        two = snapshot(c)
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2]) and not np.array_equal(one[1], two[1])
        compare(c, 1, want_of(m, c, Rn, Mn, 1), label="chain 1 after its vectors changed")
    finally:
        m.close()


@pytest.mark.parametrize("order", ["current_first", "others_first"])
def test_beside_a_bond_container_and_an_onsite_chain_container_in_either_order(order):
    """Three device sides on one handle and estimator: each one's sums are the bits it gets alone."""
    from elphdynamics_amd import chain_bond_measurements as cbm, chain_measurements as cms, current_measurements as cm
    from test_gpu_bond_measurements import snapshot as bond_snapshot
    from test_gpu_measurements import snapshot as onsite_snapshot
    nch = 2
    m, c, est = setup("hc3x2_disorder", nchains=nch, seed=12)
    X = fields(m, nch, 12)
    try:
        cb = cbm.initialize_chain_bond_container(m, {"BondBond": TD, "BondPairGreens": TD, "num_random_vectors": NV}, [""] * nch)
        co = cms.initialize_chain_measurements_container(m, {"Greens": TD, "SpinSpin": {"measure": True, "time_dependent": False},
                                                             "num_random_vectors": NV}, [""] * nch)
        # each alone first
        cm.accumulate_current_(c, m, est)
        cm.fetch_current_(c, m)
        cur_alone = snapshot(c)
        cm.reset_current_measurements_(c, m)
        cbm.accumulate_bonds_(cb, m, est)
        cbm.fetch_bonds_(cb, m)
        bonds_alone = [bond_snapshot(x) for x in cb.chains]
        cbm.reset_bond_measurements_(cb, m)
        cms.accumulate_(co, m, est, X)
        cms.fetch_(co, m)
        onsite_alone = [onsite_snapshot(x) for x in co.chains]
        cms.reset_measurements_(co, m)
        # then interleaved
        if order == "current_first":
            cm.accumulate_current_(c, m, est)
            cbm.accumulate_bonds_(cb, m, est)
            cms.accumulate_(co, m, est, X)
        else:
            cms.accumulate_(co, m, est, X)
            cbm.accumulate_bonds_(cb, m, est)
            cm.accumulate_current_(c, m, est)
        cm.fetch_current_(c, m)
        cbm.fetch_bonds_(cb, m)
        cms.fetch_(co, m)
        for ch in range(nch):
            assert np.array_equal(snapshot(c)[ch], cur_alone[ch]), (order, ch)
            got = bond_snapshot(cb.chains[ch])
            assert all(np.array_equal(got[k], bonds_alone[ch][k]) for k in got), (order, ch)
            got = onsite_snapshot(co.chains[ch])
            assert all(np.array_equal(got[k], onsite_alone[ch][k]) for k in got), (order, ch)
        compare(c, 1, want_of(m, c, est.R, est.MinvR, 1), label="beside the other containers, chain 1")
    finally:
        m.close()


@pytest.mark.parametrize("nch", [1, 2])
def test_accumulate_twice_process_write_end_to_end(nch, tmp_path):
    from elphdynamics_amd import current_measurements as cm
    m, c0, est = setup("hc3x2_disorder", nchains=nch, seed=30)
    try:
        folders = [str(tmp_path / ("run%d" % ch)) for ch in range(nch)]
        for f in folders:
            os.mkdir(f)
        info = {"num_random_vectors": NV, "CurrentCurrent": TD, "BondBond": TD}
        c = cm.initialize_current_container(m, cm.split_info(info)[1], folders if nch > 1 else folders[0])
        cm.initialize_current_folders_(c)
        cm.accumulate_current_(c, m, est)
        cm.accumulate_current_(c, m, est)
        wants = [want_of(m, c, est.R, est.MinvR, ch) for ch in range(nch)]
        cm.process_current_measurements_(c, 2, m)
        cm.write_current_measurements_(c, m, 7)
        V = 2 * 3                                                           # bin_size * binomial(3, 2), the vectors of ONE chain
        for ch, (d, want) in enumerate(zip(folders, wants)):
            pos = 2 * want / V
            files = {}
            for space in ("position", "momentum"):
                files[space] = parse(os.path.join(d, "CurrentCurrent_%s_f" % space, "CurrentCurrent_%s_00007.out" % space)).reshape(pos.shape, order="F")
            assert np.abs(files["position"].real - pos).max() <= 5e-9 and not files["position"].imag.any()
            mom = np.fft.fftn(files["position"], axes=(1, 2, 3))            # the files parse back to momentum = fft of position ...
            assert np.abs(files["momentum"] - mom).max() <= 5e-9 * (1 + pos[0, ..., 0].size), ch
            exact = np.fft.fftn(pos, axes=(1, 2, 3))                        # ... and to the yardstick's / (2 * 3)
            assert np.abs(files["momentum"].real - exact.real).max() <= 5e-9 and np.abs(files["momentum"].imag - exact.imag).max() <= 5e-9, ch
            got = c.chains[ch].intersite_corr["CurrentCurrent"]
            assert np.abs(got.momentum - np.fft.fftn(got.position, axes=(1, 2, 3))).max() <= 1e-13 * max(1.0, np.abs(got.momentum).max())
        cm.reset_current_measurements_(c, m)
        cm.fetch_current_(c, m)
        assert all(not a.any() for a in snapshot(c))
    finally:
        m.close()


def raw_create(m, nchains, defs, pairs=(1, 1), npairs=1, measure=1, Nbonds=None, t="model"):
    """elph_current_create for `npairs` pairs of bonds, time-dependent, straight through the C ABI."""
    from elphdynamics_amd._lib import dptr
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    o1, o2, v = i32([d[0] for d in defs]), i32([d[1] for d in defs]), i32([k for d in defs for k in d[2]])
    tt = np.ascontiguousarray(m.t, dtype=np.float64)
    return m._lib.elph_current_create(m._h, nchains, len(defs), ip(o1), ip(o2), ip(v), int(m.Nbonds if Nbonds is None else Nbonds),
                                      dptr(tt) if t == "model" else None, measure, 1, npairs, ip(i32(list(pairs))) if pairs is not None else None)


def test_refusals_from_the_library(oracle):
    from elphdynamics_amd import _lib, configs, current_measurements as cm, greens, models
    nch = 3
    m = device_case("hc3x2_disorder", nch, seed=2)
    defs = BOTH_WAYS
    try:
        lib = m._lib
        last = lambda: lib.elph_last_error().decode()  # noqa: E731
        # no estimator
        assert raw_create(m, nch, defs) == _lib.ELPH_E_STATE and "elph_greens_create" in last(), last()
        est = greens.EstimateGreensFunction(m, nv=NV * nch)
        # nothing created yet
        for call in (lambda: lib.elph_current_accumulate(m._h), lambda: lib.elph_current_reset(m._h), lambda: lib.elph_current_fetch(m._h, 0, None)):
            assert call() == _lib.ELPH_E_STATE and "elph_current_create" in last(), last()
        # a chain count that is not the resident one
        for n in (0, 1, 4):
            assert raw_create(m, n, defs) == _lib.ELPH_E_ARG and "created for %d chains, 3 are resident" % n in last(), last()
        # the argument and pair checks, naming definition or pair
        assert raw_create(m, nch, []) == _lib.ELPH_E_ARG and "0 bond definitions" in last(), last()
        i32 = np.ones(3, dtype=np.int32)
        ip = i32.ctypes.data_as(_lib.P_int)
        assert lib.elph_current_create(m._h, nch, 1, None, ip, ip, m.Nbonds, _lib.dptr(m.t), 1, 1, 1, ip) == _lib.ELPH_E_ARG and "null array" in last(), last()
        assert raw_create(m, nch, [(1, 3, (0, 0, 0))] + defs[1:]) == _lib.ELPH_E_ARG and "orbital 3" in last() and "definition 1" in last(), last()
        assert raw_create(m, nch, defs, npairs=0) == _lib.ELPH_E_ARG and "CurrentCurrent" in last() and "no pair" in last(), last()
        assert raw_create(m, nch, defs, pairs=None) == _lib.ELPH_E_ARG and "CurrentCurrent" in last() and "no pair" in last(), last()
        assert raw_create(m, nch, defs, pairs=(1, 4)) == _lib.ELPH_E_ARG and "bond 4" in last() and "pair 1" in last() and "CurrentCurrent" in last(), last()
        assert raw_create(m, nch, defs, pairs=(1, 1, 0, 2), npairs=2) == _lib.ELPH_E_ARG and "bond 0" in last() and "pair 2" in last(), last()
        # a bond count that is not the handle's; a null t
        assert raw_create(m, nch, defs, Nbonds=m.Nbonds - 1) == _lib.ELPH_E_ARG and "%d bonds (the handle has %d)" % (m.Nbonds - 1, m.Nbonds) in last(), last()
        assert raw_create(m, nch, defs, t=None) == _lib.ELPH_E_ARG and "null hopping array" in last(), last()
        # the handle's bonds are not n_def x ncells: two definitions where the model has three
        assert raw_create(m, nch, defs[:2]) == _lib.ELPH_E_UNSUPPORTED and "%d bonds are not 2 definitions x 6 cells" % m.Nbonds in last(), last()
        assert lib.elph_current_accumulate(m._h) == _lib.ELPH_E_STATE and "elph_current_create" in last()      # every refusal left no state
        # no vectors yet
        assert raw_create(m, nch, defs) == _lib.ELPH_OK
        assert lib.elph_current_accumulate(m._h) == _lib.ELPH_E_STATE and "no vectors" in last(), last()
        # ... then a valid create and accumulate succeeds on the same handle
        R, X = vectors(m, nch, seed=5)
        greens.set_vectors_(est, R, X)
        c = cm.initialize_current_container(m, {"num_random_vectors": NV, "CurrentCurrent": TD}, [""] * nch)
        cm.accumulate_current_(c, m, est)
        cm.fetch_current_(c, m)
        compare(c, 2, want_of(m, c, R, X, 2), label="after the refusals, chain 2")
        for chain in (3, -1):
            assert lib.elph_current_fetch(m._h, chain, None) == _lib.ELPH_E_ARG and "outside 0..2" in last(), last()
        # with no pair requested nothing is launched, and fetch leaves its output alone
        assert raw_create(m, nch, defs, measure=0, npairs=0, pairs=None) == _lib.ELPH_OK
        out = np.full(4, 7.0)
        assert lib.elph_current_accumulate(m._h) == _lib.ELPH_OK and lib.elph_current_fetch(m._h, 1, _lib.dptr(out)) == _lib.ELPH_OK
        assert lib.elph_current_reset(m._h) == _lib.ELPH_OK and (out == 7.0).all()
        none = cm.initialize_current_container(m, {"num_random_vectors": NV}, [""] * nch)
        cm.accumulate_current_(none, m, est)
        # an estimator whose vectors are not a multiple of the chains: 4 vectors, 3 chains (a new estimator drops the device side)
        est4 = greens.EstimateGreensFunction(m, nv=4)
        assert lib.elph_current_accumulate(m._h) == _lib.ELPH_E_STATE and "elph_current_create" in last()
        assert raw_create(m, nch, defs) == _lib.ELPH_OK
        assert lib.elph_current_accumulate(m._h) == _lib.ELPH_E_STATE and "4 vectors" in last() and "3 resident chains" in last(), last()
        # update_model_ drops the chains: the state was made for three
        models.update_model_(m)
        assert lib.elph_current_accumulate(m._h) == _lib.ELPH_E_STATE and "3 chains" in last() and "1 are resident" in last(), last()
        assert lib.elph_current_reset(m._h) == _lib.ELPH_OK                 # ... and is still there
        mulM_still_right(oracle, m)
        # one configuration now: a new estimator, the container notices and makes the device side again
        est3 = greens.EstimateGreensFunction(m, nv=NV)
        greens.set_vectors_(est3, R[:NV], X[:NV])
        c1 = cm.initialize_current_container(m, {"num_random_vectors": NV, "CurrentCurrent": TD}, "")
        cm.accumulate_current_(c1, m, est3)
        cm.fetch_current_(c1, m)
        compare(c1, 0, want_of(m, c1, R[:NV], X[:NV], 0), label="one configuration after the chains were dropped")
        est6 = greens.EstimateGreensFunction(m, nv=NV)                      # dropped again: the container makes it again for the new estimator
        greens.set_vectors_(est6, R[:NV], X[:NV])
        cm.accumulate_current_(c1, m, est6)
        cm.fetch_current_(c1, m)
        compare(c1, 0, want_of(m, c1, R[:NV], X[:NV], 0), label="after a new estimator")
        del est4
    finally:
        m.close()
    # a sharded Holstein handle (one rank owning the whole lattice, made as test_gpu_ssh_chain_bond_measurements.py makes one); the SSH
    # check comes first, so only a Holstein handle reaches this refusal.  The handle stays sharded: the valid create before it is what
    # the refused one must have dropped
    sh = device_case("sq4x4_uniform", 1, seed=7)
    try:
        lib = sh._lib
        greens.EstimateGreensFunction(sh, nv=NV)
        assert raw_create(sh, 1, SQUARE) == _lib.ELPH_OK and lib.elph_current_reset(sh._h) == _lib.ELPH_OK
        key = (C.c_ubyte * 64)()
        assert lib.elph_shard_create(sh._h, 0, 1, 0, sh.Nsites, 0, 0, 0, 0, 0, None, C.cast(key, C.c_void_p)) == _lib.ELPH_OK
        assert raw_create(sh, 1, SQUARE) == _lib.ELPH_E_UNSUPPORTED and "sharded" in lib.elph_last_error().decode(), lib.elph_last_error().decode()
        assert lib.elph_current_reset(sh._h) == _lib.ELPH_E_STATE and "elph_current_create" in lib.elph_last_error().decode()
        assert lib.elph_current_accumulate(sh._h) == _lib.ELPH_E_STATE
    finally:
        sh.close()
    s = configs.make_model("e")
    try:
        greens.EstimateGreensFunction(s, nv=2)
        assert raw_create(s, 1, SQUARE) == _lib.ELPH_E_UNSUPPORTED and "SSH" in s._lib.elph_last_error().decode()
        with pytest.raises(cm.UnsupportedMeasurement, match="SSH"):
            cm.initialize_current_container(s, {"CurrentCurrent": TD}, "", bond_definitions=SQUARE)
        mulM_still_right(oracle, s)
    finally:
        s.close()
