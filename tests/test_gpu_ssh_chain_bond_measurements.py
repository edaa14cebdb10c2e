"""GPU parity of the SSH bond correlations of resident chains (csrc/ssh_bondcorr.hip through
elphdynamics_amd/ssh_chain_bond_measurements.py): every chain's container against the direct sums of tests/ssh_bond_reference.py
evaluated on that chain's field and vectors [v * nchains + c], with the bound of tests/test_gpu_ssh_bond_measurements.py (its `compare`,
imported: max|got - ref| < 1e-12 * max(1, max|ref|) per key, imaginary parts exactly zero).  A chain's sums have exactly the terms of
the single-configuration sums, so that bound carries over.

Vectors go in through greens.set_vectors_ (no solve) unless a test says otherwise.  Three chains with three vectors each: three pairs,
neither count a power of two, so a chain-major / vector-major mix-up cannot pass.  The chains' fields follow the recipe chain_field of
tests/test_gpu_ssh_chain_measurements.py (x_median of the named cases of ssh_measurement_cases), a seed per chain, and go in through
models.update_model_chains_.  Against the device's single-configuration path (ssh_bond_measurements.accumulate_ssh_bonds_) the bound is
the rule of assert_close_to_single there, 2e-12 * max(1, max|single|): each side meets 1e-12 of the direct sums in the suite.

The two grid refusals of elph_ssh_bond_chains_create (a product above 65535) are not asserted: with the pairs of CurrentCurrent bounded by
n_def^2 and the definitions by what a test lattice carries they cannot be reached at test sizes.

Worst deviations measured on an MI355X, in the units of each bound (a bound of 2e-12):
  one chain resident (hc3), chain container against the single-configuration container: 0 on every key (the same bits)
  16 x 16, L = 160 (config E), two chains against the single-configuration path: BondBond 5.9e-05 of the bound (1.18e-16),
  CurrentCurrent 0 (the same bits), BondPairGreens 1.2e-05 of the bound (2.43e-17)"""
import functools
import os

import numpy as np
import pytest

import ssh_bond_reference as sbref
import ssh_cases as sc
import ssh_measurement_cases as smc
from test_gpu_ssh_bond_measurements import compare, raw_create as raw_single_create, snapshot
from test_gpu_ssh_chain_measurements import chain_field
from test_gpu_ssh_chain_measurements import snapshot as onsite_snapshot
from test_gpu_measurements import assert_same_bits_as_single
from test_gpu_ssh_measurements import mulM_still_right
from test_ssh_bond_measurements_host import ALL3, CASES, TD, build, check_files, request_of, yardstick

pytestmark = pytest.mark.gpu

DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decks")
NCH = NV = 3


def x_median_of(case):
    what = CASES[case][0]
    return smc.CASES[what][6] if isinstance(what, str) else None


def chain_inputs(m, case, nch, nv, seed):
    """(X (nch, Ndof) a field per chain from seeds seed + 1 .., R, MinvR (nv * nch, Ndim) from rng(seed))."""
    rng = np.random.default_rng(seed)
    X = np.stack([chain_field(m, seed + 1 + c, x_median_of(case)) for c in range(nch)])
    return X, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim))


def container_of(case, m, nch=NCH, nv=NV, table=None, folders=None):
    from elphdynamics_amd import ssh_chain_bond_measurements as scb
    return scb.initialize_ssh_chain_bond_container(m, dict(table or CASES[case][1], num_random_vectors=nv), folders or [""] * nch)


def want_of(m, cb, R, MinvR, X, c):
    """The direct sums of chain c: its field, its vectors."""
    nch = cb.nchains
    return sbref.measure(R[c::nch], MinvR[c::nch], X[c], smc.ref_par(m), sbref.definitions(m), request_of(cb.chains[c]))


@functools.lru_cache(maxsize=None)
def chain_yardstick(case, seed=41):
    """(X, R, MinvR, the direct sums of every chain) of three chains with three vectors each: computed once per session, never written to."""
    host = build(case)
    host._nchains = NCH
    X, R, MinvR = chain_inputs(host, case, NCH, NV, seed)
    wants = [want_of(host, container_of(case, host), R, MinvR, X, c) for c in range(NCH)]
    for a in (X, R, MinvR) + tuple(v for w in wants for v in w.values()):
        a.setflags(write=False)
    return X, R, MinvR, wants


def lockstep(case, X, R, MinvR, table=None):
    """The device model of `case` with the chains of X resident, its estimator with the vectors set, and the chain bond container."""
    from elphdynamics_amd import greens, models
    nch = X.shape[0]
    m = build(case, device=True)
    models.update_model_chains_(m, X)
    cb = container_of(case, m, nch, R.shape[0] // nch, table)
    est = greens.EstimateGreensFunction(m, nv=R.shape[0])
    greens.set_vectors_(est, R, MinvR)
    return m, cb, est


def snapshots(cb):
    return [snapshot(c) for c in cb.chains]


def same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def add(a, b):
    return {k: a[k] + b[k] for k in a}


@pytest.mark.parametrize("case", list(CASES))
def test_every_chain_matches_the_direct_sums_of_its_own_inputs(case):
    from elphdynamics_amd import ssh_chain_bond_measurements as scb
    X, R, MinvR, wants = chain_yardstick(case)
    # before any GPU call: the chains' references differ, none is a comparison of zeros, and sq12x6 changes the sign of t' in every chain
    for k in wants[0]:
        for a in range(NCH):
            assert np.abs(wants[a][k]).max() > 1e-3, (case, a, k)
            for b in range(a + 1, NCH):
                assert not np.array_equal(wants[a][k], wants[b][k]), (case, a, b, k)
    if case == "sq12x6":
        host = build(case)
        for c in range(NCH):
            tp = sbref.hopping(X[c], smc.ref_par(host))
            assert (np.sign(tp).min(axis=1) < np.sign(tp).max(axis=1)).any(), c
    m, cb, est = lockstep(case, X, R, MinvR)
    try:
        scb.accumulate_ssh_bonds_(cb, m, est, X)
        assert (est.n1, est.n2) == (1, 2)                                   # the estimator's own tables are left alone
        scb.fetch_ssh_bonds_(cb, m)
        for c in range(NCH):
            compare(cb.chains[c], wants[c], label="%s chain %d" % (case, c))
    finally:
        m.close()


def test_two_accumulates_add_up_fetch_does_not_clear_reset_zeroes_and_runs_repeat():
    from elphdynamics_amd import greens, models, ssh_chain_bond_measurements as scb
    case = "hc3x2_listed"
    X, R, MinvR, wants = chain_yardstick(case)
    m, cb, est = lockstep(case, X, R, MinvR)
    try:
        scb.accumulate_ssh_bonds_(cb, m, est, X)
        scb.fetch_ssh_bonds_(cb, m)
        one = snapshots(cb)
        X2, R2, MinvR2 = chain_inputs(m, case, NCH, NV, seed=77)
        models.update_model_chains_(m, X2)
        greens.set_vectors_(est, R2, MinvR2)
        scb.accumulate_ssh_bonds_(cb, m, est, X2)
        scb.fetch_ssh_bonds_(cb, m)
        for c in range(NCH):
            compare(cb.chains[c], add(wants[c], want_of(m, cb, R2, MinvR2, X2, c)), label="two accumulates, chain %d" % c)
        two = snapshots(cb)
        scb.fetch_ssh_bonds_(cb, m)                                         # fetch does not clear
        assert all(same_bits(a, b) for a, b in zip(two, snapshots(cb)))
        scb.reset_ssh_bond_measurements_(cb, m)
        scb.fetch_ssh_bonds_(cb, m)
        for s in snapshots(cb):
            assert all(not v.any() for v in s.values())                     # exact zeros
        models.update_model_chains_(m, X)                                   # the same inputs again: the same bits
        greens.set_vectors_(est, R, MinvR)
        scb.accumulate_ssh_bonds_(cb, m, est, X)
        scb.fetch_ssh_bonds_(cb, m)
        assert all(same_bits(a, b) for a, b in zip(one, snapshots(cb)))
    finally:
        m.close()


def test_chains_do_not_leak_into_one_another():
    from elphdynamics_amd import greens, models, ssh_chain_bond_measurements as scb
    case = "hc3x2_both_ways"
    X, R, MinvR, wants = chain_yardstick(case)
    m, cb, est = lockstep(case, X, R, MinvR)
    try:
        scb.accumulate_ssh_bonds_(cb, m, est, X)
        scb.fetch_ssh_bonds_(cb, m)
        one = snapshots(cb)
        # only chain 1's field and vectors change
        X2, R2, M2 = chain_inputs(m, case, NCH, NV, seed=99)
        Xn, Rn, Mn = X.copy(), R.copy(), MinvR.copy()
        Xn[1], Rn[1::NCH], Mn[1::NCH] = X2[1], R2[1::NCH], M2[1::NCH]
        models.update_model_chains_(m, Xn)
        greens.set_vectors_(est, Rn, Mn)
        scb.reset_ssh_bond_measurements_(cb, m)
        scb.accumulate_ssh_bonds_(cb, m, est, Xn)
        scb.fetch_ssh_bonds_(cb, m)
        two = snapshots(cb)
        assert same_bits(one[0], two[0]) and same_bits(one[2], two[2])
        assert set(one[1]) == set(sbref.CORRS) and all(not np.array_equal(one[1][k], two[1][k]) for k in one[1])
        compare(cb.chains[1], want_of(m, cb, Rn, Mn, Xn, 1), label="chain 1 after its inputs changed")
        # then only chain 1's field: CurrentCurrent alone reads it
        Xf = Xn.copy()
        Xf[1] = chain_inputs(m, case, NCH, NV, seed=123)[0][1]
        models.update_model_chains_(m, Xf)
        scb.reset_ssh_bond_measurements_(cb, m)
        scb.accumulate_ssh_bonds_(cb, m, est, Xf)
        scb.fetch_ssh_bonds_(cb, m)
        three = snapshots(cb)
        assert same_bits(one[0], three[0]) and same_bits(one[2], three[2])
        assert not np.array_equal(two[1]["CurrentCurrent"], three[1]["CurrentCurrent"])
        assert np.array_equal(two[1]["BondBond"], three[1]["BondBond"]) and np.array_equal(two[1]["BondPairGreens"], three[1]["BondPairGreens"])
    finally:
        m.close()


def test_one_correlation_alone_gives_the_same_bits():
    """A container with one correlation alone computes and transforms only that correlation's fields, here with the chain strides: same
    bits as all three together."""
    from elphdynamics_amd import ssh_chain_bond_measurements as scb
    case = "hc3x2_both_ways"
    X, R, MinvR, wants = chain_yardstick(case)
    m, both, est = lockstep(case, X, R, MinvR)
    try:
        scb.accumulate_ssh_bonds_(both, m, est, X)
        scb.fetch_ssh_bonds_(both, m)
        for name in sbref.CORRS:
            alone = container_of(case, m, table={name: TD})
            scb.accumulate_ssh_bonds_(alone, m, est, X)                     # replaces the handle's chain bond accumulators
            scb.fetch_ssh_bonds_(alone, m)
            for c in range(NCH):
                assert set(alone.chains[c].intersite_corr) == {name}
                assert np.array_equal(alone.chains[c].intersite_corr[name].position, both.chains[c].intersite_corr[name].position), (name, c)
        compare(both.chains[2], wants[2], label="all three together, chain 2")
    finally:
        m.close()


@pytest.mark.parametrize("order", ["bonds_first", "onsite_first"])
def test_beside_the_onsite_chain_container_in_either_order(order):
    """The two chain containers of the SSH model on one handle and estimator: each one's sums are the bits it gets alone."""
    from elphdynamics_amd import ssh_chain_bond_measurements as scb, ssh_chain_measurements as scm
    case = "hc3"
    X, R, MinvR, wants = chain_yardstick(case)
    m, cb, est = lockstep(case, X, R, MinvR)
    try:
        # each alone first
        cm = scm.initialize_ssh_chain_measurements_container(m, dict(smc.CASES["hc3"][4], num_random_vectors=NV), [""] * NCH)
        scm.accumulate_(cm, m, est, X)
        scm.fetch_(cm, m)
        onsite_alone = [onsite_snapshot(c) for c in cm.chains]
        scm.reset_measurements_(cm, m)
        scb.accumulate_ssh_bonds_(cb, m, est, X)
        scb.fetch_ssh_bonds_(cb, m)
        bonds_alone = snapshots(cb)
        scb.reset_ssh_bond_measurements_(cb, m)
        # then interleaved
        if order == "bonds_first":
            scb.accumulate_ssh_bonds_(cb, m, est, X)
            scm.accumulate_(cm, m, est, X)
        else:
            scm.accumulate_(cm, m, est, X)
            scb.accumulate_ssh_bonds_(cb, m, est, X)
        scm.fetch_(cm, m)
        scb.fetch_ssh_bonds_(cb, m)
        for c in range(NCH):
            got = onsite_snapshot(cm.chains[c])
            assert all(np.array_equal(got[k], onsite_alone[c][k]) for k in got), (order, c)
            assert same_bits(snapshot(cb.chains[c]), bonds_alone[c]), (order, c)
        compare(cb.chains[1], wants[1], label="beside the on-site chain container, chain 1")
    finally:
        m.close()


def assert_close_to_single(chain, single, label):
    """max|chain path - single-configuration path| <= 2e-12 * max(1, max|single|) per key (the rule of
    tests/test_gpu_ssh_chain_measurements.assert_close_to_single for a correlation)."""
    a, b = snapshot(chain), snapshot(single)
    assert set(a) == set(b) == set(sbref.CORRS)
    worst = {}
    for k in b:
        assert not a[k].imag.any() and np.abs(b[k]).max() > 0
        worst[k] = np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max())
    print(label, {k: "%.2e (%.3g of the bound 2e-12, max|single| %.3g)" % (v, v / 2e-12, np.abs(b[k]).max()) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 2e-12, (label, k, v)


def test_one_chain_resident_agrees_with_the_single_configuration_path():
    from elphdynamics_amd import greens, ssh_bond_measurements as sb, ssh_chain_bond_measurements as scb
    host, R, MinvR, want = yardstick("hc3")
    m = build("hc3", device=True)
    try:
        assert np.array_equal(m.x, host.x)
        info = dict(CASES["hc3"][1], num_random_vectors=3)
        cb = scb.initialize_ssh_chain_bond_container(m, info, [""])
        c1 = sb.initialize_ssh_bond_container(m, info, "")
        est = greens.EstimateGreensFunction(m, nv=3)
        greens.set_vectors_(est, R, MinvR)
        scb.accumulate_ssh_bonds_(cb, m, est, m.x[None, :])
        sb.accumulate_ssh_bonds_(c1, m, est)                                # both containers live on the handle side by side
        scb.fetch_ssh_bonds_(cb, m)
        sb.fetch_ssh_bonds_(c1, m)
        compare(cb.chains[0], want, label="one chain resident, chain container")
        compare(c1, want, label="one chain resident, single-configuration container")
        assert_same_bits_as_single(snapshot(cb.chains[0]), snapshot(c1), "one chain resident")
    finally:
        m.close()


def test_production_shape_against_the_single_configuration_path():
    """Config E (16 x 16, L = 160, N_ph = 512), two chains with two vectors each, all three correlations time-dependent over all pairs:
    the tau-DFTs take their matrix-core forms and the batch changes the kernel chosen.  The reference is the device's
    single-configuration path (ssh_bond_measurements) on a second handle fed the same fields and vectors."""
    from elphdynamics_amd import configs, greens, models, ssh_bond_measurements as sb, ssh_chain_bond_measurements as scb
    m, m2 = configs.make_model("E"), configs.make_model("E")
    try:
        assert (m.Nsites, m.Ltau, m.Nph) == (256, 160, 512)
        nch = nv = 2
        rng = np.random.default_rng(16)
        X = np.stack([m.x * (1.0 - 0.3 * c) + 0.02 * (c + 1) * rng.standard_normal(m.Ndof) for c in range(nch)])
        assert X.min() < 0.0 < X.max()
        R, MinvR = rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim))
        info = dict(ALL3, num_random_vectors=nv)
        models.update_model_chains_(m, X)
        cb = scb.initialize_ssh_chain_bond_container(m, info, [""] * nch)
        est = greens.EstimateGreensFunction(m, nv=nv * nch)
        greens.set_vectors_(est, R, MinvR)
        scb.accumulate_ssh_bonds_(cb, m, est, X)
        scb.fetch_ssh_bonds_(cb, m)
        for c in range(nch):
            m2.x[:] = X[c]
            models.update_model_(m2)
            single = sb.initialize_ssh_bond_container(m2, info, "")
            est2 = greens.EstimateGreensFunction(m2, nv=nv)                 # (a new estimator drops the handle's previous accumulators)
            greens.set_vectors_(est2, R[c::nch], MinvR[c::nch])
            sb.accumulate_ssh_bonds_(single, m2, est2)
            sb.fetch_ssh_bonds_(single, m2)
            assert_close_to_single(cb.chains[c], single, "16 x 16 x 160, chain %d" % c)
    finally:
        m.close()
        m2.close()


@pytest.mark.parametrize("kpm", [False, True], ids=["plain", "kpm"])
def test_deck_in_lockstep_measured_end_to_end(kpm, tmp_path):
    """process_input_file(deck, nchains = 3), one step of the deck's dynamics for all chains, the device's own solve (1e-13) for all
    chains' vectors, then accumulate, process and write; the fetched sums against the direct sums on Gr.R, Gr.MinvR per chain, the
    written files of every chain's folder at 5e-9 absolute (half a unit of the 8 decimals written)."""
    from elphdynamics_amd import greens, langevin, preconditioners as pc, process_input as pi, ssh_chain_bond_measurements as scb, synth
    nch = 3
    deck = pi.read_deck(os.path.join(DECKS, "ssh_langevin_square_L4.toml"))
    info = dict(ALL3, num_random_vectors=3)
    info["CurrentCurrent"] = {"measure": True, "time_dependent": True, "pairs": [[2, 1], [1, 1], [1, 2]]}
    deck["measurements"] = {"num_random_vectors": 3}
    sim = pi.process_input_file(deck, nchains=nch)
    dyn, m = sim.simulation_dynamics, sim.model
    try:
        m.solver.tol, m.solver.maxiter = 1e-13, 20000
        m._push_solver()
        for c in range(nch):                                                # the deck's start is constant in tau
            dyn.X[c] = m.x * (0.8 + 0.1 * c) + 0.3 * synth.randn(61 + c, m.Ndof)
        dyn.push_()
        X0 = dyn.X.copy()
        dyn.device_rng_(31)
        P = pc.SymmetricKPMPreconditioner(m, n=min(20, m.Nsites), buf=0.05, c1=1.0, c2=1.0) if kpm else None
        langevin.evolve_(m, dyn, sim.fa, P)                                 # (pulls the fields)
        assert (dyn.flags == 0).all() and np.all(np.abs(dyn.X - X0).max(axis=1) > 0)
        X = dyn.X.copy()
        folders = [str(tmp_path / ("run%d" % c)) for c in range(nch)]
        for f in folders:
            os.mkdir(f)
        cb = scb.initialize_ssh_chain_bond_container(m, info, folders)
        scb.initialize_ssh_bond_folders_(cb)
        assert sim.Gr.nv == cb.n_rand_vecs * nch
        it, res, fl = greens.update_(sim.Gr, m, P, rng=np.random.default_rng(2))
        assert not fl.any() and it.min() > 0                                # the solve raised no flags
        scb.accumulate_ssh_bonds_(cb, m, sim.Gr, X)
        wants = [want_of(m, cb, sim.Gr.R, sim.Gr.MinvR, X, c) for c in range(nch)]
        scb.fetch_ssh_bonds_(cb, m)
        for c in range(nch):
            compare(cb.chains[c], wants[c], label="deck %s, chain %d" % ("kpm" if kpm else "plain", c))
        scb.process_ssh_bond_measurements_(cb, 1, m)
        scb.write_ssh_bond_measurements_(cb, m, 3)
        for c in range(nch):
            check_files(folders[c], wants[c], 3, m.dtau, 3)                 # V = bin_size * binomial(3, 2), the vectors of ONE chain
            assert set(cb.chains[c].intersite_susc) == {"BondPairSusc"}
    finally:
        m.close()


def raw_create(m, nchains, defs, which=0, pairs=(1, 1), Nbonds=None):
    """elph_ssh_bond_chains_create with one correlation (0 BondBond, 1 CurrentCurrent, 2 BondPairGreens) requested for one pair of bonds,
    straight through the C ABI."""
    import ctypes as C
    from elphdynamics_amd._lib import dptr, iptr
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    o1, o2, v = i32([d[0] for d in defs]), i32([d[1] for d in defs]), i32([k for d in defs for k in d[2]])
    flag = i32([int(k == which) for k in range(3)])
    if m.kind != 1:
        return m._lib.elph_ssh_bond_chains_create(m._h, nchains, len(defs), ip(o1), ip(o2), ip(v), 0, None, None, None, 0, None, None, ip(flag),
                                                  ip(flag), ip(flag), ip(i32(list(pairs))))
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)  # noqa: E731
    t, b2d, b2p, al, al2 = f64(m.t), i64(m.bond_to_definition), i64(m.bond_to_phonon), f64(m.alpha), f64(m.alpha2)
    return m._lib.elph_ssh_bond_chains_create(m._h, nchains, len(defs), ip(o1), ip(o2), ip(v), m.Nbonds if Nbonds is None else Nbonds, dptr(t),
                                              iptr(b2d), iptr(b2p), m.Nph, dptr(al), dptr(al2), ip(flag), ip(flag), ip(flag), ip(i32(list(pairs))))


def test_refusals_from_the_library(oracle):
    from elphdynamics_amd import _lib, chain_bond_measurements as cbm, configs, greens, measurements as ms, models
    from elphdynamics_amd import ssh_bond_measurements as sb, ssh_chain_bond_measurements as scb, ssh_chain_measurements as scm
    E_ARG, E_STATE, E_UNS, OK = _lib.ELPH_E_ARG, _lib.ELPH_E_STATE, _lib.ELPH_E_UNSUPPORTED, _lib.ELPH_OK
    case = "hc3"
    X, R, MinvR, wants = chain_yardstick(case)
    m, cb, est = lockstep(case, X, R, MinvR)
    try:
        lib = m._lib
        last = lambda: lib.elph_last_error().decode()  # noqa: E731
        defs = sbref.definitions(m)
        # before create: every other entry point names the missing call
        for call in (lambda: lib.elph_ssh_bond_chains_accumulate(m._h, _lib.dptr(X)), lambda: lib.elph_ssh_bond_chains_reset(m._h),
                     lambda: lib.elph_ssh_bond_chains_fetch(m._h, 0, None, None, None)):
            assert call() == E_STATE and "elph_ssh_bond_chains_create" in last(), last()
        # a chain count that is not the resident one: both counts are named
        for n in (0, 2, 4):
            assert raw_create(m, n, defs, which=1) == E_ARG and "for %d chains" % n in last() and "3 are resident" in last(), last()
        # the checks of elph_ssh_bond_create, worded as there
        for which, name in enumerate(sbref.CORRS):
            assert raw_create(m, 3, defs, which=which, pairs=(1, 4)) == E_ARG
            assert "bond 4" in last() and name in last() and "1..3" in last(), last()
        assert raw_create(m, 3, [(1, 3, (0, 0, 0))] + defs[1:], which=1) == E_ARG and "orbital 3" in last() and "definition 1" in last(), last()
        assert raw_create(m, 3, defs, which=1, Nbonds=m.Nbonds - 1) == E_ARG and "bonds" in last(), last()
        assert raw_create(m, 3, defs, which=0, Nbonds=m.Nbonds - 1) == OK     # ... which BondBond alone does not read
        # a refused create drops an earlier container
        assert lib.elph_ssh_bond_chains_reset(m._h) == OK
        assert raw_create(m, 2, defs) == E_ARG
        assert lib.elph_ssh_bond_chains_reset(m._h) == E_STATE and "elph_ssh_bond_chains_create" in last(), last()
        # fetch of chain nchains (and of chain -1)
        scb.accumulate_ssh_bonds_(cb, m, est, X)
        for chain in (3, -1):
            assert lib.elph_ssh_bond_chains_fetch(m._h, chain, None, None, None) == E_ARG and "outside 0..2" in last(), last()
        cc = np.zeros(2 * cb.chains[2].intersite_corr["CurrentCurrent"].position.size)
        assert lib.elph_ssh_bond_chains_fetch(m._h, 2, None, _lib.dptr(cc), None) == OK and cc[0] != 0
        # X = NULL with CurrentCurrent requested; allowed without it
        assert lib.elph_ssh_bond_chains_accumulate(m._h, None) == E_ARG and "X is null" in last(), last()
        assert raw_create(m, 3, defs, which=2) == OK and lib.elph_ssh_bond_chains_accumulate(m._h, None) == OK
        # the single-configuration entry points and modules keep refusing the resident chains, the Holstein twin the SSH model, the
        # on-site chain container the three names
        assert raw_single_create(m, defs, which=1) == E_UNS and "chains" in last(), last()
        with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
            sb.initialize_ssh_bond_container(m, ALL3, "")
        with pytest.raises(ms.UnsupportedMeasurement, match="SSH"):
            cbm.initialize_chain_bond_container(m, {"BondBond": TD}, [""] * NCH)
        with pytest.raises(ms.UnsupportedMeasurement, match="BondBond"):
            scm.initialize_ssh_chain_measurements_container(m, {"BondBond": TD}, [""] * NCH)
        # an estimator whose vectors are not a multiple of the chains: 4 vectors, 3 chains (a new estimator drops the device side)
        est4 = greens.EstimateGreensFunction(m, nv=4)
        assert lib.elph_ssh_bond_chains_reset(m._h) == E_STATE
        assert raw_create(m, 3, defs, which=1) == OK
        assert lib.elph_ssh_bond_chains_accumulate(m._h, _lib.dptr(X)) == E_STATE and "4 vectors" in last() and "3 resident chains" in last(), last()
        # accumulate before any vectors
        est9 = greens.EstimateGreensFunction(m, nv=9)
        assert raw_create(m, 3, defs, which=1) == OK
        assert lib.elph_ssh_bond_chains_accumulate(m._h, _lib.dptr(X)) == E_STATE and "no vectors" in last(), last()
        greens.set_vectors_(est9, R, MinvR)
        assert lib.elph_ssh_bond_chains_accumulate(m._h, _lib.dptr(X)) == OK
        # update_model_ drops the chains: the container was made for three
        models.update_model_(m)
        assert lib.elph_ssh_bond_chains_accumulate(m._h, _lib.dptr(X)) == E_STATE and "3 chains" in last() and "1 are resident" in last(), last()
        assert lib.elph_ssh_bond_chains_reset(m._h) == OK                   # ... and is still there
        mulM_still_right(oracle, m)
        # a new estimator has dropped the device side; the container notices and makes it again for the new one
        models.update_model_chains_(m, X)
        scb.accumulate_ssh_bonds_(cb, m, est9, X)
        scb.fetch_ssh_bonds_(cb, m)
        for c in range(NCH):
            compare(cb.chains[c], wants[c], label="after a new estimator, chain %d" % c)
        del est4
    finally:
        m.close()
    # CurrentCurrent with Nbonds != n_def * ncells (a bond removed as a duplicate): refused, BondBond alone is measured
    norb, dims, sdefs, L = sc.SHAPES["cu3x2x2"]
    s = smc.build_model(norb, dims, sdefs, L, seed=5)
    try:
        assert s.Nbonds != s.nbonds * s.lattice.ncells
        nch, nv = 2, 2
        rng = np.random.default_rng(6)
        Xs = np.stack([chain_field(s, 50 + c) for c in range(nch)])
        R2, M2 = rng.standard_normal((nv * nch, s.Ndim)), rng.standard_normal((nv * nch, s.Ndim))
        models.update_model_chains_(s, Xs)
        est = greens.EstimateGreensFunction(s, nv=nv * nch)
        greens.set_vectors_(est, R2, M2)
        c3 = scb.initialize_ssh_chain_bond_container(s, dict(ALL3, num_random_vectors=nv), [""] * nch)
        with pytest.raises(_lib.ElphError) as e:
            scb.accumulate_ssh_bonds_(c3, s, est, Xs)
        msg = str(e.value)
        assert e.value.code == E_UNS and "CurrentCurrent" in msg and "%d bonds" % s.Nbonds in msg and "%d cells" % s.lattice.ncells in msg, msg
        assert s._lib.elph_ssh_bond_chains_reset(s._h) == E_STATE           # nothing was left behind
        mulM_still_right(oracle, s)
        bb = scb.initialize_ssh_chain_bond_container(s, {"BondBond": TD, "num_random_vectors": nv}, [""] * nch)
        scb.accumulate_ssh_bonds_(bb, s, est, Xs)
        scb.fetch_ssh_bonds_(bb, s)
        for c in range(nch):
            want = sbref.measure(R2[c::nch], M2[c::nch], Xs[c], dict(L=L, ns=norb, dims=dims), sbref.definitions(s), request_of(bb.chains[c]))
            compare(bb.chains[c], want, label="cu3x2x2 BondBond, chain %d" % c)
    finally:
        s.close()
    # the estimator first; one chain resident is accepted; a sharded handle (one rank owning the whole lattice)
    e = configs.make_model("e")
    try:
        edefs = sbref.definitions(e)
        assert raw_create(e, 1, edefs, which=1) == E_STATE and "greens" in e._lib.elph_last_error().decode().lower()
        greens.EstimateGreensFunction(e, nv=2)
        assert raw_create(e, 1, edefs, which=1) == OK
        import ctypes as C
        key = (C.c_ubyte * 64)()
        assert e._lib.elph_shard_create(e._h, 0, 1, 0, e.Nsites, 0, 0, 0, 0, 0, None, C.cast(key, C.c_void_p)) == OK
        assert raw_create(e, 1, edefs, which=1) == E_UNS and "sharded" in e._lib.elph_last_error().decode()
        assert e._lib.elph_ssh_bond_chains_reset(e._h) == E_STATE           # the refused create dropped the container made above
    finally:
        e.close()
    # a Holstein handle
    hm = configs.make_model("w")
    try:
        greens.EstimateGreensFunction(hm, nv=2)
        assert raw_create(hm, 1, [(1, 2, (0, 0, 0))]) == E_UNS and "SSH only" in hm._lib.elph_last_error().decode()
        with pytest.raises(ms.UnsupportedMeasurement, match="Holstein"):
            scb.initialize_ssh_chain_bond_container(hm, {"BondBond": TD}, [""])
        mulM_still_right(oracle, hm)
    finally:
        hm.close()
