"""GPU parity of the SSH measurements of resident chains (csrc/ssh_measure.hip through elphdynamics_amd/ssh_chain_measurements.py):
every chain's container against the direct-sum restatement tests/ssh_measurements_reference.py evaluated on that chain's field, mu row and
vectors [v * nchains + c], with the bounds of tests/test_gpu_ssh_measurements.py (its `compare`, imported: 1e-12 on the correlations, 1e-12
of the yardstick on the reduced scalars, imaginary parts exactly zero).  A chain's sums have exactly the terms of the single-configuration
sums, so that bound carries over.

Vectors go in through greens.set_vectors_ (no solve) unless a test says otherwise.  Three chains with three vectors each: three pairs,
neither count a power of two, so a chain-major / vector-major mix-up cannot pass.  The chains' fields follow the recipe of
ssh_measurement_cases.build_model (synth.phonon_field, mean removed, the same scaling rule or x_median), a seed per chain.  Against the
device's single-configuration path (ssh_measurements.accumulate_) the bound is the rule of
tests/test_gpu_chain_measurements.assert_close_to_single, 2e-12 * max(1, |single|), applied to every number of an SSH container: each
side meets 1e-12 of the direct sum in the suite.

Worst deviations measured on an MI355X, in the units of each bound (a bound of 1e-12 resp. 2e-12):
  one chain resident (hc3), chain container against the single-configuration container: 0 on every key (the same bits)
  16 x 16, L = 160 (config E), two chains against the single-configuration path: 0 on every key (the same bits)"""
import copy
import os

import numpy as np
import pytest

import ssh_cases as sc
import ssh_measurement_cases as smc
import ssh_measurements_reference as ref
from test_gpu_measurements import assert_same_bits_as_single, parse
from test_gpu_ssh_measurements import compare, raw_create as raw_single_create, snapshot

pytestmark = pytest.mark.gpu

DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decks")
NCH = NV = 3


def chain_field(m, seed, x_median=None):
    """A field of model m by the recipe of ssh_measurement_cases.build_model: rough, mean removed, both signs, scaled the same way."""
    from elphdynamics_amd import synth
    x = synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, omega=sc.OMEGA_MEAN, lam=0.0, seed=seed)
    x = x - x.mean()
    if x_median is not None:
        x = x * (x_median / np.median(np.abs(x)))
    else:
        X = x.reshape(m.Nph, m.Ltau)
        worst = np.max(np.abs(m.alpha)[:, None] * np.abs(X) + np.abs(m.alpha2)[:, None] * X ** 2)
        x = x * min(1.0, 0.5 * np.min(np.abs(m.t)) / worst)
    assert x.min() < 0.0 < x.max()
    return x


def chain_inputs(m, nch, nv, seed, x_median=None):
    """(X (nch, Ndof) a field per chain, mu (nch, Nsites) a distinct row per chain, R, MinvR (nv * nch, Ndim))."""
    rng = np.random.default_rng(seed)
    X = np.stack([chain_field(m, seed + 1 + c, x_median) for c in range(nch)])
    mu = np.stack([m.mu + 0.05 * (c + 1) + 0.1 * rng.standard_normal(m.Nsites) for c in range(nch)])
    return X, mu, rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim))


def lockstep(case, nch, nv, seed, inputs=None):
    """The model of case `case` with nch chains resident, its chain container and estimator (vectors set), and the inputs."""
    from elphdynamics_amd import greens, models, ssh_chain_measurements as scm
    m, table = smc.build_case(case)
    X, mu, R, MinvR = inputs or chain_inputs(m, nch, nv, seed, smc.CASES[case][6])
    models.update_model_chains_(m, X)
    cm = scm.initialize_ssh_chain_measurements_container(m, dict(table, num_random_vectors=nv), [""] * nch)
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    greens.set_vectors_(est, R, MinvR)
    return m, cm, est, X, mu


def want_of(m, cm, R, MinvR, X, mu, c):
    """The direct sums of chain c: its field, its mu row, its vectors."""
    nch = cm.nchains
    return ref.measure(R[c::nch], MinvR[c::nch], X[c], dict(smc.ref_par(m), mu=mu[c]), smc.request_of(cm.chains[c]))


def add(a, b):
    """The reference sums of two accumulations."""
    out = copy.deepcopy(a)
    for grp in ("glob", "onsite", "inter", "corr"):
        for k in out[grp]:
            out[grp][k] = a[grp][k] + b[grp][k]
    for grp in ("glob", "onsite", "inter"):
        for k in out["abs"][grp]:
            out["abs"][grp][k] = a["abs"][grp][k] + b["abs"][grp][k]
    return out


def same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def assert_close_to_single(chain, single, label):
    """|chain path - single-configuration path| <= 2e-12 * max(1, |single|): the scalars one by one, a correlation in its max norm (the
    rule of tests/test_gpu_chain_measurements.assert_close_to_single over every number of an SSH container)."""
    a, b = snapshot(chain), snapshot(single)
    assert set(a) == set(b)
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
    return worst


@pytest.mark.parametrize("case", ["tri4_Lt7", "hc3", "cubic3x2x2", "sq12x6"])
def test_every_chain_matches_the_direct_sums_of_its_own_inputs(case):
    from elphdynamics_amd import ssh_chain_measurements as scm
    host, table = smc.build_case(case, device=False)
    host._nchains = NCH
    X, mu, R, MinvR = chain_inputs(host, NCH, NV, 41, smc.CASES[case][6])
    cmh = scm.initialize_ssh_chain_measurements_container(host, dict(table, num_random_vectors=NV), [""] * NCH)
    wants = [want_of(host, cmh, R, MinvR, X, mu, c) for c in range(NCH)]
    assert len({tuple(w["inter"]["x"]) for w in wants}) == NCH and len({w["glob"]["mu"] for w in wants}) == NCH
    if case == "sq12x6":                                                    # before any GPU call: in every chain some, not all, t' change sign
        for w in wants:
            assert np.all(w["inter"]["sign_switch"] / 3 > 0.0) and np.all(w["inter"]["sign_switch"] / 3 < 1.0)
    if case == "tri4_Lt7":
        assert host.nph == 3 > host.lattice.norbits and host.Ltau == 7
    m, cm, est, _, _ = lockstep(case, NCH, NV, 41, inputs=(X, mu, R, MinvR))
    try:
        assert np.array_equal(m.t, host.t) and np.array_equal(m.alpha2, host.alpha2) and np.array_equal(m.omega, host.omega)
        scm.accumulate_(cm, m, est, X, mu=mu)
        scm.fetch_(cm, m)
        for c in range(NCH):
            compare(cm.chains[c], wants[c], label="%s chain %d" % (case, c))
    finally:
        m.close()


def test_two_accumulates_add_up_fetch_does_not_clear_reset_zeroes():
    from elphdynamics_amd import greens, ssh_chain_measurements as scm
    m, cm, est, X, mu = lockstep("hc3", NCH, NV, seed=5)
    try:
        scm.accumulate_(cm, m, est, X, mu=mu)
        first = [want_of(m, cm, est.R, est.MinvR, X, mu, c) for c in range(NCH)]
        X2, mu2, R2, MinvR2 = chain_inputs(m, NCH, NV, seed=77)
        greens.set_vectors_(est, R2, MinvR2)
        scm.accumulate_(cm, m, est, X2, mu=mu2)                             # the tuners moved mu in between: the second sums take the new rows
        scm.fetch_(cm, m)
        for c in range(NCH):
            compare(cm.chains[c], add(first[c], want_of(m, cm, R2, MinvR2, X2, mu2, c)), label="two accumulates, chain %d" % c)
        two = [snapshot(c) for c in cm.chains]
        scm.accumulate_(cm, m, est, X2)                                     # no mu given: the device keeps the rows it has
        scm.fetch_(cm, m)
        for c in range(NCH):
            assert abs(snapshot(cm.chains[c])["g:mu"][0] - two[c]["g:mu"][0] - 3 * mu2[c].mean()) < 1e-12
            assert np.abs(snapshot(cm.chains[c])["o:mu"] - two[c]["o:mu"] - 3 * mu2[c].reshape(-1, 2).mean(axis=0)).max() < 1e-12
        once = [snapshot(c) for c in cm.chains]
        scm.fetch_(cm, m)                                                   # fetch does not clear
        assert all(same_bits(a, snapshot(c)) for a, c in zip(once, cm.chains))
        scm.reset_measurements_(cm, m)
        scm.fetch_(cm, m)
        for c in cm.chains:
            assert all(not v.any() for v in snapshot(c).values())           # exact zeros
        # two accumulations of the same inputs are twice one, to the bit (a + a is exact)
        scm.accumulate_(cm, m, est, X2)
        scm.fetch_(cm, m)
        one = [snapshot(c) for c in cm.chains]
        scm.accumulate_(cm, m, est, X2)
        scm.fetch_(cm, m)
        for a, c in zip(one, cm.chains):
            b = snapshot(c)
            assert all(np.array_equal(b[k], 2 * a[k]) for k in a)
    finally:
        m.close()


def test_chains_do_not_leak_into_one_another_and_runs_repeat_bit_for_bit():
    from elphdynamics_amd import greens, ssh_chain_measurements as scm
    m, cm, est, X, mu = lockstep("hc3", NCH, NV, seed=8)
    try:
        scm.accumulate_(cm, m, est, X, mu=mu)
        scm.fetch_(cm, m)
        one = [snapshot(c) for c in cm.chains]
        # the same inputs again after a reset: the same bits
        scm.reset_measurements_(cm, m)
        scm.accumulate_(cm, m, est, X)
        scm.fetch_(cm, m)
        assert all(same_bits(a, snapshot(c)) for a, c in zip(one, cm.chains))
        # only chain 1's field and vectors change
        X2, _, R2, MinvR2 = chain_inputs(m, NCH, NV, seed=99)
        Xn, Rn, Mn = X.copy(), est.R.copy(), est.MinvR.copy()
        Xn[1], Rn[1::3], Mn[1::3] = X2[1], R2[1::3], MinvR2[1::3]
        greens.set_vectors_(est, Rn, Mn)
        scm.reset_measurements_(cm, m)
        scm.accumulate_(cm, m, est, Xn)
        scm.fetch_(cm, m)
        two = [snapshot(c) for c in cm.chains]
        assert same_bits(one[0], two[0]) and same_bits(one[2], two[2])
        moved = [k for k in one[1] if not np.array_equal(one[1][k], two[1][k])]
        assert set(moved) >= {"i:x", "i:x2", "i:phonon_ke", "i:el_ke", "i:elph_energy", "g:density", "g:Nsqr", "o:density", "c:Greens",
                              "c:PhononGreens"}, moved
        assert "g:mu" not in moved and "o:mu" not in moved                  # mu was not touched
        compare(cm.chains[1], want_of(m, cm, Rn, Mn, Xn, mu, 1), label="chain 1 after its inputs changed")
    finally:
        m.close()


def test_one_chain_resident_agrees_with_the_single_configuration_path():
    from elphdynamics_amd import greens, ssh_chain_measurements as scm, ssh_measurements as sm
    m, table = smc.build_case("hc3")
    try:
        info = dict(table, num_random_vectors=3)
        cm = scm.initialize_ssh_chain_measurements_container(m, info, [""])
        c1 = sm.initialize_ssh_measurements_container(m, info, "")
        est = greens.EstimateGreensFunction(m, nv=3)
        rng = np.random.default_rng(1)
        greens.set_vectors_(est, rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim)))
        scm.accumulate_(cm, m, est, m.x[None, :])
        sm.accumulate_(c1, m, est)                                          # both containers live on the handle side by side
        scm.fetch_(cm, m)
        sm.fetch_(c1, m)
        want = ref.measure(est.R, est.MinvR, m.x, smc.ref_par(m), smc.request_of(c1))
        compare(cm.chains[0], want, label="one chain resident, chain container")
        compare(c1, want, label="one chain resident, single-configuration container")
        assert_same_bits_as_single(snapshot(cm.chains[0]), snapshot(c1), "one chain resident")
    finally:
        m.close()


def test_production_shape_against_the_single_configuration_path():
    """Config E (16 x 16, L = 160, N_ph = 512), two chains with two vectors each, all five correlations time-dependent: the tau-DFTs take
    their matrix-core forms and the batch changes the kernel chosen.  The reference is the device's single-configuration path on a second
    handle fed the same fields, mu and vectors."""
    from elphdynamics_amd import configs, greens, models, ssh_chain_measurements as scm, ssh_measurements as sm
    m, m2 = configs.make_model("E"), configs.make_model("E")
    try:
        assert (m.Nsites, m.Ltau, m.Nph) == (256, 160, 512)
        nch = nv = 2
        rng = np.random.default_rng(16)
        X = np.stack([m.x * (1.0 - 0.3 * c) + 0.02 * (c + 1) * rng.standard_normal(m.Ndof) for c in range(nch)])
        assert X.min() < 0.0 < X.max()
        mu = np.stack([m.mu + 0.05 * (c + 1) + 0.1 * rng.standard_normal(m.Nsites) for c in range(nch)])
        R, MinvR = rng.standard_normal((nv * nch, m.Ndim)), rng.standard_normal((nv * nch, m.Ndim))
        info = dict(smc.ALL_TD, num_random_vectors=nv)
        models.update_model_chains_(m, X)
        cm = scm.initialize_ssh_chain_measurements_container(m, info, [""] * nch)
        est = greens.EstimateGreensFunction(m, nv=nv * nch)
        greens.set_vectors_(est, R, MinvR)
        scm.accumulate_(cm, m, est, X, mu=mu)
        scm.fetch_(cm, m)
        for c in range(nch):
            m2.x[:] = X[c]
            m2.mu[:] = mu[c]
            models.update_model_(m2)
            single = sm.initialize_ssh_measurements_container(m2, info, "")
            est2 = greens.EstimateGreensFunction(m2, nv=nv)                 # (a new estimator drops the handle's previous container)
            greens.set_vectors_(est2, R[c::nch], MinvR[c::nch])
            sm.accumulate_(single, m2, est2)
            sm.fetch_(single, m2)
            assert snapshot(single)["i:x2"].min() > 0 and np.abs(snapshot(single)["c:PhononGreens"]).max() > 0
            assert_close_to_single(cm.chains[c], single, "16 x 16 x 160, chain %d" % c)
    finally:
        m.close()
        m2.close()


@pytest.mark.parametrize("kpm", [False, True], ids=["plain", "kpm"])
def test_deck_in_lockstep_measured_end_to_end(kpm, tmp_path):
    """process_input_file(deck, nchains = 3) with a [measurements] table, one step of the deck's dynamics for all chains, then
    make_measurements_ with the device's own solve on the chains' fields; the written files against the reference at 5e-9 absolute (half
    a unit of the 8 decimals written)."""
    from elphdynamics_amd import langevin, preconditioners as pc, process_input as pi, ssh_chain_measurements as scm, synth
    nch = 3
    deck = pi.read_deck(os.path.join(DECKS, "ssh_langevin_square_L4.toml"))
    info = dict(smc.ALL_TD, num_random_vectors=3)
    info["DenDen"] = {"measure": True, "time_dependent": True, "pairs": [[1, 1]]}
    info["PhononGreens"] = {"measure": True, "time_dependent": True, "pairs": [[2, 1], [1, 1]]}
    deck["measurements"] = info
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
        cm = scm.initialize_ssh_chain_measurements_container(m, sim.input["measurements"], folders)
        scm.initialize_measurement_folders_(cm)
        assert sim.Gr.nv == cm.n_rand_vecs * nch
        it, res, fl = scm.make_measurements_(cm, m, sim.Gr, X, 1, P=P, rng=np.random.default_rng(2))
        assert not fl.any() and it.min() > 0                                # the solve raised no flags
        mu = np.tile(m.mu, (nch, 1))
        wants = [want_of(m, cm, sim.Gr.R, sim.Gr.MinvR, X, mu, c) for c in range(nch)]
        scm.fetch_(cm, m)
        for c in range(nch):
            compare(cm.chains[c], wants[c], label="deck %s, chain %d" % ("kpm" if kpm else "plain", c))
        bin_size = 1
        scm.process_measurements_(cm, bin_size, m)
        scm.write_measurements_(cm, m, 3)
        V = bin_size * 3                                                    # binomial(3, 2), the vectors of ONE chain
        susc_of = {"PairGreens": "PairSusc", "DenDen": "ChargeSusc", "SpinSpin": "SpinSusc"}
        for c, (d, want) in enumerate(zip(folders, wants)):
            rows = dict(ln.split() for ln in open(os.path.join(d, "global_measurements_f", "global_measurements_00003.out")).read().splitlines())
            for k in ref.GLOBAL_KEYS:
                assert abs(float(rows[k]) - want["glob"][k] / V) <= 5e-9 + 1e-12 * want["abs"]["glob"][k], (c, k)
            for ln in open(os.path.join(d, "onsite_measurements_f", "onsite_measurements_00003.out")).read().splitlines()[1:]:
                k, o, v = ln.split()
                assert abs(float(v) - want["onsite"][k][int(o) - 1] / V) <= 5e-9, (c, k, o)
            seen = set()
            for ln in open(os.path.join(d, "intersite_measurements_f", "intersite_measurements_00003.out")).read().splitlines()[1:]:
                k, b, v = ln.split()
                seen.add(k)
                assert abs(float(v) - want["inter"][k][int(b) - 1] / V) <= 5e-9, (c, k, b)
            assert seen == set(ref.INTERSITE_KEYS)
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
            assert set(cm.chains[c].onsite_susc) == set(susc_of.values()) and set(want["corr"]) == set(smc.ALL_TD)
    finally:
        m.close()


def raw_create(m, nchains, which=0, pairs=(1, 1), nph=None, Nph=None, mu="rows", omega="model", b2p=None, sites=None):
    """elph_ssh_meas_chains_create with one correlation requested for one pair, straight through the C ABI."""
    import ctypes as C
    from elphdynamics_amd import ssh_measurements as sm
    from elphdynamics_amd._lib import dptr, iptr
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    flag = i32([int(k == which) for k in range(5)])
    prs = i32(list(pairs))
    rows = f64(np.tile(m.mu, (max(nchains, 1), 1)))
    if m.kind != 1:
        return m._lib.elph_ssh_meas_chains_create(m._h, nchains, dptr(rows), 0.1, 0, 0, None, None, None, None, 0, 0, None, None, None, ip(flag),
                                                  ip(flag), ip(flag), ip(prs))
    s, t = sm.bond_arrays(m)
    s = s if sites is None else np.ascontiguousarray(sites, dtype=np.int64)
    b2d = np.ascontiguousarray(m.bond_to_definition, dtype=np.int64)
    b2p = np.ascontiguousarray(m.bond_to_phonon if b2p is None else b2p, dtype=np.int64)
    om, al, al2 = f64(m.omega), f64(m.alpha), f64(m.alpha2)
    return m._lib.elph_ssh_meas_chains_create(m._h, nchains, dptr(rows) if mu == "rows" else None, m.dtau, m.Nbonds, m.nbonds, iptr(s), dptr(t),
                                              iptr(b2d), iptr(b2p), m.Nph if Nph is None else Nph, m.nph if nph is None else nph,
                                              dptr(om) if omega == "model" else None, dptr(al), dptr(al2), ip(flag), ip(flag), ip(flag), ip(prs))


def test_refusals_from_the_library():
    from elphdynamics_amd import _lib, configs, greens, models, ssh_chain_measurements as scm, ssh_measurements as sm
    m, cm, est, X, mu = lockstep("hc3", NCH, NV, seed=2)
    try:
        lib = m._lib
        last = lambda: lib.elph_last_error().decode()  # noqa: E731
        E_ARG, E_STATE, E_UNS, OK = _lib.ELPH_E_ARG, _lib.ELPH_E_STATE, _lib.ELPH_E_UNSUPPORTED, _lib.ELPH_OK
        scal = np.zeros(3 + 3 * 2 + 8 * 3)
        # before create: every other entry point names the missing call
        assert lib.elph_ssh_meas_chains_accumulate(m._h, _lib.dptr(X)) == E_STATE and "elph_ssh_meas_chains_create" in last()
        assert lib.elph_ssh_meas_chains_set_mu(m._h, _lib.dptr(mu)) == E_STATE and "elph_ssh_meas_chains_create" in last()
        assert lib.elph_ssh_meas_chains_fetch(m._h, 0, _lib.dptr(scal), None, None, None, None, None) == E_STATE and "elph_ssh_meas_chains_create" in last()
        assert lib.elph_ssh_meas_chains_reset(m._h) == E_STATE and "elph_ssh_meas_chains_create" in last()
        # a chain count that is not the resident one: both counts are named
        for n in (0, 2, 4):
            assert raw_create(m, n) == E_ARG and "for %d chains" % n in last() and "3 are resident" in last(), last()
        # null arrays, bond and phonon indices out of range, as elph_ssh_meas_create words them
        assert raw_create(m, 3, mu=None) == E_ARG and "null parameter array" in last(), last()
        assert raw_create(m, 3, omega=None) == E_ARG and "null phonon array" in last(), last()
        bad = np.array(m.bond_to_phonon, dtype=np.int64)
        bad[1] = m.Nph + 1
        assert raw_create(m, 3, b2p=bad) == E_ARG and "bond 2 carries phonon %d" % (m.Nph + 1) in last(), last()
        sites = sm.bond_arrays(m)[0].copy()
        sites[0, 1] = m.Nsites + 1
        assert raw_create(m, 3, sites=sites) == E_ARG and "bond 1 joins site %d" % (m.Nsites + 1) in last(), last()
        assert raw_create(m, 3, which=4, pairs=(1, 4)) == E_ARG and "phonon type 4" in last() and "PhononGreens" in last() and "1..3" in last(), last()
        assert raw_create(m, 3, which=0, pairs=(3, 1)) == E_ARG and "orbital 3" in last(), last()
        # PhononGreens with a field that does not reshape to (Ltau, L1, L2, L3, nph), worded as in the single path
        assert raw_create(m, 3, which=4, nph=2) == E_UNS and "PhononGreens needs Nph = nph x ncells" in last(), last()
        assert raw_create(m, 3, which=0, nph=2) == OK                       # ... which Greens alone does not need
        # every refusal left the handle without the container
        assert raw_create(m, 2) == E_ARG
        assert lib.elph_ssh_meas_chains_accumulate(m._h, _lib.dptr(X)) == E_STATE and "elph_ssh_meas_chains_create" in last()
        # fetch of chain nchains (and of chain -1)
        scm.accumulate_(cm, m, est, X, mu=mu)
        for chain in (3, -1):
            assert lib.elph_ssh_meas_chains_fetch(m._h, chain, _lib.dptr(scal), None, None, None, None, None) == E_ARG
            assert "outside 0..2" in last(), last()
        assert lib.elph_ssh_meas_chains_fetch(m._h, 2, _lib.dptr(scal), None, None, None, None, None) == OK and scal[0] != 0
        # the single-configuration entry points keep refusing the resident chains
        assert raw_single_create(m) == E_UNS and "chains" in last(), last()
        # an estimator whose vectors are not a multiple of the chains: 4 vectors, 3 chains (a new estimator drops the container)
        est4 = greens.EstimateGreensFunction(m, nv=4)
        assert lib.elph_ssh_meas_chains_reset(m._h) == E_STATE
        assert raw_create(m, 3) == OK
        assert lib.elph_ssh_meas_chains_accumulate(m._h, _lib.dptr(X)) == E_STATE
        assert "4 vectors" in last() and "3 resident chains" in last(), last()
        # accumulate before any vectors
        est6 = greens.EstimateGreensFunction(m, nv=6)
        assert raw_create(m, 3) == OK
        assert lib.elph_ssh_meas_chains_accumulate(m._h, _lib.dptr(X)) == E_STATE and "no vectors" in last(), last()
        greens.set_vectors_(est6, np.ones((6, m.Ndim)), np.ones((6, m.Ndim)))
        assert lib.elph_ssh_meas_chains_accumulate(m._h, _lib.dptr(X)) == OK
        # update_model_ drops the chains: the container was made for three
        models.update_model_(m)
        assert lib.elph_ssh_meas_chains_accumulate(m._h, _lib.dptr(X)) == E_STATE
        assert "3 chains" in last() and "1 are resident" in last(), last()
        assert lib.elph_ssh_meas_chains_reset(m._h) == OK                   # ... and is still there
        # a new estimator drops the device side; the container notices and makes it again for the new one
        models.update_model_chains_(m, X)
        est9 = greens.EstimateGreensFunction(m, nv=9)
        greens.set_vectors_(est9, est.R, est.MinvR)
        scm.accumulate_(cm, m, est9, X)
        scm.fetch_(cm, m)
        for c in range(3):
            compare(cm.chains[c], want_of(m, cm, est9.R, est9.MinvR, X, np.tile(m.mu, (3, 1)), c), label="after a new estimator, chain %d" % c)
        del est4
    finally:
        m.close()
    # the estimator first
    s = configs.make_model("e")
    try:
        assert raw_create(s, 1) == _lib.ELPH_E_STATE and "greens" in s._lib.elph_last_error().decode().lower()
        greens.EstimateGreensFunction(s, nv=2)
        assert raw_create(s, 1) == _lib.ELPH_OK                             # one chain resident is accepted
        with pytest.raises(scm.UnsupportedMeasurement, match="BondBond"):
            scm.initialize_ssh_chain_measurements_container(s, {"BondBond": {"measure": True}}, [""])
        # a sharded handle (one rank owning the whole lattice); a slab handle is the library's own and is not reachable from outside,
        # and the LDS limit of PhononGreens (2560 cells) lies beyond the estimator's own (2048 sites), which create needs first
        import ctypes as C
        key = (C.c_ubyte * 64)()
        assert s._lib.elph_shard_create(s._h, 0, 1, 0, s.Nsites, 0, 0, 0, 0, 0, None, C.cast(key, C.c_void_p)) == _lib.ELPH_OK
        assert raw_create(s, 1) == _lib.ELPH_E_UNSUPPORTED and "sharded" in s._lib.elph_last_error().decode()
        assert s._lib.elph_ssh_meas_chains_reset(s._h) == _lib.ELPH_E_STATE  # the refused create dropped the container made above
    finally:
        s.close()
    # a Holstein handle: here, and still the SSH model in the Holstein twin
    hm = configs.make_model("w")
    try:
        greens.EstimateGreensFunction(hm, nv=2)
        assert raw_create(hm, 1) == _lib.ELPH_E_UNSUPPORTED and "SSH only" in hm._lib.elph_last_error().decode()
        with pytest.raises(scm.UnsupportedMeasurement, match="Holstein"):
            scm.initialize_ssh_chain_measurements_container(hm, smc.ALL_TD, [""])
    finally:
        hm.close()
