"""GPU parity of the device-resident SSH measurements (csrc/ssh_measure.hip through elphdynamics_amd/ssh_measurements.py) against the
direct-sum restatement tests/ssh_measurements_reference.py.

Vectors go in through greens.set_vectors_ (no solve) with n_v = 3; t, alpha, alpha2, omega depend on the bond, mu on the site, x is a
rough synthetic field (tests/ssh_measurement_cases.py).  Bounds, those of tests/test_gpu_measurements.py (the sums and tables have the same
structure, and no case here has more terms per sum than its small cases):
  * correlation arrays: max|got - ref| < 1e-12 * max(1, max|ref|);
  * reduced scalars: |got - ref| < 1e-12 * (sum of the absolute values of the terms, same normalisation);
  * imaginary parts: exactly zero.
End to end the device's own solve (1e-13) provides the vectors and the reference is evaluated on est.R, est.MinvR: same bounds; the written
files are compared at 5e-9 absolute, half a unit of the 8 decimals written."""
import os

import numpy as np
import pytest

import ssh_cases as sc
import ssh_measurement_cases as smc
import ssh_measurements_reference as ref
from test_gpu_measurements import in_units, parse
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decks")


def snapshot(c):
    """The container's numbers as one dict of arrays (copies)."""
    out = {"g:" + k: np.array([v]) for k, v in c.global_meas.items()}
    out.update({"o:" + k: v.copy() for k, v in c.onsite_meas.items()})
    out.update({"i:" + k: v.copy() for k, v in c.intersite_meas.items()})
    out.update({"c:" + k: v.position.copy() for k, v in list(c.onsite_corr.items()) + list(c.intersite_corr.items())})
    return out


def compare(c, want, scale=1.0, label=""):
    """Every accumulator of the (fetched, un-normalised) container against the reference `want`, both for `scale` accumulations."""
    tol = 1e-12
    worst = {}
    for k in ref.GLOBAL_KEYS:
        got, w, yard = c.global_meas[k], scale * want["glob"][k], scale * want["abs"]["glob"][k]
        assert got.imag == 0
        worst["g:" + k] = in_units(abs(got.real - w), yard)
    for tag, group, keys, name in (("o:", c.onsite_meas, ref.ONSITE_KEYS, "onsite"), ("i:", c.intersite_meas, ref.INTERSITE_KEYS, "inter")):
        assert tuple(group) == keys
        for k in keys:
            got, w, yard = group[k], scale * want[name][k], scale * want["abs"][name][k]
            assert not got.imag.any()
            worst[tag + k] = in_units(np.abs(got.real - w), yard)
    cw = {}
    for k, corr in list(c.onsite_corr.items()) + list(c.intersite_corr.items()):
        w = scale * want["corr"][k]
        assert corr.position.shape == w.shape, k
        assert not corr.position.imag.any(), k                              # exact zeros
        cw[k] = np.abs(corr.position.real - w).max() / max(1.0, np.abs(w).max())
    print(label, "scalars (units of the yardstick):", {k: "%.2e" % v for k, v in worst.items()}, "correlations:",
          {k: "%.2e" % v for k, v in cw.items()}, "bound %.2e" % tol)
    for k, v in worst.items():
        assert v < tol, (label, k, v)
    for k, v in cw.items():
        assert v < 1e-12, (label, k, v)


@pytest.mark.parametrize("case", list(smc.CASES))
def test_accumulators_match_direct_sums(case):
    from elphdynamics_amd import greens, ssh_measurements as sm
    host, table = smc.build_case(case, device=False)
    rng = np.random.default_rng(len(case))
    R, X = rng.standard_normal((3, host.Ndim)), rng.standard_normal((3, host.Ndim))
    info = dict(table, num_random_vectors=3)
    c = sm.initialize_ssh_measurements_container(host, info, "")
    want = ref.measure(R, X, host.x, smc.ref_par(host), smc.request_of(c))
    if case == "sq12x6":                                                    # before any GPU call: some, not all, t' change sign
        assert np.all(want["inter"]["sign_switch"] / 3 > 0.0) and np.all(want["inter"]["sign_switch"] / 3 < 1.0)
        assert host.t[72:].max() < 0.0
    if case == "psq6":
        assert host.nph == 1 and host.phonon_to_bond[0] != 1 and not host.bond_to_phonon[0]
    if case == "tri4_Lt7":
        assert host.nph == 3 > host.lattice.norbits
    m, _ = smc.build_case(case)
    try:
        assert np.array_equal(m.x, host.x) and np.array_equal(m.t, host.t) and np.array_equal(m.alpha2, host.alpha2)
        est = greens.EstimateGreensFunction(m, nv=3)
        greens.set_vectors_(est, R, X)
        greens.setup_(est, 1, 2)
        before = [a.copy() for a in (est.GD0, est.GD0_GD0, est.GDD_G00, est.GD0_G0D)]
        sm.accumulate_(c, m, est)
        sm.fetch_(c, m)
        compare(c, want, label=case)
        one = snapshot(c)
        # reset zeroes the accumulators; a run-to-run repeat gives the same bits
        sm.reset_measurements_(c, m)
        sm.fetch_(c, m)
        assert all(not v.any() for v in snapshot(c).values())
        sm.accumulate_(c, m, est)
        sm.fetch_(c, m)
        again = snapshot(c)
        for k in one:
            assert np.array_equal(one[k], again[k]), k
        # two accumulations equal twice one, to the bit (a + a is exact)
        sm.accumulate_(c, m, est)
        sm.fetch_(c, m)
        two = snapshot(c)
        for k in one:
            assert np.array_equal(two[k], 2 * one[k]), k
        # the estimator is left usable
        greens.setup_(est, 1, 2)
        for a, b in zip(before, (est.GD0, est.GD0_GD0, est.GDD_G00, est.GD0_G0D)):
            assert np.array_equal(a, b)
    finally:
        m.close()


@pytest.mark.parametrize("kpm", [False, True], ids=["plain", "kpm"])
def test_make_process_write_end_to_end(kpm, tmp_path):
    from elphdynamics_amd import greens, models, preconditioners as pc, process_input as pi, ssh_measurements as sm, synth
    sim = pi.process_input_file(os.path.join(DECKS, "ssh_langevin_square_L4.toml"))
    m = sim.model
    try:
        m.solver.tol, m.solver.maxiter = 1e-13, 20000
        m._push_solver()
        m.x[:] = m.x + 0.3 * synth.randn(61, m.Ndof)                         # the deck's start is constant in tau
        models.update_model_(m)
        info = dict(smc.ALL_TD, num_random_vectors=3)
        info["DenDen"] = {"measure": True, "time_dependent": True, "pairs": [[1, 1]]}
        info["PhononGreens"] = {"measure": True, "time_dependent": True, "pairs": [[2, 1], [1, 1]]}
        c = sm.initialize_ssh_measurements_container(m, info, str(tmp_path))
        sm.initialize_measurement_folders_(c)
        est = greens.EstimateGreensFunction(m, nv=3)
        R = np.stack([synth.randn(5200 + i, m.Ndim) for i in range(3)])
        P = pc.SymmetricKPMPreconditioner(m, n=min(20, m.Nsites), buf=0.05, c1=1.0, c2=1.0) if kpm else None
        it, res, fl = sm.make_measurements_(c, m, est, 1, P=P, R=R, rng=np.random.default_rng(2))
        assert not fl.any()
        want = ref.measure(est.R, est.MinvR, m.x, smc.ref_par(m), smc.request_of(c))
        sm.fetch_(c, m)
        compare(c, want, label="deck %s" % ("kpm" if kpm else "plain"))
        sm.process_measurements_(c, 1, m)
        sm.write_measurements_(c, m, 3)
        V = 3                                                               # bin_size * binomial(3, 2)
        d = str(tmp_path)
        rows = dict(ln.split() for ln in open(os.path.join(d, "global_measurements_f", "global_measurements_00003.out")).read().splitlines())
        for k in ref.GLOBAL_KEYS:
            assert abs(float(rows[k]) - want["glob"][k] / V) <= 5e-9 + 1e-12 * want["abs"]["glob"][k], k
        for ln in open(os.path.join(d, "onsite_measurements_f", "onsite_measurements_00003.out")).read().splitlines()[1:]:
            k, o, v = ln.split()
            assert abs(float(v) - want["onsite"][k][int(o) - 1] / V) <= 5e-9, (k, o)
        seen = set()
        for ln in open(os.path.join(d, "intersite_measurements_f", "intersite_measurements_00003.out")).read().splitlines()[1:]:
            k, b, v = ln.split()
            seen.add(k)
            assert abs(float(v) - want["inter"][k][int(b) - 1] / V) <= 5e-9, (k, b)
        assert seen == set(ref.INTERSITE_KEYS)
        susc_of = {"PairGreens": "PairSusc", "DenDen": "ChargeSusc", "SpinSpin": "SpinSusc"}
        for k, w in want["corr"].items():
            pos = w / V
            for space, arr in (("position", pos), ("momentum", ref.momentum(pos))):
                got = parse(os.path.join(d, "%s_%s_f" % (k, space), "%s_%s_00003.out" % (k, space))).reshape(arr.shape, order="F")
                assert np.abs(got.real - arr.real).max() <= 5e-9 and np.abs(got.imag - arr.imag).max() <= 5e-9, (k, space)
                if k in susc_of:
                    s = ref.simpson(arr, m.dtau)
                    got = parse(os.path.join(d, "%s_%s_f" % (susc_of[k], space), "%s_%s_00003.out" % (susc_of[k], space))).reshape(s.shape, order="F")
                    assert np.abs(got.real - s.real).max() <= 5e-9 and np.abs(got.imag - s.imag).max() <= 5e-9, (susc_of[k], space)
        assert set(c.onsite_susc) == set(susc_of.values()) and set(want["corr"]) == set(smc.ALL_TD)
        sm.reset_measurements_(c, m)
        sm.fetch_(c, m)
        assert all(not v.any() for v in snapshot(c).values())
    finally:
        m.close()


def mulM_still_right(oracle, m):
    """mulM_ against the oracle built from the model's own host-visible tables."""
    from elphdynamics_amd import models, synth
    from test_gpu_parity import _oracle_model
    om = _oracle_model(oracle, m)
    v = synth.randn(5, m.Ndim)
    y = np.zeros(m.Ndim)
    models.mulM_(y, m, v)
    assert rel(y, oracle.mulM(om, v)) < 1e-13


def raw_create(m, which=0, pairs=(1, 1), nph=None, Nph=None):
    """elph_ssh_meas_create with one correlation requested for one pair, straight through the C ABI."""
    import ctypes as C
    from elphdynamics_amd import ssh_measurements as sm
    from elphdynamics_amd._lib import dptr, iptr
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    flag = i32([int(k == which) for k in range(5)])
    if m.kind != 1:
        z = np.zeros(m.Nsites)
        return m._lib.elph_ssh_meas_create(m._h, dptr(z), 0.1, 0, 0, None, None, None, None, 0, 0, None, None, None, ip(flag), ip(flag), ip(flag),
                                           ip(i32(list(pairs))))
    sites, t = sm.bond_arrays(m)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    return m._lib.elph_ssh_meas_create(m._h, dptr(f64(m.mu)), m.dtau, m.Nbonds, m.nbonds, iptr(sites), dptr(t), iptr(m.bond_to_definition),
                                       iptr(m.bond_to_phonon), m.Nph if Nph is None else Nph, m.nph if nph is None else nph, dptr(f64(m.omega)),
                                       dptr(f64(m.alpha)), dptr(f64(m.alpha2)), ip(flag), ip(flag), ip(flag), ip(i32(list(pairs))))


def test_refusals_leave_the_handle_usable(oracle):
    from elphdynamics_amd import _lib, configs, greens, lattice as lat, models, ssh_measurements as sm
    m, table = smc.build_case("hc3")
    try:
        lib = m._lib
        est = greens.EstimateGreensFunction(m, nv=3)
        c = sm.initialize_ssh_measurements_container(m, dict(table, num_random_vectors=3), "")
        # accumulate before the vectors are set
        with pytest.raises(_lib.ElphError) as e:
            sm.accumulate_(c, m, est)
        assert e.value.code == _lib.ELPH_E_STATE and "no vectors" in str(e.value)
        mulM_still_right(oracle, m)
        greens.set_vectors_(est, np.ones((3, m.Ndim)), np.ones((3, m.Ndim)))
        # a phonon-type index outside 1..nph, an orbital outside 1..n_s: refused by the library, which then holds no container
        assert raw_create(m, which=4, pairs=(1, 4)) == _lib.ELPH_E_ARG
        msg = lib.elph_last_error().decode()
        assert "phonon type 4" in msg and "PhononGreens" in msg and "1..3" in msg, msg
        assert lib.elph_ssh_meas_accumulate(m._h, _lib.dptr(m.x)) == _lib.ELPH_E_STATE
        assert raw_create(m, which=0, pairs=(3, 1)) == _lib.ELPH_E_ARG and "orbital 3" in lib.elph_last_error().decode()
        bad = sm.initialize_ssh_measurements_container(m, {"num_random_vectors": 3, "PhononGreens": {"measure": True, "time_dependent": True, "pairs": [[0, 1]]}}, "")
        with pytest.raises(_lib.ElphError) as e:
            sm.accumulate_(bad, m, est)
        assert e.value.code == _lib.ELPH_E_ARG and "phonon type 0" in str(e.value)
        mulM_still_right(oracle, m)
        # several chains resident
        models.update_model_chains_(m, np.stack([m.x, 0.5 * m.x]))
        assert raw_create(m) == _lib.ELPH_E_UNSUPPORTED and "chains" in lib.elph_last_error().decode()
        with pytest.raises(sm.UnsupportedMeasurement, match="chains"):
            sm.accumulate_(c, m, est)
        models.update_model_(m)                                             # back to one configuration
        assert raw_create(m) == _lib.ELPH_OK
        models.update_model_chains_(m, np.stack([m.x, 0.5 * m.x]))
        m._nchains = 1                                                      # past the host's check: the library's own
        assert lib.elph_ssh_meas_accumulate(m._h, _lib.dptr(m.x)) == _lib.ELPH_E_UNSUPPORTED and "chains" in lib.elph_last_error().decode()
        models.update_model_(m)
        mulM_still_right(oracle, m)
        # and the container still measures after all that (its device side was replaced above: made again)
        c._device_of = None
        sm.accumulate_(c, m, est)
        sm.fetch_(c, m)
        assert abs(c.global_meas["mu"].real - 3 * m.mu.mean()) < 1e-12
        assert lib.elph_ssh_meas_free(m._h) == _lib.ELPH_OK and lib.elph_ssh_meas_reset(m._h) == _lib.ELPH_E_STATE
    finally:
        m.close()
    # PhononGreens with Nph != nph * ncells: the cubic deck of ssh_cases on an axis of two cells (duplicate bonds removed)
    norb, dims, defs, L = sc.SHAPES["cu3x2x2"]
    s = smc.build_model(norb, dims, defs, L, seed=5)
    try:
        assert s.Nph != s.nph * s.lattice.ncells
        est = greens.EstimateGreensFunction(s, nv=2)
        greens.set_vectors_(est, np.ones((2, s.Ndim)), np.ones((2, s.Ndim)))
        c = sm.initialize_ssh_measurements_container(s, dict(smc.ALL_TD, num_random_vectors=2), "")
        with pytest.raises(_lib.ElphError) as e:
            sm.accumulate_(c, s, est)
        assert e.value.code == _lib.ELPH_E_UNSUPPORTED and "PhononGreens" in str(e.value) and "nph" in str(e.value)
        mulM_still_right(oracle, s)
    finally:
        s.close()
    # a Holstein handle
    hm = configs.make_model("w")
    try:
        greens.EstimateGreensFunction(hm, nv=2)
        assert raw_create(hm) == _lib.ELPH_E_UNSUPPORTED and "Holstein" in hm._lib.elph_last_error().decode()
        with pytest.raises(sm.UnsupportedMeasurement, match="Holstein"):
            sm.initialize_ssh_measurements_container(hm, smc.ALL_TD, "")
        mulM_still_right(oracle, hm)
    finally:
        hm.close()
