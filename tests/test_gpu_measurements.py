"""GPU parity of the device-resident measurements (csrc/measure.hip through elphdynamics_amd/measurements.py) against the direct-sum
restatement tests/measurements_reference.py.

Vectors go in through greens.set_vectors_ (no solve, no solver tolerance to inherit) with n_v = 3; omega, omega4, lambda, mu depend on
the site, t on the bond, x is a rough synthetic field.  Bounds:
  * correlation arrays: max|got - ref| < 1e-12 * max(1, max|ref|) — what the estimator's tables meet in tests/test_gpu_greens_shapes.py; the
    folds combine them with coefficients of order one (the 1 covers DenDen's constant term);
  * reduced scalars: |got - ref| < 1e-12 * (sum of the absolute values of the terms, same normalisation): n * eps rounded up for the sums of
    the small cases (n <= 12 * 8 * 4 terms).  The 16 x 16 lattice at L_tau = 160 has n = 40 960 terms per orbital sum, whose worst case
    n * eps = 9.1e-12 would be a wider bound; both sides add in trees and it meets the same 1e-12 (seen: 6e-16), so one bound serves all.
End to end the device's own solve (1e-13) provides the vectors and the reference is evaluated on est.R, est.MinvR: same bounds; the written
files are compared at 5e-9 absolute, half a unit of the 8 decimals written."""
import os

import numpy as np
import pytest

import measurements_reference as ref
from test_gpu_greens import _golden_model
from test_gpu_parity import _oracle_model, rel

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
CHAIN = [(1, 1, (1, 0, 0))]
SQUARE = [(1, 1, (1, 0, 0)), (1, 1, (0, 1, 0))]
HONEYCOMB = [(1, 2, (0, 0, 0)), (1, 2, (-1, 0, 0)), (1, 2, (0, -1, 0))]
CUBIC = [(1, 1, (1, 0, 0)), (1, 1, (1, 1, 0)), (1, 1, (1, 0, 1))]        # no bond of an axis of two cells alone: none is removed as a duplicate
ALL_TD = {k: {"measure": True, "time_dependent": True} for k in ref.CORRS}

# (norbits, (L1, L2, L3), L, bond definitions, [measurements] table)
SHAPES = {
    "sq4x4": (1, (4, 4, 1), 8, SQUARE, ALL_TD),
    "hc3x2": (2, (3, 2, 1), 7, HONEYCOMB, {k: {"measure": True, "time_dependent": k != "DenDen", "pairs": [[2, 2], [1, 2]]} for k in ref.CORRS}),
    "chain12": (1, (12, 1, 1), 6, CHAIN, ALL_TD),
    "cubic3x2x2": (1, (3, 2, 2), 5, CUBIC, ALL_TD),
    "sq16x16": (1, (16, 16, 1), 160, SQUARE, ALL_TD),
}


def build_model(ns, dims, L, defs, seed, tol=1e-13):
    from elphdynamics_amd import lattice as lat, models, synth
    rng = np.random.default_rng(seed)
    m = models.HolsteinModel(lat.Lattice(ns, *dims), L * 0.1, 0.1, tol=tol, maxiter=20000)
    assert m.Ltau == L
    for k, (o1, o2, v) in enumerate(defs):
        m.assign_t_(1.0 - 0.15 * k, o1, o2, v, stddev=0.05, rng=rng)
    N = m.Nsites
    m.omega[:] = 1.0 + 0.1 * rng.standard_normal(N)
    m.omega4[:] = 0.05 * rng.random(N)
    m.lam[:] = 1.0 + 0.1 * rng.standard_normal(N)
    m.mu[:] = 0.1 * rng.standard_normal(N)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=seed)
    models.update_model_(m)
    return m


def ref_par(m, defs):
    """The reference's parameters; the bonds come from the lattice per definition, not from the model's sorted table."""
    la = m.lattice
    nc = la.ncells
    bonds = []
    for d, (o1, o2, v) in enumerate(defs):
        tab = la.calc_neighbor_table(o1, o2, v)
        assert tab.shape[0] == nc
        bonds.append((tab[:, 0], tab[:, 1], m.t[d * nc:(d + 1) * nc]))
    return dict(L=m.Ltau, ns=la.norbits, dims=(la.L1, la.L2, la.L3), dtau=m.dtau, omega=m.omega, omega4=m.omega4, lam=m.lam, mu=m.mu, bonds=bonds)


def request_of(c):
    return {k: (v.position.shape[0], v.pairs) for k, v in c.onsite_corr.items()}


def snapshot(c):
    """The container's numbers as one dict of arrays (copies)."""
    out = {"g:" + k: np.array([v]) for k, v in c.global_meas.items()}
    out.update({"o:" + k: v.copy() for k, v in c.onsite_meas.items()})
    out["el_ke"] = c.intersite_meas["el_ke"].copy()
    out.update({"c:" + k: v.position.copy() for k, v in c.onsite_corr.items()})
    return out


def assert_same_bits_as_single(chain, single, label):
    """chain, single: the snapshots of a chain container's chain 0 and of a single-configuration container measured on one handle with one
    chain resident.  The single-configuration entry points are the one-chain case of the chain entry points (same state, kernels and
    launches), so every fetched array of the two is equal bit for bit."""
    assert set(chain) == set(single)
    for k in single:
        assert np.array_equal(chain[k], single[k]), (label, k, np.abs(chain[k] - single[k]).max())


def in_units(err, yard):
    """err / yard elementwise; a yardstick of zero (every term is zero, e.g. mu = 0 everywhere) admits no error at all."""
    err, yard = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(yard, dtype=np.float64))
    out = np.where(err == 0, 0.0, np.inf)
    np.divide(err, yard, out=out, where=yard > 0)
    return out.max() if out.size else 0.0


def compare(c, want, scale=1.0, label=""):
    """Every accumulator of the (fetched, un-normalised) container against the reference `want`, both for `scale` accumulations."""
    tol = 1e-12
    worst = {}
    for k in ref.GLOBAL_KEYS:
        got, w, yard = c.global_meas[k], scale * want["glob"][k], scale * want["abs"]["glob"][k]
        assert got.imag == 0
        worst["g:" + k] = in_units(abs(got.real - w), yard)
    for k in ref.ONSITE_KEYS:
        got, w, yard = c.onsite_meas[k], scale * want["onsite"][k], scale * want["abs"]["onsite"][k]
        assert not got.imag.any()
        worst["o:" + k] = in_units(np.abs(got.real - w), yard)
    got, w, yard = c.intersite_meas["el_ke"], scale * want["el_ke"], scale * want["abs"]["el_ke"]
    assert not got.imag.any()
    worst["el_ke"] = in_units(np.abs(got.real - w), yard)
    cw = {}
    for k, corr in c.onsite_corr.items():
        w = scale * want["corr"][k]
        assert corr.position.shape == w.shape, k
        assert not corr.position.imag.any(), k                              # exact zeros
        cw[k] = np.abs(corr.position.real - w).max() / max(1.0, np.abs(w).max())
    print(label, "scalars (units of the yardstick):", {k: "%.2e" % v for k, v in worst.items()}, "correlations:",
          {k: "%.2e" % v for k, v in cw.items()}, "scalar bound %.2e" % tol)
    for k, v in worst.items():
        assert v < tol, (label, k, v)
    for k, v in cw.items():
        assert v < 1e-12, (label, k, v)


@pytest.mark.parametrize("case", list(SHAPES))
def test_accumulators_match_direct_sums(case):
    from elphdynamics_amd import greens, measurements as ms
    ns, dims, L, defs, table = SHAPES[case]
    m = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    try:
        info = dict(table, num_random_vectors=3)
        c = ms.initialize_measurements_container(m, info, "")
        est = greens.EstimateGreensFunction(m, nv=3)
        rng = np.random.default_rng(L)
        R, X = rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim))
        greens.set_vectors_(est, R, X)
        greens.setup_(est, 1, 2)
        before = [a.copy() for a in (est.GD0, est.GD0_GD0, est.GDD_G00, est.GD0_G0D)]
        want = ref.measure(R, X, m.x, ref_par(m, defs), request_of(c))
        ms.accumulate_(c, m, est)
        ms.fetch_(c, m)
        compare(c, want, label=case)
        one = snapshot(c)
        # determinism: reset, accumulate, fetch on the same inputs gives the same bits
        ms.reset_measurements_(c, m)
        ms.fetch_(c, m)
        assert all(not v.any() for v in snapshot(c).values())               # reset: exact zeros
        ms.accumulate_(c, m, est)
        ms.fetch_(c, m)
        again = snapshot(c)
        for k in one:
            assert np.array_equal(one[k], again[k]), k
        # a second accumulation without reset: twice one
        ms.accumulate_(c, m, est)
        ms.fetch_(c, m)
        two = snapshot(c)
        for k in one:
            assert np.abs(two[k] - 2 * one[k]).max() <= 4 * EPS * np.abs(two[k]).max(), k
        compare(c, want, scale=2.0, label=case + " x2")
        # the estimator is left usable
        greens.setup_(est, 1, 2)
        for a, b in zip(before, (est.GD0, est.GD0_GD0, est.GDD_G00, est.GD0_G0D)):
            assert np.array_equal(a, b)
    finally:
        m.close()


def test_what_an_accumulate_leaves_in_the_estimators_tables():
    """include/elph_gpu.h: elph_meas_accumulate leaves the estimator's tables and their doubled complex copies (elph_greens_dev_arrays)
    holding the last pair of vectors, (n_v - 1, n_v); elph_meas_chains_accumulate does not touch them, even with one chain resident."""
    from elphdynamics_amd import chain_measurements as cms, greens, measurements as ms
    from test_gpu_current_measurements import device_tables
    ns, dims, L, defs, table = SHAPES["sq4x4"]
    m = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    try:
        info = dict(table, num_random_vectors=3)
        c = ms.initialize_measurements_container(m, info, "")
        cm = cms.initialize_chain_measurements_container(m, info, [""])
        est = greens.EstimateGreensFunction(m, nv=3)
        rng = np.random.default_rng(L)
        greens.set_vectors_(est, rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim)))
        greens.setup_(est, 2, 3)
        _, last_pair = device_tables(m)
        assert all(t.any() for t in last_pair)
        greens.setup_(est, 1, 2)
        _, first_pair = device_tables(m)
        assert not any(np.array_equal(a, b) for a, b in zip(first_pair, last_pair))
        cms.accumulate_(cm, m, est, m.x[None, :])                           # scratch of its own: the tables stay those of (1, 2)
        for a, b in zip(first_pair, device_tables(m)[1]):
            assert np.array_equal(a, b)
        ms.accumulate_(c, m, est)                                           # the estimator's scratch: the tables are those of (2, 3)
        for a, b in zip(last_pair, device_tables(m)[1]):
            assert np.array_equal(a, b)
        cms.accumulate_(cm, m, est, m.x[None, :])
        for a, b in zip(last_pair, device_tables(m)[1]):
            assert np.array_equal(a, b)
    finally:
        m.close()


def parse(path):
    lines = open(path).read().splitlines()[1:]
    return np.array([float(ln.split()[1]) + 1j * float(ln.split()[2]) for ln in lines])


@pytest.mark.parametrize("kpm", [False, True], ids=["plain", "kpm"])
@pytest.mark.parametrize("tag", ["golden4x4", "w"])
def test_make_process_write_end_to_end(tag, kpm, tmp_path):
    from elphdynamics_amd import configs, greens, lattice as lat, measurements as ms, preconditioners as pc, synth
    if tag == "golden4x4":
        m = _golden_model("holstein_sq4_L8.npz")
        m.nbonds = 2                                                        # the fixture's raw table: SQUARE's two definitions in order, t per bond
        m.omega[:] = 1.0 + 0.05 * synth.randn(71, m.Nsites)
        m.omega4[:] = 0.02
        defs = SQUARE
    else:
        m = configs.make_model("w", tol=1e-13, maxiter=20000)
        defs = lat.HONEYCOMB_BONDS
    try:
        info = dict(ALL_TD, num_random_vectors=3)
        info["DenDen"] = {"measure": True, "time_dependent": True, "pairs": [[1, 1]]}
        c = ms.initialize_measurements_container(m, info, str(tmp_path))
        ms.initialize_measurement_folders_(c)
        est = greens.EstimateGreensFunction(m, nv=3)
        R = np.stack([synth.randn(5100 + i, m.Ndim) for i in range(3)])
        P = pc.SymmetricKPMPreconditioner(m, n=min(20, m.Nsites), buf=0.05, c1=1.0, c2=1.0) if kpm else None
        it, res, fl = ms.make_measurements_(c, m, est, 1, P=P, R=R, rng=np.random.default_rng(2))
        assert not fl.any()
        want = ref.measure(est.R, est.MinvR, m.x, ref_par(m, defs), request_of(c))
        ms.fetch_(c, m)
        compare(c, want, label="%s %s" % (tag, "kpm" if kpm else "plain"))
        bin_size = 1
        ms.process_measurements_(c, bin_size, m)
        ms.write_measurements_(c, m, 3)
        V = bin_size * 3                                                    # binomial(3, 2)
        d = str(tmp_path)
        rows = dict(ln.split() for ln in open(os.path.join(d, "global_measurements_f", "global_measurements_00003.out")).read().splitlines())
        for k in ref.GLOBAL_KEYS:
            assert abs(float(rows[k]) - want["glob"][k] / V) <= 5e-9 + 1e-12 * want["abs"]["glob"][k], k
        for ln in open(os.path.join(d, "onsite_measurements_f", "onsite_measurements_00003.out")).read().splitlines()[1:]:
            k, o, v = ln.split()
            assert abs(float(v) - want["onsite"][k][int(o) - 1] / V) <= 5e-9, (k, o)
        for ln in open(os.path.join(d, "intersite_measurements_f", "intersite_measurements_00003.out")).read().splitlines()[1:]:
            k, b, v = ln.split()
            assert k == "el_ke" and abs(float(v) - want["el_ke"][int(b) - 1] / V) <= 5e-9, b
        susc_of = {"PairGreens": "PairSusc", "DenDen": "ChargeSusc", "SpinSpin": "SpinSusc"}
        for k, w in want["corr"].items():
            pos = w / V
            mom = ref.momentum(pos)
            for space, arr in (("position", pos), ("momentum", mom)):
                got = parse(os.path.join(d, "%s_%s_f" % (k, space), "%s_%s_00003.out" % (k, space))).reshape(arr.shape, order="F")
                assert np.abs(got.real - arr.real).max() <= 5e-9 and np.abs(got.imag - arr.imag).max() <= 5e-9, (k, space)
                if k in susc_of:
                    s = ref.simpson(arr, m.dtau)
                    got = parse(os.path.join(d, "%s_%s_f" % (susc_of[k], space), "%s_%s_00003.out" % (susc_of[k], space))).reshape(s.shape, order="F")
                    assert np.abs(got.real - s.real).max() <= 5e-9 and np.abs(got.imag - s.imag).max() <= 5e-9, (susc_of[k], space)
        assert set(c.onsite_susc) == set(susc_of.values())
        ms.reset_measurements_(c, m)
        ms.fetch_(c, m)
        assert all(not v.any() for v in snapshot(c).values())
    finally:
        m.close()


def mulM_still_right(oracle, m):
    from elphdynamics_amd import models, synth
    om = _oracle_model(oracle, m)
    v = synth.randn(5, m.Ndim)
    y = np.zeros(m.Ndim)
    models.mulM_(y, m, v)
    assert rel(y, oracle.mulM(om, v)) < 1e-13


def raw_create(m, ns, pairs=(1, 1)):
    """elph_meas_create with Greens alone requested for one orbital pair, straight through the C ABI."""
    import ctypes as C
    from elphdynamics_amd._lib import dptr
    z = np.zeros(m.Nsites)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    meas, td, npairs, pr = i32([1, 0, 0, 0, 0]), i32([1, 0, 0, 0, 0]), i32([1, 0, 0, 0, 0]), i32(list(pairs))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    return m._lib.elph_meas_create(m._h, dptr(z), dptr(z), dptr(z), dptr(z), 0.1, 0, 0, None, None, ip(meas), ip(td), ip(npairs), ip(pr))


def test_refusals_leave_the_handle_usable(oracle):
    from elphdynamics_amd import _lib, configs, greens, measurements as ms, models
    m = build_model(2, (3, 2, 1), 7, HONEYCOMB, seed=9)
    try:
        lib = m._lib
        est = greens.EstimateGreensFunction(m, nv=3)
        c = ms.initialize_measurements_container(m, dict(ALL_TD, num_random_vectors=3), "")
        # no vectors yet
        with pytest.raises(_lib.ElphError) as e:
            ms.accumulate_(c, m, est)
        assert e.value.code == _lib.ELPH_E_STATE and "no vectors" in str(e.value)
        greens.set_vectors_(est, np.ones((3, m.Ndim)), np.ones((3, m.Ndim)))
        # an orbital pair outside 1..n_s: refused by the library, which then holds no container
        assert raw_create(m, 2, pairs=(1, 3)) == _lib.ELPH_E_ARG
        msg = lib.elph_last_error().decode()
        assert "orbital 3" in msg and "Greens" in msg, msg
        assert lib.elph_meas_accumulate(m._h, _lib.dptr(m.x)) == _lib.ELPH_E_STATE
        bad = ms.initialize_measurements_container(m, {"num_random_vectors": 3, "Greens": {"measure": True, "time_dependent": True, "pairs": [[0, 1]]}}, "")
        with pytest.raises(_lib.ElphError) as e:
            ms.accumulate_(bad, m, est)
        assert e.value.code == _lib.ELPH_E_ARG and "orbital 0" in str(e.value)
        mulM_still_right(oracle, m)
        # several chains resident
        models.update_model_chains_(m, np.stack([m.x, 0.5 * m.x]))
        assert raw_create(m, 2) == _lib.ELPH_E_UNSUPPORTED and "chains" in lib.elph_last_error().decode()
        with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
            ms.accumulate_(c, m, est)
        models.update_model_(m)                                             # back to one configuration
        assert raw_create(m, 2) == _lib.ELPH_OK
        m._lib.elph_update_model_holstein_chains(m._h, 2, _lib.dptr(np.ascontiguousarray(np.stack([m.x, 0.5 * m.x]))), _lib.dptr(m.lam),
                                                 _lib.dptr(m.lam2), _lib.dptr(m.mu), m.dtau)
        assert lib.elph_meas_accumulate(m._h, _lib.dptr(m.x)) == _lib.ELPH_E_UNSUPPORTED and "chains" in lib.elph_last_error().decode()
        models.update_model_(m)
        mulM_still_right(oracle, m)
        # and the container still measures after all that (its device side was replaced above: made again)
        c._device_of = None
        ms.accumulate_(c, m, est)
        ms.fetch_(c, m)
        assert abs(c.global_meas["mu"].real - 3 * m.mu.mean()) < 1e-12
    finally:
        m.close()
    s = configs.make_model("e")
    try:
        greens.EstimateGreensFunction(s, nv=2)
        assert raw_create(s, 1) == _lib.ELPH_E_UNSUPPORTED and "SSH" in s._lib.elph_last_error().decode()
        with pytest.raises(ms.UnsupportedMeasurement, match="SSH"):
            ms.initialize_measurements_container(s, ALL_TD, "")
        mulM_still_right(oracle, s)
    finally:
        s.close()
