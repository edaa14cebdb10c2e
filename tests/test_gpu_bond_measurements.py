"""GPU parity of the device-resident bond correlations (csrc/bondcorr.hip through elphdynamics_amd/bond_measurements.py) against the
direct-sum restatement tests/bond_reference.py.

Vectors go in through greens.set_vectors_ (no solve, no solver tolerance to inherit) with n_v = 3; t depends on the bond as in
test_gpu_measurements.build_model.  Bound on the arrays: max|got - ref| < 1e-12 * max(1, max|ref|), the bound the on-site correlations
are held to in tests/test_gpu_measurements.py, for every case, the 16 x 16 lattice at L_tau = 160 included.  There the direct sums over all
displacements are too slow in numpy, so the yardstick is evaluated by direct sums on a seeded sample: all 256 cell displacements at
dtau = 0 (they hold D = 0, every delta-term position and everything the tau = beta slices read) and 256 more displacements; the other
entries of the device's arrays are compared with the yardstick's np.fft evaluation, itself within the printed distance of the direct sums
on the sample.
End to end the device's own solve (1e-13) provides the vectors and the yardstick is evaluated on est.R, est.MinvR: same bound; the written
files are compared at 5e-9 absolute, half a unit of the 8 decimals written."""
import os

import numpy as np
import pytest

import bond_reference as bref
import measurements_reference as mref
from test_bond_measurements_host import SMALL, SQUARE, TD
from test_gpu_greens import _golden_model
from test_gpu_measurements import build_model, mulM_still_right, parse, ref_par
from test_gpu_measurements import request_of as onsite_request_of
from test_gpu_measurements import snapshot as onsite_snapshot

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SHAPES = dict(SMALL, sq16x16=(1, (16, 16, 1), 160, SQUARE, {"BondBond": TD, "BondPairGreens": TD}))
SAMPLED = {"sq16x16": 256}                                                  # displacements beyond the dtau = 0 slice
ONSITE = {"Greens": TD, "SpinSpin": {"measure": True, "time_dependent": False}}


def request_of(c):
    return {k: (v.position.shape[0], v.pairs) for k, v in c.intersite_corr.items()}


def snapshot(c):
    return {k: v.position.copy() for k, v in c.intersite_corr.items()}


def compare(c, want, scale=1.0, label="", where=None):
    """Every accumulator of the (fetched, un-normalised) container against the yardstick `want`, both for `scale` accumulations; NaN
    entries of the yardstick (displacements a sampled evaluation left out) are not compared."""
    worst = {}
    for k, corr in c.intersite_corr.items():
        w = scale * want[k]
        assert corr.position.shape == w.shape, k
        assert not corr.position.imag.any(), k                              # exact zeros
        ok = np.isfinite(w)
        assert ok.any() and (where is None or ok.sum() >= where), (k, ok.sum())
        worst[k] = np.abs(corr.position.real - w)[ok].max() / max(1.0, np.abs(w[ok]).max())
    print(label, "bond correlations:", {k: "%.2e" % v for k, v in worst.items()}, "bound 1e-12")
    for k, v in worst.items():
        assert v < 1e-12, (label, k, v)


@pytest.mark.parametrize("case", list(SHAPES))
def test_accumulators_match_direct_sums(case):
    from elphdynamics_amd import bond_measurements as bm, greens, measurements as ms
    ns, dims, L, defs, table = SHAPES[case]
    m = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    try:
        assert m.bond_definitions == defs
        c = bm.initialize_bond_container(m, dict(table, num_random_vectors=3), "")
        cm = ms.initialize_measurements_container(m, dict(ONSITE, num_random_vectors=3), "")
        est = greens.EstimateGreensFunction(m, nv=3)
        rng = np.random.default_rng(L)
        R, X = rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim))
        greens.set_vectors_(est, R, X)
        greens.setup_(est, 1, 2)
        before = [a.copy() for a in (est.GD0, est.GD0_GD0, est.GDD_G00, est.GD0_G0D)]
        ms.accumulate_(cm, m, est)                                          # the on-site container first ...
        ms.fetch_(cm, m)
        onsite_before = onsite_snapshot(cm)
        npts = None
        if case in SAMPLED:
            pts = bref.sample_points(L, dims, SAMPLED[case], seed=L)
            npts = len(pts)
            want = bref.measure(R, X, L, ns, dims, defs, request_of(c), points=pts)
            full = bref.measure(R, X, L, ns, dims, defs, request_of(c), star=bref.star_fft)
            for k in want:
                ok = np.isfinite(want[k])
                print(case, k, "yardstick: direct sums on %d sampled displacements against np.fft: %.2e (max|ref| %.3g)"
                      % (npts, np.abs(want[k] - full[k])[ok].max(), np.abs(full[k]).max()))
        else:
            want = bref.measure(R, X, L, ns, dims, defs, request_of(c))
        bm.accumulate_bonds_(c, m, est)
        assert (est.n1, est.n2) == (2, 3)
        bm.fetch_bonds_(c, m)
        compare(c, want, label=case, where=npts)
        if case in SAMPLED:
            compare(c, full, label=case + " (np.fft evaluation, every entry)")
        one = snapshot(c)
        # determinism: reset, accumulate, fetch on the same inputs gives the same bits
        bm.reset_bond_measurements_(c, m)
        bm.fetch_bonds_(c, m)
        assert all(not v.any() for v in snapshot(c).values())               # reset: exact zeros
        bm.accumulate_bonds_(c, m, est)
        bm.fetch_bonds_(c, m)
        again = snapshot(c)
        for k in one:
            assert np.array_equal(one[k], again[k]), k
        # a second accumulation without reset: twice one
        bm.accumulate_bonds_(c, m, est)
        bm.fetch_bonds_(c, m)
        two = snapshot(c)
        for k in one:
            assert np.abs(two[k] - 2 * one[k]).max() <= 4 * EPS * np.abs(two[k]).max(), k
        compare(c, want, scale=2.0, label=case + " x2", where=npts)
        # the estimator and the on-site container are left as they were: their own results bit for bit
        greens.setup_(est, 1, 2)
        for a, b in zip(before, (est.GD0, est.GD0_GD0, est.GDD_G00, est.GD0_G0D)):
            assert np.array_equal(a, b)
        ms.fetch_(cm, m)
        for k, v in onsite_snapshot(cm).items():
            assert np.array_equal(v, onsite_before[k]), k                   # untouched by the bond accumulations
        ms.reset_measurements_(cm, m)
        ms.accumulate_(cm, m, est)                                          # ... and after
        ms.fetch_(cm, m)
        for k, v in onsite_snapshot(cm).items():
            assert np.array_equal(v, onsite_before[k]), k
        bm.fetch_bonds_(c, m)
        for k, v in snapshot(c).items():
            assert np.array_equal(v, two[k]), k
    finally:
        m.close()


def test_one_correlation_alone_gives_the_same_bits():
    """A container with BondBond alone, or BondPairGreens alone, transforms only that correlation's fields: same bits as together."""
    from elphdynamics_amd import bond_measurements as bm, greens
    ns, dims, L, defs, table = SHAPES["hc3x2_both_ways"]
    m = build_model(ns, dims, L, defs, seed=3)
    try:
        est = greens.EstimateGreensFunction(m, nv=3)
        rng = np.random.default_rng(8)
        greens.set_vectors_(est, rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim)))
        both = bm.initialize_bond_container(m, dict(table, num_random_vectors=3), "")
        bm.accumulate_bonds_(both, m, est)
        bm.fetch_bonds_(both, m)
        for name in bref.CORRS:
            alone = bm.initialize_bond_container(m, {name: table[name], "num_random_vectors": 3}, "")
            bm.accumulate_bonds_(alone, m, est)                             # replaces the handle's bond accumulators
            bm.fetch_bonds_(alone, m)
            assert set(alone.intersite_corr) == {name}
            assert np.array_equal(alone.intersite_corr[name].position, both.intersite_corr[name].position), name
    finally:
        m.close()


@pytest.mark.parametrize("kpm", [False, True], ids=["plain", "kpm"])
@pytest.mark.parametrize("tag", ["golden4x4", "w"])
def test_accumulate_process_write_end_to_end(tag, kpm, tmp_path):
    from elphdynamics_amd import bond_measurements as bm, configs, greens, lattice as lat, measurements as ms, preconditioners as pc, synth
    if tag == "golden4x4":
        m = _golden_model("holstein_sq4_L8.npz")                            # tables filled without assign_t_: definitions passed explicitly
        m.nbonds = 2
        assert m.bond_definitions == []
        defs, given = SQUARE, SQUARE
    else:
        m = configs.make_model("w", tol=1e-13, maxiter=20000)
        defs, given = lat.HONEYCOMB_BONDS, None
        assert m.bond_definitions == defs
    try:
        la = m.lattice
        ns, dims, L = la.norbits, (la.L1, la.L2, la.L3), m.Ltau
        info = {"num_random_vectors": 3, "BondBond": TD, "BondPairGreens": {"measure": True, "time_dependent": True, "pairs": [[2, 1], [1, 1], [1, 2]]}}
        c = bm.initialize_bond_container(m, info, str(tmp_path), bond_definitions=given)
        cm = ms.initialize_measurements_container(m, dict(ONSITE, num_random_vectors=3), str(tmp_path))
        bm.initialize_bond_folders_(c)
        ms.initialize_measurement_folders_(cm)
        est = greens.EstimateGreensFunction(m, nv=3)
        R = np.stack([synth.randn(5100 + i, m.Ndim) for i in range(3)])
        P = pc.SymmetricKPMPreconditioner(m, n=min(20, m.Nsites), buf=0.05, c1=1.0, c2=1.0) if kpm else None
        # the bond container first, the on-site one after it, on the same vectors
        it, res, fl = greens.update_(est, m, P, rng=np.random.default_rng(2), R=R)
        assert not fl.any()
        bm.accumulate_bonds_(c, m, est)
        ms.accumulate_(cm, m, est)
        want = bref.measure(est.R, est.MinvR, L, ns, dims, defs, request_of(c))
        bm.fetch_bonds_(c, m)
        compare(c, want, label="%s %s" % (tag, "kpm" if kpm else "plain"))
        ms.fetch_(cm, m)
        onsite = mref.measure(est.R, est.MinvR, m.x, ref_par(m, defs), onsite_request_of(cm))
        for k, v in cm.onsite_corr.items():
            assert np.abs(v.position.real - onsite["corr"][k]).max() < 1e-12 * max(1.0, np.abs(onsite["corr"][k]).max()), k
        bin_size = 1
        bm.process_bond_measurements_(c, bin_size, m)
        bm.write_bond_measurements_(c, m, 3)
        V = bin_size * 3                                                    # binomial(3, 2)
        d = str(tmp_path)
        for k, w in want.items():
            pos = w / V
            mom = mref.momentum(pos)
            for space, arr in (("position", pos), ("momentum", mom)):
                got = parse(os.path.join(d, "%s_%s_f" % (k, space), "%s_%s_00003.out" % (k, space))).reshape(arr.shape, order="F")
                assert np.abs(got.real - arr.real).max() <= 5e-9 and np.abs(got.imag - arr.imag).max() <= 5e-9, (k, space)
                if k == "BondPairGreens":
                    s = mref.simpson(arr, m.dtau)
                    got = parse(os.path.join(d, "BondPairSusc_%s_f" % space, "BondPairSusc_%s_00003.out" % space)).reshape(s.shape, order="F")
                    assert np.abs(got.real - s.real).max() <= 5e-9 and np.abs(got.imag - s.imag).max() <= 5e-9, ("BondPairSusc", space)
        assert set(c.intersite_susc) == {"BondPairSusc"}
        bm.reset_bond_measurements_(c, m)
        bm.fetch_bonds_(c, m)
        assert all(not v.any() for v in snapshot(c).values())
    finally:
        m.close()


def raw_create(m, defs, pairs=(1, 1), which=0):
    """elph_bond_create with one correlation requested for one pair of bonds, straight through the C ABI."""
    import ctypes as C
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    o1, o2, v = i32([d[0] for d in defs]), i32([d[1] for d in defs]), i32([k for d in defs for k in d[2]])
    flag = i32([which == 0, which == 1])
    return m._lib.elph_bond_create(m._h, len(defs), ip(o1), ip(o2), ip(v), ip(flag), ip(flag), ip(flag), ip(i32(list(pairs))))


def test_refusals_leave_the_handle_usable(oracle):
    from elphdynamics_amd import _lib, bond_measurements as bm, configs, greens, measurements as ms, models
    ns, dims, L, defs, table = SHAPES["hc3x2"]
    m = build_model(ns, dims, L, defs, seed=9)
    try:
        lib = m._lib
        est = greens.EstimateGreensFunction(m, nv=3)
        c = bm.initialize_bond_container(m, dict(table, num_random_vectors=3), "")
        # no vectors yet
        with pytest.raises(_lib.ElphError) as e:
            bm.accumulate_bonds_(c, m, est)
        assert e.value.code == _lib.ELPH_E_STATE and "no vectors" in str(e.value)
        greens.set_vectors_(est, np.ones((3, m.Ndim)), np.ones((3, m.Ndim)))
        # a bond index outside 1..n_def: refused by the library, which then holds no accumulators
        assert raw_create(m, defs, pairs=(1, 4), which=1) == _lib.ELPH_E_ARG
        msg = lib.elph_last_error().decode()
        assert "bond 4" in msg and "BondPairGreens" in msg, msg
        assert lib.elph_bond_accumulate(m._h) == _lib.ELPH_E_STATE
        assert raw_create(m, defs, pairs=(0, 1)) == _lib.ELPH_E_ARG and "bond 0" in lib.elph_last_error().decode() and "BondBond" in lib.elph_last_error().decode()
        # an orbital outside 1..n_s
        assert raw_create(m, [(1, 3, (0, 0, 0))]) == _lib.ELPH_E_ARG
        msg = lib.elph_last_error().decode()
        assert "orbital 3" in msg and "definition 1" in msg, msg
        bad = bm.initialize_bond_container(m, {"num_random_vectors": 3, "BondBond": {"measure": True, "time_dependent": True, "pairs": [[1, 5]]}}, "")
        with pytest.raises(_lib.ElphError) as e:
            bm.accumulate_bonds_(bad, m, est)
        assert e.value.code == _lib.ELPH_E_ARG and "bond 5" in str(e.value)
        mulM_still_right(oracle, m)
        # several chains resident
        models.update_model_chains_(m, np.stack([m.x, 0.5 * m.x]))
        assert raw_create(m, defs) == _lib.ELPH_E_UNSUPPORTED and "chains" in lib.elph_last_error().decode()
        with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
            bm.accumulate_bonds_(c, m, est)
        models.update_model_(m)                                             # back to one configuration
        assert raw_create(m, defs) == _lib.ELPH_OK
        m._lib.elph_update_model_holstein_chains(m._h, 2, _lib.dptr(np.ascontiguousarray(np.stack([m.x, 0.5 * m.x]))), _lib.dptr(m.lam),
                                                 _lib.dptr(m.lam2), _lib.dptr(m.mu), m.dtau)
        assert lib.elph_bond_accumulate(m._h) == _lib.ELPH_E_UNSUPPORTED and "chains" in lib.elph_last_error().decode()
        models.update_model_(m)
        mulM_still_right(oracle, m)
        # and the container still measures after all that (its device side was replaced above: made again)
        c._device_of = None
        rng = np.random.default_rng(4)
        R, X = rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim))
        greens.set_vectors_(est, R, X)
        bm.accumulate_bonds_(c, m, est)
        bm.fetch_bonds_(c, m)
        compare(c, bref.measure(R, X, L, ns, dims, defs, request_of(c)), label="after the refusals")
    finally:
        m.close()
    s = configs.make_model("e")
    try:
        greens.EstimateGreensFunction(s, nv=2)
        assert raw_create(s, SQUARE) == _lib.ELPH_E_UNSUPPORTED and "SSH" in s._lib.elph_last_error().decode()
        with pytest.raises(ms.UnsupportedMeasurement, match="SSH"):
            bm.initialize_bond_container(s, {"BondBond": TD}, "", bond_definitions=SQUARE)
        mulM_still_right(oracle, s)
    finally:
        s.close()
