"""GPU parity of the device-resident inter-site correlations of the SSH model (csrc/ssh_bondcorr.hip through
elphdynamics_amd/ssh_bond_measurements.py) against the direct sums of tests/ssh_bond_reference.py.

Vectors go in through greens.set_vectors_ (no solve) with n_v = 3; the models are those of tests/ssh_measurement_cases.py (t, alpha,
alpha2 per bond, a rough field with both signs).  Bound on every entry of BondBond, CurrentCurrent and BondPairGreens, the one the
Holstein bond correlations are held to in tests/test_gpu_bond_measurements.py: max|got - ref| < 1e-12 * max(1, max|ref|); imaginary
parts are exact zeros.  The direct sums themselves agree with the transcript of the reference's text within a tenth of that
(tests/test_ssh_bond_measurements_host.py).  End to end the device's own solve (1e-13) provides the vectors and the direct sums are
evaluated on est.R, est.MinvR: same bound; the written files are compared at 5e-9 absolute, half a unit of the 8 decimals written."""
import os

import numpy as np
import pytest

import ssh_bond_reference as sbref
import ssh_cases as sc
import ssh_measurement_cases as smc
from test_gpu_ssh_measurements import mulM_still_right
from test_gpu_ssh_measurements import snapshot as onsite_snapshot
from test_ssh_bond_measurements_host import ALL3, CASES, TD, build, check_files, container_of, request_of, yardstick

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decks")
ONSITE = {"Greens": TD, "DenDen": {"measure": True, "time_dependent": False}, "PhononGreens": TD}


def snapshot(c):
    return {k: v.position.copy() for k, v in c.intersite_corr.items()}


def compare(c, want, scale=1.0, label=""):
    """Every entry of every accumulator of the (fetched, un-normalised) container against the direct sums, both for `scale` accumulations."""
    worst = {}
    assert set(c.intersite_corr) == set(want)
    for k, corr in c.intersite_corr.items():
        w = scale * want[k]
        assert corr.position.shape == w.shape and np.isfinite(w).all(), k
        assert not corr.position.imag.any(), k                              # exact zeros
        worst[k] = np.abs(corr.position.real - w).max() / max(1.0, np.abs(w).max())
    print(label, "SSH bond correlations:", {k: "%.2e" % v for k, v in worst.items()}, "bound 1e-12")
    for k, v in worst.items():
        assert v < 1e-12, (label, k, v)


@pytest.mark.parametrize("case", list(CASES))
def test_accumulators_match_direct_sums(case):
    from elphdynamics_amd import greens, ssh_bond_measurements as sb, ssh_measurements as sm
    host, R, X, want = yardstick(case)
    m = build(case, device=True)
    try:
        assert np.array_equal(m.x, host.x) and np.array_equal(m.t, host.t) and np.array_equal(m.alpha2, host.alpha2)
        c = container_of(case, m)
        info = {k: v for k, v in ONSITE.items() if k != "PhononGreens" or m.nph > 0}
        cm = sm.initialize_ssh_measurements_container(m, dict(info, num_random_vectors=3), "")
        est = greens.EstimateGreensFunction(m, nv=3)
        greens.set_vectors_(est, R, X)
        greens.setup_(est, 1, 2)
        before = [a.copy() for a in (est.GD0, est.GD0_GD0, est.GDD_G00, est.GD0_G0D)]
        sm.accumulate_(cm, m, est)                                          # the SSH measurements container first ...
        sm.fetch_(cm, m)
        onsite_before = onsite_snapshot(cm)
        sb.accumulate_ssh_bonds_(c, m, est)
        assert (est.n1, est.n2) == (2, 3)
        sb.fetch_ssh_bonds_(c, m)
        compare(c, want, label=case)
        one = snapshot(c)
        # determinism: reset, accumulate, fetch on the same inputs gives the same bits
        sb.reset_ssh_bond_measurements_(c, m)
        sb.fetch_ssh_bonds_(c, m)
        assert all(not v.any() for v in snapshot(c).values())               # reset: exact zeros
        sb.accumulate_ssh_bonds_(c, m, est)
        sb.fetch_ssh_bonds_(c, m)
        again = snapshot(c)
        for k in one:
            assert np.array_equal(one[k], again[k]), k
        # a second accumulation without reset: twice one
        sb.accumulate_ssh_bonds_(c, m, est)
        sb.fetch_ssh_bonds_(c, m)
        two = snapshot(c)
        for k in one:
            assert np.abs(two[k] - 2 * one[k]).max() <= 4 * EPS * np.abs(two[k]).max(), k
        compare(c, want, scale=2.0, label=case + " x2")
        # the estimator and the SSH measurements container are left as they were: their own results bit for bit
        greens.setup_(est, 1, 2)
        for a, b in zip(before, (est.GD0, est.GD0_GD0, est.GDD_G00, est.GD0_G0D)):
            assert np.array_equal(a, b)
        sm.fetch_(cm, m)
        for k, v in onsite_snapshot(cm).items():
            assert np.array_equal(v, onsite_before[k]), k                   # untouched by the bond accumulations
        sm.reset_measurements_(cm, m)
        sm.accumulate_(cm, m, est)                                          # ... and after
        sm.fetch_(cm, m)
        for k, v in onsite_snapshot(cm).items():
            assert np.array_equal(v, onsite_before[k]), k
        sb.fetch_ssh_bonds_(c, m)
        for k, v in snapshot(c).items():
            assert np.array_equal(v, two[k]), k
    finally:
        m.close()


def test_one_correlation_alone_gives_the_same_bits():
    """A container with one correlation alone computes and transforms only that correlation's fields: same bits as all three together."""
    from elphdynamics_amd import greens, ssh_bond_measurements as sb
    host, R, X, want = yardstick("hc3x2_both_ways")
    m = build("hc3x2_both_ways", device=True)
    try:
        est = greens.EstimateGreensFunction(m, nv=3)
        greens.set_vectors_(est, R, X)
        both = container_of("hc3x2_both_ways", m)
        sb.accumulate_ssh_bonds_(both, m, est)
        sb.fetch_ssh_bonds_(both, m)
        for name in sbref.CORRS:
            alone = sb.initialize_ssh_bond_container(m, {name: TD, "num_random_vectors": 3}, "")
            sb.accumulate_ssh_bonds_(alone, m, est)                         # replaces the handle's accumulators
            sb.fetch_ssh_bonds_(alone, m)
            assert set(alone.intersite_corr) == {name}
            assert np.array_equal(alone.intersite_corr[name].position, both.intersite_corr[name].position), name
    finally:
        m.close()


@pytest.mark.parametrize("kpm", [False, True], ids=["plain", "kpm"])
def test_accumulate_process_write_end_to_end(kpm, tmp_path):
    from elphdynamics_amd import greens, models, preconditioners as pc, process_input as pi, ssh_bond_measurements as sb, synth
    sim = pi.process_input_file(os.path.join(DECKS, "ssh_langevin_square_L4.toml"))
    m = sim.model
    try:
        m.solver.tol, m.solver.maxiter = 1e-13, 20000
        m._push_solver()
        m.x[:] = m.x + 0.3 * synth.randn(61, m.Ndof)                         # the deck's start is constant in tau
        models.update_model_(m)
        info = dict(ALL3, num_random_vectors=3)
        info["CurrentCurrent"] = {"measure": True, "time_dependent": True, "pairs": [[2, 1], [1, 1], [1, 2]]}
        c = sb.initialize_ssh_bond_container(m, info, str(tmp_path))
        sb.initialize_ssh_bond_folders_(c)
        est = greens.EstimateGreensFunction(m, nv=3)
        R = np.stack([synth.randn(5300 + i, m.Ndim) for i in range(3)])
        P = pc.SymmetricKPMPreconditioner(m, n=min(20, m.Nsites), buf=0.05, c1=1.0, c2=1.0) if kpm else None
        it, res, fl = greens.update_(est, m, P, rng=np.random.default_rng(2), R=R)
        assert not fl.any()
        sb.accumulate_ssh_bonds_(c, m, est)
        want = sbref.measure(est.R, est.MinvR, m.x, smc.ref_par(m), sbref.definitions(m), request_of(c))
        sb.fetch_ssh_bonds_(c, m)
        compare(c, want, label="deck %s" % ("kpm" if kpm else "plain"))
        sb.process_ssh_bond_measurements_(c, 1, m)
        sb.write_ssh_bond_measurements_(c, m, 3)
        check_files(str(tmp_path), want, 3, m.dtau, 3)                      # V = bin_size * binomial(3, 2)
        assert set(c.intersite_susc) == {"BondPairSusc"}
        sb.reset_ssh_bond_measurements_(c, m)
        sb.fetch_ssh_bonds_(c, m)
        assert all(not v.any() for v in snapshot(c).values())
    finally:
        m.close()


def raw_create(m, defs, which=0, pairs=(1, 1), Nbonds=None):
    """elph_ssh_bond_create with one correlation (0 BondBond, 1 CurrentCurrent, 2 BondPairGreens) requested for one pair of bonds, straight
    through the C ABI."""
    import ctypes as C
    from elphdynamics_amd._lib import dptr, iptr
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    o1, o2, v = i32([d[0] for d in defs]), i32([d[1] for d in defs]), i32([k for d in defs for k in d[2]])
    flag = i32([int(k == which) for k in range(3)])
    if m.kind != 1:
        return m._lib.elph_ssh_bond_create(m._h, len(defs), ip(o1), ip(o2), ip(v), 0, None, None, None, 0, None, None, ip(flag), ip(flag), ip(flag),
                                           ip(i32(list(pairs))))
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)  # noqa: E731
    t, b2d, b2p, al, al2 = f64(m.t), i64(m.bond_to_definition), i64(m.bond_to_phonon), f64(m.alpha), f64(m.alpha2)
    return m._lib.elph_ssh_bond_create(m._h, len(defs), ip(o1), ip(o2), ip(v), m.Nbonds if Nbonds is None else Nbonds, dptr(t), iptr(b2d), iptr(b2p),
                                       m.Nph, dptr(al), dptr(al2), ip(flag), ip(flag), ip(flag), ip(i32(list(pairs))))


def test_refusals_leave_the_handle_usable(oracle):
    from elphdynamics_amd import _lib, configs, greens, measurements as ms, models, ssh_bond_measurements as sb
    host, R, X, want = yardstick("hc3")
    m = build("hc3", device=True)
    try:
        lib = m._lib
        defs = sbref.definitions(m)
        est = greens.EstimateGreensFunction(m, nv=3)
        c = container_of("hc3", m)
        # no vectors yet
        with pytest.raises(_lib.ElphError) as e:
            sb.accumulate_ssh_bonds_(c, m, est)
        assert e.value.code == _lib.ELPH_E_STATE and "no vectors" in str(e.value)
        mulM_still_right(oracle, m)
        greens.set_vectors_(est, R, X)
        # a bond index outside 1..n_def: refused by the library, which then holds no accumulators
        for which, name in enumerate(sbref.CORRS):
            assert raw_create(m, defs, which=which, pairs=(1, 4)) == _lib.ELPH_E_ARG
            msg = lib.elph_last_error().decode()
            assert "bond 4" in msg and name in msg and "1..3" in msg, msg
            assert lib.elph_ssh_bond_accumulate(m._h, _lib.dptr(m.x)) == _lib.ELPH_E_STATE
        assert raw_create(m, defs, which=1, pairs=(0, 1)) == _lib.ELPH_E_ARG and "bond 0" in lib.elph_last_error().decode()
        # an orbital outside 1..n_s
        assert raw_create(m, [(1, 3, (0, 0, 0))] + defs[1:], which=1) == _lib.ELPH_E_ARG
        msg = lib.elph_last_error().decode()
        assert "orbital 3" in msg and "definition 1" in msg, msg
        # a bond count that is not the handle's
        assert raw_create(m, defs, which=1, Nbonds=m.Nbonds - 1) == _lib.ELPH_E_ARG and "bonds" in lib.elph_last_error().decode()
        bad = sb.initialize_ssh_bond_container(m, {"num_random_vectors": 3, "CurrentCurrent": {"measure": True, "time_dependent": True, "pairs": [[1, 5]]}}, "")
        with pytest.raises(_lib.ElphError) as e:
            sb.accumulate_ssh_bonds_(bad, m, est)
        assert e.value.code == _lib.ELPH_E_ARG and "bond 5" in str(e.value) and "CurrentCurrent" in str(e.value)
        mulM_still_right(oracle, m)
        # several chains resident
        models.update_model_chains_(m, np.stack([m.x, 0.5 * m.x]))
        assert raw_create(m, defs, which=1) == _lib.ELPH_E_UNSUPPORTED and "chains" in lib.elph_last_error().decode()
        with pytest.raises(ms.UnsupportedMeasurement, match="chains"):
            sb.accumulate_ssh_bonds_(c, m, est)
        models.update_model_(m)                                             # back to one configuration
        assert raw_create(m, defs, which=1) == _lib.ELPH_OK
        models.update_model_chains_(m, np.stack([m.x, 0.5 * m.x]))
        m._nchains = 1                                                      # past the host's check: the library's own
        assert lib.elph_ssh_bond_accumulate(m._h, _lib.dptr(m.x)) == _lib.ELPH_E_UNSUPPORTED and "chains" in lib.elph_last_error().decode()
        models.update_model_(m)
        mulM_still_right(oracle, m)
        # and the container still measures after all that (its device side was replaced above: made again)
        c._device_of = None
        sb.accumulate_ssh_bonds_(c, m, est)
        sb.fetch_ssh_bonds_(c, m)
        compare(c, want, label="after the refusals")
    finally:
        m.close()
    # CurrentCurrent with Nbonds != n_def * ncells: the cubic deck of ssh_cases on an axis of two cells (duplicate bonds removed);
    # BondBond on the same model still measures right
    norb, dims, sdefs, L = sc.SHAPES["cu3x2x2"]
    s = smc.build_model(norb, dims, sdefs, L, seed=5)
    try:
        assert s.Nbonds != s.nbonds * s.lattice.ncells
        est = greens.EstimateGreensFunction(s, nv=2)
        rng = np.random.default_rng(6)
        R2, X2 = rng.standard_normal((2, s.Ndim)), rng.standard_normal((2, s.Ndim))
        greens.set_vectors_(est, R2, X2)
        c = sb.initialize_ssh_bond_container(s, dict(ALL3, num_random_vectors=2), "")
        with pytest.raises(_lib.ElphError) as e:
            sb.accumulate_ssh_bonds_(c, s, est)
        msg = str(e.value)
        assert e.value.code == _lib.ELPH_E_UNSUPPORTED and "CurrentCurrent" in msg and "%d bonds" % s.Nbonds in msg and "%d cells" % s.lattice.ncells in msg
        assert s._lib.elph_ssh_bond_reset(s._h) == _lib.ELPH_E_STATE        # nothing was left behind
        mulM_still_right(oracle, s)
        c = sb.initialize_ssh_bond_container(s, {"BondBond": TD, "num_random_vectors": 2}, "")
        sb.accumulate_ssh_bonds_(c, s, est)
        sb.fetch_ssh_bonds_(c, s)
        compare(c, sbref.measure(R2, X2, s.x, dict(L=L, ns=norb, dims=dims), sbref.definitions(s), request_of(c)), label="cu3x2x2 BondBond")
    finally:
        s.close()
    # a Holstein handle
    hm = configs.make_model("w")
    try:
        greens.EstimateGreensFunction(hm, nv=2)
        assert raw_create(hm, [(1, 2, (0, 0, 0))]) == _lib.ELPH_E_UNSUPPORTED and "Holstein" in hm._lib.elph_last_error().decode()
        with pytest.raises(ms.UnsupportedMeasurement, match="Holstein"):
            sb.initialize_ssh_bond_container(hm, {"BondBond": TD}, "")
        mulM_still_right(oracle, hm)
    finally:
        hm.close()


def test_the_holstein_bond_path_still_meets_its_bound():
    """elph_bond_* runs the kernels that moved into bondcorr_dev.h: one small case of tests/test_gpu_bond_measurements.py, its bound."""
    import bond_reference as bref
    from elphdynamics_amd import bond_measurements as bm, greens
    from test_bond_measurements_host import SMALL
    from test_gpu_measurements import build_model
    ns, dims, L, defs, table = SMALL["hc3x2_both_ways"]
    m = build_model(ns, dims, L, defs, seed=3)
    try:
        c = bm.initialize_bond_container(m, dict(table, num_random_vectors=3), "")
        est = greens.EstimateGreensFunction(m, nv=3)
        rng = np.random.default_rng(8)
        R, X = rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim))
        greens.set_vectors_(est, R, X)
        bm.accumulate_bonds_(c, m, est)
        bm.fetch_bonds_(c, m)
        compare(c, bref.measure(R, X, L, ns, dims, defs, request_of(c)), label="Holstein hc3x2_both_ways")
    finally:
        m.close()
