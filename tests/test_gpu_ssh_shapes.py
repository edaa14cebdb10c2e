"""GPU (-m gpu): the bond-phonon (SSH) kernels beyond the uniform square lattice — every case of tests/ssh_cases.py (honeycomb,
triangular, odd / rectangular squares, chains, cubic, partial models with bare bonds, time axes 1, 2, 7, 161, every sites-per-lane
count of the lane-program kernels and the generic family), with disordered t and alpha, alpha2 of both signs and mu per site.

The device's per-(tau, bond) tables are compared with the numpy formula on the host arrays first; the oracle is then built from the
HOST tables (ssh_cases.host_view), never from what the device computed, and the dense-size cases are held to the numpy.linalg
restatement of tests/ssh_reference.py as well.  Bounds are those of the tests named in each docstring (test_gpu_parity.py,
test_gpu_hmc.py, test_gpu_langevin.py)."""
import contextlib

import numpy as np
import pytest

import ssh_cases as sc
import ssh_reference as ref
from test_gpu_parity import _ssh_oracle_force, _wg_info, _wg_resident_vs_streaming, rel

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _model(name, tol=1e-5, maxiter=20000):
    """(case, model) — SSHModel + assign_hopping_ + initialize_model_ with the case's disorder widths, then the per-phonon and
    per-site arrays written over, as test_gpu_hmc.py::_ssh_golden_model does; the handle is closed on the way out."""
    from elphdynamics_amd import lattice as lat
    from elphdynamics_amd import models
    case = sc.make_case(name)
    tab = case.tab
    m = models.SSHModel(lat.Lattice(case.norb, *case.Ls), case.beta, case.dtau, tol=tol, maxiter=maxiter)
    try:
        assert m.Ltau == case.Ltau
        for (o1, o2, d, has_phonon, nm, tmean) in case.definitions:
            m.assign_hopping_(tmean, sc.ALPHA_MEAN, 0.0, sc.OMEGA_MEAN, o1, o2, d, has_phonon=has_phonon, name=nm, t_std=sc.T_STD,
                              alpha_std=sc.ALPHA_STD)
        m.initialize_model_(rng=np.random.default_rng(case.seed))
        assert np.array_equal(m.neighbor_table, tab.table) and np.array_equal(m.checkerboard_perm, tab.cb_perm)
        assert np.array_equal(m.phonon_to_bond, tab.phonon_to_bond) and m.Nph == tab.Nph and m.Nbonds == tab.Nbonds
        assert np.array_equal(m.t, case.t) and np.array_equal(m.alpha, case.alpha)       # the model drew the case's t and alpha itself
        assert m.alpha.size == m.alpha2.size == m.Nph and not m.has_shared_fields      # no slot for a coupling on a bare bond
        m.alpha2[:], m.mu[:] = case.alpha2, case.mu
        m.omega, m.omega4 = case.omega.copy(), case.omega4.copy()
        m.x[:] = case.x
        models.update_model_(m)
        yield case, m
    finally:
        m.close()


def _rhs(oracle, om, case, nrhs):
    R = np.stack([case.vector(20 + r) for r in range(nrhs)])
    return R, np.stack([oracle.mulMT(om, R[r]) for r in range(nrhs)])


def _check_tables(case, m):
    """m.cosht / m.sinht (fetched from the device) against the numpy formula on the host arrays: the bounds of
    test_ssh_device_update_equals_host_tables_at_config_E."""
    hv = sc.host_view(case, m.x)
    assert m.cosht.shape == hv.cosht.shape == (case.Nbonds, case.Ltau)
    assert rel(m.cosht, hv.cosht) < 1e-15 and rel(m.sinht, hv.sinht) < 1e-14
    return hv


def _check_matvecs(oracle, case, m, om):
    """As test_matvec_vs_oracle; on the dense-size cases also against the dense M."""
    from elphdynamics_amd import models
    v, u = case.vector(1), case.vector(2)
    y = np.empty(m.Ndim)
    D = ref.DenseSSH(case.tab, case.Ltau, case.dtau, case.t, case.alpha, case.alpha2, case.mu, case.x) if sc.is_dense(case.name) else None
    for fn, ofn, dense in ((models.mulM_, oracle.mulM, lambda w: D.M @ w), (models.mulMt_, oracle.mulMT, lambda w: D.M.T @ w),
                           (models.mulMtM_, oracle.mulMTM, lambda w: D.A @ w)):
        fn(y, m, v)
        assert rel(y, ofn(om, v)) < 1e-13
        if D is not None:
            assert rel(y, dense(v)) < 1e-13
    Mv, Mtu, a = np.empty(m.Ndim), np.empty(m.Ndim), np.empty(m.Ndim)
    models.mulM_(Mv, m, v)
    models.mulMt_(Mtu, m, u)
    assert abs(u @ Mv - Mtu @ v) < 1e-11 * np.linalg.norm(u) * np.linalg.norm(v)          # adjointness
    models.mulMt_(a, m, Mv)
    models.mulMtM_(y, m, v)
    assert rel(y, a) < 1e-14                                                                # fused MtM == Mt(M v)
    models.mulM_(a, m, Mtu)
    models.mulMMt_(y, m, u)
    assert rel(y, a) < 1e-14 and rel(y, oracle.mulM(om, oracle.mulMT(om, u))) < 1e-13
    if D is not None:
        assert rel(y, D.M @ (D.M.T @ u)) < 1e-13
    models.mulM_(a, m, 2.0 * v - 3.0 * u)
    Mu = np.empty(m.Ndim)
    models.mulM_(Mu, m, u)
    assert rel(a, 2.0 * Mv - 3.0 * Mu) < 1e-13                                              # linearity
    return D


def _check_force(oracle, case, m, hv, D):
    """hmc.calc_dSfdx_ against the oracle's force (solves at 1e-11, bound 1e-8: test_ssh_fermion_force_vs_oracle) and the dense one."""
    from elphdynamics_amd import hmc
    bp, bm = case.vector(5), case.vector(6)
    Fo, _ = _ssh_oracle_force(oracle, hv, bp, bm, 1e-11)
    F = np.zeros(m.Ndof)
    it, fl = hmc.calc_dSfdx_(F, m, bp, bm, None, power=1.0)
    assert F.size == m.Nph * m.Ltau == case.Nph * case.Ltau
    assert fl == 0 and rel(F, Fo) < 1e-8
    if D is not None:
        assert rel(F, D.force(bp, bm)[0]) < 1e-8


@pytest.mark.parametrize("name", sc.ALL)
def test_device_tables_and_matvecs(oracle, name):
    with _model(name) as (case, m):
        hv = _check_tables(case, m)
        _check_matvecs(oracle, case, m, sc.oracle_model(oracle, hv))


@pytest.mark.parametrize("name", sc.ALL)
def test_solves_vs_oracle(oracle, name):
    """As test_cg_vs_oracle (iteration count at 1e-5 with its knife-edge rule, early eps history to 1e-10, the 1e-13 solve to 1e-10)
    and test_batched_equals_single (three right-hand sides bit-identical to three single solves)."""
    from elphdynamics_amd import models
    with _model(name, tol=1e-5) as (case, m):
        hv = _check_tables(case, m)
        om = sc.oracle_model(oracle, hv)
        R, B = _rhs(oracle, om, case, 3)
        b = np.ascontiguousarray(B[0])
        x = np.zeros(m.Ndim)
        it, hist = models.solve_(x, m, b, tol=1e-5, history=True)
        xo, ito, histo = oracle.cg_solve(om, b, tol=1e-5, maxiter=20000, history=True)
        assert it == ito or (abs(it - ito) == 1 and (ito < 100 or abs(histo[min(it, ito)] / 1e-5 - 1) < 0.05)), (it, ito)
        n = min(41, it // 4 + 1)
        assert np.max(np.abs(hist[:n] - histo[:n]) / histo[:n]) < 1e-10
        assert hist[-1] < 1e-5 <= hist[-2]
        X = np.zeros_like(B)
        itb, resb, flb = models.ldiv_batched_(X, m, B)
        for i in range(3):
            xi = np.zeros(m.Ndim)
            it1, res1, fl1 = models.ldiv_(xi, m, np.ascontiguousarray(B[i]))
            assert it1 == itb[i] and fl1 == flb[i] == 0 and res1 == resb[i]
            assert np.array_equal(xi, X[i])
        assert np.array_equal(x, X[0])                                                       # deterministic re-run
        m.solver.tol = 1e-13
        x3 = np.zeros(m.Ndim)
        it3, res3, flag3 = models.ldiv_(x3, m, b)
        xo3, ito3, *_ = oracle.ldiv(om, b, solver_tol=1e-13, solver_maxiter=20000)
        assert flag3 == 0 and abs(it3 - ito3) <= max(3, ito3 // 100)
        assert rel(x3, xo3) < 1e-10
        if sc.is_dense(name):
            D = ref.DenseSSH(case.tab, case.Ltau, case.dtau, case.t, case.alpha, case.alpha2, case.mu, case.x)
            assert rel(x3, np.linalg.solve(D.M, R[0])) < 1e-10
        Mx = np.empty(m.Ndim)
        models.mulM_(Mx, m, x3)
        assert rel(Mx, R[0]) < 1e-8


@pytest.mark.parametrize("name", sc.ALL)
def test_kpm_vs_oracle(oracle, name):
    """As test_kpm_vs_oracle with the oracle's bounds injected: orders equal, kpm_ldiv_ to 1e-11, preconditioned iteration count
    equal.  'The preconditioner reduces the count' is asserted where the oracle's own counts show it (not a given at Ltau = 1, 2)."""
    from elphdynamics_amd import models, preconditioners as pc
    with _model(name, tol=1e-5) as (case, m):
        hv = _check_tables(case, m)
        om = sc.oracle_model(oracle, hv)
        n_arn = min(20, m.Nsites)
        oP = oracle.make_kpm(om, n=n_arn, buf=0.05, c1=1.0, c2=1.0)
        rng = np.random.default_rng(case.seed + 11)
        e_min, e_max = oracle.kpm_setup(oP, b_max=rng.standard_normal(m.Nsites), b_min=rng.standard_normal(m.Nsites))
        P = pc.SymmetricKPMPreconditioner(m, n_arn, 0.05, 1.0, 1.0)
        pc.setup_(P, e_min=e_min, e_max=e_max)
        assert P.active and oP.active == 1
        assert P.lam_lo == oP.lam_lo and P.lam_hi == oP.lam_hi
        Lo2 = (m.Ltau + 1) // 2
        assert np.array_equal(P.orders, oP._keep["order"][:Lo2])
        R, B = _rhs(oracle, om, case, 1)
        r, b = np.ascontiguousarray(R[0]), np.ascontiguousarray(B[0])
        z = np.empty(m.Ndim)
        pc.kpm_ldiv_(z, P, r)
        assert rel(z, oracle.kpm_apply(oP, r)) < 1e-11
        x = np.zeros(m.Ndim)
        it, hist = models.solve_(x, m, b, P=P, tol=1e-5, history=True)
        xo, ito, histo = oracle.cg_solve(om, b, tol=1e-5, maxiter=20000, P=oP, history=True)
        assert it == ito, (it, ito)
        n = min(21, it // 4 + 1)
        assert np.max(np.abs(hist[:n] - histo[:n]) / histo[:n]) < 1e-10
        x1, x0 = np.zeros(m.Ndim), np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x1, m, b, P=P)
        it0, res0, fl0 = models.ldiv_(x0, m, b)
        assert fl1 == 0 and fl0 == 0 and it1 == it
        _, ito_plain = oracle.cg_solve(om, b, tol=1e-5, maxiter=20000)
        if ito < ito_plain:
            assert it1 < it0
        assert rel(x1, x0) < 5e-3


@pytest.mark.parametrize("name", sc.ALL)
def test_fermion_force_vs_oracle(oracle, name):
    with _model(name, tol=1e-11) as (case, m):
        hv = _check_tables(case, m)
        D = ref.DenseSSH(case.tab, case.Ltau, case.dtau, case.t, case.alpha, case.alpha2, case.mu, case.x) if sc.is_dense(name) else None
        _check_force(oracle, case, m, hv, D)


@pytest.mark.parametrize("name", sc.BOTH_FAMILIES)
def test_generic_kernels_on_lane_program_lattices(oracle, name, monkeypatch):
    """ELPH_NO_FAST=1: the mat-vec and force checks once more on the generic LDS kernels, one case per lattice family."""
    assert sc.family(sc.make_case(name).tab)[0] == "lane"
    monkeypatch.setenv("ELPH_NO_FAST", "1")
    with _model(name, tol=1e-11) as (case, m):
        assert _wg_info(m)[0] == 0                        # (the resident solve belongs to the lane-program family: off with it)
        hv = _check_tables(case, m)
        D = _check_matvecs(oracle, case, m, sc.oracle_model(oracle, hv))
        _check_force(oracle, case, m, hv, D)


@pytest.mark.parametrize("name", sc.RESIDENT)
def test_wg_resident_cg_equals_the_two_kernel_iteration_on_ssh_shapes(oracle, name, monkeypatch):
    """The comparison of test_wg_resident_cg_equals_the_two_kernel_iteration (its helper, its switches, its bounds).  The resident
    solve takes four-colour lane programs of at most five sites per lane (elph_wg_usable): the honeycomb and the partial square
    model; the six-colour triangular lattice is outside it by design for bond phonons, stays on the streaming iteration, and the
    test says so."""
    with _model(name, tol=1e-5) as (case, m):
        fam, npl = sc.family(case.tab)
        expected = 1 if (fam == "lane" and case.tab.ncolours <= 4 and npl <= 5) else 0
        assert expected == (0 if name.startswith("tri") else 1)
        assert _wg_info(m)[0] == expected, name
        hv = _check_tables(case, m)
        R, B = _rhs(oracle, sc.oracle_model(oracle, hv), case, 3)
        variants = [{}, {"ELPH_WG_T": "1"}, {"ELPH_WG_T": "2"}, {"ELPH_WG_NO_DPP": "1", "ELPH_WG_T": "2"}, {"ELPH_WG_NO_DPP": "1", "ELPH_WG_T": "1"}]
        _wg_resident_vs_streaming(m, B, variants, monkeypatch, name)


@pytest.mark.parametrize("with_kpm", [False, True])
@pytest.mark.parametrize("name", sc.DYNAMICS)
def test_hmc_update_vs_oracle(oracle, name, with_kpm):
    """As test_ssh_hmc_update_vs_oracle: an accepted update, then a forced reject; 1e-6 on x and v, 1e-8 on H0."""
    from elphdynamics_amd import hmc, preconditioners as pc
    with _model(name, tol=1e-7) as (case, m):
        hv = _check_tables(case, m)
        om = sc.oracle_model(oracle, hv)
        fa = pc.FourierAccelerator(m)
        pc.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
        nt, dt, nb = 2, 0.05, 1
        n_arn = min(20, m.Nsites)
        Po = oracle.make_kpm(om, n=n_arn) if with_kpm else None
        P = pc.SymmetricKPMPreconditioner(m, n=n_arn, buf=0.05, c1=1.0, c2=1.0) if with_kpm else None
        H = hmc.HybridMonteCarlo(m, fa, dt, nt * dt, alpha=0.3, Nb=nb)
        H.v[:] = 0.2 * case.vector(30, m.Ndof)
        H.push_()
        for k, u in enumerate((0.0, 1.5)):      # accepted, then (u > 1) rejected
            rnd = dict(R=case.vector(31 + 4 * k, m.Ndof), Rp=case.vector(32 + 4 * k), Rm=case.vector(33 + 4 * k),
                       kpm_randn=case.vector(34 + 4 * k, (nt + 2) * 2 * m.Nsites) if with_kpm else None, u=u)
            x_in, v_in = m.x.copy(), H.v.copy()
            acc_o, x_o, v_o, info = oracle.hmc_update_ssh(om, x_in, v_in, m.omega, m.omega4, m.mu, m.dtau, fa.M, m.t, m.alpha, m.alpha2,
                                                          m.phonon_to_bond, m.checkerboard_perm, dt, nt, nb, 0.3, rnd, P=Po, tol=1e-7,
                                                          maxiter=20000)
            acc, its = hmc.update_(m, H, fa, P, randoms=rnd)
            assert acc == acc_o == (u == 0.0) and H.flag == 0 and info["flag"] == 0
            assert abs(H.H0 - info["H0"]) < 1e-8 * abs(info["H0"]) and abs(H.H1 - info["H1"]) < 1e-6 * abs(info["H1"])
            assert rel(m.x, x_o) < 1e-6 and rel(H.v, v_o) < 1e-6
            if not acc:
                assert np.array_equal(m.x, x_in)
            _check_tables(case, m)              # the device tables belong to the field the update left


@pytest.mark.parametrize("with_kpm", [False, True])
@pytest.mark.parametrize("name", sc.DYNAMICS)
def test_langevin_step_vs_oracle(oracle, name, with_kpm):
    """As test_ssh_langevin_step_vs_oracle_at_config_E: one Heun step, 1e-6 on the displacement, the iteration count within one."""
    from elphdynamics_amd import langevin, preconditioners as pc
    with _model(name, tol=1e-8) as (case, m):
        hv = _check_tables(case, m)
        om = sc.oracle_model(oracle, hv)
        fa = pc.FourierAccelerator(m)
        pc.update_Q_(fa, m, 0.0, np.inf, 0.7)
        n_arn = min(20, m.Nsites)
        Po = oracle.make_kpm(om, n=n_arn) if with_kpm else None
        P = pc.SymmetricKPMPreconditioner(m, n=n_arn, buf=0.05, c1=1.0, c2=1.0) if with_kpm else None
        dyn = langevin.HeunsDynamics(m, fa, 0.01)
        rnd = dict(eta=case.vector(40, m.Ndof), g1=case.vector(41), g2=case.vector(42),
                   kpm_randn=case.vector(43, 4 * m.Nsites) if with_kpm else None)
        x_in = m.x.copy()
        ssh = dict(t=m.t, alpha=m.alpha, alpha2=m.alpha2, phonon_to_bond=m.phonon_to_bond, cb_perm=m.checkerboard_perm)
        x_o, it_o = oracle.langevin_evolve_ssh(2, om, x_in, fa.Q, 0.01, rnd["eta"], rnd["g1"], rnd["g2"], m.omega, m.omega4, m.mu, m.dtau,
                                               ssh, P=Po, kpm_randn=rnd["kpm_randn"], tol=1e-8, maxiter=20000)
        it = langevin.evolve_(m, dyn, fa, P, randoms=rnd)
        assert dyn.flag == 0 and abs(it - it_o) <= 1
        assert rel(m.x - x_in, x_o - x_in) < 1e-6
