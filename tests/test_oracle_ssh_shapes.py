"""CPU: the oracle's bond-phonon (SSH) code on every lattice family of tests/ssh_cases.py against the dense numpy restatement of
tests/ssh_reference.py — honeycomb, triangular (even and odd), odd and rectangular squares, chains, cubic, models with bare
bonds among phonon bonds, time axes of 1, 2, 7 and 161 slices; disordered t, alpha, alpha2 of both signs, mu per site.

The GPU tests (test_gpu_ssh_shapes.py) hold the device to the oracle on these shapes; this module is what pins the oracle there.
Bounds are those the 4 x 4 golden tests hold the oracle to (test_oracle_golden.py, test_oracle_hmc.py)."""
import ctypes as C

import numpy as np
import pytest

import ssh_cases as sc
import ssh_reference as ref
from test_gpu_parity import _ssh_oracle_force


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _dense(case):
    return ref.DenseSSH(case.tab, case.Ltau, case.dtau, case.t, case.alpha, case.alpha2, case.mu, case.x)


def test_every_case_builds_and_the_dense_rule_covers_each_family():
    """The couplings' regime is asserted where a case is built (ssh_cases.Case); every family has a dense-size case."""
    for name in sc.ALL:
        sc.make_case(name)
    for prefix in ("hc", "tri", "sq", "ch", "cu", "psq", "phc"):
        assert any(n.startswith(prefix) for n in sc.DENSE), prefix
    assert {"sq4_Lt1", "hc3_Lt2", "tri4_Lt7", "ch12_Lt161"} <= set(sc.DENSE)
    # every instantiated sites-per-lane count of the lane-program kernels, and the generic family on three kinds of lattice
    lane = {sc.family(sc.make_case(n).tab)[1] for n in sc.ALL if sc.family(sc.make_case(n).tab)[0] == "lane"}
    assert lane == set(range(1, 9)), lane
    generic = {n for n in sc.ALL if sc.family(sc.make_case(n).tab)[0] == "generic"}
    assert {"tri3", "tri5", "sq26", "hc18"} <= generic, generic


@pytest.mark.parametrize("name", sc.DENSE)
def test_tables_equal_the_dense_helpers(oracle, name):
    """calc_neighbor_table + initialize_checkerboard (product) and the oracle's table set-up against the helper's restatement of
    the same deterministic rule: table, colours, checkerboard_perm; phonon_to_bond of the partial models."""
    from elphdynamics_amd import lattice as lat
    case = sc.make_case(name)
    tab = case.tab
    la = lat.Lattice(case.norb, *case.Ls)
    raws = [la.calc_neighbor_table(d[0], d[1], d[2]) for d in case.definitions]
    assert [r.shape[0] for r in raws] == tab.per_definition
    raw = np.concatenate(raws, axis=0)
    assert np.array_equal(raw, tab.raw)
    cb = lat.initialize_checkerboard(raw)
    assert np.array_equal(cb["table"], tab.table) and np.array_equal(cb["colours"], tab.colours)
    assert np.array_equal(cb["cb_perm"], tab.cb_perm) and cb["ncolours"] == tab.ncolours
    oraw = oracle.neighbor_table(case.norb, *case.Ls, [(d[0], d[1], d[2]) for d in case.definitions])
    assert np.array_equal(oraw, tab.raw)
    otab, operm, oiperm, ogrp, ong = oracle.ssh_initialize_table(oraw)
    assert np.array_equal(otab, tab.table) and np.array_equal(operm, tab.cb_perm) and ong == tab.ncolours
    assert np.array_equal(operm[oiperm - 1], np.arange(1, tab.Nbonds + 1))
    # a colour is a set of site-disjoint bonds, and the colours come in blocks
    assert np.all(np.diff(tab.colours) >= 0)
    for g in range(1, tab.ncolours + 1):
        sites = tab.table[tab.colours == g].reshape(-1)
        assert len(set(sites)) == sites.size
    if not all(d[3] for d in case.definitions):
        assert 0 < tab.Nph < tab.Nbonds and not np.array_equal(tab.phonon_to_bond, np.arange(1, tab.Nph + 1))
        assert np.count_nonzero(tab.bond_to_phonon_cb) == tab.Nph


@pytest.mark.parametrize("name", sc.DENSE)
def test_update_model_matvecs_and_solve_vs_dense(oracle, name):
    from oracle.oracle import dp, ip
    case = sc.make_case(name)
    tab, L, N = case.tab, case.Ltau, case.N
    D = _dense(case)
    # update_model! (SSHModels.jl:510-562): bare bonds keep cosh / sinh(dtau t), phonon bonds get t'
    tcb = np.zeros(tab.Nbonds)
    tcb[tab.cb_perm - 1] = case.t
    c = np.ascontiguousarray(np.repeat(np.cosh(case.dtau * tcb)[:, None], L, axis=1)).reshape(-1)
    s = np.ascontiguousarray(np.repeat(np.sinh(case.dtau * tcb)[:, None], L, axis=1)).reshape(-1)
    Emu = np.zeros(N)
    oracle.lib.elpho_update_model_ssh(N, L, tab.Nbonds, tab.Nph, case.dtau, dp(case.x), dp(case.t), dp(case.alpha), dp(case.alpha2),
                                      dp(case.mu), ip(tab.phonon_to_bond), ip(tab.cb_perm), dp(c), dp(s), dp(Emu))
    assert rel(c, D.cosht.reshape(-1)) < 1e-15 and rel(s, D.sinht.reshape(-1)) < 1e-15 and rel(Emu, D.expDtauMu) < 1e-15
    om = oracle.make_model(1, N, L, tab.table, c, s, Emu)
    v = case.vector(1)
    assert rel(oracle.mulM(om, v), D.M @ v) < 1e-13
    assert rel(oracle.mulMT(om, v), D.M.T @ v) < 1e-13
    assert rel(oracle.mulMTM(om, v), D.A @ v) < 1e-13
    R = case.vector(2)
    b = D.M.T @ R
    x, it, res, fl = oracle.ldiv(om, np.ascontiguousarray(b), solver_tol=1e-13, solver_maxiter=20000)
    assert fl == 0 and rel(x, D.solve(b)) < 1e-10
    assert rel(x, np.linalg.solve(D.M, R)) < 1e-10                      # M^-1 R, the Green's-function observable


@pytest.mark.parametrize("name", sc.DENSE)
def test_muldMdx_and_fermion_force_vs_dense(oracle, name):
    from oracle.oracle import dp, ip
    case = sc.make_case(name)
    tab = case.tab
    hv = sc.host_view(case)
    om = sc.oracle_model(oracle, hv)
    D = _dense(case)
    u, v = case.vector(3), case.vector(4)
    d = np.zeros(hv.Ndof)
    oracle.lib.elpho_muldMdx_ssh(dp(d), dp(u), C.byref(om), dp(v), case.dtau, ip(tab.bond_to_phonon_cb), dp(case.alpha), dp(case.alpha2),
                                 dp(case.x), tab.Nph)
    assert rel(d, D.dMdx(u, v)) < 1e-10
    bp, bm = case.vector(5), case.vector(6)
    F, Sf = _ssh_oracle_force(oracle, hv, bp, bm, 1e-13)
    Fd, Sfd = D.force(bp, bm)
    assert F.size == tab.Nph * case.Ltau
    assert rel(F, Fd) < 1e-10 and abs(Sf - Sfd) < 1e-10 * abs(Sfd)


def test_dense_force_is_the_complex_step_gradient_when_alpha2_vanishes():
    """The helper's own cross-check: with alpha2 = 0 the reference's force is the true gradient of the dense S_f — on the partial
    honeycomb model (bare bonds among phonon bonds, mu per site, disordered t and alpha)."""
    case = sc.make_case("phc4")
    zero = np.zeros(case.Nph)
    D = ref.DenseSSH(case.tab, case.Ltau, case.dtau, case.t, case.alpha, zero, case.mu, case.x)
    bp, bm = case.vector(7), case.vector(8)
    F, _ = D.force(bp, bm)
    G = ref.complex_step_gradient(case.tab, case.Ltau, case.dtau, case.t, case.alpha, case.mu, case.x, bp, bm)
    assert rel(F, G) < 1e-11


@pytest.mark.parametrize("name", sc.DENSE)
def test_kpm_vs_dense_polynomial(oracle, name):
    """kpm_apply against the dense Chebyshev polynomial of the tau-MEAN matrix with the oracle's own expansion coefficients
    (update_A! for bond phonons, KPMPreconditioners.jl:355-381), and the preconditioned solve against the plain one."""
    case = sc.make_case(name)
    hv = sc.host_view(case)
    om = sc.oracle_model(oracle, hv)
    P = oracle.make_kpm(om, n=min(20, case.N), buf=0.05, c1=1.0, c2=1.0)
    rng = np.random.default_rng(case.seed)
    oracle.kpm_setup(P, b_max=rng.standard_normal(case.N), b_min=rng.standard_normal(case.N))
    assert P.active == 1
    Lo2 = (case.Ltau + 1) // 2
    orders, coff = P._keep["order"][:Lo2], P._keep["coff"]
    cz = P._keep["coeff"]
    coeffs = [cz[2 * coff[w]:2 * (coff[w] + orders[w]):2] + 1j * cz[2 * coff[w] + 1:2 * (coff[w] + orders[w]):2] for w in range(Lo2)]
    r = case.vector(9)
    dense = ref.dense_kpm_apply(case.tab, case.Ltau, hv.cosht, hv.sinht, hv.expDtauMu, P.lam_lo, P.lam_hi, orders, coeffs, r)
    assert rel(oracle.kpm_apply(P, r), dense) < 1e-12
    b = oracle.mulMT(om, case.vector(2))
    x0, it0, res0, fl0 = oracle.ldiv(om, b, solver_tol=1e-13, solver_maxiter=20000)
    x1, it1, res1, fl1 = oracle.ldiv(om, b, P=P, solver_tol=1e-13, solver_maxiter=20000)
    assert fl0 == 0 and fl1 == 0 and rel(x1, x0) < 1e-10


@pytest.mark.parametrize("name", ["hc3", "psq6"])
def test_hmc_update_vs_dense_leapfrog(oracle, name):
    """One elpho_hmc_update_ssh trajectory against a dense leapfrog built from the helper (exact solves, the reference's force);
    bounds of test_oracle_hmc.py::test_ssh_trajectory_matches_dense_golden."""
    case = sc.make_case(name)
    hv = sc.host_view(case)
    om = sc.oracle_model(oracle, hv)
    faM = ref.accelerator_mass(case.Ltau, case.dtau, case.omega)
    dt, nt = 0.05, 4
    rnd = dict(R=case.vector(10, case.Nph * case.Ltau), Rp=case.vector(11), Rm=case.vector(12), u=0.0, kpm_randn=None)
    g = ref.dense_leapfrog(_dense(case), case.omega, case.omega4, faM, case.x, rnd["R"], rnd["Rp"], rnd["Rm"], dt, nt)
    acc, x1, v1, info = oracle.hmc_update_ssh(om, case.x, np.zeros(case.x.size), case.omega, case.omega4, case.mu, case.dtau,
                                              np.ascontiguousarray(faM).reshape(-1), case.t, case.alpha, case.alpha2,
                                              case.tab.phonon_to_bond, case.tab.cb_perm, dt, nt, 1, 0.0, rnd, tol=1e-7, maxiter=20000)
    assert acc and info["flag"] == 0
    assert abs(info["H0"] - g["H0"]) < 1e-9 * abs(g["H0"])
    assert abs(info["H0"] - g["H0_closed"]) < 1e-9 * abs(g["H0"])
    assert abs(info["H1"] - g["H1"]) < 1e-6
    assert rel(x1, g["x1"]) < 1e-6 and rel(v1, g["v1"]) < 1e-6
