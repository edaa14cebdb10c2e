"""GPU parity of simple-cubic Holstein lattices in the 2 x 2 x 2 patch layout (pgrid_dev.h: pgrid::Cu; L x L x L with L = 6, 8 on one wavefront
per time slice, 10 on two, 12 on four) against the CPU oracle: the mat-vecs, the KPM apply, the preconditioned solve (one and several
right-hand sides, two resident chains with an expansion each, the p/x-fused iteration), the plan each solve took, and the patch kernels against
the kernels the lattice had before (ELPH_NO_PG=1, read per call).

Which kernels a case reaches.  6^3 and 8^3 (4 and 8 sites per lane) still fit the six-colour lane programs: their stand-alone mat-vecs and their
un-fused k_cg_ap are lane-program kernels (neither elph_mulM ... nor elph_bench_run's mat-vec unit reaches k_mul_pg on such a handle); the patch
layout gives them the Chebyshev recursion k_kpm_cheb_pg<Cu<1>> and, in the p/x-fused iteration, k_cg_ap_pg<Cu<1>, PX>.  A handle made with
ELPH_NO_FAST=1 has no lane program: there k_mul_pg<Cu<1>> and the un-fused k_cg_ap_pg<Cu<1>> run (test_matvec_one_wavefront_without_lane_program,
test_solve_without_lane_program).  10^3 and 12^3 are beyond the lane programs: every kernel of theirs is a patch kernel.  The batched mat-vec
launch has no entry of its own in the interface: it computes A x0 of a batched solve that starts from a non-zero guess and the true residuals a
batched solve returns (test_batched_matvec).

Every input is made on the CPU (fields and vectors from seeds, b = M^T R by the oracle, the eigenvalue bounds by the oracle's Arnoldi), so the
condition on the solves — the oracle's eps at its last iteration and at the one before differ from the tolerance by more than 1e-6 relative, so
that an equal iteration count is no coin toss — was checked without a device when the seeds were chosen (field seed 4343: the margins are 0.37
and more in every case below) and is asserted again by every solve."""
import numpy as np
import pytest

import cubic_cases as cc
from test_gpu_parity import _oracle_model, _pg_info, _px_fused, rel

pytestmark = pytest.mark.gpu

FIELD_SEED = 4343          # (chosen and checked on the CPU, module docstring)
TOL = 1e-5


def kpm_pair(oracle, m, om, seed=11):
    """The device's and the oracle's expansion on the oracle's own Arnoldi bounds (n = 20, as test_kpm_vs_oracle)."""
    from elphdynamics_amd import preconditioners as pc
    oP = oracle.make_kpm(om, n=20, buf=0.05, c1=1.0, c2=1.0)
    rng = np.random.default_rng(seed)
    e_min, e_max = oracle.kpm_setup(oP, b_max=rng.standard_normal(m.Nsites), b_min=rng.standard_normal(m.Nsites))
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, e_min=e_min, e_max=e_max)
    assert P.active and oP.active == 1
    assert P.lam_lo == oP.lam_lo and P.lam_hi == oP.lam_hi
    return P, oP


def rhs(oracle, oms, nrhs, ndim, seed=100):
    """b_r = M^T R_r on the CPU, right-hand side r on the configuration r % len(oms)."""
    from elphdynamics_amd import synth
    return np.stack([oracle.mulMT(oms[r % len(oms)], synth.randn(seed + r, ndim)) for r in range(nrhs)])


def oracle_solves(oracle, oms, oPs, B, tol):
    out = []
    for r in range(B.shape[0]):
        om, oP = oms[r % len(oms)], oPs[r % len(oPs)]
        b = np.ascontiguousarray(B[r])
        if tol == TOL:
            xo, ito, histo = oracle.cg_solve(om, b, tol=tol, maxiter=10000, P=oP, history=True)
            # the condition on the inputs: no knife edge at the stop test
            assert abs(histo[-1] / tol - 1) > 1e-6 and abs(histo[-2] / tol - 1) > 1e-6
            assert histo[-1] < tol <= histo[-2]
            out.append((xo, ito, histo))
        else:
            xo, ito, reso, flo = oracle.ldiv(om, b, P=oP, solver_tol=tol, solver_maxiter=10000)
            assert flo == 0
            out.append((xo, ito, None))
    return out


def check_plan(m, L, fused=None):
    assert _pg_info(m)[:4] == (4, 2, 2, cc.NW[L]), _pg_info(m)
    if fused is not None:
        assert _px_fused(m) is fused


def check_batched_solves(oracle, m, oms, P, oPs, B, L, fused=None):
    """tol = 1e-5: the oracle's iteration counts and flags; tol = 1e-13: its solutions within 1e-10."""
    from elphdynamics_amd import models
    ref = oracle_solves(oracle, oms, oPs, B, TOL)
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B, P=P)
    check_plan(m, L, fused)
    assert not fl.any() and [int(i) for i in it] == [r[1] for r in ref], (it, [r[1] for r in ref])
    for r in range(B.shape[0]):
        assert rel(X[r], ref[r][0]) < 1e-8          # (both within round-off of the same iterate: the same count)
    m.solver.tol = 1e-13
    ref13 = oracle_solves(oracle, oms, oPs, B, 1e-13)
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B, P=P)
    check_plan(m, L)
    assert not fl.any()
    for r in range(B.shape[0]):
        assert rel(X[r], ref13[r][0]) < 1e-10, r


# ------------------------------------------------------------------------------------------ mat-vecs

def check_matvecs(oracle, m):
    from elphdynamics_amd import models, synth
    om = _oracle_model(oracle, m)
    v, u, y = synth.randn(77, m.Ndim), synth.randn(78, m.Ndim), np.empty(m.Ndim)
    for fn, ofn in ((models.mulM_, oracle.mulM), (models.mulMt_, oracle.mulMT), (models.mulMtM_, oracle.mulMTM)):
        fn(y, m, v)
        assert rel(y, ofn(om, v)) < 1e-13
    Mv, Mtu = np.empty(m.Ndim), np.empty(m.Ndim)
    models.mulM_(Mv, m, v)
    models.mulMt_(Mtu, m, u)
    assert abs(u @ Mv - Mtu @ v) < 1e-11 * np.linalg.norm(u) * np.linalg.norm(v)          # adjointness
    return om


@pytest.mark.parametrize("L,ltau", [(6, 5), (8, 5), (10, 5), (12, 5), (12, 2)])
def test_matvec_vs_oracle(oracle, L, ltau):
    """One vector.  10^3 and 12^3: k_mul_pg<Cu<2>>, <Cu<4>>; 6^3 and 8^3: the lane program the handle keeps for them (module docstring)."""
    m = cc.cubic_model(L, ltau, seed=FIELD_SEED)
    try:
        check_matvecs(oracle, m)
        assert _pg_info(m)[:4] == (4, 2, 2, cc.NW[L])
    finally:
        m.close()


@pytest.mark.parametrize("L", [6, 8])
def test_matvec_one_wavefront_without_lane_program(oracle, L, monkeypatch):
    """k_mul_pg<Cu<1>>: a handle made with ELPH_NO_FAST=1 has no lane program and takes the patch mat-vec."""
    monkeypatch.setenv("ELPH_NO_FAST", "1")
    m = cc.cubic_model(L, 5, seed=FIELD_SEED)
    try:
        check_matvecs(oracle, m)
    finally:
        m.close()


@pytest.mark.parametrize("L,ltau", [(6, 5), (8, 5), (10, 5), (12, 5), (12, 2)])
def test_batched_matvec(oracle, L, ltau):
    """The batched mat-vec launch (three vectors at once) has two users in a batched solve: A x0 when the solve starts from a non-zero guess, and
    the true residuals |b - A x| / |b| it returns.  Un-preconditioned solves from x0 != 0: the oracle's iteration count from the same guess and
    its solution (a wrong A x0 would solve another system); the returned residual against the oracle's mat-vec on the returned x within 1e-12
    ABSOLUTE — it is already divided by |b|, and |A x| is about |b|: 1e-13 for the mat-vec, a factor of ten for the norm and the subtraction."""
    from elphdynamics_amd import models, synth
    m = cc.cubic_model(L, ltau, seed=FIELD_SEED, varied=(L == 8))
    try:
        om = _oracle_model(oracle, m)
        B = rhs(oracle, [om], 3, m.Ndim)
        X0 = np.stack([0.1 * synth.randn(300 + r, m.Ndim) for r in range(3)])
        X = X0.copy()
        it, res, fl = models.ldiv_batched_(X, m, B)
        assert not fl.any()
        for r in range(3):
            xo, ito, histo = oracle.cg_solve(om, np.ascontiguousarray(B[r]), x0=X0[r], tol=TOL, maxiter=10000, history=True)
            assert abs(histo[-1] / TOL - 1) > 1e-6 and abs(histo[-2] / TOL - 1) > 1e-6
            assert it[r] == ito and rel(X[r], xo) < 1e-8
            true = np.linalg.norm(B[r] - oracle.mulMTM(om, X[r])) / np.linalg.norm(B[r])
            assert abs(res[r] - true) < 1e-12
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ the KPM apply

@pytest.mark.parametrize("L,ltau", [(6, 8), (8, 8), (10, 8), (12, 8), (6, 40), (6, 7)])
def test_kpm_apply_vs_oracle(oracle, L, ltau):
    """elph_kpm_apply through k_kpm_cheb_pg<Cu<NW>>: Ltau = 8 on every side; 6^3 at Ltau = 40, where the lowest frequency recurses tens of
    times (asserted: an order of at least 20); an odd time axis, whose last frequency has no mirror."""
    from elphdynamics_amd import preconditioners as pc, synth
    m = cc.cubic_model(L, ltau, seed=FIELD_SEED, varied=(L == 8))
    try:
        om = _oracle_model(oracle, m)
        P, oP = kpm_pair(oracle, m, om)
        assert np.array_equal(P.orders, oP._keep["order"][:(ltau + 1) // 2])
        if ltau == 40:
            assert P.orders.max() >= 20
        r = synth.randn(55, m.Ndim)
        z = np.empty(m.Ndim)
        pc.kpm_ldiv_(z, P, r)
        assert rel(z, oracle.kpm_apply(oP, r)) < 1e-11
        assert _pg_info(m)[:4] == (4, 2, 2, cc.NW[L])
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ the preconditioned solve

@pytest.mark.parametrize("L,varied", [(6, False), (8, False), (8, True), (10, False), (12, False)])
def test_solve_one_rhs(oracle, L, varied):
    """One right-hand side at Ltau = 8 (the un-fused iteration: CH_PG with the lane program's k_cg_ap at 6^3 and 8^3, with k_cg_ap_pg beyond):
    the oracle's count and eps history at 1e-5, its solution at 1e-13.  varied: lambda and mu per site."""
    from elphdynamics_amd import models
    m = cc.cubic_model(L, 8, seed=FIELD_SEED, varied=varied)
    try:
        om = _oracle_model(oracle, m)
        P, oP = kpm_pair(oracle, m, om)
        B = rhs(oracle, [om], 1, m.Ndim)
        b = np.ascontiguousarray(B[0])
        (xo, ito, histo), = oracle_solves(oracle, [om], [oP], B, TOL)
        x = np.zeros(m.Ndim)
        it, hist = models.solve_(x, m, b, P=P, tol=TOL, history=True)
        check_plan(m, L, fused=False)
        assert it == ito
        n = min(len(hist), len(histo))
        assert np.max(np.abs(hist[:n] - histo[:n]) / histo[:n]) < 1e-10
        x1 = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x1, m, b, P=P)
        assert (it1, fl1) == (ito, 0)
        check_batched_solves(oracle, m, [om], P, [oP], B, L)
    finally:
        m.close()


@pytest.mark.parametrize("L", [6, 10])
def test_solve_three_rhs(oracle, L):
    m = cc.cubic_model(L, 8, seed=FIELD_SEED)
    try:
        om = _oracle_model(oracle, m)
        P, oP = kpm_pair(oracle, m, om)
        check_batched_solves(oracle, m, [om], P, [oP], rhs(oracle, [om], 3, m.Ndim), L, fused=False)
    finally:
        m.close()


@pytest.mark.parametrize("L", [8, 12])
def test_solve_two_chains(oracle, L):
    """Two resident configurations with an expansion each, two right-hand sides per chain (right-hand side r on chain r % 2)."""
    from elphdynamics_amd import models, preconditioners as pc, synth
    m = cc.cubic_model(L, 8, seed=FIELD_SEED)
    try:
        X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, omega=1.0, lam=1.0, seed=FIELD_SEED + 1 + c) for c in range(2)])
        models.update_model_chains_(m, X)
        oms, oPs, bounds = [], [], []
        for c in range(2):
            E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, X[c], m.lam, m.lam2, m.mu)
            oms.append(oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E))
            oPs.append(oracle.make_kpm(oms[c], n=20, buf=0.05, c1=1.0, c2=1.0))
            rng = np.random.default_rng(11 + c)
            bounds.append(oracle.kpm_setup(oPs[c], b_max=rng.standard_normal(m.Nsites), b_min=rng.standard_normal(m.Nsites)))
            assert oPs[c].active == 1
        P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
        act, lo, hi = pc.setup_chains_(P, e_min=np.array([b[0] for b in bounds]), e_max=np.array([b[1] for b in bounds]))
        assert all(act) and [float(v) for v in lo] == [oP.lam_lo for oP in oPs] and [float(v) for v in hi] == [oP.lam_hi for oP in oPs]
        check_batched_solves(oracle, m, oms, P, oPs, rhs(oracle, oms, 4, m.Ndim), L)
    finally:
        m.close()


# (L, Ltau, nrhs): the smallest even time axis and batch at which elph_plan_cg fuses — the forward transform takes the residual update and the
# inverse the p/x update (elph_plan_dft: the streaming matrix-core pair from 100 column-tile waves, one row group; found with _lib.dft_plan, no device)
FUSED = [(6, 8, 32), (8, 8, 16), (10, 16, 8), (12, 28, 6)]


@pytest.mark.parametrize("L,ltau,nrhs", FUSED)
def test_solve_fused(oracle, L, ltau, nrhs):
    """The p/x-fused iteration: k_cg_ap_pg<Cu<NW>, PX> + k_kpm_cheb_pg with r.z in frequency space, asserted taken."""
    from elphdynamics_amd import _lib
    assert _lib.dft_plan(ltau, 0, False, L ** 3, nrhs)["xr"] and _lib.dft_plan(ltau, 0, True, L ** 3, nrhs)["px"]
    assert not (_lib.dft_plan(ltau - 2, 0, False, L ** 3, nrhs)["xr"] and _lib.dft_plan(ltau - 2, 0, True, L ** 3, nrhs)["px"])
    m = cc.cubic_model(L, ltau, seed=FIELD_SEED)
    try:
        om = _oracle_model(oracle, m)
        P, oP = kpm_pair(oracle, m, om)
        check_batched_solves(oracle, m, [om], P, [oP], rhs(oracle, [om], nrhs, m.Ndim), L, fused=True)
    finally:
        m.close()


@pytest.mark.parametrize("L", [6, 8])
def test_solve_without_lane_program(oracle, L, monkeypatch):
    """The un-fused k_cg_ap_pg<Cu<1>> (a handle without a lane program, ELPH_NO_FAST=1)."""
    monkeypatch.setenv("ELPH_NO_FAST", "1")
    m = cc.cubic_model(L, 8, seed=FIELD_SEED)
    try:
        om = _oracle_model(oracle, m)
        P, oP = kpm_pair(oracle, m, om)
        check_batched_solves(oracle, m, [om], P, [oP], rhs(oracle, [om], 3, m.Ndim), L, fused=False)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ A/B on the device

@pytest.mark.parametrize("L,ltau,nrhs", [(6, 8, 32), (8, 8, 3), (10, 8, 3), (12, 8, 3)])
def test_patch_kernels_equal_the_previous_path(oracle, L, ltau, nrhs, monkeypatch):
    """One handle, ELPH_NO_PG=1 (the kernels a cubic lattice had before: the lane program and the LDS-slab recursion at 6^3 and 8^3, the generic
    LDS kernels beyond) against the patch kernels, read per call: equal iteration counts at 1e-5, solutions within 1e-10; the mat-vecs of the
    lattices beyond the lane programs within 1e-14."""
    from elphdynamics_amd import models, synth
    m = cc.cubic_model(L, ltau, seed=FIELD_SEED)
    try:
        om = _oracle_model(oracle, m)
        P, oP = kpm_pair(oracle, m, om)
        B = rhs(oracle, [om], nrhs, m.Ndim)
        v = synth.randn(9, m.Ndim)
        out = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("ELPH_NO_PG", mode)
            X = np.zeros_like(B)
            it, res, fl = models.ldiv_batched_(X, m, B, P=P)
            assert not fl.any()
            y = np.empty(m.Ndim)
            models.mulMtM_(y, m, v)
            out[mode] = (X, it, y, _px_fused(m))
        assert _pg_info(m)[:4] == (4, 2, 2, cc.NW[L])
        assert np.array_equal(out["0"][1], out["1"][1])
        assert rel(out["0"][0], out["1"][0]) < 1e-10
        assert rel(out["0"][2], out["1"][2]) < 1e-14
        if L == 6:
            assert out["0"][3] is True and out["1"][3] is False      # (the six-colour lane program has no fused iteration of its own)
    finally:
        m.close()
