"""GPU (-m gpu): site-dependent ω, ω₄, λ, λ₂ and μ (assign_omega!, assign_lambda!, assign_mu! ... per orbital and with a standard
deviation, HolsteinModels.jl:323-420; one generator: tests/site_disorder_cases.py) on every caller and kernel form that reads a
parameter by site: par[s] and lam3[s] of the force, muldMdx and Λ kernels over the (block size, sites per thread) classes of the
generic kernels, exp(−Δτ V), ϕ±, dS_b/dx and S_b of the resident dynamics (hmc.hip), their [chain][ndim] forms, the per-chain row of μ,
and the special moves, whose swap changes S_b only when ω and ω₄ differ from site to site.

Every test is the twin of a uniform test and runs that test's checker with the disorder as its prepare= hook: the assertions and
their bounds are the twin's, nothing is restated here.  tests/test_site_disorder_host.py shows on the CPU oracle that a parameter
read one site off, or from the other orbital, moves every quantity asserted here by at least 1000 bounds.
The sharded twins (a slab's slice of every array) are in tests/test_gpu_shard.py.
"""
import numpy as np
import pytest

import site_disorder_cases as sdc
import special_update_reference as sur
from test_gpu_hmc import (assert_chain_ends_as_the_single_chain, assert_special_actions, chain_randoms, chains_inputs,
                          check_hmc_chains_in_lockstep_equal_single_chain_updates, check_hmc_update_vs_oracle,
                          check_hmc_update_with_kpm_vs_oracle, check_special_moves_of_chains_equal_single_chain_moves)
from test_gpu_langevin import check_langevin_chains_match_single_trajectories, check_langevin_step_vs_oracle
from test_gpu_muldmdx import check_muldMdx_holstein_device_pointer_twin, check_muldMdx_holstein_vs_oracle
from test_gpu_parity import (_oracle_model, check_calc_OinvLambda_phi_vs_oracle, check_fermion_force_is_the_gradient_of_the_action,
                             check_fermion_force_vs_oracle, check_matvec_vs_oracle)
from test_gpu_special_updates import check_device_drawn_moves_equal_their_explicit_replay

pytestmark = pytest.mark.gpu

# tag: (sites, threads per workgroup, sites per thread) of the generic kernels (kernels.hip: gen_bs, gen_npl) — each class once,
# on the smallest configuration that has it
FORCE_SHAPES = {"d": (18, 64, 1), "q": (100, 64, 2), "z": (200, 64, 4), "Y": (512, 64, 8), "g": (576, 320, 2), "l34": (1156, 640, 2),
                "l64": (4096, 1024, 4)}
FORCE_TAGS = list(FORCE_SHAPES)
# b: lane program; d; t: odd triangular, ragged colours; q: GRID; z: HGRID, two cells per lane; r: rectangle; t12, k: PGRID; g: several wavefronts
DYNAMICS_TAGS = ["b", "d", "t", "q", "z", "r", "t12", "k", "g"]


def _generic_shape(N):
    """gen_bs / gen_npl of kernels.hip restated: one wave up to 512 sites, beyond that one thread per two sites, at most 1024.
    A restatement, not a reading of what the device launched: it says why these tags were chosen and keeps the table above
    consistent with itself; if kernels.hip changes its rule this does not follow."""
    bs = 64 if N <= 512 else min(1024, 64 * -(-(N // 2) // 64))
    return bs, -(-N // bs)


def _disordered(tag, **kw):
    from elphdynamics_amd import configs
    return sdc.prepare(tag)(configs.make_model(tag, **kw))


# ------------------------------------------------------------------------------------------ update_model! and the mat-vecs

@pytest.mark.parametrize("tag", FORCE_TAGS)
def test_matvec_with_site_disorder_vs_oracle(oracle, tag):
    """mulM, mulMᵀ, mulMᵀM (1e-13) of the disordered model against the oracle's, E from the oracle's update_model! on m.lam, m.lam2, m.mu."""
    m = _disordered(tag)
    N, bs, npl = FORCE_SHAPES[tag]
    assert m.Nsites == N and _generic_shape(N) == (bs, npl) and (bs * npl == N) == (tag in ("Y", "l64"))      # the other classes are ragged
    for k in ("omega", "omega4", "lam", "lam2", "mu"):
        assert len(np.unique(getattr(m, k))) == N
    check_matvec_vs_oracle(oracle, m)
    m.close()


# ------------------------------------------------------------------------------------------ the fermion force and its pieces

@pytest.mark.parametrize("tag", FORCE_TAGS)
def test_fermion_force_with_site_disorder_vs_oracle(oracle, tag):
    check_fermion_force_vs_oracle(oracle, tag, prepare=sdc.prepare(tag))


def test_fermion_force_with_site_disorder_is_the_gradient_of_the_action(oracle):
    """Probed: the first element and one of site 2 (the first orbital, two cells), one each of sites 1 and 5 (the second orbital) and
    the last element of the field."""
    def probes(m):
        L, orb = m.Ltau, sdc.orbitals(m)
        p = (0, L, 2 * L + 7, 5 * L + 3, m.Ndim - 1)
        assert [int(orb[k // L]) for k in p] == [0, 1, 0, 1, 1]
        return p
    check_fermion_force_is_the_gradient_of_the_action(oracle, "d", probes, prepare=sdc.prepare("d"))


@pytest.mark.parametrize("tag", ["d", "z", "g"])
def test_muldMdx_with_site_disorder_vs_oracle(oracle, tag):
    check_muldMdx_holstein_vs_oracle(oracle, tag, prepare=sdc.prepare(tag))


@pytest.mark.parametrize("tag", ["d", "z", "g"])
def test_muldMdx_device_pointer_twin_with_site_disorder(tag):
    from elphdynamics_amd import _lib
    check_muldMdx_holstein_device_pointer_twin(_lib.load(), tag, prepare=sdc.prepare(tag))


def test_calc_OinvLambda_phi_with_site_disorder_vs_oracle(oracle):
    """k_lambda_rhs with a different λ on the two orbitals."""
    check_calc_OinvLambda_phi_vs_oracle(oracle, "d", prepare=sdc.prepare("d"))


# ------------------------------------------------------------------------------------------ the resident dynamics against the oracle

@pytest.mark.parametrize("tag,nb", [(t, 1) for t in DYNAMICS_TAGS] + [("d", 3)])
def test_hmc_update_with_site_disorder_vs_oracle(oracle, tag, nb):
    check_hmc_update_vs_oracle(oracle, tag, nb, 2, prepare=sdc.prepare(tag))


def test_hmc_update_with_site_disorder_and_the_kpm_preconditioner(oracle):
    check_hmc_update_with_kpm_vs_oracle(oracle, "d", prepare=sdc.prepare("d"))


@pytest.mark.parametrize("tag,scheme,with_kpm", [("d", s, k) for s in (0, 1, 2) for k in (False, True)]
                         + [("b", 2, False), ("q", 2, True), ("z", 2, True), ("t12", 2, True)])
def test_langevin_step_with_site_disorder_vs_oracle(oracle, tag, scheme, with_kpm):
    """Two steps; the shifted action's lam_shift[s] term (k_hmc_dsb) meets a λ that depends on the site."""
    check_langevin_step_vs_oracle(oracle, tag, scheme, with_kpm, prepare=sdc.prepare(tag))


# ------------------------------------------------------------------------------------------ chains in lockstep

@pytest.mark.parametrize("tag,nch,with_kpm", [("d", 3, False), ("q", 3, True), ("z", 2, False)])
def test_hmc_chains_with_site_disorder_equal_single_chain_updates(tag, nch, with_kpm):
    """The single-chain updates are held to the oracle above: an index error of the [chain][ndim] forms shows here."""
    check_hmc_chains_in_lockstep_equal_single_chain_updates(tag, nch, 1, with_kpm, prepare=sdc.prepare(tag))


def test_langevin_chains_with_site_disorder_match_single_trajectories():
    check_langevin_chains_match_single_trajectories("d", 1, True, prepare=sdc.prepare("d"))


@pytest.mark.parametrize("tag,nch", [("d", 3), ("q", 2)])
def test_a_chemical_potential_per_chain_and_site(tag, nch):
    """elph_hmc_set_mu_chains with rows that differ in every site (k_hmc_expV: mu_ch[(i / ndim) * N + s]): after one lockstep update
    chain c is where the single chain with m.mu = mu[c] ends; then the rows are installed again in another order, and the next
    update follows the new rows — the bounds of the lockstep twin."""
    from elphdynamics_amd import hmc, models, preconditioners as pc
    nt, dt = 4, 0.05

    def make():
        m = _disordered(tag, tol=1e-9, maxiter=20000)
        fa = pc.FourierAccelerator(m)
        pc.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
        return m, fa

    m, fa = make()
    mu = sdc.chain_mu(m, nch, sdc.seed_of(tag))
    assert mu.shape == (nch, m.Nsites) and all(not np.allclose(mu[a], mu[b]) for a in range(nch) for b in range(a))
    X0, V0, rnd = chains_inputs(m, nch, nt, False)
    H = hmc.HybridMonteCarlo(m, fa, dt=dt, tr=nt * dt, alpha=0.2, Nb=1, nchains=nch)
    H.X[:], H.V[:] = X0, V0
    H.push_()
    rounds = []
    for rows in (mu, mu[np.roll(np.arange(nch), 1)]):
        start = (H.X.copy(), H.V.copy())
        hmc.set_mu_(m, H, rows)
        acc, its = hmc.update_chains_(m, H, fa, None, randoms=rnd, pull=True)
        assert not H.flags.any()
        rounds.append((rows, start, acc.copy(), its.copy(), H.X.copy(), H.V.copy(), H.energies.copy()))
    m.close()
    assert not np.array_equal(rounds[0][4], rounds[1][4])
    for rows, (Xs, Vs), acc, its, Xb, Vb, Eb in rounds:
        for c in range(nch):
            m1, fa1 = make()
            m1.mu[:] = rows[c]
            m1.x[:] = Xs[c]
            models.update_model_(m1)
            H1 = hmc.HybridMonteCarlo(m1, fa1, dt=dt, tr=nt * dt, alpha=0.2, Nb=1)
            H1.v[:] = Vs[c]
            H1.push_()
            a1, i1 = hmc.update_(m1, H1, fa1, None, randoms=chain_randoms(rnd, c, False))
            assert_chain_ends_as_the_single_chain(c, a1, i1, m1, H1, acc, its, Xb, Vb, Eb, Xs)
            m1.close()


# ------------------------------------------------------------------------------------------ special moves

def test_special_moves_with_site_disorder_vs_oracle(oracle):
    """A reflection on each orbital and the swap of the two columns tests/test_site_disorder_host.py holds to |ΔS_b| >= 1e-3 |S_b|
    (k_hmc_sb_part with ω, ω₄ of the site) against oracle.special_move: S₀ and S₁ at the bounds of the golden twin, the decision for
    a u on either side of P and at least 1e-6 away from it, the field bit for bit.  P = min(1, e^{−(S₁−S₀)}) <= 1 inherits the
    bounds of the two actions: |ΔP| <= 1e-11 |S₀| + 1e-8 |S₁|."""
    from elphdynamics_amd import hmc, preconditioners as pc, synth
    m = _disordered("d", tol=1e-6, maxiter=20000)
    fa = pc.FourierAccelerator(m)
    pc.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
    i, j = sdc.swap_columns(m)
    orb = sdc.orbitals(m)
    assert (i, j) == (0, 1) and orb[2] == 0 and orb[3] == 1
    assert abs(sdc.swap_delta_Sb(m, i, j)) >= 1e-3 * abs(sdc.bosonic_action(m))
    Rp, Rm = synth.randn(3100, m.Ndim), synth.randn(3101, m.Ndim)
    x_in = m.x.copy()

    def oracle_move(kind, ci, cj, u):
        m.x[:] = x_in
        return oracle.special_move(_oracle_model(oracle, m), x_in, kind, ci, cj, Rp, Rm, u, m.omega, m.omega4, m.lam, m.lam2, m.mu, m.dtau,
                                   tol=1e-6, maxiter=20000)

    decisions = set()
    for kind, ci, cj in ((hmc.REFLECT, 2, 0), (hmc.REFLECT, 3, 0), (hmc.SWAP, i, j)):
        P = oracle_move(kind, ci, cj, 0.5)[2]["P"]
        us = [u for u in (0.5 * P, 0.5 * (1.0 + P), 1.5) if abs(u - P) > 1e-6]
        assert any(u > P for u in us)
        for u in us:
            acc_o, x_o, info = oracle_move(kind, ci, cj, u)
            m.x[:] = x_in
            H = hmc.HybridMonteCarlo(m, fa, 0.05, 0.1)
            acc, S0, S1, it, fl = hmc.special_move_(m, H, kind, ci, cj, randoms=dict(Rp=Rp, Rm=Rm, kpm_randn=None, u=u))
            H.pull_()
            print(f"special move {kind} ({ci}, {cj}) u = {u:.6f}: P = {info['P']:.6e}, S0 {S0:.12e} vs {info['S0']:.12e}, S1 {S1:.12e} vs {info['S1']:.12e}")
            assert fl == 0 and info["flag"] == 0 and info["P"] == P
            assert_special_actions(S0, S1, info["S0"], info["S1"])
            assert abs(min(1.0, np.exp(-(S1 - S0))) - P) <= 1e-11 * abs(info["S0"]) + 1e-8 * abs(info["S1"])
            assert acc == acc_o == (u < P)
            assert np.array_equal(m.x, x_o)
            decisions.add(bool(acc))
    assert decisions == {True, False}
    m.close()


@pytest.mark.parametrize("with_kpm", [False, True])
def test_special_moves_of_chains_with_site_disorder_equal_single_chain_moves(with_kpm):
    check_special_moves_of_chains_equal_single_chain_moves(with_kpm, tag="d", prepare=sdc.prepare("d"))


@pytest.mark.parametrize("kind,nch", [(sur.SWAP, 3), (sur.REFLECT, 1)])
def test_device_drawn_moves_with_site_disorder_equal_their_explicit_replay(kind, nch):
    check_device_drawn_moves_equal_their_explicit_replay("d", kind, nch, False, prepare=sdc.prepare("d"))
