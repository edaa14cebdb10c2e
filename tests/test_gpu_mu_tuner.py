"""GPU tests of the chemical-potential tuner's device side (csrc/density_moments.hip through elphdynamics_amd/mu_tuner.py).

elph_density_moments returns, per resident chain, the <N> and <N^2> that update_mu! averages over the pairs of the estimator's vectors.  The
reference value is `direct` below, an einsum restatement of the slice-by-slice identity
    C_pq(tau) = sum_site (M^-1 r_p)[site, tau] r_q[site, tau],  T_p = (1/L) sum_tau C_pp,  N_p = 2 (N - T_p),
    N_pq = (N_p + N_q) / 2,  N^2_pq = N_p N_q + T_p + T_q - (2/L) sum_tau C_pq C_qp
and the yardstick the same expression with the absolute value of every product,
    Y = sum_pairs [4 (N + |T|_p)(N + |T|_q) + |T|_p + |T|_q + (2/L) sum_tau |C|_pq |C|_qp].
Bounds: 1e-12 Y / npairs on N^2 and 1e-12 (N + |T|) on N (|T| the pairs' mean), the project's bound for reduced scalars (`compare` of
tests/test_gpu_measurements.py); against the measurement containers 2e-12 of the same yardsticks, each side meeting 1e-12 of the direct sum.

Vectors go in through greens.set_vectors_ (no solve) except in the end-to-end loop.  TILE = 5 rows of a wavefront's register tile and
64 sites per pass of the site axis (density_moments.hip) set the cases beyond the issue's list: n_v = 7 is two tiles (5 + 2), and the
20 x 13 lattice has N = 260 sites, four full passes and a ragged fifth (16 x 16 is exactly four passes, the small lattices part of one)."""
import copy
import os

import numpy as np
import pytest

from test_gpu_chain_measurements import chain_inputs, lockstep
from test_gpu_measurements import SHAPES, SQUARE, build_model

pytestmark = pytest.mark.gpu

TOL = 1e-12
SCALARS_ONLY = {"Greens": {"measure": False}}                              # a request that measures no correlation
SHAPES_HERE = dict(SHAPES, sq20x13=(1, (20, 13, 1), 3, SQUARE, None))


def direct(R, X, N, L):
    """(N, N^2, yardstick of N, yardstick of N^2) of one chain's vectors R, X = M^-1 R, each (n_v, N L) in the reference layout
    [site][tau]; the yardsticks are per pair (already divided by npairs)."""
    nv = R.shape[0]
    r, x = R.reshape(nv, N, L), X.reshape(nv, N, L)
    Cm, Ca = np.einsum("pst,qst->tpq", x, r), np.einsum("pst,qst->tpq", np.abs(x), np.abs(r))
    T, Ta = np.einsum("tpp->p", Cm) / L, np.einsum("tpp->p", Ca) / L
    S, Sa = np.einsum("tpq,tqp->pq", Cm, Cm), np.einsum("tpq,tqp->pq", Ca, Ca)
    Np = 2 * (N - T)
    n1 = n2 = y1 = y2 = 0.0
    npairs = 0
    for p in range(nv - 1):
        for q in range(p + 1, nv):
            n1 += (Np[p] + Np[q]) / 2
            n2 += Np[p] * Np[q] + T[p] + T[q] - (2.0 / L) * S[p, q]
            y1 += N + (Ta[p] + Ta[q]) / 2
            y2 += 4 * (N + Ta[p]) * (N + Ta[q]) + Ta[p] + Ta[q] + (2.0 / L) * Sa[p, q]
            npairs += 1
    return n1 / npairs, n2 / npairs, y1 / npairs, y2 / npairs


def resident(case, nch, nv, seed):
    """A model of SHAPES_HERE[case] with nch chains resident (one: the model's own configuration) and an estimator holding nv vectors per
    chain, vector v of chain c at row v nch + c."""
    from elphdynamics_amd import greens, models
    ns, dims, L, defs, _ = SHAPES_HERE[case]
    m = build_model(ns, dims, L, defs, seed=sum(dims) + L)
    X, _, R, MinvR = chain_inputs(m, nch, nv, seed)
    if nch > 1:
        models.update_model_chains_(m, X)
    est = greens.EstimateGreensFunction(m, nv=nv * nch)
    greens.set_vectors_(est, R, MinvR)
    return m, est


def check_against_direct(m, est, nch, got, label, factor=1.0):
    N, Nsqr = got
    worst = [0.0, 0.0]
    for c in range(nch):
        w1, w2, y1, y2 = direct(est.R[c::nch], est.MinvR[c::nch], m.Nsites, m.Ltau)
        worst = [max(worst[0], abs(N[c] - w1) / y1), max(worst[1], abs(Nsqr[c] - w2) / y2)]
    print(label, "worst deviation in units of the yardstick: N %.2e, Nsqr %.2e (bound %.1e)" % (worst[0], worst[1], factor * TOL))
    assert worst[0] <= factor * TOL and worst[1] <= factor * TOL, (label, worst)


@pytest.mark.parametrize("case,nch,nv", [("sq4x4", 3, 3), ("hc3x2", 3, 3), ("cubic3x2x2", 3, 3), ("sq4x4", 1, 2), ("hc3x2", 2, 7),
                                         ("sq16x16", 2, 3), ("sq20x13", 2, 3)])
def test_moments_match_the_direct_sums_of_each_chains_own_vectors(case, nch, nv):
    from elphdynamics_amd import mu_tuner as mt
    m, est = resident(case, nch, nv, seed=23)
    try:
        got = mt.density_moments(m, est, nch)
        check_against_direct(m, est, nch, got, "%s, %d chains, n_v = %d:" % (case, nch, nv))
        if nch > 1:                                                         # the chains' numbers differ: a mix-up of rows cannot pass
            assert len(set(got[0])) == nch and len(set(got[1])) == nch
    finally:
        m.close()


def check_against_container(m, est, nch, got, sums, label):
    """sums[c]: (density, Nsqr) of chain c's container, sums over the pairs."""
    nvc = est.nv // nch
    npairs = nvc * (nvc - 1) // 2
    for c in range(nch):
        _, _, y1, y2 = direct(est.R[c::nch], est.MinvR[c::nch], m.Nsites, m.Ltau)
        dens, nsqr = sums[c]
        assert dens.imag == 0 and nsqr.imag == 0
        d1, d2 = abs(got[0][c] - dens.real * m.Nsites / npairs) / y1, abs(got[1][c] - nsqr.real / npairs) / y2
        print(label, "chain %d: N %.2e, Nsqr %.2e of the yardstick (bound 2e-12)" % (c, d1, d2))
        assert d1 <= 2 * TOL and d2 <= 2 * TOL, (label, c, d1, d2)


def test_agrees_with_the_single_configuration_container():
    from elphdynamics_amd import measurements as ms, mu_tuner as mt
    m, est = resident("hc3x2", 1, 3, seed=4)
    try:
        c = ms.initialize_measurements_container(m, dict(SCALARS_ONLY, num_random_vectors=3), "")
        assert not c.onsite_corr
        ms.accumulate_(c, m, est)
        ms.fetch_(c, m)
        got = mt.density_moments(m, est)
        check_against_container(m, est, 1, got, [(c.global_meas["density"], c.global_meas["Nsqr"])], "single configuration,")
        check_against_direct(m, est, 1, got, "single configuration:")
    finally:
        m.close()


def test_agrees_with_the_chain_container():
    from elphdynamics_amd import chain_measurements as cms, mu_tuner as mt
    m, defs, cm, est, X, mu = lockstep("hc3x2", 3, 3, seed=6, table=SCALARS_ONLY)
    try:
        assert not cm.chains[0].onsite_corr
        cms.accumulate_(cm, m, est, X, mu=mu)
        cms.fetch_(cm, m)
        got = mt.density_moments(m, est, 3)
        check_against_container(m, est, 3, got, [(c.global_meas["density"], c.global_meas["Nsqr"]) for c in cm.chains], "Holstein chains,")
    finally:
        m.close()


def test_agrees_with_the_ssh_chain_container():
    """The entry point takes a bond-phonon handle as it takes a Holstein one."""
    from elphdynamics_amd import mu_tuner as mt, ssh_chain_measurements as scm
    from test_gpu_ssh_chain_measurements import lockstep as ssh_lockstep
    m, _, est, X, mu = ssh_lockstep("hc3", 3, 3, seed=12)
    try:
        cm = scm.initialize_ssh_chain_measurements_container(m, dict(SCALARS_ONLY, num_random_vectors=3), [""] * 3)
        scm.accumulate_(cm, m, est, X, mu=mu)
        scm.fetch_(cm, m)
        got = mt.density_moments(m, est, 3)
        check_against_container(m, est, 3, got, [(c.global_meas["density"], c.global_meas["Nsqr"]) for c in cm.chains], "SSH chains,")
        check_against_direct(m, est, 3, got, "SSH chains:")
    finally:
        m.close()


def test_repeats_bit_for_bit_and_chains_do_not_leak_into_one_another():
    from elphdynamics_amd import greens, mu_tuner as mt
    m, est = resident("hc3x2", 3, 7, seed=9)                                # two row tiles
    try:
        one = mt.density_moments(m, est, 3)
        two = mt.density_moments(m, est, 3)
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
        _, _, R2, M2 = chain_inputs(m, 3, 7, seed=90)
        Rn, Mn = est.R.copy(), est.MinvR.copy()
        Rn[1::3], Mn[1::3] = R2[1::3], M2[1::3]                             # the rows of chain 1 alone
        greens.set_vectors_(est, Rn, Mn)
        new = mt.density_moments(m, est, 3)
        for a, b in zip(one, new):
            assert a[0] == b[0] and a[2] == b[2] and a[1] != b[1]
        check_against_direct(m, est, 3, new, "after chain 1's rows changed:")
    finally:
        m.close()


def test_refusals_leave_the_handle_usable():
    from elphdynamics_amd import _lib, greens, models, mu_tuner as mt
    ns, dims, L, defs, _ = SHAPES["hc3x2"]
    m = build_model(ns, dims, L, defs, seed=3)
    try:
        lib = m._lib
        last = lambda: lib.elph_last_error().decode()  # noqa: E731
        out = np.zeros(8)
        call = lambda n: lib.elph_density_moments(m._h, n, _lib.dptr(out), _lib.dptr(out[4:]))  # noqa: E731
        assert call(1) == _lib.ELPH_E_STATE and "elph_greens_create has not been called" in last(), last()
        est = greens.EstimateGreensFunction(m, nv=3)
        assert call(1) == _lib.ELPH_E_STATE and "no vectors" in last(), last()
        rng = np.random.default_rng(1)
        greens.set_vectors_(est, rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim)))
        for n in (0, 2, 3):                                                 # one configuration is resident
            assert call(n) == _lib.ELPH_E_ARG and "%d chains" % n in last() and "1 are resident" in last(), last()
        assert lib.elph_density_moments(m._h, 1, None, _lib.dptr(out)) == _lib.ELPH_E_ARG and "null" in last(), last()
        assert call(1) == _lib.ELPH_OK
        check_against_direct(m, est, 1, (out[:1], out[4:5]), "after the refusals, one configuration:")
        # three chains resident, four vectors
        X, _, R, MinvR = chain_inputs(m, 3, 3, seed=5)
        models.update_model_chains_(m, X)
        assert call(1) == _lib.ELPH_E_ARG and "1 chains" in last() and "3 are resident" in last(), last()
        est4 = greens.EstimateGreensFunction(m, nv=4)
        greens.set_vectors_(est4, R[:4], MinvR[:4])
        assert call(3) == _lib.ELPH_E_STATE and "4 vectors" in last() and "3 resident chains" in last(), last()
        est3 = greens.EstimateGreensFunction(m, nv=3)                       # a vector per chain: no pair
        greens.set_vectors_(est3, R[:3], MinvR[:3])
        assert call(3) == _lib.ELPH_E_STATE and "a pair needs two" in last(), last()
        est9 = greens.EstimateGreensFunction(m, nv=9)                       # a new estimator drops the scratch; the next call makes it again
        assert call(3) == _lib.ELPH_E_STATE and "no vectors" in last(), last()
        greens.set_vectors_(est9, R, MinvR)
        check_against_direct(m, est9, 3, mt.density_moments(m, est9, 3), "after the refusals, three chains:")
        del est4, est3
    finally:
        m.close()


def tuners_for(m, init_mus, folder):
    from elphdynamics_amd import mu_tuner as mt
    return [mt.MuTuner(True, mu0, 0.9 * m.Nsites, m.Nsites, m.beta, m.dtau, 0.75, 0.5 * m.Nsites, os.path.join(folder, "mu_tuner_log_%d.out" % c))
            for c, mu0 in enumerate(init_mus)]


def replay(tuner, scratch_log):
    """A copy of the tuner that logs elsewhere: the host's step on the same numbers must give the same bits."""
    t = copy.deepcopy(tuner)
    t.logfile = scratch_log
    return t


def test_the_loop_end_to_end_with_a_tuner_per_chain(tmp_path):
    from elphdynamics_amd import chain_measurements as cms, greens, hmc, mu_tuner as mt, preconditioners as pc
    nch, nv = 3, 3
    ns, dims, L, defs, _ = SHAPES["sq4x4"]
    m = build_model(ns, dims, L, defs, seed=sum(dims) + L, tol=1e-10)
    try:
        fa = pc.FourierAccelerator(m)
        pc.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
        H = hmc.HybridMonteCarlo(m, fa, dt=0.05, tr=0.15, nchains=nch)
        H.X[:] = chain_inputs(m, nch, nv, seed=61)[0]
        H.push_()
        H.device_rng_(17)
        mu = np.stack([m.mu + 0.1 * c - 0.1 for c in range(nch)])           # a different mean per chain from the start
        tuners = tuners_for(m, mu.mean(axis=1), str(tmp_path))
        hmc.set_mu_(m, H, mu)
        est = greens.EstimateGreensFunction(m, nv=nv * nch)
        cm = cms.initialize_chain_measurements_container(m, dict(SCALARS_ONLY, num_random_vectors=nv), [""] * nch)
        rng = np.random.default_rng(8)
        for rnd in range(2):
            hmc.update_chains_(m, H, fa, None, pull=True)
            assert not H.flags.any(), (rnd, H.flags)
            _, _, fl = greens.update_(est, m, None, rng=rng)
            assert not fl.any()
            copies = [replay(t, str(tmp_path / "replay.out")) for t in tuners]
            before = mu.copy()
            mu = mt.tune_mu_chains_(m, tuners, est, mu, hmc=H)
            N, Nsqr = mt.density_moments(m, est, nch)                       # the numbers the step took: the call repeats bit for bit
            check_against_direct(m, est, nch, (N, Nsqr), "round %d:" % rnd)
            steps = []
            for c in range(nch):
                assert mt.update_mu_(copies[c], N[c], Nsqr[c]) == tuners[c].mu == tuners[c].mu_traj[-1]
                assert len(tuners[c].N_traj) == rnd + 1 and tuners[c].N_traj[-1] == N[c] and tuners[c].Nsqr_traj[-1] == Nsqr[c]
                dmu = tuners[c].mu - before[c].mean()
                steps.append(dmu)
                assert np.abs(mu[c] - before[c] - dmu).max() <= 4 * np.finfo(float).eps * max(1.0, np.abs(before[c]).max(), abs(dmu))
                assert abs(mu[c].mean() - tuners[c].mu) <= 1e-14 * max(1.0, abs(tuners[c].mu))
            assert len(set(steps)) == nch and all(s != 0.0 for s in steps)
            for given in (mu, None):                                        # handed over once, the container keeps the rows
                cms.accumulate_(cm, m, est, H.X, mu=given)
                cms.fetch_(cm, m)
                for c in range(nch):
                    g = cm.chains[c].global_meas["mu"]                      # a sum over the chain's three pairs
                    assert g.imag == 0 and abs(g.real - 3 * mu[c].mean()) <= 1e-12 * 3 * max(1.0, np.abs(mu[c]).mean())
                cms.reset_measurements_(cm, m)
        hmc.update_chains_(m, H, fa, None, pull=False)                       # the dynamics runs on with the chains' new mu
        assert not H.flags.any()
        for c in range(nch):
            lines = open(tuners[c].logfile).read().splitlines()
            assert len(lines) == 3 and lines[0] == mt.LOG_HEADER.strip()
    finally:
        m.close()


def test_the_loop_end_to_end_for_one_configuration(tmp_path):
    from elphdynamics_amd import greens, hmc, mu_tuner as mt, preconditioners as pc
    ns, dims, L, defs, _ = SHAPES["sq4x4"]
    m = build_model(ns, dims, L, defs, seed=sum(dims) + L, tol=1e-10)
    try:
        fa = pc.FourierAccelerator(m)
        pc.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
        H = hmc.HybridMonteCarlo(m, fa, dt=0.05, tr=0.15)
        H.device_rng_(19)
        tuner = tuners_for(m, [float(np.mean(m.mu))], str(tmp_path))[0]
        est = greens.EstimateGreensFunction(m, nv=3)
        rng = np.random.default_rng(9)
        for rnd in range(2):
            hmc.update_(m, H, fa, None)
            assert H.flag == 0
            _, _, fl = greens.update_(est, m, None, rng=rng)
            assert not fl.any()
            twin, before = replay(tuner, str(tmp_path / "replay.out")), m.mu.copy()
            mu1 = mt.tune_mu_(m, tuner, est, hmc=H)
            N, Nsqr = mt.density_moments(m, est)
            check_against_direct(m, est, 1, (N, Nsqr), "one configuration, round %d:" % rnd)
            assert mt.update_mu_(twin, N[0], Nsqr[0]) == mu1 == tuner.mu
            dmu = mu1 - before.mean()
            assert dmu != 0.0 and np.abs(m.mu - before - dmu).max() <= 4 * np.finfo(float).eps * max(1.0, np.abs(before).max(), abs(dmu))
        hmc.update_(m, H, fa, None)
        assert H.flag == 0
        assert len(open(tuner.logfile).read().splitlines()) == 3
    finally:
        m.close()
