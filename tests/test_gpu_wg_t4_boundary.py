"""The team-boundary work of the 4-slice workgroup-resident CG iteration (csrc/cg_wg.hip: 16 x 16 DPP form, ELPH_WG_T=4): the boundary
wave W-1's static priority and the order of the fused pass's stores of r' around the barrier behind it (boundary slices in front of it,
interior slices behind it).  The bits of 25 iterations are pinned by test_gpu_wg_t4_chain.py and test_gpu_wg_t4_tail.py; here are the paths those do not
take at this shape:
  * the cancellation branch (a second meeting between the poll window and the pass) in teams of two and three workgroups;
  * a batch of more than one round of 48 right-hand sides (the kernel must not depend on which round a right-hand side runs in);
  * solves that run to their tolerance on the team of five, whose right-hand sides leave through `done` at different iterations.

Tolerances: the cancellation case takes those of test_gpu_wg_fused_tail.py::test_cancellation_branch (1e-10 at tol = 1e-10), the solve
those of test_gpu_wg_t4_tail.py (|X - X_two_kernel| / |X| < 1e-11, |M x - R| / |R| < 1e-9 with the oracle's M at tol = 1e-13)."""
import numpy as np
import pytest

import wg_t4_chain_cases as chain
import wg_t4_tail_cases as cases

pytestmark = pytest.mark.gpu

SWITCHES = ("ELPH_NO_WG", "ELPH_WG_T", "ELPH_WG_NO_DPP", "ELPH_WG_W", "ELPH_WG_ALWAYS")
NRHS = 3
MU_CANCEL = -80.0               # test_gpu_wg_fused_tail.py: the least negative of -20, -40, -80 at which the oracle's history cancels


def _oracle_model(orc, m):
    """The oracle's model of the GPU model's (Holstein) tables and fields."""
    E = orc.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
    return orc.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _env(mp, **kw):
    for k in SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in kw.items():
        mp.setenv(k, v)


@pytest.mark.parametrize("ltau", [64, 96])
def test_cancellation_branch_in_teams_of_two_and_three(oracle, monkeypatch, ltau):
    """mu = -80 (test_gpu_wg_fused_tail.py::test_cancellation_branch: M^T M close to the identity, every step shrinks r.r by ~2e-7, the
    identity for r'.r' cancels and the direct sum is taken in a second meeting) on 64 and 96 slices at 4 slices per wave: 3 right-hand
    sides against the two-kernel iteration — the same iteration counts, |X - X_two_kernel| / |X| < 1e-10 — and the oracle's own history
    has a cancelling step."""
    from elphdynamics_amd import configs, models
    m = cases.model(ltau)
    try:
        m.assign_mu_(MU_CANCEL)
        models.update_model_(m)
        om = _oracle_model(oracle, m)
        _, B = configs.rhs(m, NRHS)
        out = {}
        for name, env in (("two-kernel", {"ELPH_NO_WG": "1"}), ("resident", {"ELPH_WG_T": "4"})):
            _env(monkeypatch, **env)
            if name == "resident":
                assert cases.wg_shape(m, 1) == cases.SHAPES[ltau], cases.wg_shape(m, 1)
                assert cases.resident_plan(m, 1)["resident"] == 1
            X, its = np.zeros((NRHS, m.Ndim)), []
            for i in range(NRHS):
                its.append(models.solve_(X[i], m, np.ascontiguousarray(B[i]), tol=1e-10))
            out[name] = (X, its)
        assert cases.wg_fallbacks(m) == (0, 0)
        for i in range(NRHS):
            _, _, histo = oracle.cg_solve(om, np.ascontiguousarray(B[i]), tol=1e-10, maxiter=10000, history=True)
            ratio = (histo[1:] / histo[:-1]) ** 2
            assert ratio.min() < 1e-4, ratio                  # the oracle's own history has a step that cancels
        (Xw, itw), (Xs, its) = out["resident"], out["two-kernel"]
        print(f"Ltau {ltau}: iterations resident {itw} two-kernel {its}; |X - X_two_kernel| / |X| = {rel(Xw, Xs):.2e}")
        assert itw == its
        assert rel(Xw, Xs) < 1e-10
    finally:
        m.close()


def test_rows_of_a_batch_of_more_than_one_round(monkeypatch):
    """Config C at 4 slices per wave, 50 right-hand sides on 25 chains (right-hand side r runs on chain r % 25), 25 fixed iterations
    from x0 = 0: two right-hand sides more than one round of 48.  Rows 0, 24, 48 and 49 equal, bit for bit, the same rows run as the
    batch of their chain's two right-hand sides; no launch gave up."""
    from elphdynamics_amd import configs, models, synth
    nrhs, nchains = 50, 25
    _env(monkeypatch, ELPH_WG_T="4")
    m = configs.make_model("C", tol=1e-5)
    try:
        _, B = configs.rhs(m, nrhs)
        Xc = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=synth.SEED_FIELDS + 17 * c) for c in range(nchains)])
        models.update_model_chains_(m, Xc)
        shape = chain.wg_shape(m, nrhs)
        assert shape == (1, 4, 8, 5), shape
        X = chain.fixed_iterations_from_zero(m, B)
        assert chain.wg_fallbacks(m) == (0, 0)
        for c in sorted({r % nchains for r in (0, 24, 48, 49)}):
            models.update_model_chains_(m, Xc[[c]])
            assert chain.wg_shape(m, 2) == shape, chain.wg_shape(m, 2)
            X2 = chain.fixed_iterations_from_zero(m, B[[c, c + nchains]])
            for k, r in enumerate((c, c + nchains)):
                if r in (0, 24, 48, 49):
                    same = np.array_equal(X[r].view(np.uint64), X2[k].view(np.uint64))
                    print(f"row {r} (chain {c}): |x|= {np.linalg.norm(X[r]):.6e}, bits equal to the batch of two: {same}")
                    assert same, r
        assert chain.wg_fallbacks(m) == (0, 0)
    finally:
        m.close()


def test_solve_on_the_team_of_five_from_a_nonzero_guess(oracle, monkeypatch):
    """Config C (160 slices, teams of five workgroups) at 4 slices per wave: 3 right-hand sides from the non-zero guess to tol = 1e-13
    against the two-kernel iteration from the same guess and against the oracle's M.  The right-hand sides stop at iterations of their
    own."""
    from elphdynamics_amd import configs, models
    m = configs.make_model("C", tol=1e-5)
    try:
        R, B = configs.rhs(m, NRHS)
        X0 = chain.guess(m.Ndim, NRHS)
        m.solver.tol, out = 1e-13, {}
        for name, env in (("two-kernel", {"ELPH_NO_WG": "1"}), ("resident", {"ELPH_WG_T": "4"})):
            _env(monkeypatch, **env)
            if name == "resident":
                assert chain.wg_shape(m, NRHS) == (1, 4, 8, 5), chain.wg_shape(m, NRHS)
                assert chain.resident_plan(m, NRHS)["resident"] == 1
            X = np.array(X0)
            it, res, fl = models.ldiv_batched_(X, m, B)
            assert not fl.any(), (name, fl)
            out[name] = (X, it)
        assert chain.wg_fallbacks(m) == (0, 0)
        (Xw, itw), (Xs, its) = out["resident"], out["two-kernel"]
        om = _oracle_model(oracle, m)
        res_o = [rel(oracle.mulM(om, Xw[i]), R[i]) for i in range(NRHS)]
        assert len(set(int(i) for i in itw)) > 1, itw      # the right-hand sides leave through `done` at different iterations
        print(f"iterations resident {itw} two-kernel {its}; |X - X_two_kernel| / |X| = {rel(Xw, Xs):.2e}; |M x - R| / |R| (oracle's M) = {max(res_o):.2e}")
        assert rel(Xw, Xs) < 1e-11
        assert max(res_o) < 1e-9
    finally:
        m.close()
