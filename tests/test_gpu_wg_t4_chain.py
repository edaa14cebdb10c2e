"""The 4-slice shape of the workgroup-resident CG kernel (csrc/cg_wg.hip: 16 x 16 DPP form, ELPH_WG_T=4) where the benchmark does not look:
the instantiation that reads x0, a team shape whose waves carry two boundary segments, a second round of teams — and, bit for bit, the
x of 25 iterations against a fixture recorded on the GPU before the kernel's LDS waits and register copies were re-ordered
(tests/golden/wg_t4_bits.json, tools/record_wg_t4_bits.py).

Tolerances: those of test_gpu_parity.py::test_wg_resident_cg_equals_the_two_kernel_iteration at tol = 1e-13 (|X - X_two_kernel| / |X| < 1e-11:
both forms run the same recurrences from the same guess, only the summation trees differ), and for the oracle the bound its neighbour
test_wg_resident_cg_dpp_form_with_hopping_disorder takes at the same tolerance, |M x - R| / |R| < 1e-9 with the oracle's M (x solves
Mt M x = Mt R; a comparison of solutions from different guesses would carry the condition number, the residual does not)."""
import json
import os

import numpy as np
import pytest

import wg_t4_chain_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SWITCHES = ("ELPH_NO_WG", "ELPH_WG_T", "ELPH_WG_NO_DPP", "ELPH_WG_W", "ELPH_WG_ALWAYS")


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _env(mp, **kw):
    for k in SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in kw.items():
        mp.setenv(k, v)


def _oracle_model(oracle, m):
    E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
    return oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)


def _model_ltau48():
    """The 16 x 16 lattice of config C on 48 time slices (beta = 4.8), made the way configs.make_model makes a configuration."""
    from elphdynamics_amd import lattice as lat, models, synth
    beta, dtau = 4.8, 0.1
    m = models.HolsteinModel(lat.Lattice(1, 16, 16, 1), beta, dtau, tol=1e-5, maxiter=10000)
    rng = np.random.default_rng(synth.SEED_FIELDS + 991)
    for (o1, o2, d) in lat.SQUARE_BONDS:
        m.assign_t_(1.0, o1, o2, d, stddev=0.0, rng=rng)
    m.assign_omega_(1.0)
    m.assign_lambda_(1.0)
    m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, beta, dtau, omega=1.0, lam=1.0, rough=True, seed=synth.SEED_FIELDS)
    models.update_model_(m)
    assert m.Ltau == 48
    return m


@pytest.fixture(scope="module")
def cfg_c():
    """Config C (solver tolerance 1e-5), 3 right-hand sides and their non-zero guess: made once; a test that needs another tolerance puts
    this one back."""
    from elphdynamics_amd import configs
    m = configs.make_model("C", tol=1e-5)
    R, B = configs.rhs(m, cases.NRHS)
    X0 = cases.guess(m.Ndim, cases.NRHS)
    for a in (R, B, X0):
        a.setflags(write=False)
    yield {"m": m, "R": R, "B": B, "X0": X0}
    m.close()


def _solve_from_guess_against_two_kernel_and_oracle(m, R, B, X0, shape, oracle, mp):
    from elphdynamics_amd import models
    tol0, out = m.solver.tol, {}
    m.solver.tol = 1e-13
    try:
        for name, env in (("two-kernel", {"ELPH_NO_WG": "1"}), ("resident", {"ELPH_WG_T": "4"})):
            _env(mp, **env)
            if name == "resident":
                assert cases.wg_shape(m, B.shape[0]) == shape, cases.wg_shape(m, B.shape[0])
                assert cases.resident_plan(m, B.shape[0])["resident"] == 1
            X = np.array(X0)
            it, res, fl = models.ldiv_batched_(X, m, B)
            assert not fl.any(), (name, fl)
            out[name] = (X, it)
    finally:
        m.solver.tol = tol0
    assert cases.wg_fallbacks(m) == (0, 0)
    (Xw, itw), (Xs, its) = out["resident"], out["two-kernel"]
    om = _oracle_model(oracle, m)
    res_o = [rel(oracle.mulM(om, Xw[i]), R[i]) for i in range(B.shape[0])]
    print(f"iterations resident {itw} two-kernel {its}; |X - X_two_kernel| / |X| = {rel(Xw, Xs):.2e}; |M x - R| / |R| (oracle's M) = {max(res_o):.2e}")
    assert rel(Xw, Xs) < 1e-11
    assert max(res_o) < 1e-9


def test_config_c_from_a_nonzero_guess(cfg_c, oracle, monkeypatch):
    """Config C at 4 slices per wave (teams of 5 workgroups of 8 waves), 3 right-hand sides from a non-zero initial guess: the instantiation that
    reads x0.  To tol = 1e-13 against the two-kernel iteration from the same guess and against the oracle's M."""
    _solve_from_guess_against_two_kernel_and_oracle(cfg_c["m"], cfg_c["R"], cfg_c["B"], cfg_c["X0"], (1, 4, 8, 5), oracle, monkeypatch)


def test_48_slices_teams_of_two_workgroups_of_six_waves(oracle, monkeypatch):
    """48 time slices at 4 slices per wave: W = 6 waves, G = 2 workgroups — a wave fetches two segments of the boundary slices, and the wave that
    trades the records is another one.  5 right-hand sides from a non-zero guess, the comparisons of the case above."""
    from elphdynamics_amd import configs
    m = _model_ltau48()
    R, B = configs.rhs(m, 5)
    _solve_from_guess_against_two_kernel_and_oracle(m, R, B, cases.guess(m.Ndim, 5), (1, 4, 6, 2), oracle, monkeypatch)
    m.close()


def test_second_round_of_teams_carries_the_bits_of_a_small_batch(cfg_c, monkeypatch):
    """50 right-hand sides at 4 slices per wave: 48 teams fill the chip, two more start when the first teams end.  Every right-hand side's
    solution is bit-equal to the one it has in a batch of 3 at the same pin."""
    from elphdynamics_amd import configs, models
    m = cfg_c["m"]
    assert m.solver.tol == 1e-5
    _env(monkeypatch, ELPH_WG_T="4")
    n = 50
    assert cases.wg_shape(m, n) == (1, 4, 8, 5)
    _, B = configs.rhs(m, n)
    X = np.zeros_like(B)
    it, _, fl = models.ldiv_batched_(X, m, B)
    assert not fl.any()
    for i0 in range(0, n, 3):
        Bs = np.ascontiguousarray(B[i0:i0 + 3])
        Xs = np.zeros_like(Bs)
        its, _, fls = models.ldiv_batched_(Xs, m, Bs)
        assert not fls.any()
        assert np.array_equal(its, it[i0:i0 + 3]), (i0, its, it[i0:i0 + 3])
        assert np.array_equal(Xs, X[i0:i0 + 3]), (i0, rel(Xs, X[i0:i0 + 3]))
    assert cases.wg_fallbacks(m) == (0, 0)


@pytest.mark.parametrize("start", ["x0_zero", "x0_guess"])
def test_bits_of_25_iterations_are_those_of_the_recorded_fixture(cfg_c, monkeypatch, start):
    """25 fixed iterations of 3 right-hand sides of config C at ELPH_WG_T=4 against tests/golden/wg_t4_bits.json, recorded on the GPU at the commit
    before the kernel's chain was re-ordered: from x0 = 0 through elph_bench_prepare / elph_bench_run(what = 9) / elph_bench_get_x (the
    benchmark's instantiation), and from the non-zero guess through elph_cg_solve stopped by maxiter = 25 (the measurement hooks take no
    initial guess; wg_t4_chain_cases.py).  The SHA-256 of the bytes decides; the sampled values make a failure readable."""
    m = cfg_c["m"]
    with open(os.path.join(GOLDEN, "wg_t4_bits.json")) as f:
        want = json.load(f)
    assert (want["nrhs"], want["iterations"]) == (cases.NRHS, cases.ITERS)
    _env(monkeypatch, ELPH_WG_T="4")
    assert cases.wg_shape(m, cases.NRHS)[:2] == (1, 4) and cases.wg_shape(m, 1)[:2] == (1, 4)
    X = cases.fixed_iterations_from_zero(m, cfg_c["B"]) if start == "x0_zero" else cases.fixed_iterations_from_guess(m, cfg_c["B"], cfg_c["X0"])
    assert cases.wg_fallbacks(m) == (0, 0)
    got = cases.digest(X)
    diff = [(i, a, b) for (i, a), (_, b) in zip(got["samples"], want[start]["samples"]) if a != b]
    assert not diff, f"sampled values (index, now, recorded): {diff}"
    assert got["sha256"] == want[start]["sha256"]
