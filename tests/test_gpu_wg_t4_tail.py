"""The fused tail of the 4-slice workgroup-resident CG iteration (csrc/cg_wg.hip: 16 x 16 DPP form, ELPH_WG_T=4) at the team shapes config C
does not reach: a team of one workgroup (32 time slices: no poll window, no boundary granules), a team of two (64: both neighbours of a
workgroup are the same workgroup) and a ring of three (96: distinct neighbours).  Bit for bit, the x of 25 iterations against a fixture
recorded on the GPU before the tail's LDS reads were moved into the meeting's wait (tests/golden/wg_t4_tail_bits.json,
tools/record_wg_t4_tail_bits.py) — and, so that the fixture is anchored to something other than this kernel, a solve to tol = 1e-13 against
the two-kernel iteration and the oracle's M.

Tolerances: those of test_gpu_wg_t4_chain.py at the same solver tolerance: |X - X_two_kernel| / |X| < 1e-11 (both forms run the same
recurrences from the same guess, only the summation trees differ) and |M x - R| / |R| < 1e-9 with the oracle's M."""
import json
import os

import numpy as np
import pytest

import wg_t4_tail_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SWITCHES = ("ELPH_NO_WG", "ELPH_WG_T", "ELPH_WG_NO_DPP", "ELPH_WG_W", "ELPH_WG_ALWAYS")
LTAUS = sorted(cases.SHAPES)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _env(mp, **kw):
    for k in SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in kw.items():
        mp.setenv(k, v)


@pytest.fixture(scope="module")
def shapes():
    """One model, 3 right-hand sides and their non-zero guess per time axis: made on first use, shared by the tests, left unchanged."""
    from elphdynamics_amd import configs
    made = {}

    def get(ltau):
        if ltau not in made:
            m = cases.model(ltau)
            R, B = configs.rhs(m, cases.NRHS)
            X0 = cases.guess(m.Ndim, cases.NRHS)
            for a in (R, B, X0):
                a.setflags(write=False)
            made[ltau] = {"m": m, "R": R, "B": B, "X0": X0}
        return made[ltau]
    yield get
    for s in made.values():
        s["m"].close()


@pytest.mark.parametrize("start", ["x0_zero", "x0_guess"])
@pytest.mark.parametrize("ltau", LTAUS)
def test_bits_of_25_iterations_are_those_of_the_recorded_fixture(shapes, monkeypatch, ltau, start):
    """25 fixed iterations of 3 right-hand sides at ELPH_WG_T=4 against tests/golden/wg_t4_tail_bits.json: from x0 = 0 through the measurement
    hooks (the benchmark's instantiation) and from the non-zero guess through elph_cg_solve stopped by maxiter = 25 (the one that reads x0).
    The SHA-256 of the bytes decides; the sampled values make a failure readable."""
    s = shapes(ltau)
    m = s["m"]
    with open(os.path.join(GOLDEN, "wg_t4_tail_bits.json")) as f:
        want = json.load(f)
    assert (want["nrhs"], want["iterations"]) == (cases.NRHS, cases.ITERS)
    want = want["shapes"][str(ltau)]
    _env(monkeypatch, ELPH_WG_T="4")
    assert cases.wg_shape(m, cases.NRHS) == cases.SHAPES[ltau] and cases.wg_shape(m, 1) == cases.SHAPES[ltau], cases.wg_shape(m, cases.NRHS)
    X = cases.fixed_iterations_from_zero(m, s["B"]) if start == "x0_zero" else cases.fixed_iterations_from_guess(m, s["B"], s["X0"])
    assert cases.wg_fallbacks(m) == (0, 0)
    got = cases.digest(X)
    diff = [(i, a, b) for (i, a), (_, b) in zip(got["samples"], want[start]["samples"]) if a != b]
    assert not diff, f"sampled values (index, now, recorded): {diff}"
    assert got["sha256"] == want[start]["sha256"]


@pytest.mark.parametrize("ltau", LTAUS)
def test_solve_from_a_nonzero_guess_against_two_kernel_and_oracle(shapes, oracle, monkeypatch, ltau):
    """3 right-hand sides from the non-zero guess to tol = 1e-13: the resident kernel at the asserted team shape against the two-kernel
    iteration from the same guess and against the oracle's M."""
    from elphdynamics_amd import models
    s = shapes(ltau)
    m, R, B = s["m"], s["R"], s["B"]
    tol0, out = m.solver.tol, {}
    m.solver.tol = 1e-13
    try:
        for name, env in (("two-kernel", {"ELPH_NO_WG": "1"}), ("resident", {"ELPH_WG_T": "4"})):
            _env(monkeypatch, **env)
            if name == "resident":
                assert cases.wg_shape(m, B.shape[0]) == cases.SHAPES[ltau], cases.wg_shape(m, B.shape[0])
                assert cases.resident_plan(m, B.shape[0])["resident"] == 1
            X = np.array(s["X0"])
            it, res, fl = models.ldiv_batched_(X, m, B)
            assert not fl.any(), (name, fl)
            out[name] = (X, it)
    finally:
        m.solver.tol = tol0
    assert cases.wg_fallbacks(m) == (0, 0)
    (Xw, itw), (Xs, its) = out["resident"], out["two-kernel"]
    E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
    om = oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)
    res_o = [rel(oracle.mulM(om, Xw[i]), R[i]) for i in range(B.shape[0])]
    print(f"Ltau {ltau}: iterations resident {itw} two-kernel {its}; |X - X_two_kernel| / |X| = {rel(Xw, Xs):.2e}; |M x - R| / |R| (oracle's M) = {max(res_o):.2e}")
    assert rel(Xw, Xs) < 1e-11
    assert max(res_o) < 1e-9
