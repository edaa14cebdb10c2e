"""GPU test of the tau-axis transform plan on a handle (csrc/dft_mfma.hip: elph_plan_dft over h->dft.shape): what the preconditioned CG
iteration may fuse into the twisted pair — a question the Green's-function shapes of tests/test_gpu_greens_shapes.py never ask — equals
what the device-free probe says (tests/test_dft_plan.py holds the probe to the recorded rule), and the solves those capabilities select
agree at the bounds tests/test_gpu_parity.py uses for the same pairs."""
import numpy as np
import pytest

from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

SWITCHES = ("ELPH_DFT_MFMA", "ELPH_FUSE_XR", "ELPH_FUSE_PX")
SETTINGS = [{}, {"ELPH_FUSE_XR": "0"}, {"ELPH_FUSE_PX": "0"}]
SETTINGS += [dict(s, ELPH_DFT_MFMA="1") for s in SETTINGS]      # (16 right-hand sides of 64 sites are below the split form's crossover)


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_capabilities_on_the_handle_equal_the_probe_and_the_fused_solves_agree(monkeypatch):
    """Config B's lattice (8 x 8 sites, Ltau = 20) at 1 and 16 right-hand sides, with and without ELPH_FUSE_XR=0 / ELPH_FUSE_PX=0."""
    from elphdynamics_amd import _lib, configs, models, preconditioners as pc
    m = configs.make_model("B", tol=1e-8)
    try:
        N, L = m.Nsites, m.Ltau
        seen = set()
        for env in SETTINGS:
            _set(monkeypatch, env)
            for nrhs in (1, 16):
                for inv in (0, 1):
                    got, want = _lib.dft_plan(L, 0, inv, N, nrhs, handle=m._h), _lib.dft_plan(L, 0, inv, N, nrhs)
                    assert got == want, (env, nrhs, inv)
                    seen.add((got["xr"], got["px"], got["fold"]))
        assert {c[0] for c in seen} == {0, 1} and {c[1] for c in seen} == {0, 1} and {c[2] for c in seen} == {0, 1}
        P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
        pc.setup_(P, rng=np.random.default_rng(3))
        _, B = configs.rhs(m, 16)
        out = {}
        for mode, env in (("fused", {}), ("no_xr", {"ELPH_FUSE_XR": "0"}), ("no_px", {"ELPH_FUSE_PX": "0"})):
            _set(monkeypatch, dict(env, ELPH_DFT_MFMA="1"))
            X = np.zeros_like(B)
            it, res, fl = models.ldiv_batched_(X, m, B, P=P)
            assert not fl.any()
            out[mode] = (X, it)
        for mode, bound in (("no_xr", 1e-10), ("no_px", 1e-13)):
            assert np.array_equal(out["fused"][1], out[mode][1]), mode
            assert rel(out[mode][0], out["fused"][0]) < bound, mode
    finally:
        m.close()
