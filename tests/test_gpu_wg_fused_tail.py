"""The tail of the workgroup-resident CG iteration (csrc/cg_wg.hip, FUSED): with two and more slices per wave the stop decision and
beta are made from the meeting's four sums BEFORE the vector update, and one pass over the own slices makes r', x and p; the
square-lattice DPP forms add their four sums per batch of reverse sweeps.  What that order could break, under the team shapes of large
batches (ELPH_WG_T pins them for a single right-hand side) and next to the one-slice shapes that keep the old order:
  * a solve that stops right after the pass must hand back the x of exactly that iteration;
  * the eps history (made before the pass now) under the 2- and 4-slice shapes;
  * the cancellation branch — r'.r' < r.r / 1000, the direct sum in a second meeting — which no other test takes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _oracle_model(orc, m):
    """The oracle's model of the GPU model's tables and fields, as bench.py's cpu_baseline leg builds it."""
    if m.kind == 0:
        E = orc.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
        return orc.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)
    return orc.make_model(1, m.Nsites, m.Ltau, m.neighbor_table, np.ascontiguousarray(m.cosht).reshape(-1),
                          np.ascontiguousarray(m.sinht).reshape(-1), m.expDtauMu)


def _wg_shape(m, nrhs=1):
    """(usable, slices per wave, waves per workgroup, workgroups per team) of the resident solve of nrhs right-hand sides"""
    from elphdynamics_amd import _lib
    us, T, W, G = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().elph_bench_wg_info(m._h, nrhs, C.byref(us), C.byref(T), C.byref(W), C.byref(G)))
    return us.value, T.value, W.value, G.value


def _pin(monkeypatch, m, pin):
    if pin is None:
        monkeypatch.delenv("ELPH_WG_T", raising=False)
        assert _wg_shape(m)[0] == 1
    else:
        monkeypatch.setenv("ELPH_WG_T", pin)
        assert _wg_shape(m)[:2] == (1, int(pin)), _wg_shape(m)


NRHS = 2


@pytest.mark.parametrize("tag,pin", [("C", "1"), ("C", "2"), ("C", "4"), ("S", "4"), ("B", None), ("D", None), ("E", None), ("s", None)])
def test_stop_right_after_the_fused_pass(oracle, monkeypatch, tag, pin):
    """maxiter = k = 1, 2, 3 with a tolerance no residual meets: exactly k iterations, and x is the oracle's x after k iterations to
    1e-12 — stored after the k-th x += alpha p, with nothing of the p-update of the same pass in it."""
    from elphdynamics_amd import configs, models
    m = configs.make_model(tag, tol=1e-5)
    _pin(monkeypatch, m, pin)
    om = _oracle_model(oracle, m)
    _, B = configs.rhs(m, NRHS)
    for i in range(NRHS):
        b = np.ascontiguousarray(B[i])
        for k in (1, 2, 3):
            x = np.zeros(m.Ndim)
            it = models.solve_(x, m, b, tol=1e-30, maxiter=k)
            xo, ito = oracle.cg_solve(om, b, tol=1e-30, maxiter=k)
            err = rel(x, xo)
            print(f"{tag} pin {pin} rhs {i} maxiter {k}: iterations {it} (oracle {ito}), |x - x_oracle| / |x_oracle| = {err:.2e}")
            assert it == k and ito == k
            assert err < 1e-12
    m.close()


@pytest.mark.parametrize("tag,pin", [("C", "2"), ("C", "4"), ("S", "4")])
def test_history_under_the_batch_shapes(oracle, monkeypatch, tag, pin):
    """The first 40 entries of the eps history against the oracle's to 1e-10, under the shapes a large batch runs."""
    from elphdynamics_amd import configs, models
    m = configs.make_model(tag, tol=1e-5)
    _pin(monkeypatch, m, pin)
    om = _oracle_model(oracle, m)
    _, B = configs.rhs(m, NRHS)
    for i in range(NRHS):
        b = np.ascontiguousarray(B[i])
        x = np.zeros(m.Ndim)
        it, hist = models.solve_(x, m, b, tol=1e-5, history=True)
        xo, ito, histo = oracle.cg_solve(om, b, tol=1e-5, maxiter=10000, history=True)
        assert it >= 40 and ito >= 40, (it, ito)
        err = np.max(np.abs(hist[:40] - histo[:40]) / histo[:40])
        print(f"{tag} pin {pin} rhs {i}: iterations {it} (oracle {ito}), eps history [:40] max rel diff {err:.2e}")
        assert err < 1e-10
    m.close()


MU_CANCEL = -80.0


@pytest.mark.parametrize("tag,pin", [("C", "1"), ("C", "2"), ("C", "4"), ("B", None)])
def test_cancellation_branch(oracle, monkeypatch, tag, pin):
    """mu = -80: exp(-dtau (V - mu)) ~ 3e-4, M^T M is close to the identity and every CG step shrinks r.r by ~2e-7 — the identity
    r'.r' = r.r - 2 alpha r.z + alpha^2 z.z cancels and the kernel takes the direct sum in a second meeting (teams of 20, 10, 5 and 1).
    The value is the least negative of -20, -40, -80 for which the ORACLE's history, on the CPU, has a step with r'.r' / r.r < 1e-4 —
    a factor 10 inside the kernel's 1e-3, so rounding cannot move it across: -20 gives 3.5e-2 at best, -40 gives 6.0e-4 (C and B alike),
    -80 gives 2.0e-7 (every one of its 4 steps at tol = 1e-10 is below 3.2e-7)."""
    from elphdynamics_amd import configs, models
    m = configs.make_model(tag, tol=1e-10)
    m.assign_mu_(MU_CANCEL)
    models.update_model_(m)
    _pin(monkeypatch, m, pin)
    om = _oracle_model(oracle, m)
    _, B = configs.rhs(m, NRHS)
    for i in range(NRHS):
        b = np.ascontiguousarray(B[i])
        xo, ito, histo = oracle.cg_solve(om, b, tol=1e-10, maxiter=10000, history=True)
        ratio = (histo[1:] / histo[:-1]) ** 2
        assert ratio.min() < 1e-4, ratio                      # the oracle's own history has a step that cancels
        x = np.zeros(m.Ndim)
        it, hist = models.solve_(x, m, b, tol=1e-10, history=True)
        errh = np.max(np.abs(hist - histo) / histo) if it == ito else np.inf
        errx = rel(x, xo)
        print(f"{tag} pin {pin} rhs {i}: iterations {it} (oracle {ito}), min r'.r'/r.r {ratio.min():.2e}, history max rel diff {errh:.2e}, "
              f"|x - x_oracle| / |x_oracle| = {errx:.2e}")
        assert it == ito
        assert errh < 1e-10
        assert errx < 1e-10
    m.close()
