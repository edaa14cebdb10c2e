"""The order of the 16 x 16 DPP sweeps in the workgroup-resident CG kernel (csrc/cg_wg.hip, the SQ branch; cg_wg_dev.h, sq_cross_issue):
at 4 slices per wave the y-odd colour's crossing of one pair of slabs is issued early and applied after work that does not need it.
Only the interleaving may differ from the colour-major order of 1 and 2 slices per wave — every fma keeps its operands, every sum its
order.  Checked on the shortest time axis on which ELPH_WG_T = 1, 2 and 4 each select the DPP form (Ltau = 32: teams of 4, 2 and 1
workgroups of 8 waves), with 3 right-hand sides on 2 chains, for every pinned shape:
  * iteration counts and solutions of the batch against the two-kernel iteration (the bounds of
    test_gpu_parity.py::test_wg_resident_cg_equals_the_two_kernel_iteration);
  * iteration count and eps history of every right-hand side against the CPU oracle and against the two-kernel iteration (the bounds of
    test_gpu_parity.py::check_cg_vs_oracle);
  * a right-hand side solved alone, on a single-chain model, carries the bits it has in the batch.
(Hopping disorder runs at 1 and 2 slices per wave only and keeps the colour-major order: no case of its own.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LTAU, NCHAINS, NRHS = 32, 2, 3
TEAM = {1: 4, 2: 2, 4: 1}          # workgroups per team at W = 8 waves


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _model(x=None):
    from elphdynamics_amd import lattice as lat, models, synth
    m = models.HolsteinModel(lat.Lattice(1, 16, 16, 1), 3.2, 0.1, tol=1e-5, maxiter=10000)
    m.assign_t_(1.0, 1, 1, (1, 0, 0)); m.assign_t_(1.0, 1, 1, (0, 1, 0))
    m.assign_omega_(1.0); m.assign_lambda_(1.0); m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, 3.2, 0.1, omega=1.0, lam=1.0, seed=21) if x is None else x
    models.update_model_(m)
    assert m.Ltau == LTAU
    return m


def _wg_shape(m, nrhs):
    from elphdynamics_amd import _lib
    us, T, W, G = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().elph_bench_wg_info(m._h, nrhs, C.byref(us), C.byref(T), C.byref(W), C.byref(G)))
    return us.value, T.value, W.value, G.value


def _env(mp, **kw):
    for k in ("ELPH_NO_WG", "ELPH_WG_T", "ELPH_WG_NO_DPP"):
        mp.delenv(k, raising=False)
    for k, v in kw.items():
        mp.setenv(k, v)


@pytest.fixture(scope="module")
def ref(oracle):
    """The models (one with both chains, one per chain), the right-hand sides, and the references — the two-kernel iteration's batch and
    histories, the oracle's histories — computed once."""
    from elphdynamics_amd import models, synth
    m = _model()
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, 3.2, 0.1, omega=1.0, lam=1.0, seed=5000 + c) for c in range(NCHAINS)])
    assert X.shape[1] == m.Ndof
    models.update_model_chains_(m, X)
    singles = [_model(X[c]) for c in range(NCHAINS)]
    B = np.stack([synth.randn(7000 + r, m.Ndim) for r in range(NRHS)])
    r = {"m": m, "singles": singles, "B": B, "hist_o": [], "it_o": [], "hist_s": [], "it_s": []}
    with pytest.MonkeyPatch.context() as mp:
        _env(mp, ELPH_NO_WG="1")
        Xs = np.zeros_like(B)
        its, _, fl = models.ldiv_batched_(Xs, m, B)
        assert not fl.any()
        r["Xs"], r["its"] = Xs, its
        for i in range(NRHS):
            m1 = singles[i % NCHAINS]
            b = np.ascontiguousarray(B[i])
            E = oracle.update_model_holstein(m1.Nsites, m1.Ltau, m1.dtau, m1.x, m1.lam, m1.lam2, m1.mu)
            om = oracle.make_model(0, m1.Nsites, m1.Ltau, m1.neighbor_table, m1.cosht, m1.sinht, E)
            _, ito, histo = oracle.cg_solve(om, b, tol=1e-5, maxiter=10000, history=True)
            x = np.zeros(m.Ndim)
            it, hist = models.solve_(x, m1, b, tol=1e-5, history=True)
            r["it_o"].append(ito); r["hist_o"].append(histo); r["it_s"].append(it); r["hist_s"].append(hist)
    for k in ("Xs", "its", "B"):
        r[k].setflags(write=False)
    yield r
    m.close()
    for s in singles:
        s.close()


def _same_count(it, ito, histo):
    """check_cg_vs_oracle's rule: the same count, or +-1 when eps sits on the tolerance at the last step"""
    return it == ito or (abs(it - ito) == 1 and (ito < 100 or abs(histo[min(it, ito)] / 1e-5 - 1) < 0.05))


@pytest.mark.parametrize("pin", [1, 2, 4])
def test_pinned_shape_against_two_kernel_iteration_and_oracle(ref, monkeypatch, pin):
    from elphdynamics_amd import models
    m, B = ref["m"], ref["B"]
    _env(monkeypatch, ELPH_WG_T=str(pin))
    for mm, n in [(m, NRHS)] + [(s, 1) for s in ref["singles"]]:
        assert _wg_shape(mm, n) == (1, pin, 8, TEAM[pin]), (pin, n, _wg_shape(mm, n))
    Xw = np.zeros_like(B)
    itw, _, fl = models.ldiv_batched_(Xw, m, B)
    assert not fl.any()
    its = ref["its"]
    print(f"T={pin}: iterations resident {itw} two-kernel {its}, |X - X_two_kernel| / |X| = {rel(Xw, ref['Xs']):.2e}")
    assert np.max(np.abs(itw - its)) <= max(1, int(its.max()) // 150), (itw, its)
    assert rel(Xw, ref["Xs"]) < 5e-5
    for i in range(NRHS):
        m1 = ref["singles"][i % NCHAINS]
        b = np.ascontiguousarray(B[i])
        x = np.zeros(m.Ndim)
        it, hist = models.solve_(x, m1, b, tol=1e-5, history=True)
        for name, ito, histo in (("oracle", ref["it_o"][i], ref["hist_o"][i]), ("two-kernel", ref["it_s"][i], ref["hist_s"][i])):
            n = min(41, it // 4 + 1)
            err = np.max(np.abs(hist[:n] - histo[:n]) / histo[:n])
            print(f"T={pin} rhs {i}: iterations {it} ({name} {ito}), eps history [:{n}] max rel diff {err:.2e}")
            assert _same_count(it, ito, histo), (name, it, ito)
            assert err < 1e-10, name
        assert hist[-1] < 1e-5 <= hist[-2]
        # alone, on a model that holds only this right-hand side's chain: the bits of the batch
        x1 = np.zeros(m.Ndim)
        it1, _, fl1 = models.ldiv_(x1, m1, b)
        assert fl1 == 0 and it1 == itw[i] == it, (it1, itw[i], it)
        assert np.array_equal(x1, Xw[i]) and np.array_equal(x, Xw[i])
