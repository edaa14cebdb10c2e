"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI of
libelphgpu.so, against (i) the committed golden fixtures and (ii) the CPU oracle on the same seeded inputs.

Tolerances (north_star: 1e-10 relative on residuals / Green's-function elements):
  * mat-vecs, preconditioner apply, FFTs: 1e-12 relative (observed ~1e-16) — only FMA contraction and
    summation order differ from the oracle;
  * CG: identical iteration count at the production tolerance (1e-5); eps history within 1e-10 relative
    for the first 40 iterations (round-off then grows exponentially with the iteration index in ANY two
    implementations that sum in different orders — SURVEY.md §7 "hard parts"); the solution M^-1 R (the Green's-function
    observable, GreensFunctions.jl:223-225) within 1e-10 of the oracle / the dense solve when both sides solve to 1e-13
    (measured on MI355X, tools/parity_tight.py: 4e-14 ... 1e-13 at configs b, B, C, D, E).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def lib():
    from elphdynamics_amd import _lib
    L = _lib.load()
    assert L.elph_device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return L


class RawModel:
    """Minimal driver of the raw C ABI (no Python mirror): what a Julia ccall wrapper would do."""

    def __init__(self, lib, kind, N, L, table, c=None, s=None):
        from elphdynamics_amd import _lib
        self.lib, self.N, self.L, self.n = lib, N, L, N * L
        self.h = _lib.Handle()
        tab = np.ascontiguousarray(table, dtype=np.int64)
        nb = tab.shape[0]
        _lib.check(lib.elph_create(C.byref(self.h), kind, N, L, nb, _lib.iptr(tab) if nb else None,
                                   _lib.dptr(np.ascontiguousarray(c)) if c is not None and nb else None,
                                   _lib.dptr(np.ascontiguousarray(s)) if s is not None and nb else None, 0))

    def close(self):
        self.lib.elph_destroy(self.h)

    def op(self, name, v):
        from elphdynamics_amd import _lib
        y = np.zeros(self.n)
        _lib.check(getattr(self.lib, name)(self.h, _lib.dptr(y), _lib.dptr(np.ascontiguousarray(v))))
        return y

    def ldiv(self, b, tol, maxiter, use_prec=0, call_maxiter=0, x0=None):
        from elphdynamics_amd import _lib
        _lib.check(self.lib.elph_solver_set(self.h, tol, maxiter, 1e12))
        x = np.zeros(self.n) if x0 is None else x0.copy()
        it, fl, res = C.c_int64(), C.c_int(), C.c_double()
        _lib.check(self.lib.elph_ldiv(self.h, _lib.dptr(x), _lib.dptr(np.ascontiguousarray(b)), use_prec, call_maxiter,
                                      C.byref(it), C.byref(res), C.byref(fl)))
        return x, it.value, res.value, fl.value


# ------------------------------------------------------------------------------------------ golden fixtures

@pytest.mark.parametrize("name", ["holstein_sq4_L8.npz", "holstein_hc3_L6.npz", "holstein_tri3_L5.npz",
                                  "holstein_sq4_L40.npz"])
def test_holstein_golden(lib, name):
    from elphdynamics_amd import _lib
    g = golden(name)
    N, L = int(g["N"]), int(g["Ltau"])
    m = RawModel(lib, 0, N, L, g["table"], g["cosht"], g["sinht"])
    try:
        # update_model! on the device vs the golden exp(-dtau V)
        _lib.check(lib.elph_update_model_holstein(m.h, _lib.dptr(np.ascontiguousarray(g["x"])), _lib.dptr(g["lam"]),
                                                  _lib.dptr(g["lam2"]), _lib.dptr(g["mu"]), float(g["dtau"])))
        assert rel(m.op("elph_mulM", g["v"]), g["Mv"]) < 1e-13
        assert rel(m.op("elph_mulMT", g["v"]), g["MTv"]) < 1e-13
        assert rel(m.op("elph_mulMTM", g["v"]), g["MTMv"]) < 1e-13
        # same through elph_set_expV (caller-supplied expnDtauV)
        _lib.check(lib.elph_set_expV(m.h, _lib.dptr(np.ascontiguousarray(g["E"]))))
        assert rel(m.op("elph_mulM", g["v"]), g["Mv"]) < 1e-13
        x, it, res, flag = m.ldiv(g["b"], 1e-13, 5000)
        assert flag == 0 and res < 1e-6
        assert rel(x, g["xsol"]) < 1e-10 and rel(x, g["Minv_R"]) < 1e-10
        # flag logic (Models.jl:157-180)
        x, it, res, flag = m.ldiv(g["b"], 1e-14, 3)
        assert it == 3 and flag == 1 and not x.any()
        x, it, res, flag = m.ldiv(g["b"], 1e-14, 5000, call_maxiter=3)
        assert it == 3 and flag == 2 and not x.any()
    finally:
        m.close()


def test_single_site_golden(lib):
    """config A (examples/holstein_hmc_single_site.toml): 1 site, no bonds, closed form."""
    from elphdynamics_amd import _lib
    g = golden("holstein_single_site.npz")
    L = int(g["Ltau"])
    m = RawModel(lib, 0, 1, L, np.zeros((0, 2), dtype=np.int64))
    try:
        _lib.check(lib.elph_update_model_holstein(m.h, _lib.dptr(np.ascontiguousarray(g["x"])), _lib.dptr(np.ones(1)),
                                                  _lib.dptr(np.zeros(1)), _lib.dptr(np.zeros(1)), float(g["dtau"])))
        assert rel(m.op("elph_mulM", g["b"]), g["Mb"]) < 1e-14
        assert rel(m.op("elph_mulMT", g["b"]), g["MTb"]) < 1e-14
        # M^-1 b via MtM x = Mt b
        x, it, res, flag = m.ldiv(g["MTb"], 1e-13, 200)
        assert flag == 0 and rel(x, g["Minv_b"]) < 1e-10
    finally:
        m.close()


def test_ssh_golden(lib):
    from elphdynamics_amd import _lib
    g = golden("ssh_sq4_L8.npz")
    N, L = int(g["N"]), int(g["Ltau"])
    m = RawModel(lib, 1, N, L, g["table"])
    try:
        _lib.check(lib.elph_update_model_ssh(m.h, _lib.dptr(np.ascontiguousarray(g["cosht"])),
                                             _lib.dptr(np.ascontiguousarray(g["sinht"])), _lib.dptr(g["expDtauMu"])))
        assert rel(m.op("elph_mulM", g["v"]), g["Mv"]) < 1e-13
        assert rel(m.op("elph_mulMT", g["v"]), g["MTv"]) < 1e-13
        assert rel(m.op("elph_mulMTM", g["v"]), g["MTMv"]) < 1e-13
        x, it, res, flag = m.ldiv(g["b"], 1e-13, 5000)
        assert flag == 0 and rel(x, g["xsol"]) < 1e-10
    finally:
        m.close()


@pytest.mark.parametrize("L", [8, 20, 40, 120, 160, 7])
def test_fft_golden(lib, L):
    from elphdynamics_amd import _lib
    g = golden("fft.npz")
    N = 3
    m = RawModel(lib, 0, N, L, np.zeros((0, 2), dtype=np.int64))
    try:
        v = np.ascontiguousarray(g[f"L{L}_v"])
        nu = np.zeros(2 * N * L)
        _lib.check(lib.elph_tau_to_omega(m.h, _lib.dptr(nu), _lib.dptr(v)))
        assert rel(nu[0::2], g[f"L{L}_nu_re"]) < 1e-13 and rel(nu[1::2], g[f"L{L}_nu_im"]) < 1e-13
        back = np.zeros(N * L)
        _lib.check(lib.elph_omega_to_tau(m.h, _lib.dptr(back), _lib.dptr(nu)))
        assert rel(back, v) < 1e-13
        diag = np.tile(g[f"L{L}_Mi"], N)
        for power in (-1.0, -0.5, 1.0):
            out = np.zeros(N * L)
            _lib.check(lib.elph_fourier_accelerate(m.h, _lib.dptr(out), _lib.dptr(v), _lib.dptr(diag), power, N))
            assert rel(out, g[f"L{L}_fa_M_p{power}"]) < 1e-13
        # a non-symmetric diagonal: the reference keeps only the real part, i.e. the symmetrised diagonal
        rng = np.random.default_rng(L)
        d2 = rng.uniform(0.5, 2.0, N * L)
        out = np.zeros(N * L)
        _lib.check(lib.elph_fourier_accelerate(m.h, _lib.dptr(out), _lib.dptr(v), _lib.dptr(d2), 1.0, N))
        ref = np.real(np.fft.ifft(d2.reshape(N, L) * np.fft.fft(v.reshape(N, L), axis=1), axis=1)).reshape(-1)
        assert rel(out, ref) < 1e-13
    finally:
        m.close()


@pytest.mark.parametrize("blocked", ["0", "1"])
@pytest.mark.parametrize("L", [1280, 2048, 1155, 4096, 1031, 480, 800, 1000, 404, 422, 409, 1024])
def test_long_time_axis_transforms(lib, L, blocked, monkeypatch):
    """Time axes beyond 1024 slices (dft_big.hip: one Cooley-Tukey split, both factors <= 1024; a prime length — 1031 — runs a
    direct transform; the reference's FFTW plans take any length, TimeFreqFFTs.jl:32-45) against numpy's FFT: the twisted pair,
    the round trip and fourier_accelerate!.  Round 6: the split also serves 401 … 1024 slices where the length has a divisor >= 4 below
    its square root (480, 800, 1000, 404 = 4 x 101, 1024); 422 = 2 x 211 and the prime 409 keep the scalar-twiddle kernels.  blocked: the
    one-output-row-per-wave kernels of round 4 ("0") and the register-blocked, fused pair k_big_s1 / k_big_s2 ("1": what batches run)."""
    from elphdynamics_amd import _lib
    monkeypatch.setenv("ELPH_DFT_BIG_BLOCKED", blocked)
    N = 3 if L != 800 else 70        # (800: two site tiles, the second ragged)
    rng = np.random.default_rng(L)
    m = RawModel(lib, 0, N, L, np.zeros((0, 2), dtype=np.int64))
    try:
        v = rng.standard_normal(N * L)
        theta = np.exp(-1j * np.pi * np.arange(L) / L)
        ref = np.fft.fft(theta[None, :] * v.reshape(N, L), axis=1).reshape(-1)
        nu = np.zeros(2 * N * L)
        _lib.check(lib.elph_tau_to_omega(m.h, _lib.dptr(nu), _lib.dptr(v)))
        assert rel(nu[0::2], ref.real) < 1e-12 and rel(nu[1::2], ref.imag) < 1e-12
        back = np.zeros(N * L)
        _lib.check(lib.elph_omega_to_tau(m.h, _lib.dptr(back), _lib.dptr(nu)))
        assert rel(back, v) < 1e-12
        d2 = rng.uniform(0.5, 2.0, N * L)
        for power in (-1.0, 0.5):
            out = np.zeros(N * L)
            _lib.check(lib.elph_fourier_accelerate(m.h, _lib.dptr(out), _lib.dptr(v), _lib.dptr(d2), power, N))
            refa = np.real(np.fft.ifft(d2.reshape(N, L) ** power * np.fft.fft(v.reshape(N, L), axis=1), axis=1)).reshape(-1)
            assert rel(out, refa) < 1e-12
    finally:
        m.close()


@pytest.mark.parametrize("blocked", ["0", "1"])
@pytest.mark.parametrize("tag,ltau", [("l", 1280), ("l800", 800)])
def test_long_time_axis_kpm_and_cg_vs_oracle(oracle, tag, ltau, blocked, monkeypatch):
    """Configs l, l800: the 4 x 4 Holstein lattice with 1280 / 800 time slices — mat-vec, KPM apply (two-step transforms around the Chebyshev
    kernel) and the preconditioned solve against the oracle."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    monkeypatch.setenv("ELPH_DFT_BIG_BLOCKED", blocked)
    m = configs.make_model(tag, tol=1e-5)
    assert m.Ltau == ltau
    om = _oracle_model(oracle, m)
    v = synth.randn(77, m.Ndim)
    y = np.empty(m.Ndim)
    models.mulMtM_(y, m, v)
    assert rel(y, oracle.mulMTM(om, v)) < 1e-13
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    oP = oracle.make_kpm(om, n=20, buf=0.05, c1=1.0, c2=1.0)
    rng = np.random.default_rng(17)
    e_min, e_max = oracle.kpm_setup(oP, b_max=rng.standard_normal(m.Nsites), b_min=rng.standard_normal(m.Nsites))
    pc.setup_(P, e_min=e_min, e_max=e_max)
    assert P.active and oP.active == 1
    R, B = configs.rhs(m, 1)
    z = np.empty(m.Ndim)
    pc.kpm_ldiv_(z, P, np.ascontiguousarray(R[0]))
    assert rel(z, oracle.kpm_apply(oP, np.ascontiguousarray(R[0]))) < 1e-10
    b = np.ascontiguousarray(B[0])
    x = np.zeros(m.Ndim)
    it, hist = models.solve_(x, m, b, P=P, tol=1e-5, history=True)
    xo, ito, histo = oracle.cg_solve(om, b, tol=1e-5, maxiter=10000, P=oP, history=True)
    assert abs(it - ito) <= 1 and rel(x, xo) < 1e-6
    m.close()


@pytest.mark.parametrize("tag", ["sq4_L8", "sq4_L40"])
def test_kpm_golden(lib, tag):
    from elphdynamics_amd import _lib
    g = golden(f"holstein_{tag}.npz")
    k = golden(f"kpm_{tag}.npz")
    N, L = int(g["N"]), int(g["Ltau"])
    m = RawModel(lib, 0, N, L, g["table"], g["cosht"], g["sinht"])
    try:
        _lib.check(lib.elph_set_expV(m.h, _lib.dptr(np.ascontiguousarray(g["E"]))))
        _lib.check(lib.elph_kpm_create(m.h, 20, float(k["buf"]), float(k["c1"]), float(k["c2"])))
        act, lo, hi = C.c_int(), C.c_double(), C.c_double()
        # own Arnoldi (n = min(20,N) = N steps => exact spectrum of the 16x16 A)
        rng = np.random.default_rng(3)
        _lib.check(lib.elph_kpm_setup(m.h, _lib.dptr(rng.standard_normal(N)), _lib.dptr(rng.standard_normal(N)),
                                      float("nan"), float("nan"), C.byref(act), C.byref(lo), C.byref(hi)))
        assert act.value == 1
        assert abs(lo.value - float(k["lam_lo"])) < 1e-7 and abs(hi.value - float(k["lam_hi"])) < 1e-7
        # injected bounds -> bit-identical lam_lo/hi; orders; apply
        _lib.check(lib.elph_kpm_create(m.h, 20, float(k["buf"]), float(k["c1"]), float(k["c2"])))
        _lib.check(lib.elph_kpm_setup(m.h, None, None, float(k["e_min"]), float(k["e_max"]), C.byref(act), C.byref(lo),
                                      C.byref(hi)))
        assert lo.value == float(k["lam_lo"]) and hi.value == float(k["lam_hi"])
        orders = np.zeros((L + 1) // 2, dtype=np.int64)
        tot = C.c_int64()
        _lib.check(lib.elph_kpm_orders(m.h, _lib.iptr(orders), C.byref(tot)))
        assert np.array_equal(orders, k["orders"]) and tot.value == k["orders"].sum()
        assert rel(m.op("elph_kpm_apply", k["vin"]), k["vout"]) < 1e-12
        # preconditioned ldiv! reaches the dense solution
        x, it, res, flag = m.ldiv(g["b"], 1e-13, 5000, use_prec=1)
        assert flag == 0 and rel(x, g["xsol"]) < 1e-10
        x0, it0, *_ = m.ldiv(g["b"], 1e-13, 5000, use_prec=0)
        if L >= 40:
            assert it < it0
        # implausible bounds deactivate -> identity (KPMPreconditioners.jl:312-318,475-478)
        _lib.check(lib.elph_kpm_setup(m.h, None, None, 1.5, 1.2, C.byref(act), C.byref(lo), C.byref(hi)))
        assert act.value == 0
        assert np.array_equal(m.op("elph_kpm_apply", k["vin"]), k["vin"])
        x, it2, res, flag = m.ldiv(g["b"], 1e-13, 5000, use_prec=1)
        assert flag == 0 and rel(x, g["xsol"]) < 1e-10 and it2 == it0
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ oracle, same seeded inputs

def _oracle_model(orc, m):
    if m.kind == 0:
        E = orc.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
        return orc.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)
    return orc.make_model(1, m.Nsites, m.Ltau, m.neighbor_table, np.ascontiguousarray(m.cosht).reshape(-1),
                          np.ascontiguousarray(m.sinht).reshape(-1), m.expDtauMu)


@pytest.mark.parametrize("tag", ["A", "b", "d", "t", "u", "e", "B", "C", "D", "E", "T", "g", "G", "h", "s", "q", "Q", "S", "y", "z", "Y", "r", "R", "w", "W", "k", "j", "i", "l30", "h20", "h21", "h24", "t6", "t12", "t20", "t24", "t32", "l22", "l26", "l36", "l34", "l40", "l48", "l64", "h30", "h22", "e8", "e12", "e20", "e24"])      # h30, h22: honeycomb cells on two wavefronts; l36: 4 x 6 patches (round 6); l34 … l64: several wavefronts per slice; l22, l26: square 22 x 22 / 26 x 26 — no register form (2 x 11, 2 x 13), the LDS kernels
def test_matvec_vs_oracle(oracle, tag):
    from elphdynamics_amd import configs
    m = configs.make_model(tag)
    check_matvec_vs_oracle(oracle, m)
    m.close()


def check_matvec_vs_oracle(oracle, m):
    """The mat-vec family of the model's handle against the oracle's on the same tables and field (the model stays open)."""
    from elphdynamics_amd import models, synth
    om = _oracle_model(oracle, m)
    v = synth.randn(77, m.Ndim)
    u = synth.randn(78, m.Ndim)
    y = np.empty(m.Ndim)
    for fn, ofn in ((models.mulM_, oracle.mulM), (models.mulMt_, oracle.mulMT), (models.mulMtM_, oracle.mulMTM)):
        fn(y, m, v)
        assert rel(y, ofn(om, v)) < 1e-13
    # size-independent properties on the GPU results themselves
    Mv, Mtu, a = np.empty(m.Ndim), np.empty(m.Ndim), np.empty(m.Ndim)
    models.mulM_(Mv, m, v)
    models.mulMt_(Mtu, m, u)
    assert abs(u @ Mv - Mtu @ v) < 1e-11 * np.linalg.norm(u) * np.linalg.norm(v)          # adjointness
    models.mulMt_(a, m, Mv)
    models.mulMtM_(y, m, v)
    assert rel(y, a) < 1e-14                                                                # fused MtM == Mt(M v)
    models.mulM_(a, m, Mtu)
    models.mulMMt_(y, m, u)
    assert rel(y, a) < 1e-14 and rel(y, oracle.mulM(om, oracle.mulMT(om, u))) < 1e-13       # mulMMᵀ! (Models.jl:229-238)
    models.transpose_(m)
    models.mul_(y, m, u)                                                                    # mul! honours model.transposed (:192-209)
    assert rel(y, a) < 1e-14
    models.transpose_(m)
    models.mulM_(a, m, 2.0 * v - 3.0 * u)
    Mu = np.empty(m.Ndim)
    models.mulM_(Mu, m, u)
    assert rel(a, 2.0 * Mv - 3.0 * Mu) < 1e-13                                              # linearity


@pytest.mark.parametrize("tag", ["b", "d", "t", "u", "e", "B", "C", "D", "E", "T", "g", "h", "s", "q", "Q", "S", "y", "z", "Y", "r", "R", "w", "W", "G", "k", "j", "i", "l30", "h20", "h21", "h24", "H18", "t6", "t12", "t24", "t32", "l22", "l26", "l36", "l34", "l40", "l48", "l64", "h30", "h22", "e8", "e12", "e20", "e24"])      # h30, h22: honeycomb cells on two wavefronts; l36: 4 x 6 patches (round 6); l34 … l64: several wavefronts per slice; l22, l26: square 22 x 22 / 26 x 26 — no register form (2 x 11, 2 x 13), the LDS kernels
def test_cg_vs_oracle(oracle, tag):
    from elphdynamics_amd import configs
    m = configs.make_model(tag, tol=1e-5)
    check_cg_vs_oracle(oracle, m)
    m.close()


def check_cg_vs_oracle(oracle, m):
    """Plain CG on a model made with tol = 1e-5 against the oracle's: production tolerance, then the tight solve (the model stays open,
    its solver tolerance at 1e-13)."""
    from elphdynamics_amd import configs, models
    om = _oracle_model(oracle, m)
    R, B = configs.rhs(m, 1)
    b = np.ascontiguousarray(B[0])
    # production tolerance: same iteration count, same flags, early history to 1e-10
    x = np.zeros(m.Ndim)
    it, hist = models.solve_(x, m, b, tol=1e-5, history=True)
    xo, ito, histo = oracle.cg_solve(om, b, tol=1e-5, maxiter=10000, history=True)
    # same count, except when eps sits on the tolerance at the last step (round-off knife edge): then +-1
    assert it == ito or (abs(it - ito) == 1 and (ito < 100 or abs(histo[min(it, ito)] / 1e-5 - 1) < 0.05))
    n = min(41, it // 4 + 1)          # round-off grows with the iteration index; tiny systems converge in < 100
    assert np.max(np.abs(hist[:n] - histo[:n]) / histo[:n]) < 1e-10
    assert hist[-1] < 1e-5 <= hist[-2]
    x2 = np.zeros(m.Ndim)
    it2, res2, flag2 = models.ldiv_(x2, m, b)
    xo2, ito2, reso2, flago2 = oracle.ldiv(om, b, solver_tol=1e-5, solver_maxiter=10000)
    assert it2 == it and abs(it2 - ito2) <= 1 and flag2 == flago2 == 0
    # the true residual at exit carries the accumulated round-off of ~it iterations: same magnitude, not same digits
    assert 0.5 * reso2 < res2 < 2.0 * reso2 and res2 <= np.sqrt(1e-5)
    assert np.array_equal(x, x2)                                                            # deterministic re-run
    # tight solve: Green's-function observable M^-1 R (GreensFunctions.jl:223-225, :334-346)
    m.solver.tol = 1e-13
    x3 = np.zeros(m.Ndim)
    it3, res3, flag3 = models.ldiv_(x3, m, b)
    xo3, ito3, *_ = oracle.ldiv(om, b, solver_tol=1e-13, solver_maxiter=10000)
    assert flag3 == 0 and abs(it3 - ito3) <= max(3, ito3 // 100)
    assert rel(x3, xo3) < 1e-10                                                             # the north_star's bound
    Mx = np.empty(m.Ndim)
    models.mulM_(Mx, m, x3)
    assert rel(Mx, R[0]) < 1e-8                                                             # x = M^-1 R indeed


@pytest.mark.parametrize("tag", ["b", "C", "T"])
def test_batched_equals_single(tag):
    """Batched right-hand sides follow the single-RHS recurrences exactly => bit-identical results."""
    from elphdynamics_amd import configs, models
    m = configs.make_model(tag, tol=1e-5)
    nrhs = 3
    R, B = configs.rhs(m, nrhs)
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B)
    for i in range(nrhs):
        x = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x, m, np.ascontiguousarray(B[i]))
        assert it1 == it[i] and fl1 == fl[i] == 0 and res1 == res[i]
        assert np.array_equal(x, X[i])
    m.close()


def test_nonzero_initial_guess_and_kappa_bailout(oracle):
    from elphdynamics_amd import configs, models
    m = configs.make_model("b", tol=1e-8)
    om = _oracle_model(oracle, m)
    R, B = configs.rhs(m, 1)
    b = np.ascontiguousarray(B[0])
    x0 = 0.1 * R[0]
    x = x0.copy()
    it = models.solve_(x, m, b, tol=1e-8)
    xo, ito = oracle.cg_solve(om, b, x0=x0, tol=1e-8, maxiter=10000)
    assert it == ito and rel(x, xo) < 1e-7
    # kappa_max bail-out (IterativeSolvers.jl:289-295): tiny kmax stops at the first iteration it is exceeded
    x = np.zeros(m.Ndim)
    it = models.solve_(x, m, b, tol=1e-12, kmax=50.0)
    xo, ito = oracle.cg_solve(om, b, tol=1e-12, maxiter=10000, kmax=50.0)
    assert it == ito and it < 60
    m.close()


@pytest.mark.parametrize("tag", ["b", "u", "B", "C", "D", "T", "g", "e", "E", "s", "q", "Q", "S", "d", "y", "z", "Y", "r", "W", "G", "k", "j", "i", "l30", "K", "h", "h20", "h21", "h24", "H18", "t6", "t12", "t20", "t24", "t32", "l22", "l26", "l36", "l34", "l40", "l48", "l64", "h30", "h22", "e8", "e12", "e20", "e24"])      # h30, h22: honeycomb cells on two wavefronts; l36: 4 x 6 patches (round 6); l34 … l64: several wavefronts per slice; l22, l26: square 22 x 22 / 26 x 26 — no register form (2 x 11, 2 x 13), the LDS kernels
def test_kpm_vs_oracle(oracle, tag):
    """setup!(P) with injected eigenvalue bounds, ldiv!(z,P,r) and the preconditioned CG vs the oracle.  e / E: bond phonons — the
    expansion is built on the tau-means of the per-(tau, bond) hopping tables (update_A!, KPMPreconditioners.jl:355-381)."""
    from elphdynamics_amd import configs, models, preconditioners as pc
    m = configs.make_model(tag, tol=1e-5)
    om = _oracle_model(oracle, m)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    oP = oracle.make_kpm(om, n=20, buf=0.05, c1=1.0, c2=1.0)
    rng = np.random.default_rng(11)
    bmax, bmin = rng.standard_normal(m.Nsites), rng.standard_normal(m.Nsites)
    e_min, e_max = oracle.kpm_setup(oP, b_max=bmax, b_min=bmin)
    pc.setup_(P, b_max=bmax, b_min=bmin)                       # own Arnoldi, same start vectors (one chain: the HOST path, kpm_host.cpp; the device kernel: test_gpu_kpm_bounds.py)
    assert P.active and oP.active == 1
    # The largest Ritz value of a 20-step Krylov space of a 256 x 256 non-normal matrix moves by 2-3e-6 with the summation order of
    # the Gram-Schmidt dot products alone (sequential vs tree vs BLAS: checked in numpy on this very matrix); the device kernel sums each
    # dot product as a DPP tree, the host path and the oracle sequentially.  The expansion takes the bounds with a 5 % margin (KPMPreconditioners.jl:282-285).
    assert abs(P.lam_lo - oP.lam_lo) < 2e-5 and abs(P.lam_hi - oP.lam_hi) < 2e-5
    # parity of everything downstream: inject the oracle's bounds (parity runs take explicit inputs)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, e_min=e_min, e_max=e_max)
    assert P.lam_lo == oP.lam_lo and P.lam_hi == oP.lam_hi
    Lo2 = (m.Ltau + 1) // 2
    assert np.array_equal(P.orders, oP._keep["order"][:Lo2])
    R, B = configs.rhs(m, 1)
    r = np.ascontiguousarray(R[0])
    z = np.empty(m.Ndim)
    pc.kpm_ldiv_(z, P, r)
    assert rel(z, oracle.kpm_apply(oP, r)) < 1e-11
    b = np.ascontiguousarray(B[0])
    x = np.zeros(m.Ndim)
    it, hist = models.solve_(x, m, b, P=P, tol=1e-5, history=True)
    xo, ito, histo = oracle.cg_solve(om, b, tol=1e-5, maxiter=10000, P=oP, history=True)
    assert it == ito
    n = min(21, it // 4 + 1)
    assert np.max(np.abs(hist[:n] - histo[:n]) / histo[:n]) < 1e-10
    x1 = np.zeros(m.Ndim)
    it1, res1, fl1 = models.ldiv_(x1, m, b, P=P)
    x0 = np.zeros(m.Ndim)
    it0, res0, fl0 = models.ldiv_(x0, m, b)
    assert fl1 == 0 and fl0 == 0 and it1 == it
    assert it1 < it0                                             # the preconditioner reduces the iteration count
    assert rel(x1, x0) < 5e-3                                    # both within tol (times the condition number) of the same solution
    m.close()


def _pg_info(m):
    from elphdynamics_amd import _lib
    v = [C.c_int() for _ in range(5)]
    _lib.check(_lib.load().elph_bench_pg_info(m._h, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)      # (kind, px, py, wavefronts per slice, disorder tables)


@pytest.mark.parametrize("tag", ["B", "C", "g", "h", "G", "i", "k", "j", "l22", "l26", "l30", "l34", "l36"])
def test_kpm_with_hopping_disorder_vs_oracle(oracle, tag):
    """Hopping disorder (assign_t! with a standard deviation, HolsteinModels.jl:427-447): the register-exchange Chebyshev kernels
    carry one (cosh, sinh) per site and colour instead of two scalars — the row layout on 16 x 16, one site per lane on 8 x 8.
    Square lattices in the patch layout (round 6): g, k (24, 20: 2 x 6, 2 x 4 patches on one wavefront), l22, l26, l34 (2 x 2 patches on two, three,
    five) and G, j, l30 (32, 28, 30: as 2 x 2 patches on four wavefronts when the hopping is disordered) keep it — a (cosh, sinh) pair per bond from
    a table in LDS (pgrid_dev.h: Sq<..., UNI = false>) — asserted taken; l36 (no table variant), i (18 x 18: measured slower) and h (honeycomb) keep
    the other kernels."""
    from elphdynamics_amd import configs, models, preconditioners as pc
    m = configs.make_model(tag, tol=1e-5, t_stddev=0.1)
    if tag in ("g", "G", "k", "j", "l22", "l26", "l30", "l34"):
        assert _pg_info(m)[0] == 1 and _pg_info(m)[4] == 1, _pg_info(m)
        if tag in ("G", "j", "l30"):
            assert _pg_info(m)[1:4] == (2, 2, 4)        # (disordered 32 x 32, 28 x 28, 30 x 30: 2 x 2 patches on four wavefronts instead of the uniform lattice's one-wavefront shape)
    elif tag in ("l36", "h", "i"):
        assert _pg_info(m)[4] == 0, _pg_info(m)
    check_kpm_with_injected_bounds_vs_oracle(oracle, m)
    m.close()


def check_kpm_with_injected_bounds_vs_oracle(oracle, m):
    """Mat-vecs, the KPM apply and the preconditioned CG of a model made with tol = 1e-5 against the oracle, the expansion set up on the
    oracle's eigenvalue bounds (the model stays open)."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    om = _oracle_model(oracle, m)
    v, y = synth.randn(177, m.Ndim), np.empty(m.Ndim)
    for fn, ofn in ((models.mulM_, oracle.mulM), (models.mulMt_, oracle.mulMT), (models.mulMtM_, oracle.mulMTM)):
        fn(y, m, v)
        assert rel(y, ofn(om, v)) < 1e-13
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    oP = oracle.make_kpm(om, n=20, buf=0.05, c1=1.0, c2=1.0)
    rng = np.random.default_rng(13)
    e_min, e_max = oracle.kpm_setup(oP, b_max=rng.standard_normal(m.Nsites), b_min=rng.standard_normal(m.Nsites))
    pc.setup_(P, e_min=e_min, e_max=e_max)
    assert P.active and oP.active == 1
    R, B = configs.rhs(m, 1)
    z = np.empty(m.Ndim)
    pc.kpm_ldiv_(z, P, np.ascontiguousarray(R[0]))
    assert rel(z, oracle.kpm_apply(oP, np.ascontiguousarray(R[0]))) < 1e-11
    b = np.ascontiguousarray(B[0])
    x = np.zeros(m.Ndim)
    it, hist = models.solve_(x, m, b, P=P, tol=1e-5, history=True)
    xo, ito, histo = oracle.cg_solve(om, b, tol=1e-5, maxiter=10000, P=oP, history=True)
    assert it == ito and rel(x, xo) < 1e-8


@pytest.mark.parametrize("tag", ["G40", "j", "h20", "l30", "l36"])
def test_patch_shape_chosen_per_launch(tag, monkeypatch):
    """32 x 32 and 28 x 28 lattices (and the honeycomb lattice of 20 x 20 cells, 4 x 2 cells per lane): from 48 right-hand sides a launch of the
    Chebyshev kernel / the p/x-fused k_cg_ap_pg takes 2 x 2 patches on four (two) wavefronts instead of the handle's 4 x 4 on one (pgrid.hip: pg_launch_shape) — the memory layout does not depend on the shape and every site sees the
    same operations in the same order, so the solve must agree with the one-shape solve (ELPH_PG_2X2_FROM=0) to rounding of the inner products: equal
    iteration counts up to the knife edge, solutions 1e-10."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    m = configs.make_model(tag, tol=1e-8)
    nchains, per = 24, 2
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=7700 + c) for c in range(nchains)])
    models.update_model_chains_(m, X)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_chains_(P, rng=np.random.default_rng(25))
    B = np.stack([synth.randn(7800 + r, m.Ndim) for r in range(nchains * per)])
    out = {}
    for mode in ("0", "48"):
        monkeypatch.setenv("ELPH_PG_2X2_FROM", mode)
        Xs = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
        assert not fl.any()
        out[mode] = (Xs, it)
    assert np.abs(out["0"][1] - out["48"][1]).max() <= 1
    assert rel(out["48"][0], out["0"][0]) < 1e-10
    m.close()


@pytest.mark.parametrize("tag,nchains,per", [("K", 8, 2), ("G40", 4, 2), ("L26", 8, 2)])
def test_hopping_disorder_in_the_patch_layout_batched(tag, nchains, per, monkeypatch):
    """The preconditioned BATCH iteration on a disordered square lattice in the patch layout (24 x 24, 32 x 32, 26 x 26 on three wavefronts; tables of
    (cosh, sinh) per bond in LDS): the p/x-fused pipeline around the table variants of k_cg_ap_pg / k_kpm_cheb_pg against the generic LDS kernels
    (ELPH_PG_DIS=0) — iteration counts within one, solutions of two tol = 1e-8 solves to 1e-9, the patch form and the fused form asserted taken."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ELPH_PG_DIS", mode)
        m = configs.make_model(tag, tol=1e-8, t_stddev=0.1)
        assert _pg_info(m)[4] == int(mode)
        nrhs = nchains * per
        X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=8800 + c) for c in range(nchains)])
        models.update_model_chains_(m, X)
        P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
        pc.setup_chains_(P, rng=np.random.default_rng(15))
        B = np.stack([synth.randn(8900 + r, m.Ndim) for r in range(nrhs)])
        Xs = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
        assert not fl.any()
        out[mode] = (Xs, it, _px_fused(m))
        m.close()
    assert out["1"][2] is True, "the p/x-fused form was not taken"
    assert np.abs(out["0"][1] - out["1"][1]).max() <= 1
    assert rel(out["1"][0], out["0"][0]) < 1e-9


def _holstein_16x16_ltau80():
    """Config C's lattice with 80 time slices: the smallest model on which both resident kernels exist (k_pcg_wg: 5 CG workgroups)."""
    from elphdynamics_amd import lattice as lat, models, synth
    m = models.HolsteinModel(lat.Lattice(1, 16, 16, 1), 8.0, 0.1, tol=1e-5, maxiter=10000)
    m.assign_t_(1.0, 1, 1, (1, 0, 0)); m.assign_t_(1.0, 1, 1, (0, 1, 0))
    m.assign_omega_(1.0); m.assign_lambda_(1.0); m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, 8.0, 0.1, omega=1.0, lam=1.0, seed=21)
    models.update_model_(m)
    assert m.Ltau == 80
    return m


@pytest.mark.parametrize("ltau", [160, 80])
def test_resident_preconditioned_cg_vs_streaming_and_oracle(oracle, monkeypatch, ltau):
    """pcg_wg.hip (ELPH_PCG_WG=1: the whole KPM-preconditioned solve of 1..8 right-hand sides in one launch — CG workgroups, helper
    workgroups for the two tau-transforms and the Chebyshev recursions, flags through L2 instead of kernel boundaries) against the
    five-kernel streaming form and the oracle on config C (160 time slices: 40 reduction tiles per transform tile) and on the same
    lattice with 80 slices (the 20-tile instantiation; 5 CG workgroups, helpers with two frequencies per wave pair idle in part):
    same iteration counts, same residual history, solutions to 1e-10."""
    from elphdynamics_amd import configs, models, preconditioners as pc
    m = configs.make_model("C", tol=1e-5) if ltau == 160 else _holstein_16x16_ltau80()
    om = _oracle_model(oracle, m)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    oP = oracle.make_kpm(om, n=20, buf=0.05, c1=1.0, c2=1.0)
    rng = np.random.default_rng(11)
    e_min, e_max = oracle.kpm_setup(oP, b_max=rng.standard_normal(m.Nsites), b_min=rng.standard_normal(m.Nsites))
    pc.setup_(P, e_min=e_min, e_max=e_max)
    R, B = configs.rhs(m, 3)
    out = {}
    for name, flag in (("stream", "0"), ("resident", "1")):
        monkeypatch.setenv("ELPH_PCG_WG", flag)
        m.solver.tol = 1e-5
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B, P=P)
        assert not fl.any(), name
        x1 = np.zeros(m.Ndim)
        it1, hist = models.solve_(x1, m, np.ascontiguousarray(B[0]), P=P, tol=1e-5, history=True)
        m.solver.tol = 1e-13
        X13 = np.zeros_like(B)
        it13, _, fl13 = models.ldiv_batched_(X13, m, B, P=P)
        assert not fl13.any(), name
        out[name] = (X, it, hist, it1, X13, it13)
    a, b = out["resident"], out["stream"]
    assert np.array_equal(a[1], b[1]) and a[3] == b[3] and np.max(np.abs(a[5] - b[5])) <= 1
    assert rel(a[0], b[0]) < 1e-9 and rel(a[4], b[4]) < 1e-11
    n = min(len(a[2]), len(b[2]))
    assert np.max(np.abs(a[2][:n] - b[2][:n]) / b[2][:n]) < 1e-9
    xo, ito, histo = oracle.cg_solve(om, np.ascontiguousarray(B[0]), tol=1e-5, maxiter=10000, P=oP, history=True)
    assert a[3] == ito
    k = min(21, ito // 4 + 1)
    assert np.max(np.abs(a[2][:k] - histo[:k]) / histo[:k]) < 1e-10
    xo13, _, _, _ = oracle.ldiv(om, np.ascontiguousarray(B[0]), P=oP, solver_tol=1e-13, solver_maxiter=20000)
    assert rel(a[4][0], xo13) < 1e-10
    m.close()


@pytest.mark.parametrize("inactive", [None, 2])
def test_resident_preconditioned_cg_default_batch_of_chains(monkeypatch, inactive):
    """What the defaults select for 3-4 HMC chains: 4 chains x 2 = 8 right-hand sides, KPM-preconditioned, ELPH_PCG_WG unset — the
    resident kernel (k_pcg_wg) when every chain's expansion is active, against the streaming form (ELPH_PCG_WG=0): same iteration
    counts, solutions to 1e-9 at tol 1e-5 and 1e-11 at 1e-13.  With ONE chain's expansion inactive (its injected bounds fail the test
    of KPMPreconditioners.jl:280: identity, z = r) the resident kernel — which runs every chain's series without looking at the
    active flag — must not be taken: both settings then run the streaming form and agree bit for bit, and the inactive chain's
    right-hand sides need the un-preconditioned iteration count."""
    import ctypes as C
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    m = configs.make_model("C", tol=1e-5)
    nch = 4
    Xc = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=300 + 17 * c) for c in range(nch)])
    models.update_model_chains_(m, Xc)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    rng = np.random.default_rng(5)
    act, lo, hi = pc.setup_chains_(P, b_max=rng.standard_normal((nch, m.Nsites)), b_min=rng.standard_normal((nch, m.Nsites)))
    assert act.all()
    if inactive is not None:      # the same bounds again, chain `inactive` with e_min > 1: not accepted -> identity expansion for that chain
        e_min, e_max = lo / 0.9, hi / 1.1
        e_min[inactive] = 1.5
        act, _, _ = pc.setup_chains_(P, e_min=e_min, e_max=e_max)
        assert act.tolist() == [1 if c != inactive else 0 for c in range(nch)]
    R, B = configs.rhs(m, 2 * nch)
    out = {}
    for name, flag in (("default", None), ("stream", "0")):
        if flag is None:
            monkeypatch.delenv("ELPH_PCG_WG", raising=False)
        else:
            monkeypatch.setenv("ELPH_PCG_WG", flag)
        m.solver.tol = 1e-5
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B, P=P)
        assert not fl.any(), (name, fl)
        m.solver.tol = 1e-13
        X13 = np.zeros_like(B)
        it13, _, fl13 = models.ldiv_batched_(X13, m, B, P=P)
        assert not fl13.any(), name
        out[name] = (X, it, X13, it13)
    a, b = out["default"], out["stream"]
    assert np.array_equal(a[1], b[1]) and np.max(np.abs(a[3] - b[3])) <= 1
    if inactive is None:
        assert rel(a[0], b[0]) < 1e-9 and rel(a[2], b[2]) < 1e-11
        assert not np.array_equal(a[0], b[0])                   # (two different kernels did run: summation orders differ)
    else:
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        own = [r for r in range(2 * nch) if r % nch == inactive]
        others = [r for r in range(2 * nch) if r % nch != inactive]
        assert min(a[1][own]) > 5 * max(a[1][others])           # identity preconditioner: hundreds of iterations against ~25
    m.close()


def test_resident_preconditioned_cg_recovers_after_a_timeout(monkeypatch):
    """A handle that only runs PRECONDITIONED solves: k_pcg_wg gives up (1 ms bound with eight teams side by side is not reliably
    enough — so the time-out is forced by ELPH_WG_TIMEOUT_MS=0-like bound of 1 tick through the environment), the solve is redone by
    the streaming form, elph_wg_status counts the fallback and the cool-down runs DOWN over the following preconditioned solves
    (round 3: only un-preconditioned solves counted it down) until the resident kernel is taken again."""
    import ctypes as C
    from elphdynamics_amd import configs, models, preconditioners as pc
    m = configs.make_model("C", tol=1e-5)
    lib = m._lib
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, rng=np.random.default_rng(3))
    R, B = configs.rhs(m, 8)
    monkeypatch.setenv("ELPH_PCG_WG", "1")
    monkeypatch.setenv("ELPH_WG_COOLDOWN", "3")
    X0 = np.zeros_like(B)
    it0, _, fl0 = models.ldiv_batched_(X0, m, B, P=P)            # healthy resident solve
    cool, falls = C.c_int(), C.c_int64()
    lib.elph_wg_status(m._h, C.byref(cool), C.byref(falls))
    assert not fl0.any() and cool.value == 0 and falls.value == 0
    monkeypatch.setenv("ELPH_WG_TIMEOUT_MS", "-1")               # every wait gives up at its first look at the clock
    X1 = np.zeros_like(B)
    it1, _, fl1 = models.ldiv_batched_(X1, m, B, P=P)
    lib.elph_wg_status(m._h, C.byref(cool), C.byref(falls))
    assert not fl1.any() and np.array_equal(it1, it0) and rel(X1, X0) < 1e-9      # redone by the streaming form
    assert falls.value == 1 and cool.value == 3
    monkeypatch.setenv("ELPH_WG_TIMEOUT_MS", "60000")
    seen = []
    for k in range(4):
        X = np.zeros_like(B)
        it, _, fl = models.ldiv_batched_(X, m, B, P=P)
        assert not fl.any() and np.array_equal(it, it0)
        lib.elph_wg_status(m._h, C.byref(cool), C.byref(falls))
        seen.append(cool.value)
    assert seen == [2, 1, 0, 0] and falls.value == 1, seen      # two solves on the streaming form, then the resident kernel again
    m.close()


def test_kpm_fallback_to_unpreconditioned(oracle):
    """Models.jl:129-133: a preconditioned solve that fails (maxiter) is redone without P and 10x maxiter."""
    from elphdynamics_amd import configs, models, preconditioners as pc
    m = configs.make_model("b", tol=1e-8, maxiter=40)
    om = _oracle_model(oracle, m)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, e_min=0.5, e_max=1.9)                           # deliberately poor bounds: weak preconditioner
    oP = oracle.make_kpm(om)
    oracle.kpm_setup(oP, e_min=0.5, e_max=1.9)
    R, B = configs.rhs(m, 1)
    b = np.ascontiguousarray(B[0])
    x = np.zeros(m.Ndim)
    it, res, fl = models.ldiv_(x, m, b, P=P, maxiter=5)
    xo, ito, reso, flo = oracle.ldiv(om, b, P=oP, maxiter=5, solver_tol=1e-8, solver_maxiter=40)
    assert (it, fl) == (ito, flo)
    assert rel(x, xo) < 1e-6 if fl == 0 else not x.any()
    m.close()


def test_fourier_accelerate_full_size(oracle):
    from elphdynamics_amd import configs, preconditioners as pc, synth
    from oracle.oracle import dp
    m = configs.make_model("C")
    fa = pc.FourierAccelerator(m)
    pc.update_M_(fa, m, 0.0, 10.0, 0.1, 2.0)
    pc.update_Q_(fa, m, 0.0, 10.0, 0.5)
    oM = np.zeros(m.Ndim)
    oracle.lib.elpho_update_M(dp(oM), m.Nph, m.Ltau, m.dtau, dp(m.omega), 0.0, 10.0, 0.1, 2.0)
    assert rel(fa.M, oM) < 1e-15
    v = synth.randn(5, m.Ndim)
    for power, use_mass in ((-1.0, True), (-0.5, True), (1.0, True), (1.0, False)):
        out = np.empty(m.Ndim)
        pc.fourier_accelerate_(out, fa, v, power, use_mass=use_mass)
        ref = np.zeros(m.Ndim)
        oracle.lib.elpho_fourier_accelerate(dp(ref), dp(v), dp(fa.M if use_mass else fa.Q), power, m.Nph, m.Ltau)
        assert rel(out, ref) < 1e-12
    back = np.empty(m.Ndim)
    tmp = np.empty(m.Ndim)
    pc.fourier_accelerate_(tmp, fa, v, -1.0, use_mass=True)
    pc.fourier_accelerate_(back, fa, tmp, 1.0, use_mass=True)
    assert rel(back, v) < 1e-12                                  # D^-1 then D is the identity
    m.close()


def test_error_paths(lib):
    from elphdynamics_amd import _lib
    h = _lib.Handle()
    tab = np.array([[1, 2], [2, 9]], dtype=np.int64)
    assert lib.elph_create(C.byref(h), 0, 4, 4, 2, _lib.iptr(tab), _lib.dptr(np.ones(2)), _lib.dptr(np.ones(2)), 0) == -1
    assert b"out of range" in lib.elph_last_error()
    assert lib.elph_create(C.byref(h), 7, 4, 4, 0, None, None, None, 0) == -1
    assert lib.elph_create(C.byref(h), 0, 4, 4, 0, None, None, None, 99) == -1
    m = RawModel(lib, 0, 4, 4, np.zeros((0, 2), dtype=np.int64))
    y = np.zeros(16)
    assert lib.elph_mulM(m.h, _lib.dptr(y), _lib.dptr(y)) == -3          # update_model not called yet
    assert lib.elph_kpm_apply(m.h, _lib.dptr(y), _lib.dptr(y)) == -3
    m.close()
    # a table that is NOT in checkerboard order is still applied in the given sequential order
    g = golden("holstein_sq4_L8.npz")
    N, L = int(g["N"]), int(g["Ltau"])
    perm = np.random.default_rng(0).permutation(g["table"].shape[0])
    m2 = RawModel(lib, 0, N, L, g["table"][perm], g["cosht"][perm], g["sinht"][perm])
    _lib.check(lib.elph_set_expV(m2.h, _lib.dptr(np.ascontiguousarray(g["E"]))))
    from oracle.oracle import Oracle
    orc = Oracle()
    om = orc.make_model(0, N, L, g["table"][perm], g["cosht"][perm], g["sinht"][perm], g["E"])
    assert rel(m2.op("elph_mulM", g["v"]), orc.mulM(om, np.ascontiguousarray(g["v"]))) < 1e-13
    assert rel(m2.op("elph_mulMTM", g["v"]), orc.mulMTM(om, np.ascontiguousarray(g["v"]))) < 1e-13
    m2.close()


# ------------------------------------------------------------------------------------------ callers (a22, a23)

def test_calc_OinvLambda_phi_vs_oracle(oracle):
    """HMC.calc_O⁻¹Λϕ! (HMC.jl:820-915): Λ construction, the two solves as one batch, tol^power, cld(iters,2)."""
    check_calc_OinvLambda_phi_vs_oracle(oracle, "B")


def check_calc_OinvLambda_phi_vs_oracle(oracle, tag, prepare=None):
    """prepare(m): called on the model before anything reads its parameter arrays."""
    from elphdynamics_amd import configs, hmc, synth
    from oracle.oracle import dp
    m = configs.make_model(tag, tol=1e-4)
    if prepare is not None:
        prepare(m)
    om = _oracle_model(oracle, m)
    N, L, n = m.Nsites, m.Ltau, m.Ndim
    phi_p, phi_m = synth.randn(301, n), synth.randn(302, n)
    Lam = np.zeros(n)
    oracle.lib.elpho_update_Lambda(dp(Lam), N, L, m.dtau, dp(m.x), dp(m.lam), dp(m.lam2))
    Lg = np.empty(n)
    hmc.update_Lambda_(Lg, m)
    assert rel(Lg, Lam) < 1e-15
    tot, xs = 0, []
    for phi in (phi_p, phi_m):
        b = np.zeros(n)
        oracle.lib.elpho_mulLambda(dp(b), dp(phi), dp(Lam), N, L)
        bg = np.empty(n)
        hmc.mulLambda_(bg, phi, Lg, m)
        assert rel(bg, b) < 1e-15
        back = np.empty(n)
        hmc.mulLambdaInv_(back, bg, Lg, m)
        assert rel(back, phi) < 1e-14
        x, it, res, fl = oracle.ldiv(om, b, solver_tol=(1e-4) ** 2.0, solver_maxiter=10000)
        assert fl == 0
        tot += it
        xs.append(x)
    Xp, Xm, iters, flag = hmc.calc_OinvLambda_phi(m, phi_p, phi_m, None, power=2.0)
    assert flag == 0 and abs(iters - (-(-tot // 2))) <= 1
    assert rel(Xp, xs[0]) < 1e-6 and rel(Xm, xs[1]) < 1e-6        # both within tol^2 = 1e-8 of the same solution
    assert m.solver.tol == 1e-4                                    # restored (HMC.jl:912)
    m.close()


@pytest.mark.parametrize("tag", ["B", "e"])
def test_calc_OinvLambda_phi_when_the_first_solve_fails(oracle, tag):
    """HMC.jl:880: a flagged phi+ solve suppresses the phi- solve — its output stays zero, the iteration count is that of the first
    solve alone and is not halved (:907-909).  The device runs both solves as one batch; the bookkeeping follows the reference."""
    from elphdynamics_amd import configs, hmc, synth
    from oracle.oracle import dp
    m = configs.make_model(tag, tol=1e-9, maxiter=4)
    om = _oracle_model(oracle, m)
    n = m.Ndim
    phi_p, phi_m = synth.randn(311, n), synth.randn(312, n)
    if m.kind == 0:
        Lam = np.zeros(n)
        oracle.lib.elpho_update_Lambda(dp(Lam), m.Nsites, m.Ltau, m.dtau, dp(m.x), dp(m.lam), dp(m.lam2))
        b = np.zeros(n)
        oracle.lib.elpho_mulLambda(dp(b), dp(phi_p), dp(Lam), m.Nsites, m.Ltau)
    else:
        b = phi_p                                                  # SSH: mulLambda! is a no-op (HMC.jl:943-946,970-973)
    xo, ito, reso, flo = oracle.ldiv(om, b, solver_tol=1e-9, solver_maxiter=4)
    assert flo != 0 and ito == 4
    Xp, Xm, iters, flag = hmc.calc_OinvLambda_phi(m, phi_p, phi_m, None, power=1.0)
    assert flag == flo and iters == ito
    assert not Xm.any() and not Xp.any()                           # ldiv! zero-fills a flagged solution (Models.jl:160-166)
    m.close()


def test_greens_estimator_vs_oracle(oracle):
    """GreensFunctions.update!/estimate (:201-234,:334-346): M^-1 R for n_v vectors, G = (M^-1 r)[n] r[m]."""
    from elphdynamics_amd import configs, hmc, synth
    m = configs.make_model("b", tol=1e-13)
    om = _oracle_model(oracle, m)
    est = hmc.GreensEstimator(m, nv=3)
    R = np.stack([synth.randn(900 + i, m.Ndim) for i in range(3)])
    it, res, fl = est.update_(None, R=R)
    assert not fl.any()
    for i in range(3):
        r = np.ascontiguousarray(R[i])
        xo, ito, reso, flo = oracle.ldiv(om, oracle.mulMT(om, r), solver_tol=1e-13, solver_maxiter=10000)
        assert rel(est.MinvR[i], xo) < 1e-10
    g = est.estimate(2, 3, 4, 5, n=1)
    L = m.Ltau
    assert g == est.MinvR[1, (2 - 1) * L + 3] * R[1, (3 - 1) * L + 4]
    # a Green's-function element averaged over vectors agrees with the oracle's to 1e-10 relative to its scale
    go = np.mean([oracle.ldiv(om, oracle.mulMT(om, np.ascontiguousarray(R[i])), solver_tol=1e-13, solver_maxiter=10000)[0][(2 - 1) * L + 3]
                  * R[i, (3 - 1) * L + 4] for i in range(3)])
    gg = np.mean([est.estimate(2, 3, 4, 5, n=i) for i in range(3)])
    assert abs(gg - go) < 1e-10 * max(1.0, abs(go))
    m.close()


@pytest.mark.parametrize("tag", ["C", "D", "E", "T"])
def test_streaming_cg_with_ragged_chunks(tag, oracle, monkeypatch):
    """k_cg_ap_chunk_rt: the batched streaming kernel with a run-time chunk length and a ragged last chunk (what a batch runs when the
    template sizes would need more waves than the chip has slots: 288 right-hand sides of config C take 7 chunks of 23, ..., 22
    slices).  Forced here through ELPH_CHUNK_T on small batches: against the unrolled template kernel (same operations per element:
    solutions within the rounding of the regrouped p.z sums) and against the oracle; Holstein square / honeycomb / triangular
    (six colours) and SSH; un-preconditioned and (C) KPM-preconditioned."""
    from elphdynamics_amd import configs, models, preconditioners as pc
    monkeypatch.setenv("ELPH_NO_WG", "1")
    out = {}
    for T in ("0", "23", "7", "3"):
        monkeypatch.setenv("ELPH_CHUNK_T", T)
        m = configs.make_model(tag, tol=1e-13, maxiter=20000)
        R, B = configs.rhs(m, 5)
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B)
        assert not fl.any(), (tag, T)
        out[T] = (X, it)
        if T == "23":
            om = _oracle_model(oracle, m)
            xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(B[0]), solver_tol=1e-13, solver_maxiter=20000)
            assert flo == 0 and rel(X[0], xo) < 1e-10 and abs(int(it[0]) - ito) <= max(3, ito // 100)
            if tag == "C":
                P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
                pc.setup_(P, rng=np.random.default_rng(3))
                Xp = np.zeros_like(B)
                itp, resp, flp = models.ldiv_batched_(Xp, m, B, P=P)
                assert not flp.any() and itp.max() < it.min() and rel(Xp, X) < 1e-10
        m.close()
    for T in ("23", "7", "3"):
        assert np.max(np.abs(out[T][1] - out["0"][1])) <= max(3, int(out["0"][1].max()) // 100), (tag, T, out[T][1], out["0"][1])   # (1e-13: the residual history is flat at the end)
        assert rel(out[T][0], out["0"][0]) < 1e-11, (tag, T, rel(out[T][0], out["0"][0]))


def test_repeated_solves_are_bit_identical():
    """Regression for a same-kernel reader/writer race on the double-buffered CG state: every solve of the same
    system must return the same bits and the same iteration count (single and batched, tiny and full size)."""
    import hashlib
    from elphdynamics_amd import configs, models
    for tag, nrhs, reps in (("b", 1, 150), ("b", 8, 60), ("C", 1, 40), ("C", 8, 15)):
        m = configs.make_model(tag, tol=1e-10 if tag == "b" else 1e-5)
        R, B = configs.rhs(m, nrhs)
        seen = set()
        for _ in range(reps):
            X = np.zeros_like(B)
            it, res, fl = models.ldiv_batched_(X, m, B)
            seen.add((tuple(it.tolist()), hashlib.md5(X.tobytes()).hexdigest()))
        assert len(seen) == 1, (tag, nrhs, len(seen))
        m.close()


def _oracle_force(oracle, om, m, phi_p, phi_m, tol):
    """calc_O⁻¹Λϕ! + calc_dSfdx! composed from the oracle's pieces; also returns S_f."""
    from oracle.oracle import dp
    import ctypes as C
    N, L, n = m.Nsites, m.Ltau, m.Ndim
    Lam = np.zeros(n)
    oracle.lib.elpho_update_Lambda(dp(Lam), N, L, m.dtau, dp(np.ascontiguousarray(m.x)), dp(m.lam), dp(m.lam2))
    X, Sf = [], 0.0
    for phi in (phi_p, phi_m):
        b = np.zeros(n)
        oracle.lib.elpho_mulLambda(dp(b), dp(np.ascontiguousarray(phi)), dp(Lam), N, L)
        x, it, res, fl = oracle.ldiv(om, b, solver_tol=tol, solver_maxiter=20000)
        assert fl == 0
        X.append(x)
        Sf += 0.5 * (b @ x)
    F = np.zeros(n)
    u, d = np.zeros(n), np.zeros(n)
    oracle.lib.elpho_calc_dSfdx_holstein(dp(F), C.byref(om), dp(X[0]), dp(X[1]), dp(np.ascontiguousarray(phi_p)),
                                         dp(np.ascontiguousarray(phi_m)), dp(Lam), m.dtau, dp(m.lam), dp(m.lam2),
                                         dp(np.ascontiguousarray(m.x)), dp(u), dp(d))
    return F, X, Sf


@pytest.mark.parametrize("tag", ["b", "B", "d", "g", "C", "D"])
def test_fermion_force_vs_oracle(oracle, tag):
    """update_model! + calc_O⁻¹Λϕ! + calc_dSfdx! on the device vs the oracle's composition."""
    check_fermion_force_vs_oracle(oracle, tag)


# the relative bound of check_fermion_force_vs_oracle on the solutions and on F, by name (tests/test_site_disorder_host.py)
FORCE_BOUND = 1e-8


def check_fermion_force_vs_oracle(oracle, tag, prepare=None):
    """prepare(m): called on the model before anything reads its parameter arrays."""
    from elphdynamics_amd import configs, hmc, synth
    m = configs.make_model(tag, tol=1e-11)
    m.lam2[:] = 0.03 * synth.randn(5, m.Nsites)                 # exercise the lambda2 terms too
    if prepare is not None:
        prepare(m)
    om_E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
    om = oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, om_E)
    phi_p, phi_m = synth.randn(41, m.Ndim), synth.randn(42, m.Ndim)
    Fo, Xo, _ = _oracle_force(oracle, om, m, phi_p, phi_m, 1e-11)
    F = np.ones(m.Ndim)                                           # accumulation: starts from a non-zero array
    it, fl, Xp, Xm = hmc.calc_dSfdx_(F, m, phi_p, phi_m, None, power=1.0, return_solutions=True)
    assert fl == 0 and it > 0
    assert rel(Xp, Xo[0]) < FORCE_BOUND and rel(Xm, Xo[1]) < FORCE_BOUND
    assert rel(F - 1.0, Fo) < FORCE_BOUND
    m.close()


def test_fermion_force_is_the_gradient_of_the_action(oracle):
    """dS_f/dx_k from the device force equals a central finite difference of
    S_f(x) = 1/2 sum_± (Λϕ±)ᵀ (MᵀM)⁻¹ (Λϕ±)  (HMC.jl:757-783) evaluated with the oracle."""
    check_fermion_force_is_the_gradient_of_the_action(oracle, "b", lambda m: (0, 7, m.Ltau, 5 * m.Ltau + 3, m.Ndim - 1))


def check_fermion_force_is_the_gradient_of_the_action(oracle, tag, probes, prepare=None):
    """probes(m): the elements of the field the difference quotient is taken at; prepare(m): called on the model before anything
    reads its parameter arrays."""
    from elphdynamics_amd import configs, hmc, synth
    m = configs.make_model(tag, tol=1e-12)
    m.lam2[:] = 0.02
    if prepare is not None:
        prepare(m)
    phi_p, phi_m = synth.randn(51, m.Ndim), synth.randn(52, m.Ndim)
    F = np.zeros(m.Ndim)
    it, fl = hmc.calc_dSfdx_(F, m, phi_p, phi_m, None, power=1.0)
    assert fl == 0
    x0 = m.x.copy()
    h = 1e-5
    for k in probes(m):
        S = []
        for sgn in (+1, -1):
            m.x[:] = x0
            m.x[k] += sgn * h
            E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
            om = oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)
            S.append(_oracle_force(oracle, om, m, phi_p, phi_m, 1e-13)[2])
        fd = (S[0] - S[1]) / (2 * h)
        assert abs(fd - F[k]) < 2e-6 * max(1.0, abs(F[k])), (k, fd, F[k])
    m.x[:] = x0
    m.close()


@pytest.mark.parametrize("tag,nchains,per", [("b", 3, 2), ("C", 4, 2), ("C", 32, 2), ("e", 3, 2), ("E", 4, 2), ("E", 16, 2),
                                             ("C", 64, 2), ("E", 64, 2),      # 128 right-hand sides: 20 slices per wave
                                             ("D", 4, 2), ("D", 16, 2)])     # honeycomb DPP form of the resident kernel, 1 and 2 slices per wave
def test_independent_chains_in_one_batch(tag, nchains, per):
    """Several phonon configurations resident in one handle (the reference runs chains as separate processes,
    ElPhDynamics.jl:90-95): right-hand side r of a batch uses the fermion matrix of chain r % nchains, and each
    solve is bit-identical to the same solve done alone on a single-configuration model."""
    from elphdynamics_amd import configs, models, synth
    m = configs.make_model(tag, tol=1e-5)
    if m.kind == models.SSH:      # bond phonons: every chain its own hopping tables (cosh/sinh per bond and time slice)
        X = np.stack([m.x * (0.55 + 0.9 * c / nchains) * (1.0 + 0.2 * synth.randn(5000 + c, m.Ndof)) for c in range(nchains)])
    else:
        X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=5000 + c) for c in range(nchains)])
    nrhs = nchains * per
    B = np.stack([synth.randn(7000 + r, m.Ndim) for r in range(nrhs)])
    models.update_model_chains_(m, X)
    Xs = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(Xs, m, B)
    assert not fl.any()
    check_r = range(nrhs) if nrhs <= 8 else (0, 1, nchains - 1, nchains, nrhs - 1)
    for r in check_r:
        m1 = configs.make_model(tag, tol=1e-5)
        m1.x[:] = X[r % nchains]
        models.update_model_(m1)
        x1 = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x1, m1, np.ascontiguousarray(B[r]))
        assert fl1 == 0
        if nrhs * m.Ltau // 5 < 1024 and _wg_info(m, nrhs)[1] == _wg_info(m, 1)[1]:   # same kernel variant (slices per wave) as the single solve => same bits
            if not (it1 == it[r] and np.array_equal(x1, Xs[r])):      # diagnostics: is it the handle (tables) or the launch?
                x2 = np.zeros(m.Ndim)
                it2, _, _ = models.ldiv_(x2, m1, np.ascontiguousarray(B[r]))
                Xs2 = np.zeros_like(B)
                itb2, _, _ = models.ldiv_batched_(Xs2, m, B)
                raise AssertionError((r, it1, int(it[r]), "again on the same handle", it2, bool(np.array_equal(x2, x1)), bool(np.array_equal(x2, Xs[r])),
                                      "batch again", int(itb2[r]), bool(np.array_equal(Xs2[r], Xs[r])), "rel", rel(x1, Xs[r]),
                                      _wg_status(m1), _wg_status(m), _wg_info(m1, 1)))
        else:                                 # large batches use k_cg_ap_chunk<T>: p.z partial sums grouped per chunk,
            assert abs(it1 - it[r]) <= 5      # so round-off (not the arithmetic per element) differs from the T=1 kernel
            assert rel(x1, Xs[r]) < 2e-4      # two tol=1e-5 solves of the same system
        m1.close()
    # going back to a single configuration resets the chain count
    models.update_model_(m)
    x = np.zeros(m.Ndim)
    models.ldiv_(x, m, np.ascontiguousarray(B[0]))
    m.close()


def _ssh_oracle_bits(oracle, m):
    om = oracle.make_model(1, m.Nsites, m.Ltau, m.neighbor_table, np.ascontiguousarray(m.cosht).reshape(-1),
                           np.ascontiguousarray(m.sinht).reshape(-1), m.expDtauMu)
    b2p = np.zeros(m.Nbonds, dtype=np.int64)
    b2p[m.checkerboard_perm[m.phonon_to_bond - 1] - 1] = np.arange(1, m.Nph + 1)
    return om, b2p


def _ssh_oracle_force(oracle, m, bp, bm, tol):
    from oracle.oracle import dp, ip
    import ctypes as C
    om, b2p = _ssh_oracle_bits(oracle, m)
    F = np.zeros(m.Ndof)
    Sf = 0.0
    for b in (bp, bm):
        x, it, res, fl = oracle.ldiv(om, np.ascontiguousarray(b), solver_tol=tol, solver_maxiter=20000)
        assert fl == 0
        Sf += 0.5 * (b @ x)
        u = oracle.mulM(om, x)
        d = np.zeros(m.Ndof)
        oracle.lib.elpho_muldMdx_ssh(dp(d), dp(u), C.byref(om), dp(x), m.dtau, ip(b2p), dp(m.alpha), dp(m.alpha2),
                                     dp(np.ascontiguousarray(m.x)), m.Nph)
        F -= d
    return F, Sf


@pytest.mark.parametrize("tag", ["e", "E"])
def test_ssh_fermion_force_vs_oracle(oracle, tag):
    """SURVEY §8f-1 for the SSH model: muldMdx! on bond phonons (SSHModels.jl:707-829) through the device path."""
    from elphdynamics_amd import configs, hmc, models, synth
    m = configs.make_model(tag, tol=1e-11)
    m.alpha2[:] = 0.02
    models.update_model_(m)
    bp, bm = synth.randn(61, m.Ndim), synth.randn(62, m.Ndim)
    Fo, _ = _ssh_oracle_force(oracle, m, bp, bm, 1e-11)
    F = np.zeros(m.Ndof)
    it, fl = hmc.calc_dSfdx_(F, m, bp, bm, None, power=1.0)
    assert fl == 0 and rel(F, Fo) < 1e-8
    m.close()


def test_ssh_fermion_force_is_the_gradient_of_the_action(oracle):
    """With alpha2 = 0 the reference's dK/dx = alpha + 2 alpha2 x (SSHModels.jl:803) is the exact derivative of
    update_model!'s t' = t - (alpha x + sign(x) alpha2 x^2) (:528); for alpha2 != 0 and x < 0 the two differ by the
    sign(x) factor — a reference quirk that the mirror reproduces (parity test above), not a gradient."""
    from elphdynamics_amd import configs, hmc, models, synth
    m = configs.make_model("e", tol=1e-12)
    bp, bm = synth.randn(71, m.Ndim), synth.randn(72, m.Ndim)
    F = np.zeros(m.Ndof)
    it, fl = hmc.calc_dSfdx_(F, m, bp, bm, None, power=1.0)
    assert fl == 0
    x0 = m.x.copy()
    h = 1e-5
    for k in (0, 3, m.Ltau + 1, 7 * m.Ltau + 5, m.Ndof - 1):
        S = []
        for sgn in (+1, -1):
            m.x[:] = x0
            m.x[k] += sgn * h
            models.update_model_(m)                      # host-side cosh/sinh of the perturbed field
            S.append(_ssh_oracle_force(oracle, m, bp, bm, 1e-13)[1])
        fd = (S[0] - S[1]) / (2 * h)
        assert abs(fd - F[k]) < 2e-6 * max(1.0, abs(F[k])), (k, fd, F[k])
    m.close()


# ------------------------------------------------------------------------------------------ matrix-core DFT

@pytest.mark.parametrize("L", [7, 8, 40, 120, 160])
def test_mfma_dft_matches_golden_and_scalar_kernels(lib, L, monkeypatch):
    """dft_mfma.hip (v_mfma_f64_16x16x4 GEMM form, used for batches) against the golden FFTs and against the
    scalar-twiddle kernels of dft.hip on the same input — ragged N (3 and 70 sites: column clamps), odd L."""
    from elphdynamics_amd import _lib
    g = golden("fft.npz")
    for N in (3, 70):
        m = RawModel(lib, 0, N, L, np.zeros((0, 2), dtype=np.int64))
        try:
            v = np.ascontiguousarray(g[f"L{L}_v"]) if N == 3 else np.random.default_rng(L).standard_normal(N * L)
            res = {}
            for mode in ("0", "1"):
                monkeypatch.setenv("ELPH_DFT_MFMA", mode)
                nu = np.zeros(2 * N * L)
                _lib.check(lib.elph_tau_to_omega(m.h, _lib.dptr(nu), _lib.dptr(v)))
                back = np.zeros(N * L)
                _lib.check(lib.elph_omega_to_tau(m.h, _lib.dptr(back), _lib.dptr(nu)))
                res[mode] = (nu, back)
                assert rel(back, v) < 1e-13
                if N == 3:
                    assert rel(nu[0::2], g[f"L{L}_nu_re"]) < 1e-13 and rel(nu[1::2], g[f"L{L}_nu_im"]) < 1e-13
            assert rel(res["1"][0], res["0"][0]) < 1e-14 and rel(res["1"][1], res["0"][1]) < 1e-14
        finally:
            m.close()


def test_mfma_dft_inside_batched_preconditioned_solve(monkeypatch):
    """A 24-right-hand-side KPM-preconditioned solve at config B runs the GEMM-form DFTs (forward, and the inverse with
    its fused r.z partial sums); same iteration counts and solutions as the scalar-kernel path."""
    from elphdynamics_amd import configs, models, preconditioners as pc
    m = configs.make_model("B", tol=1e-8)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, rng=np.random.default_rng(3))
    _, B = configs.rhs(m, 24)
    out = {}
    # scalar kernels | GEMM form with the even/odd split and k_cg_xr folded into the forward transform | split, separate k_cg_xr |
    # direct GEMM form
    for mode, env in (("0", {"ELPH_DFT_MFMA": "0"}), ("1", {"ELPH_DFT_MFMA": "1"}), ("nofuse", {"ELPH_DFT_MFMA": "1", "ELPH_FUSE_XR": "0"}),
                      ("direct", {"ELPH_DFT_MFMA": "1", "ELPH_DFT_R2": "0"})):
        for k in ("ELPH_DFT_MFMA", "ELPH_FUSE_XR", "ELPH_DFT_R2"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B, P=P)
        assert not fl.any()
        out[mode] = (X, it)
    for mode in ("1", "nofuse", "direct"):
        assert np.array_equal(out["0"][1], out[mode][1]), mode
        assert rel(out[mode][0], out["0"][0]) < 1e-10, mode
    m.close()


@pytest.mark.parametrize("tag", ["C", "D", "b", "q", "S", "d", "z", "Y"])
def test_kpm_register_exchange_recursion_equals_the_lds_recursion(tag, monkeypatch):
    """The Chebyshev recursion of the KPM apply in registers (square lattice: 2 x 2 patches; honeycomb of 12 x 12 cells: three cells
    per lane, four lanes of a DPP quad per lattice row) against the lane-program recursion in LDS (ELPH_NO_SQ=1): the same series
    (KPMPreconditioners.jl:606-693), factored colours and another summation order — P^-1 r to 1e-12, and the same iteration counts."""
    from elphdynamics_amd import configs, models, preconditioners as pc
    m = configs.make_model(tag, tol=1e-10)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, rng=np.random.default_rng(7))
    R, B = configs.rhs(m, 3)
    out = {}
    for name, env in (("reg", None), ("lds", "1")):
        if env is None:
            monkeypatch.delenv("ELPH_NO_SQ", raising=False)
        else:
            monkeypatch.setenv("ELPH_NO_SQ", env)
        z = np.zeros(m.Ndim)
        pc.kpm_ldiv_(z, P, np.ascontiguousarray(B[0]))
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B, P=P)
        assert not fl.any()
        out[name] = (z, X, it)
    assert rel(out["reg"][0], out["lds"][0]) < 1e-12
    assert np.max(np.abs(out["reg"][2] - out["lds"][2])) <= 1 and rel(out["reg"][1], out["lds"][1]) < 1e-9
    m.close()


@pytest.mark.parametrize("tag", ["g", "G", "k", "j", "i", "l30", "K", "h", "h20", "h21", "h24", "H18", "u", "T", "t6", "t12", "t20", "t24", "t32"])
def test_kpm_patch_recursion_equals_the_generic_recursion(tag, monkeypatch):
    """Even-L square lattices beyond 16 x 16 (L = 18, 20, 24, 28, 32) and honeycomb lattices beyond 16 x 16 cells (L = 18, 20, 21, 24): the
    Chebyshev recursion with a PX x PY patch of sites (cells) per lane (csrc/pgrid.hip) against the generic kernel's recursion through LDS (ELPH_NO_PG=1) — the same series, factored colours: P^-1 r to
    1e-12, and the preconditioned solves agree in iteration count and solution."""
    from elphdynamics_amd import configs, models, preconditioners as pc
    m = configs.make_model(tag, tol=1e-10)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, rng=np.random.default_rng(7))
    R, B = configs.rhs(m, 3)
    out = {}
    for name, env in (("patch", None), ("generic", "1")):
        if env is None:
            monkeypatch.delenv("ELPH_NO_PG", raising=False)
        else:
            monkeypatch.setenv("ELPH_NO_PG", env)
        z = np.zeros(m.Ndim)
        pc.kpm_ldiv_(z, P, np.ascontiguousarray(B[0]))
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B, P=P)
        assert not fl.any()
        out[name] = (z, X, it)
    assert rel(out["patch"][0], out["generic"][0]) < 1e-12
    assert np.max(np.abs(out["patch"][2] - out["generic"][2])) <= 1 and rel(out["patch"][1], out["generic"][1]) < 1e-9
    m.close()


@pytest.mark.parametrize("tag", ["k", "i", "t12", "t20", "u"])
def test_patch_matvec_kernels_on_lattices_of_the_lane_program_family(oracle, tag, monkeypatch):
    """L = 18 / 20 square and triangular lattices up to L = 22 still fit the lane-program family, which brings its own mat-vec kernels — the
    patch-layout ones (k_mul_pg, k_cg_ap_pg with 2 x 4 / 2 x 2 patches and the triangular 2 x 4) would never run on them.  With the family
    switched off (ELPH_NO_FAST=1, read when the handle is created) they do: mat-vecs, a batched solve and a preconditioned solve against
    the oracle."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    monkeypatch.setenv("ELPH_NO_FAST", "1")
    m = configs.make_model(tag, tol=1e-9)
    om = _oracle_model(oracle, m)
    v = synth.randn(5, m.Ndim)
    y = np.empty(m.Ndim)
    for fn, ofn in ((models.mulM_, oracle.mulM), (models.mulMt_, oracle.mulMT), (models.mulMtM_, oracle.mulMTM)):
        fn(y, m, v)
        assert rel(y, ofn(om, v)) < 1e-13
    R, B = configs.rhs(m, 3)
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B)
    assert not fl.any()
    for r in range(3):
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(B[r]), solver_tol=1e-9, solver_maxiter=10000)
        assert flo == 0 and abs(int(it[r]) - ito) <= 2 and rel(X[r], xo) < 1e-6
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, rng=np.random.default_rng(3))
    xk = np.zeros(m.Ndim)
    itk, resk, flk = models.ldiv_(xk, m, np.ascontiguousarray(B[0]), P=P)
    assert flk == 0 and rel(xk, X[0]) < 1e-6
    m.close()


def test_kpm_preconditioner_per_chain_generic_family(monkeypatch):
    """The same with the generic kernel family (ELPH_NO_FAST=1: lattices without a lane program) on bond phonons: every chain's Chebyshev
    recursion takes ITS τ-averaged hopping tables — the LDS copy of the bond program used chain 0's for all (found in round 5 by running the
    suite under ELPH_NO_FAST=1: 20 iterations where the chain alone needs 15)."""
    monkeypatch.setenv("ELPH_NO_FAST", "1")
    test_kpm_preconditioner_per_chain("e", 3, 2, monkeypatch)
    test_kpm_preconditioner_per_chain("E", 8, 2, monkeypatch)


@pytest.mark.parametrize("tag,nchains,per", [("b", 3, 2), ("B", 4, 2), ("C", 8, 2), ("e", 3, 2), ("E", 8, 2), ("D", 4, 2),
                                             ("G", 3, 2), ("h", 2, 2)])      # (G, h: the PGRID kernels, one expansion per chain)
def test_kpm_preconditioner_per_chain(tag, nchains, per, monkeypatch):
    """One KPM expansion per resident phonon configuration (elph_kpm_setup_chains): every right-hand side of the batch
    is preconditioned with ITS chain's Ē, eigenvalue bounds, orders and coefficients — same bounds, same iteration
    count and the same solution as the single-configuration model given the same Arnoldi start vectors."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    m = configs.make_model(tag, tol=1e-8)
    # chains with visibly different spectra: different seeds AND different roughness
    if m.kind == models.SSH:      # bond phonons: per-chain averaged hopping tables (cbar, sbar) in every Chebyshev kernel
        X = np.stack([m.x * (0.4 + 1.2 * c / nchains) * (1.0 + 0.3 * synth.randn(5100 + c, m.Ndof)) for c in range(nchains)])
    else:
        X = np.stack([(0.6 + 0.25 * c) * synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=5100 + c) for c in range(nchains)])
    nrhs = nchains * per
    B = np.stack([synth.randn(7100 + r, m.Ndim) for r in range(nrhs)])
    rng = np.random.default_rng(11)
    bmax, bmin = rng.standard_normal((nchains, m.Nsites)), rng.standard_normal((nchains, m.Nsites))
    models.update_model_chains_(m, X)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    # (one and two chains take their Arnoldi bounds on the host, three and more on the device, kpm_dev.hip: pin the device kernel so
    #  that a chain of the batch and the same configuration alone go through the same arithmetic)
    monkeypatch.setenv("ELPH_KPM_DEVICE", "1")
    # the single-chain entry point refuses while several configurations are resident
    with pytest.raises(Exception):
        pc.setup_(P, b_max=bmax[0], b_min=bmin[0])
    act, lo, hi = pc.setup_chains_(P, b_max=bmax, b_min=bmin)
    assert act.all() and len(set(np.round(hi, 6))) > 1          # the chains really have different bounds
    Xs = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
    assert not fl.any() and (res < 1e-7).all()
    plain = np.zeros_like(B)
    it0, _, fl0 = models.ldiv_batched_(plain, m, B)
    assert not fl0.any() and (it < it0).all()                    # and they precondition: far fewer iterations
    for r in range(nrhs) if nrhs <= 8 else (0, 1, nchains, nrhs - 1):
        c = r % nchains
        m1 = configs.make_model(tag, tol=1e-8)
        m1.x[:] = X[c]
        models.update_model_(m1)
        P1 = pc.SymmetricKPMPreconditioner(m1, 20, 0.05, 1.0, 1.0)
        pc.setup_(P1, b_max=bmax[c], b_min=bmin[c])
        assert P1.lam_lo == lo[c] and P1.lam_hi == hi[c]
        x1 = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x1, m1, np.ascontiguousarray(B[r]), P=P1)
        assert fl1 == 0 and abs(it1 - it[r]) <= 1
        assert rel(x1, Xs[r]) < 1e-6 and rel(plain[r], Xs[r]) < 1e-6
        m1.close()
    # injected bounds, one chain made inactive (e_max - e_min >= 2 fails the test of KPMPreconditioners.jl:280):
    # that chain is preconditioned with the identity, the others keep their expansions
    emin, emax = np.full(nchains, 0.5), np.full(nchains, 1.8)
    emax[1] = 2.6
    act, lo2, hi2 = pc.setup_chains_(P, e_min=emin, e_max=emax)
    assert act.tolist() == [1, 0] + [1] * (nchains - 2)
    Xi = np.zeros_like(B)
    it2, res2, fl2 = models.ldiv_batched_(Xi, m, B, P=P)
    assert not fl2.any()
    assert abs(int(it2[1]) - int(it0[1])) <= 2                   # identity-preconditioned == plain CG
    assert rel(Xi, plain) < 1e-6
    # back to one configuration: the per-chain expansions are dropped, the single-chain set-up works again
    models.update_model_(m)
    with pytest.raises(Exception):
        models.ldiv_(np.zeros(m.Ndim), m, np.ascontiguousarray(B[0]), P=P)
    pc.setup_(P, rng=np.random.default_rng(5))
    x = np.zeros(m.Ndim)
    itx, _, flx = models.ldiv_(x, m, np.ascontiguousarray(B[0]), P=P)
    assert flx == 0
    m.close()


# ------------------------------------------------------------------------------------------ SSH update_model! on the device

def test_ssh_update_model_on_device_matches_golden(lib):
    """elph_update_model_ssh_fields (SSHModels.jl:510-562 computed on the GPU: cosh/sinh of t' per (tau, bond), exp(dtau mu))
    against the golden tables and against the host-table entry point — both kernel families see the same matrix."""
    from elphdynamics_amd import _lib
    g = golden("ssh_sq4_L8.npz")
    N, L = int(g["N"]), int(g["Ltau"])
    nb = g["table"].shape[0]
    nph = g["phonon_to_bond"].shape[0]
    cbperm = g["cbperm"]
    cb_index = np.ascontiguousarray(cbperm[g["phonon_to_bond"] - 1], dtype=np.int64)
    t_ph = np.ascontiguousarray(g["t"][g["phonon_to_bond"] - 1])
    t_cb = np.zeros(nb)
    t_cb[cbperm - 1] = g["t"]
    mu, dtau = np.ascontiguousarray(g["mu"]), float(g["dtau"])
    m = RawModel(lib, 1, N, L, g["table"])
    try:
        _lib.check(lib.elph_update_model_ssh_fields(m.h, _lib.dptr(np.ascontiguousarray(g["x"])), nph, _lib.iptr(cb_index),
                                                    _lib.dptr(t_ph), _lib.dptr(np.ascontiguousarray(g["alpha"])),
                                                    _lib.dptr(np.ascontiguousarray(g["alpha2"])), _lib.dptr(t_cb), _lib.dptr(mu), dtau))
        c, s = np.zeros(nb * L), np.zeros(nb * L)
        _lib.check(lib.elph_get_cosh_sinh(m.h, _lib.dptr(c), _lib.dptr(s)))
        assert rel(c, g["cosht"]) < 1e-15 and rel(s, g["sinht"]) < 1e-14        # libm vs device cosh/sinh: last-bit differences
        for name in ("Mv", "MTv", "MTMv"):
            op = {"Mv": "elph_mulM", "MTv": "elph_mulMT", "MTMv": "elph_mulMTM"}[name]
            assert rel(m.op(op, g["v"]), g[name]) < 1e-13
        x, it, res, flag = m.ldiv(g["b"], 1e-13, 5000)
        assert flag == 0 and rel(x, g["xsol"]) < 1e-10
        # the KPM set-up reads its tau-averaged cosh/sinh from the device tables now
        _lib.check(lib.elph_kpm_create(m.h, 8, 0.05, 1.0, 1.0))
        rng = np.random.default_rng(0)
        act = C.c_int()
        _lib.check(lib.elph_kpm_setup(m.h, _lib.dptr(rng.standard_normal(N)), _lib.dptr(rng.standard_normal(N)), float("nan"),
                                      float("nan"), C.byref(act), None, None))
        xk, itk, resk, flagk = m.ldiv(g["b"], 1e-13, 5000, use_prec=1)
        assert flagk == 0 and rel(xk, g["xsol"]) < 1e-10
        # bad checkerboard position
        bad = cb_index.copy(); bad[0] = nb + 1
        assert lib.elph_update_model_ssh_fields(m.h, _lib.dptr(np.ascontiguousarray(g["x"])), nph, _lib.iptr(bad), _lib.dptr(t_ph),
                                                _lib.dptr(np.ascontiguousarray(g["alpha"])), _lib.dptr(np.ascontiguousarray(g["alpha2"])),
                                                _lib.dptr(t_cb), _lib.dptr(mu), dtau) == _lib.ELPH_E_ARG
    finally:
        m.close()


@pytest.mark.parametrize("no_fast", ["0", "1"])
def test_ssh_device_update_equals_host_tables_at_config_E(no_fast, monkeypatch):
    """Config E (OSSH square L=16, Ltau=160, alpha2 = 0.02 switched on): the model built by the device-side update_model!
    applies the same operator as one fed with numpy cosh/sinh tables through elph_update_model_ssh — lane-program (fast)
    and generic kernels."""
    monkeypatch.setenv("ELPH_NO_FAST", no_fast)
    from elphdynamics_amd import _lib, configs, models
    m = configs.make_model("E")
    m.alpha2[:] = 0.02
    models.update_model_(m)                                    # device path
    v = np.cos(0.3 * np.arange(m.Ndim))
    y_dev = np.zeros(m.Ndim)
    models.mulMtM_(y_dev, m, v)
    X = m.x.reshape(m.Nph, m.Ltau)
    tp = m.t[m.phonon_to_bond - 1][:, None] - (m.alpha[:, None] * X + np.sign(X) * m.alpha2[:, None] * X ** 2)
    idx = m.checkerboard_perm[m.phonon_to_bond - 1] - 1
    c = np.tile(np.cosh(m.dtau * m.t_bare_cb)[:, None], (1, m.Ltau))
    s = np.tile(np.sinh(m.dtau * m.t_bare_cb)[:, None], (1, m.Ltau))
    c[idx, :], s[idx, :] = np.cosh(m.dtau * tp), np.sinh(m.dtau * tp)
    assert rel(m.cosht, c) < 1e-15 and rel(m.sinht, s) < 1e-14            # lazily fetched from the device
    _lib.check(m._lib.elph_update_model_ssh(m._h, _lib.dptr(np.ascontiguousarray(c).reshape(-1)),
                                            _lib.dptr(np.ascontiguousarray(s).reshape(-1)), _lib.dptr(np.exp(m.dtau * m.mu))))
    y_host = np.zeros(m.Ndim)
    models.mulMtM_(y_host, m, v)
    assert rel(y_dev, y_host) < 1e-13
    m.close()


# ------------------------------------------------------------------------------------------ odd shapes

@pytest.mark.parametrize("norb,L1,L2,bonds,Ltau", [
    (1, 2, 1, [(1, 1, (1, 0, 0))], 1),        # two sites, one bond, ONE time slice (tau-1 wraps onto tau)
    (1, 2, 1, [(1, 1, (1, 0, 0))], 2),
    (1, 5, 1, [(1, 1, (1, 0, 0))], 3),        # odd ring: three ragged colours
    (1, 3, 3, "tri", 7),                      # 9 colours (generic kernels), prime Ltau
    (2, 2, 2, "hc", 5),                       # honeycomb 2x2: wrap bonds coincide
    (1, 6, 4, "sq", 161),                     # Ltau not divisible by 2, 4 or 8: no chunk kernel
    (1, 10, 10, "sq", 12),                    # N = 100: ragged last lane group
])
def test_odd_lattices_and_time_extents_vs_oracle(oracle, norb, L1, L2, bonds, Ltau):
    """Shapes the decks never use but the kernels must not trip over: a single time slice, odd rings, prime Ltau, ragged
    site counts — mat-vecs, a batched solve of 3 right-hand sides and the KPM-preconditioned solve against the oracle."""
    from elphdynamics_amd import lattice as lat
    from elphdynamics_amd import models, preconditioners as pc, synth
    if isinstance(bonds, str):
        bonds = {"tri": lat.TRIANGULAR_BONDS, "hc": lat.HONEYCOMB_BONDS, "sq": lat.SQUARE_BONDS}[bonds]
    la = lat.Lattice(norb, L1, L2, 1)
    dtau = 0.1
    m = models.HolsteinModel(la, Ltau * dtau, dtau, tol=1e-9, maxiter=20000)
    assert m.Ltau == Ltau
    for (o1, o2, d) in bonds:
        m.assign_t_(1.0, o1, o2, d)
    m.assign_omega_(1.0); m.assign_lambda_(1.0); m.assign_mu_(0.1)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, Ltau, Ltau * dtau, dtau, seed=4242)
    models.update_model_(m)
    om = _oracle_model(oracle, m)
    v = synth.randn(1, m.Ndim)
    for f_gpu, f_orc in ((models.mulM_, oracle.mulM), (models.mulMt_, oracle.mulMT), (models.mulMtM_, oracle.mulMTM)):
        y = np.zeros(m.Ndim)
        f_gpu(y, m, v)
        assert rel(y, f_orc(om, v)) < 1e-13
    B = np.stack([oracle.mulMT(om, synth.randn(10 + r, m.Ndim)) for r in range(3)])
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B)
    assert not fl.any()
    for r in range(3):
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(B[r]), solver_tol=1e-9, solver_maxiter=20000)
        assert flo == 0 and abs(int(it[r]) - ito) <= 2 and rel(X[r], xo) < 1e-6
    P = pc.SymmetricKPMPreconditioner(m, n=min(20, m.Nsites), buf=0.05, c1=1.0, c2=1.0)
    pc.setup_(P, rng=np.random.default_rng(2))
    xk = np.zeros(m.Ndim)
    itk, resk, flk = models.ldiv_(xk, m, np.ascontiguousarray(B[0]), P=P)
    assert flk == 0 and rel(xk, X[0]) < 1e-6
    m.close()


@pytest.mark.parametrize("L", [10, 18, 50, 90, 150, 200, 256, 320, 400])
def test_mfma_dft_long_time_axes(lib, L, monkeypatch):
    """The split GEMM form of the twisted transform on time axes with L = 2 (mod 4) (odd half length: the middle frequency is
    its own mirror) and on long ones (W panel of 64 ... 128 KB in LDS, several row groups for L > 320): against numpy's FFT of the twisted sequence (TimeFreqFFTs.jl:55-73,112-130) and against the scalar kernels."""
    from elphdynamics_amd import _lib
    N = 37
    m = RawModel(lib, 0, N, L, np.zeros((0, 2), dtype=np.int64))
    try:
        v = np.random.default_rng(L).standard_normal(N * L)
        V = v.reshape(N, L)
        ref = np.fft.fft(V * np.exp(-1j * np.pi * np.arange(L) / L)[None, :], axis=1)            # nu[site, omega]
        res = {}
        for mode in ("0", "1"):
            monkeypatch.setenv("ELPH_DFT_MFMA", mode)
            nu = np.zeros(2 * N * L)
            _lib.check(lib.elph_tau_to_omega(m.h, _lib.dptr(nu), _lib.dptr(v)))
            back = np.zeros(N * L)
            _lib.check(lib.elph_omega_to_tau(m.h, _lib.dptr(back), _lib.dptr(nu)))
            z = (nu[0::2] + 1j * nu[1::2]).reshape(N, L)
            assert np.abs(z - ref).max() < 1e-12 * np.abs(ref).max(), mode
            assert rel(back, v) < 1e-13, mode
            res[mode] = nu
        assert rel(res["1"], res["0"]) < 1e-13
    finally:
        m.close()


def _px_fused(m):
    from elphdynamics_amd import _lib
    f = C.c_int()
    _lib.check(_lib.load().elph_bench_px_info(m._h, C.byref(f)))
    return bool(f.value)


@pytest.mark.parametrize("tag,nchains,per,chunk_T", [("C", 16, 2, None), ("C", 1, 48, None), ("C", 64, 2, None), ("C", 144, 2, None), ("C", 20, 2, "5"),
                                                      ("D", 16, 2, None), ("D", 64, 2, None), ("B", 64, 2, None), ("S", 32, 2, None),
                                                      ("E", 16, 2, None), ("E", 64, 2, None), ("E", 1, 48, None)])      # bond phonons (BASELINE config 5)
def test_px_fused_preconditioned_iteration_equals_the_unfused_one(tag, nchains, per, chunk_T, monkeypatch):
    """The batched KPM-preconditioned iteration with x += alpha p and p = P^-1 r + beta p moved into the epilogue of the inverse
    tau-transform (dft_mfma.hip: PxFuse; k_cg_ap_chunk<PX> reads the ready p): same arithmetic per element and the same summation
    order for r.z as the unfused form, so iteration counts are EQUAL and the solutions agree to round-off of the last bit
    (IterativeSolvers.jl:153-234 — the recurrences are untouched, only where they are evaluated moves)."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    if chunk_T:
        monkeypatch.setenv("ELPH_CHUNK_T", chunk_T)
    # (the statement is about WHERE the p- and x-update are evaluated: both forms with the lane-program k_cg_ap — the register-exchange k_cg_ap of
    #  the 16 x 16 lattice rounds differently and has its own test below)
    monkeypatch.setenv("ELPH_SQ16_AP", "0")
    m = configs.make_model(tag, tol=1e-8)
    nrhs = nchains * per
    if nchains > 1 and m.kind == models.SSH:      # bond phonons: the deck's field rescaled and roughened per chain (|alpha x| stays below t)
        X = np.stack([m.x * (0.55 + 0.9 * c / nchains) * (1.0 + 0.2 * synth.randn(8000 + c, m.Ndof)) for c in range(nchains)])
        models.update_model_chains_(m, X)
    elif nchains > 1:
        X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=8000 + c) for c in range(nchains)])
        models.update_model_chains_(m, X)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    (pc.setup_chains_ if nchains > 1 else pc.setup_)(P, rng=np.random.default_rng(11))
    B = np.stack([synth.randn(8100 + r, m.Ndim) for r in range(nrhs)])
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ELPH_FUSE_PX", mode)
        Xs = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
        assert not fl.any()
        out[mode] = (Xs, it, _px_fused(m))
    assert out["0"][2] is False and out["1"][2] is True, "the fused form was not taken: the A/B compares a kernel with itself"
    assert np.array_equal(out["0"][1], out["1"][1])
    assert rel(out["1"][0], out["0"][0]) < 1e-13
    m.close()


@pytest.mark.parametrize("nchains,per,chunk_T", [(16, 2, None), (64, 2, None), (128, 2, None), (20, 2, "5"), (24, 2, "20")])
def test_register_exchange_k_cg_ap_honeycomb12(nchains, per, chunk_T, monkeypatch):
    """cg_sq16.hip: k_cg_ap_hc12_px — the p/x-fused k_cg_ap of BASELINE config D (honeycomb 12 x 12 cells, uniform hopping) with the checkerboard in
    registers (the QUAD layout of the Chebyshev recursion: six consecutive sites per lane on 48 lanes, DPP quad rotations + one ds_bpermute round trip
    per sweep) against the lane-program kernel it stands in front of (ELPH_SQ16_AP=0): iteration counts within one, solutions of two tol = 1e-8
    solves to 1e-9, the post-solve residual."""
    from elphdynamics_amd import _lib, configs, models, preconditioners as pc, synth
    if chunk_T:
        monkeypatch.setenv("ELPH_CHUNK_T", chunk_T)
    m = configs.make_model("D", tol=1e-8)
    nrhs = nchains * per
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=9300 + c) for c in range(nchains)])
    models.update_model_chains_(m, X)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_chains_(P, rng=np.random.default_rng(17))
    B = np.stack([synth.randn(9400 + r, m.Ndim) for r in range(nrhs)])
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ELPH_SQ16_AP", mode)
        Xs = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
        assert not fl.any() and (res < 1e-6).all()
        f = C.c_int()
        _lib.check(_lib.load().elph_bench_px_info(m._h, C.byref(f)))
        out[mode] = (Xs, it, f.value)
    assert out["0"][2] == 1 and out["1"][2] == 2, f"forms taken: {out['0'][2]}, {out['1'][2]} (1 = lane program, 2 = registers)"
    assert np.abs(out["0"][1] - out["1"][1]).max() <= 1
    assert rel(out["1"][0], out["0"][0]) < 1e-9
    m.close()


@pytest.mark.parametrize("tag,nchains,per", [("K", 8, 2), ("K", 1, 24), ("X32", 4, 2), ("k40", 32, 2), ("k", 12, 2), ("j", 8, 2),
                                             ("X24", 4, 2), ("XT24", 8, 2), ("L36", 4, 2), ("T", 32, 2), ("G40", 4, 2), ("L26", 8, 2), ("L40", 4, 2), ("H27", 4, 2)])      # honeycomb 24 x 24 cells, triangular 24 x 24: the same pipeline around their patch sweeps
def test_px_fused_iteration_on_patch_form_lattices(oracle, tag, nchains, per, monkeypatch):
    """Round 6: the p/x-fused preconditioned batch iteration on the patch-form lattices of the generic family (square L = 18 … 32: `k_cg_ap_pg<PX>`
    reads the ready p, the residual update rides on the forward transform, r.z comes from `k_kpm_cheb_pg` in frequency space, the p/x-update is
    the inverse transform's epilogue) against the unfused form (ELPH_PG_PX=0: `k_cg_xr`, time-domain r.z): the same recurrences
    (IterativeSolvers.jl:153-234), another summation of r.z — iteration counts within one, solutions of two tol = 1e-8 solves to 1e-9 — and,
    where the time axis admits the fused form, the form must actually be taken.  One right-hand side of K also against the oracle's own
    preconditioned solve."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    m = configs.make_model(tag, tol=1e-8)
    nrhs = nchains * per
    if nchains > 1:
        X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=8800 + c) for c in range(nchains)])
        models.update_model_chains_(m, X)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    (pc.setup_chains_ if nchains > 1 else pc.setup_)(P, rng=np.random.default_rng(15))
    B = np.stack([synth.randn(8900 + r, m.Ndim) for r in range(nrhs)])
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ELPH_PG_PX", mode)
        Xs = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
        assert not fl.any()
        out[mode] = (Xs, it, _px_fused(m))
    assert out["0"][2] is False
    # the fused form needs the MFMA transforms with the residual update (N / 16 column tiles <= Ltau, enough waves): K (24 x 24, Ltau = 40), X32 and k40 (20 x 20, Ltau = 40: lane-program family, patch-form Chebyshev) have it
    if tag in ("K", "X32", "k40", "X24", "XT24", "L36", "T", "G40", "L26", "L40", "H27"):      # (T: triangular 16 x 16 — a six-colour lane program riding on the patch-form pair)
        assert out["1"][2] is True, "the p/x-fused form was not taken on a lattice that admits it"
    assert np.abs(out["0"][1] - out["1"][1]).max() <= 1
    assert rel(out["1"][0], out["0"][0]) < 1e-9
    if tag == "K" and nchains == 1:
        om = _oracle_model(oracle, m)
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(B[0]), solver_tol=1e-12, solver_maxiter=20000)
        assert flo == 0 and rel(out["1"][0][0], xo) < 1e-6            # (a tol = 1e-8 solve against a tight one)
    m.close()


@pytest.mark.parametrize("tag,nchains,per,no_fast,disorder", [("C", 32, 2, True, 0.0), ("E", 32, 2, True, 0.0), ("l22", 32, 2, False, 0.0), ("l22", 1, 64, False, 0.0),
                                                              ("l26", 8, 2, False, 0.0), ("K", 8, 2, False, 0.1), ("D", 16, 2, True, 0.0)])
def test_px_fused_iteration_generic_family(oracle, tag, nchains, per, no_fast, disorder, monkeypatch):
    """Round 6: the p/x-fused preconditioned batch iteration for the lattices that run the GENERIC LDS kernels — no lane program, no patch form:
    square L = 22, 26 (2 x 11, 2 x 13: no even patch fits a wavefront), hopping disorder on a lattice beyond 16 x 16 (K with a disordered
    hopping table), and, forced with ELPH_NO_FAST=1, the generic kernels on configs C, D and E (bond phonons) — `k_cg_ap<PX>` reads the ready
    p, `k_kpm_cheb` delivers r.z in frequency space, the transforms carry the residual and the p/x-update — against the unfused form
    (ELPH_GEN_PX=0): iteration counts within one, solutions of two tol = 1e-8 solves to 1e-9, the fused form asserted taken; one right-hand
    side of l22 against the oracle (IterativeSolvers.jl:153-234)."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    if no_fast:
        monkeypatch.setenv("ELPH_NO_FAST", "1")
    monkeypatch.setenv("ELPH_PG_MW", "0")      # (l22, l26 have multi-wavefront patch kernels since later in round 6: this test is about the LDS kernels)
    monkeypatch.setenv("ELPH_PG_DIS", "0")     # (... and a disordered 24 x 24 lattice the table variant of the patch kernels)
    m = configs.make_model(tag, tol=1e-8, t_stddev=disorder)
    nrhs = nchains * per
    if nchains > 1 and m.kind == models.SSH:
        X = np.stack([m.x * (0.55 + 0.9 * c / nchains) * (1.0 + 0.2 * synth.randn(9000 + c, m.Ndof)) for c in range(nchains)])
        models.update_model_chains_(m, X)
    elif nchains > 1:
        X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=9000 + c) for c in range(nchains)])
        models.update_model_chains_(m, X)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    (pc.setup_chains_ if nchains > 1 else pc.setup_)(P, rng=np.random.default_rng(16))
    B = np.stack([synth.randn(9100 + r, m.Ndim) for r in range(nrhs)])
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ELPH_GEN_PX", mode)
        monkeypatch.setenv("ELPH_LDS_CHEB_PX", mode)             # (l22 is a lane-program lattice whose recursion runs through the LDS slab: k_kpm_cheb_ri)
        Xs = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
        assert not fl.any()
        out[mode] = (Xs, it, _px_fused(m))
    assert out["0"][2] is False and out["1"][2] is True, (out["0"][2], out["1"][2])
    assert np.abs(out["0"][1] - out["1"][1]).max() <= 1
    assert rel(out["1"][0], out["0"][0]) < 1e-9
    if tag == "l22" and nchains == 1:
        om = _oracle_model(oracle, m)
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(B[0]), solver_tol=1e-12, solver_maxiter=20000)
        assert flo == 0 and rel(out["1"][0][0], xo) < 1e-6
    m.close()


@pytest.mark.parametrize("nchains,per,chunk_T,disorder", [(16, 2, None, 0.0), (1, 48, None, 0.0), (64, 2, None, 0.0), (144, 2, None, 0.0), (20, 2, "5", 0.0), (24, 2, "2", 0.0),
                                                          (24, 2, "20", 0.0), (16, 2, None, 0.1), (64, 2, "8", 0.1)])
def test_register_exchange_k_cg_ap_of_the_fused_iteration(nchains, per, chunk_T, disorder, monkeypatch):
    """cg_sq16.hip: the p/x-fused k_cg_ap of the 16 x 16 square lattice (BASELINE config C) with the checkerboard in registers (2 x 2 patch per
    lane, DPP rotations + one ds_bpermute pair, uniform hopping as c^4 prod (I + th P)) against the lane-program kernel it stands in front of
    (ELPH_SQ16_AP=0): same recurrences (HolsteinModels.jl:569-684, IterativeSolvers.jl:153-234), rounding differs — iteration counts within
    one, solutions of two tol = 1e-8 solves to 1e-9 — and against the oracle's preconditioned solve on sampled right-hand sides (1e-7: two
    solves stopped at 1e-8).  disorder > 0: hopping disorder, i.e. the per-site (cosh, sinh) variant of the kernel."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    if chunk_T:
        monkeypatch.setenv("ELPH_CHUNK_T", chunk_T)
    m = configs.make_model("C", tol=1e-8, t_stddev=disorder)
    nrhs = nchains * per
    if nchains > 1:
        X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=8600 + c) for c in range(nchains)])
        models.update_model_chains_(m, X)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    (pc.setup_chains_ if nchains > 1 else pc.setup_)(P, rng=np.random.default_rng(13))
    B = np.stack([synth.randn(8700 + r, m.Ndim) for r in range(nrhs)])
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ELPH_SQ16_AP", mode)
        Xs = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
        assert not fl.any()
        f = C.c_int()
        from elphdynamics_amd import _lib
        _lib.check(_lib.load().elph_bench_px_info(m._h, C.byref(f)))
        out[mode] = (Xs, it, f.value)
    assert out["0"][2] == 1 and out["1"][2] == 2, f"forms taken: {out['0'][2]}, {out['1'][2]} (1 = lane program, 2 = registers)"
    assert np.abs(out["0"][1] - out["1"][1]).max() <= 1
    assert rel(out["1"][0], out["0"][0]) < 1e-9
    # the post-solve residual of every right-hand side, computed by the un-fused mat-vec: |MtM x - b| / |b| <= a few tol
    for r in range(0, nrhs, max(1, nrhs // 6)):
        if nchains > 1:
            continue                     # (chains: models.mulMtM_ applies chain 0's matrix)
        y = np.empty(m.Ndim)
        models.mulMtM_(y, m, np.ascontiguousarray(out["1"][0][r]))
        assert np.linalg.norm(y - B[r]) / np.linalg.norm(B[r]) < 5e-8
    m.close()


@pytest.mark.parametrize("tag,nchains,per,chunk_T", [("C", 32, 2, "4"), ("C", 64, 2, None), ("C", 144, 2, None), ("C", 1, 64, "4"), ("D", 64, 2, "4")])
def test_preconditioned_batch_as_two_half_batches_on_two_streams(tag, nchains, per, chunk_T, monkeypatch):
    """elph_ldiv_batched of a large KPM-preconditioned batch runs as two half-batches on two streams (cg_solve.hip: SplitRun; default
    from 192 right-hand sides, forced here): every right-hand side goes through the same kernels with the same partial-sum layout as in
    one stream.  With the chunk length pinned (ELPH_CHUNK_T) the two forms give the SAME BITS; with the library's own choice the
    halves may take another chunk length than the whole batch (another grouping of the p.z partial sums): iteration counts within
    one, solutions to 1e-9 of two tol = 1e-8 solves."""
    from elphdynamics_amd import configs, models, preconditioners as pc, synth
    if chunk_T:
        monkeypatch.setenv("ELPH_CHUNK_T", chunk_T)
    m = configs.make_model(tag, tol=1e-8)
    nrhs = nchains * per
    if nchains > 1:
        X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=8300 + c) for c in range(nchains)])
        models.update_model_chains_(m, X)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    (pc.setup_chains_ if nchains > 1 else pc.setup_)(P, rng=np.random.default_rng(12))
    B = np.stack([synth.randn(8400 + r, m.Ndim) for r in range(nrhs)])
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ELPH_SPLIT_STREAMS", mode)
        Xs = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
        assert not fl.any() and _px_fused(m)
        out[mode] = (Xs, it)
    if chunk_T:
        assert np.array_equal(out["0"][1], out["1"][1]) and np.array_equal(out["0"][0], out["1"][0])
    else:
        assert np.abs(out["0"][1] - out["1"][1]).max() <= 1 and rel(out["1"][0], out["0"][0]) < 1e-9
    # the solve after a split one is an ordinary one again (the view and its stream are gone with the solve)
    monkeypatch.setenv("ELPH_SPLIT_STREAMS", "0")
    x1 = np.zeros(m.Ndim)
    it1, _, fl1 = models.ldiv_(x1, m, np.ascontiguousarray(B[0]), P=P)
    assert fl1 == 0 and abs(it1 - int(out["0"][1][0])) <= 1 and rel(x1, out["0"][0][0]) < 1e-9
    m.close()


@pytest.mark.parametrize("Lt", [30, 50, 400])
def test_batched_preconditioned_solve_with_odd_half_length(Lt, monkeypatch):
    """Ltau = 2 (mod 4): the split transforms (odd half length), the folded residual update and the frequency-space r.z inside a
    batched KPM-preconditioned solve — same iteration counts and solutions as the scalar-kernel path, and as the oracle.
    Ltau = 400: the long-axis form (three row groups, 128 KB W panel in LDS, residual update NOT folded)."""
    from elphdynamics_amd import lattice as lat, models, preconditioners as pc, synth
    from oracle.oracle import Oracle
    la = lat.Lattice(1, 8, 8, 1)
    m = models.HolsteinModel(la, Lt * 0.1, 0.1, tol=1e-8, maxiter=20000)
    for (o1, o2, d) in lat.SQUARE_BONDS:
        m.assign_t_(1.0, o1, o2, d)
    m.assign_omega_(1.0), m.assign_lambda_(1.0), m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau)
    models.update_model_(m)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    bmax, bmin = synth.randn(1, m.Nsites), synth.randn(2, m.Nsites)
    pc.setup_(P, b_max=bmax, b_min=bmin)
    B = np.stack([synth.randn(300 + r, m.Ndim) for r in range(24)])
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ELPH_DFT_MFMA", mode)
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B, P=P)
        assert not fl.any()
        out[mode] = (X, it)
    if Lt <= 100:
        assert np.array_equal(out["0"][1], out["1"][1]) and rel(out["1"][0], out["0"][0]) < 1e-10
    else:      # beta = 40: > 100 iterations even preconditioned — round-off moves the crossing of the tolerance by an iteration or two
        assert np.abs(out["0"][1] - out["1"][1]).max() <= 3 and rel(out["1"][0], out["0"][0]) < 1e-6
    orc = Oracle()
    E = orc.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
    om = orc.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)
    Po = orc.make_kpm(om, n=20)
    orc.kpm_setup(Po, b_max=bmax, b_min=bmin)
    xo, ito, reso, flo = orc.ldiv(om, B[0], P=Po, solver_tol=1e-8, solver_maxiter=20000)
    assert flo == 0 and abs(int(out["1"][1][0]) - ito) <= (1 if Lt <= 100 else 3) and rel(out["1"][0][0], xo) < 1e-6
    m.close()


def test_lattice_beyond_the_register_resident_family(oracle):
    """N = 576 sites (square L = 24, > 512): the generic LDS-slab kernels with one thread per two sites and the Chebyshev kernel
    with its bond program in LDS — mat-vec, plain and KPM-preconditioned solves (single and batched) against the oracle."""
    from elphdynamics_amd import lattice as lat, models, preconditioners as pc, synth
    la = lat.Lattice(1, 24, 24, 1)
    m = models.HolsteinModel(la, 24 * 0.1, 0.1, tol=1e-8, maxiter=20000)
    for (o1, o2, d) in lat.SQUARE_BONDS:
        m.assign_t_(1.0, o1, o2, d)
    m.assign_omega_(1.0), m.assign_lambda_(1.0), m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau)
    models.update_model_(m)
    E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
    om = oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)
    v = synth.randn(5, m.Ndim)
    y = np.zeros(m.Ndim)
    models.mulMtM_(y, m, v)
    assert rel(y, oracle.mulMTM(om, v)) < 1e-13
    b = np.zeros(m.Ndim)
    models.mulMt_(b, m, v)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    bmax, bmin = synth.randn(1, m.Nsites), synth.randn(2, m.Nsites)
    pc.setup_(P, b_max=bmax, b_min=bmin)
    x = np.zeros(m.Ndim)
    it, res, fl = models.ldiv_(x, m, b, P=P)
    Po = oracle.make_kpm(om, n=20)
    oracle.kpm_setup(Po, b_max=bmax, b_min=bmin)
    xo, ito, reso, flo = oracle.ldiv(om, b, P=Po, solver_tol=1e-8, solver_maxiter=20000)
    assert fl == 0 and flo == 0 and abs(it - ito) <= 1 and rel(x, xo) < 1e-6
    Mx = np.zeros(m.Ndim)
    models.mulM_(Mx, m, x)
    assert rel(Mx, v) < 1e-6                                   # b = Mᵀv, so x = M⁻¹v
    x2 = np.zeros(m.Ndim)
    it2, res2, fl2 = models.ldiv_(x2, m, b)
    assert fl2 == 0 and it2 > 5 * it and rel(x2, x) < 1e-5
    B = np.stack([b, 2 * b, synth.randn(6, m.Ndim)])
    X = np.zeros_like(B)
    itb, resb, flb = models.ldiv_batched_(X, m, B, P=P)
    assert not flb.any() and rel(X[0], x) < 1e-10 and rel(X[1], 2 * x) < 1e-6
    m.close()


def test_lds_sync_build_is_bit_identical():
    """The lane-program kernels order their wave-private LDS traffic with a COMPILER barrier only (cg_fast_common.h:
    WAVE_LDS_ORDER); libelphgpu_ldssync.so is the same code with a real s_waitcnt + s_barrier per colour.  Identical bits
    from both builds on configs C, D, E (4-colour lane programs, 4 and 5 sites per lane, SSH tables) and on a triangular
    lattice (6-colour program) — a compiler that reordered the slab accesses would show up here."""
    import json
    import os
    import subprocess
    import sys
    from elphdynamics_amd import build as ebuild
    assert os.path.exists(ebuild.LIB_LDSSYNC), "libelphgpu_ldssync.so missing: __graft_entry__.build() makes it"
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lds_sync_worker.py")
    tags = ["C", "D", "E", "u"]
    outs = []
    for lib in (ebuild.LIB, ebuild.LIB_LDSSYNC):
        env = dict(os.environ, ELPH_LIB=lib)
        r = subprocess.run([sys.executable, worker, *tags], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0]["lib"] == "libelphgpu.so" and outs[1]["lib"] == "libelphgpu_ldssync.so"
    for tag in tags:
        assert outs[0][tag] == outs[1][tag], (tag, outs[0][tag], outs[1][tag])


# ------------------------------------------------------------------------------------------ workgroup-resident CG (cg_wg.hip)

def _wg_status(m):
    """(solves left on the streaming iteration after a resident launch gave up, launches given up so far)"""
    from elphdynamics_amd import _lib
    cd, fb = C.c_int(), C.c_int64()
    _lib.check(_lib.load().elph_wg_status(m._h, C.byref(cd), C.byref(fb)))
    return cd.value, fb.value


def _wg_info(m, nrhs=1):
    from elphdynamics_amd import _lib
    us, T, W, G = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().elph_bench_wg_info(m._h, nrhs, C.byref(us), C.byref(T), C.byref(W), C.byref(G)))
    return us.value, T.value, W.value, G.value


def _wg_resident_vs_streaming(m, B, variants, monkeypatch, tag):
    """The comparison of test_wg_resident_cg_equals_the_two_kernel_iteration on a model and a batch of right-hand sides: every
    variant (environment switches of the resident kernel) against the streaming iteration (ELPH_NO_WG=1) at 1e-5 and at 1e-13."""
    from elphdynamics_amd import models

    def solve(env, tol):
        for k in ("ELPH_NO_WG", "ELPH_WG_T", "ELPH_WG_NO_DPP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m.solver.tol = tol
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B)
        assert not fl.any()
        return X, it

    Xs, its = solve({"ELPH_NO_WG": "1"}, 1e-5)
    for env in variants:
        Xw, itw = solve(env, 1e-5)
        # (another summation tree: the stop test crosses the tolerance within a step — within a few steps where the residual curve is
        #  flat at the end of a solve of several hundred iterations)
        assert np.max(np.abs(itw - its)) <= max(1, int(its.max()) // 150), (tag, env, itw, its)
        assert rel(Xw, Xs) < 5e-5, (tag, env)
    Xs13, _ = solve({"ELPH_NO_WG": "1"}, 1e-13)
    for env in variants:
        Xw13, _ = solve(env, 1e-13)
        assert rel(Xw13, Xs13) < 1e-11, (tag, env, rel(Xw13, Xs13))


@pytest.mark.parametrize("tag", ["b", "d", "e", "B", "C", "D", "E", "s", "q", "Q", "S", "y", "z", "Y", "r", "R", "w", "W", "u", "T", "t6", "t12"])
def test_wg_resident_cg_equals_the_two_kernel_iteration(tag, monkeypatch):
    """The whole solve in one launch (Krylov vectors in registers / LDS, teams of workgroups meeting through L2) against the
    streaming two-kernel iteration: same algorithm, different summation trees for p.z and r.r — same iteration count up to
    the knife edge, solutions equal to the solver tolerance at 1e-5 and to 1e-11 when both solve to 1e-13; both slices-per-wave
    shapes and, on the 16 x 16 square lattice, both forms of the checkerboard (DPP exchange / lane program in LDS)."""
    from elphdynamics_amd import configs
    m = configs.make_model(tag, tol=1e-5)
    usable, T, W, G = _wg_info(m)
    assert usable == 1, tag
    R, B = configs.rhs(m, 3)
    variants = [{}, {"ELPH_WG_T": "1"}, {"ELPH_WG_T": "2"}]
    if tag == "C":      # 4 slices per wave is the shape of large batches (DPP form only)
        variants += [{"ELPH_WG_T": "4"}, {"ELPH_WG_NO_DPP": "1"}, {"ELPH_WG_NO_DPP": "1", "ELPH_WG_T": "1"}]
    if tag in ("D", "E"):   # honeycomb (mirror lanes) / bond phonons (a table set per time slice): the DPP form is the default, the lane-program form the A/B
        variants += [{"ELPH_WG_NO_DPP": "1", "ELPH_WG_T": "2"}, {"ELPH_WG_NO_DPP": "1", "ELPH_WG_T": "1"}]
    if tag in ("u", "T", "t6", "t12"):   # triangular lattices: the GRID layout with two diagonal colours (FORM 7); no lane-program form to compare with
        if tag in ("T", "t12"):
            variants += [{"ELPH_WG_T": "4"}]
    if tag in ("b", "s", "q", "Q", "S", "d", "y", "z", "r", "R", "w", "W"):   # the GRID / HGRID forms (other even-L square lattices, other honeycomb lattices on a grid of lanes) and their lane-program A/B
        variants += [{"ELPH_WG_NO_DPP": "1"}, {"ELPH_WG_NO_DPP": "1", "ELPH_WG_T": "1"}]
        if tag in ("S", "Q"):          # 4 slices per wave: the shape of batches beyond one round of 2 (time axes that are multiples of 4)
            variants += [{"ELPH_WG_T": "4"}]
    if tag == "B":          # the 8 x 8 DPP form (one site per lane; default: one workgroup per right-hand side, 5 slices per wave) and its lane-program A/B
        variants += [{"ELPH_WG_T": "5"}, {"ELPH_WG_T": "8"}, {"ELPH_WG_NO_DPP": "1"}, {"ELPH_WG_NO_DPP": "1", "ELPH_WG_T": "5"}, {"ELPH_WG_NO_DPP": "1", "ELPH_WG_T": "8"}]
    _wg_resident_vs_streaming(m, B, variants, monkeypatch, tag)
    m.close()


def test_wg_resident_cg_dpp_form_with_hopping_disorder(oracle, monkeypatch):
    """Holstein on the 16 x 16 lattice with a disordered hopping table (assign_t! with stddev, HolsteinModels.jl:427-447): the DPP
    form keeps the (cosh, sinh) of each site's four bonds in registers.  Against the streaming iteration and the oracle's M."""
    from elphdynamics_amd import lattice as lat
    from elphdynamics_amd import configs, models, synth
    m = models.HolsteinModel(lat.Lattice(1, 16, 16, 1), 4.0, 0.1, tol=1e-13, maxiter=10000)
    rng = np.random.default_rng(5)
    m.assign_t_(1.0, 1, 1, (1, 0, 0), stddev=0.1, rng=rng)
    m.assign_t_(1.0, 1, 1, (0, 1, 0), stddev=0.1, rng=rng)
    m.assign_omega_(1.0); m.assign_lambda_(1.0); m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, 4.0, 0.1, omega=1.0, lam=1.0, seed=11)
    models.update_model_(m)
    usable, T, W, G = _wg_info(m)
    assert usable == 1 and T == 1 and _wg_info(m, 60)[1] == 2          # Ltau = 40: 1 slice per wave up to 48 right-hand sides, then 2 (per-site hopping: never 4)
    R, B = configs.rhs(m, 3)
    out = {}
    for name, env in (("stream", {"ELPH_NO_WG": "1"}), ("dpp2", {"ELPH_WG_T": "2"}), ("dpp1", {}), ("lds", {"ELPH_WG_NO_DPP": "1"})):
        for k in ("ELPH_NO_WG", "ELPH_WG_T", "ELPH_WG_NO_DPP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B)
        assert not fl.any(), name
        out[name] = X
    for name in ("dpp2", "dpp1", "lds"):
        assert rel(out[name], out["stream"]) < 1e-11, (name, rel(out[name], out["stream"]))
    # M x = R for the oracle's M (x solves Mt M x = Mt R)
    om = _oracle_model(oracle, m)
    for i in range(3):
        assert rel(oracle.mulM(om, out["dpp2"][i]), R[i]) < 1e-9
    m.close()


def test_wg_resident_cg_with_more_teams_than_the_chip_holds(monkeypatch):
    """40 right-hand sides of config C at 2 slices per wave (pinned: a batch this size would pick 4) = 400 workgroups for 256 CUs:
    teams at the dispatch frontier wait for their members; every solution equals the single solve of that right-hand side bit
    for bit."""
    from elphdynamics_amd import configs, models
    monkeypatch.setenv("ELPH_WG_T", "2")
    m = configs.make_model("C", tol=1e-5)
    assert _wg_info(m)[0] == 1
    nrhs = 40
    R, B = configs.rhs(m, nrhs)
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B)
    assert not fl.any() and (res < 1e-4).all()
    for i in (0, 7, 25, 26, 39):
        x = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x, m, np.ascontiguousarray(B[i]))
        assert it1 == it[i] and np.array_equal(x, X[i]), i
    m.close()


def test_wg_resident_cg_large_batch_shape():
    """A batch that 2 slices per wave cannot hold in one round (config C: more than 24 right-hand sides) runs 4 slices per wave on
    the DPP form (48 right-hand sides per round): another summation tree, the same algorithm — iteration counts within 1 of the single solves, solutions equal to the tolerance."""
    from elphdynamics_amd import configs, models
    m = configs.make_model("C", tol=1e-5)
    nrhs = 50
    assert _wg_info(m)[1] == 1 and _wg_info(m, 20)[1] == 2 and _wg_info(m, nrhs)[1] == 4
    R, B = configs.rhs(m, nrhs)
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B)
    assert not fl.any() and (res < 1e-4).all()
    for i in (0, 23, 49):
        x = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x, m, np.ascontiguousarray(B[i]))
        assert abs(it1 - it[i]) <= 1 and rel(X[i], x) < 5e-5, i
    m.close()


@pytest.mark.parametrize("dpp", [True, False])
def test_wg_resident_cg_one_workgroup_per_rhs_shape(oracle, monkeypatch, dpp):
    """Config B (8 x 8, one site per lane): the whole time axis of a right-hand side in ONE workgroup (8 waves x 5 slices, a team of
    one: no records, no polls; 256 per round) — in the 8 x 8 DPP form at every batch size, in the lane-program form (ELPH_WG_NO_DPP=1)
    for batches beyond one round of 2 slices per wave (64) — against single solves and, solved to 1e-13, against the oracle at 1e-10."""
    from elphdynamics_amd import configs, models
    if not dpp:
        monkeypatch.setenv("ELPH_WG_NO_DPP", "1")
    m = configs.make_model("B", tol=1e-13, maxiter=20000)
    nrhs = 70
    assert _wg_info(m)[1:] == ((5, 8, 1) if dpp else (2, 5, 4)) and _wg_info(m, nrhs)[1:] == (5, 8, 1)
    om = _oracle_model(oracle, m)
    R, B = configs.rhs(m, nrhs)
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B)
    assert not fl.any() and (res < 1e-12).all()
    for i in (0, 33, 69):
        x = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x, m, np.ascontiguousarray(B[i]))
        assert abs(it1 - it[i]) <= 3 and rel(X[i], x) < 1e-10, i
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(B[i]), solver_tol=1e-13, solver_maxiter=20000)
        assert flo == 0 and rel(X[i], xo) < 1e-10, (i, rel(X[i], xo))
    m.close()


def test_wg_resident_cg_bench_shape_vs_oracle(oracle):
    """The shape bench.py times — config C, independent chains side by side (right-hand side r on the matrix of chain r % nchains), a
    batch large enough for 4 slices per wave (T = 4, G = 5) — against the ORACLE directly: every checked right-hand side, solved to
    1e-13 on both sides, is within the north_star's 1e-10 of the oracle's solve on that chain's matrix."""
    from elphdynamics_amd import configs, models, synth
    m = configs.make_model("C", tol=1e-13, maxiter=20000)
    nch, nrhs = 26, 52
    Xc = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=synth.SEED_FIELDS + 17 * c) for c in range(nch)])
    models.update_model_chains_(m, Xc)
    usable, T, W, G = _wg_info(m, nrhs)
    assert usable == 1 and (T, W, G) == (4, 8, 5)
    R = np.stack([synth.rhs(m.Ndim, seed=synth.SEED_RHS + 7919 * i) for i in range(nrhs)])
    X = np.zeros_like(R)
    it, res, fl = models.ldiv_batched_(X, m, R)                  # (the right-hand sides need not be Mt R for this comparison)
    assert not fl.any() and (res < 1e-12).all()
    for i in (0, 1, 25, 26, 27, 51):
        c = i % nch
        E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, Xc[c], m.lam, m.lam2, m.mu)
        om = oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(R[i]), solver_tol=1e-13, solver_maxiter=20000)
        assert flo == 0 and abs(int(it[i]) - ito) <= max(3, ito // 100), (i, int(it[i]), ito)
        assert rel(X[i], xo) < 1e-10, (i, rel(X[i], xo))
    m.close()


def test_exact_bench_batch_vs_oracle(oracle):
    """The EXACT batch bench.py times by default — config C, 288 right-hand sides of 144 chains (right-hand side r on the matrix of chain
    r % 144) — through both of its legs: the un-preconditioned resident kernel (k_cg_wg<T=4,W=8,G=5>: six rounds of 48) and the KPM-preconditioned
    iteration (two half-batches of 144 on two streams, p/x-fused, the register-exchange k_cg_ap of cg_sq16.hip), each solved tightly, against the
    ORACLE's solve of six sampled columns on that chain's matrix: the north_star's 1e-10 on the solution (the Green's-function elements are
    products of its entries).  (Round 5 checked this shape at 52 right-hand sides and the 288 one only from a tool.)"""
    from elphdynamics_amd import _lib, configs, models, preconditioners as pc, synth
    m = configs.make_model("C", tol=1e-13, maxiter=20000)
    nch, nrhs = 144, 288
    Xc = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=100 + c) for c in range(nch)])      # (bench.py's fields)
    models.update_model_chains_(m, Xc)
    usable, T, W, G = _wg_info(m, nrhs)
    assert usable == 1 and (T, W, G) == (4, 8, 5)
    R = np.stack([synth.rhs(m.Ndim, seed=synth.SEED_RHS + 7919 * i) for i in range(nrhs)])
    X = np.zeros_like(R)
    it, res, fl = models.ldiv_batched_(X, m, R)
    assert not fl.any() and (res < 1e-12).all()
    # the preconditioned leg: every chain's own expansion (device Arnoldi), tolerance 1e-12 — the oracle below is the un-preconditioned
    # solve: both are the solution of the same system
    m.solver.tol = 1e-12
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_chains_(P, rng=np.random.default_rng(7))
    Xp = np.zeros_like(R)
    itp, resp, flp = models.ldiv_batched_(Xp, m, R, P=P)
    f = C.c_int()
    _lib.check(_lib.load().elph_bench_px_info(m._h, C.byref(f)))
    assert f.value == 2, f"the preconditioned leg did not take the p/x-fused register-exchange form ({f.value})"
    assert not flp.any() and (resp < 1e-11).all() and itp.max() < it.min()
    for i in (0, 47, 143, 144, 200, 287):                        # first / last of a round, both copies of a chain, both half-batches
        c = i % nch
        E = oracle.update_model_holstein(m.Nsites, m.Ltau, m.dtau, Xc[c], m.lam, m.lam2, m.mu)
        om = oracle.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(R[i]), solver_tol=1e-13, solver_maxiter=20000)
        assert flo == 0 and abs(int(it[i]) - ito) <= max(3, ito // 100), (i, int(it[i]), ito)
        assert rel(X[i], xo) < 1e-10, ("plain", i, rel(X[i], xo))
        assert rel(Xp[i], xo) < 1e-10, ("preconditioned", i, rel(Xp[i], xo))
    m.close()


def test_wg_resident_cg_honeycomb_and_ssh_batches_vs_oracle(oracle):
    """Configs D and E in the shape a batch of chains runs — 3 resp. 2 slices per wave, the register-exchange checkerboards (honeycomb: mirror
    lanes; bond phonons: one hopping-table set per time slice, one of three in LDS) — against the ORACLE directly: solved to 1e-13 on
    both sides, every checked right-hand side is within the north_star's 1e-10 of the oracle's solve on that chain's matrix."""
    from elphdynamics_amd import configs, models, synth
    for tag, nch in (("D", 13), ("E", 13)):
        m = configs.make_model(tag, tol=1e-13, maxiter=20000)
        nrhs = 2 * nch
        if m.kind == models.SSH:
            Xc = np.stack([m.x * (0.6 + 0.8 * c / nch) * (1.0 + 0.2 * synth.randn(synth.SEED_FIELDS + 17 * c, m.Ndof)) for c in range(nch)])
        else:
            Xc = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=synth.SEED_FIELDS + 17 * c) for c in range(nch)])
        models.update_model_chains_(m, Xc)
        usable, T, W, G = _wg_info(m, nrhs)
        assert usable == 1 and T == (3 if tag == "D" else 2), (tag, T, W, G)      # (26 right-hand sides: D takes 3 slices per wave, 48 per round)
        R = np.stack([synth.rhs(m.Ndim, seed=synth.SEED_RHS + 7919 * i) for i in range(nrhs)])
        X = np.zeros_like(R)
        it, res, fl = models.ldiv_batched_(X, m, R)
        assert not fl.any() and (res < 1e-12).all(), tag
        for i in (0, nch - 1, nch, nrhs - 1):
            c = i % nch
            m1 = configs.make_model(tag, tol=1e-13, maxiter=20000)      # (a host-side model of chain c: its tables for the oracle)
            m1.x[:] = Xc[c]
            models.update_model_(m1)
            om = _oracle_model(oracle, m1)
            xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(R[i]), solver_tol=1e-13, solver_maxiter=20000)
            assert flo == 0 and abs(int(it[i]) - ito) <= max(3, ito // 100), (tag, i, int(it[i]), ito)
            assert rel(X[i], xo) < 1e-10, (tag, i, rel(X[i], xo))
            m1.close()
        m.close()


def test_wg_resident_cg_two_workgroups_per_cu_do_not_lose_records(monkeypatch):
    """The experimental 4-wave shape (ELPH_WG_W=4: two workgroups per CU, teams of 20, three teams per XCD) — the shape in which a member
    of a team was late enough READING the records of iteration k to find those of k + 1 in their place while the slots were re-used
    every iteration (time-out within a few hundred iterations; profiles/r03/wg_record_reuse_stall.log).  With records, boundary granules
    and ghost rows double-buffered by the parity of the iteration the solves complete in the resident kernel — no fallback — and
    agree with the default shape."""
    from elphdynamics_amd import configs, models
    m = configs.make_model("C", tol=1e-9)
    R, B = configs.rhs(m, 24)
    X0 = np.zeros_like(B)
    it0, res0, fl0 = models.ldiv_batched_(X0, m, B)
    assert not fl0.any()
    monkeypatch.setenv("ELPH_WG_T", "2")
    monkeypatch.setenv("ELPH_WG_W", "4")
    monkeypatch.setenv("ELPH_WG_TIMEOUT_MS", "500")
    usable, T, W, G = _wg_info(m, 24)
    assert usable == 1 and (T, W, G) == (2, 4, 20)
    for _ in range(3):                      # ~1400 iterations each
        X1 = np.zeros_like(B)
        it1, res1, fl1 = models.ldiv_batched_(X1, m, B)
        assert not fl1.any() and _wg_status(m) == (0, 0), _wg_status(m)
        assert np.max(np.abs(it1 - it0)) <= 3 and rel(X1, X0) < 1e-7      # (another team shape: other summation trees)
    m.close()


def test_wg_resident_cg_shape_pin_makes_bits_independent_of_the_batch(monkeypatch):
    """Which team shape runs decides the last bits of a solution (another summation tree), and the shape follows the batch size
    (config C: 1 slice per wave up to 8 right-hand sides, 2 up to 24, 4 above).  ELPH_WG_T pins it: with the pin a right-hand side's solution
    and iteration count are bit-identical whether it is solved alone, in a batch of 3 or in a batch of 50 — what a deployment that
    must reproduce a chain's trajectory on another batch size sets."""
    from elphdynamics_amd import configs, models
    m = configs.make_model("C", tol=1e-9)
    R, B = configs.rhs(m, 50)
    for pin in ("4", "2"):
        monkeypatch.setenv("ELPH_WG_T", pin)
        assert _wg_info(m, 1)[1] == int(pin) and _wg_info(m, 50)[1] == int(pin)
        Xb = np.zeros_like(B)
        itb, _, fl = models.ldiv_batched_(Xb, m, B)
        assert not fl.any()
        X3 = np.zeros((3, m.Ndim))
        it3, _, _ = models.ldiv_batched_(X3, m, np.ascontiguousarray(B[:3]))
        assert np.array_equal(X3, Xb[:3]) and np.array_equal(it3, itb[:3])
        for i in (0, 31, 49):
            x = np.zeros(m.Ndim)
            it1, _, fl1 = models.ldiv_(x, m, np.ascontiguousarray(B[i]))
            assert fl1 == 0 and it1 == itb[i] and np.array_equal(x, Xb[i]), (pin, i)
    # without the pin the two batch sizes take different shapes (documented behaviour, not a defect): same solution to the tolerance
    monkeypatch.delenv("ELPH_WG_T")
    assert _wg_info(m, 1)[1] == 1 and _wg_info(m, 20)[1] == 2 and _wg_info(m, 50)[1] == 4
    m.close()


def test_resident_kernels_alternate_on_one_handle(oracle, monkeypatch):
    """k_cg_wg and k_pcg_wg share one control block per handle — one tag numbering, one abort word — and lay it out differently (records +
    boundary granules, records + flags).  One handle runs them alternately (16 x 16 sites, 80 time slices; ELPH_PCG_WG=1 and
    ELPH_WG_ALWAYS=1 make every solve resident); the batch of 24 grows the block, which is reallocated and zeroed.  Both kernels sum in
    a fixed order, so every solve must be BIT-identical — iteration counts and solution — to the same solve on a fresh handle that has
    run nothing else, with no fallback counted anywhere; a preconditioned solve of the streaming form (other summation order) must differ
    in bits, which shows that k_pcg_wg did run."""
    from elphdynamics_amd import configs, models, preconditioners as pc
    monkeypatch.setenv("ELPH_PCG_WG", "1")
    monkeypatch.setenv("ELPH_WG_ALWAYS", "1")
    bounds = {}

    def handle():
        m = _holstein_16x16_ltau80()
        P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
        if not bounds:
            oP = oracle.make_kpm(_oracle_model(oracle, m), n=20, buf=0.05, c1=1.0, c2=1.0)
            rng = np.random.default_rng(11)
            bounds["e_min"], bounds["e_max"] = oracle.kpm_setup(oP, b_max=rng.standard_normal(m.Nsites), b_min=rng.standard_normal(m.Nsites))
        pc.setup_(P, **bounds)
        return m, P

    def solve(m, P, B, prec):
        if not prec:
            assert _wg_info(m, len(B))[0] == 1
        X = np.zeros_like(B)
        it, _, fl = models.ldiv_batched_(X, m, B, P=P if prec else None)
        assert not fl.any() and _wg_status(m) == (0, 0), (prec, len(B), _wg_status(m))
        return X, it

    m, P = handle()
    _, B = configs.rhs(m, 24)
    for step, (prec, nr) in enumerate([(True, 8), (False, 1), (False, 24), (True, 3), (False, 2), (True, 8)]):
        Bs = np.ascontiguousarray(B[:nr])
        X, it = solve(m, P, Bs, prec)
        m1, P1 = handle()
        X1, it1 = solve(m1, P1, Bs, prec)
        assert np.array_equal(it, it1) and np.array_equal(X, X1), (step, prec, nr)
        if prec:
            monkeypatch.setenv("ELPH_PCG_WG", "0")
            Xs, its = solve(m1, P1, Bs, prec)
            monkeypatch.setenv("ELPH_PCG_WG", "1")
            assert np.array_equal(its, it1) and rel(X1, Xs) < 1e-9 and not np.array_equal(X1, Xs), (step, nr)
        m1.close()
    m.close()


def test_wg_resident_cg_record_numbering_across_batches(monkeypatch):
    """The meeting records are numbered per launch and not zeroed in between (WgCtl::epoch0); their memory is reinterpreted with every
    batch size.  One handle, batches of changing size back to back: every solution equals the streaming form's."""
    from elphdynamics_amd import configs, models
    m = configs.make_model("C", tol=1e-5)
    R, B = configs.rhs(m, 50)
    monkeypatch.setenv("ELPH_NO_WG", "1")
    Xref = np.zeros_like(B)
    itref, _, fl = models.ldiv_batched_(Xref, m, B)
    assert not fl.any()
    monkeypatch.setenv("ELPH_NO_WG", "0")
    for rnd in range(2):
        for nr in (1, 48, 3, 24, 50, 2, 40, 25):
            X = np.zeros((nr, m.Ndim))
            it, res, fl = models.ldiv_batched_(X, m, np.ascontiguousarray(B[:nr]))
            assert not fl.any(), (rnd, nr)
            assert max(rel(X[i], Xref[i]) for i in range(nr)) < 1e-4 and np.max(np.abs(it - itref[:nr])) <= 3, (rnd, nr)
    m.close()


def test_wg_resident_cg_timeout_falls_back_to_the_streaming_iteration(monkeypatch):
    """A team that cannot meet within the wall-clock bound gives up, every other wave leaves, and the host solves the batch again with
    the two-kernel iteration from the caller's initial guess (run_cg).  Forced here: 400 workgroups for 256 CUs (teams at the
    dispatch frontier wait for a whole solve of the resident ones, ~3 ms) with a bound of 1 ms.  Same bits as the streaming form."""
    from elphdynamics_amd import configs, models
    R, B = None, None
    out = {}
    for name, env in (("stream", {"ELPH_NO_WG": "1"}), ("timeout", {"ELPH_WG_T": "2", "ELPH_WG_TIMEOUT_MS": "1"})):
        for k in ("ELPH_NO_WG", "ELPH_WG_T", "ELPH_WG_TIMEOUT_MS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = configs.make_model("C", tol=1e-5)
        if B is None:
            R, B = configs.rhs(m, 40)
        X = np.full_like(B, 0.25)                                  # a non-zero initial guess must survive the aborted attempt
        it, res, fl = models.ldiv_batched_(X, m, B)
        assert not fl.any() and (res < 1e-4).all(), name
        out[name] = (X, it)
        if name == "timeout":
            # the fallback is visible (elph_wg_status), the handle stays on the streaming iteration for ELPH_WG_COOLDOWN solves and
            # then takes the resident kernel again (a single right-hand side meets the 1 ms bound)
            from elphdynamics_amd import _lib
            cd, fb = C.c_int(), C.c_int64()
            _lib.check(_lib.load().elph_wg_status(m._h, C.byref(cd), C.byref(fb)))
            assert fb.value == 1 and cd.value == 16 and _wg_info(m)[0] == 0
            monkeypatch.setenv("ELPH_WG_TIMEOUT_MS", "2000")
            for k in range(17):
                x = np.zeros(m.Ndim)
                it1, res1, fl1 = models.ldiv_(x, m, np.ascontiguousarray(B[0]))
                assert fl1 == 0
            _lib.check(_lib.load().elph_wg_status(m._h, C.byref(cd), C.byref(fb)))
            assert fb.value == 1 and cd.value == 0 and _wg_info(m)[0] == 1
        m.close()
    assert np.array_equal(out["timeout"][1], out["stream"][1]) and np.array_equal(out["timeout"][0], out["stream"][0])


def test_wg_resident_cg_honeycomb_two_slices_per_wave():
    """Config D (honeycomb, 5 sites per lane): a batch beyond the 16 right-hand sides one round holds at 1 slice per wave runs
    2 slices per wave (24 per round) — against single solves (1 slice per wave) of the same right-hand sides."""
    from elphdynamics_amd import configs, models
    m = configs.make_model("D", tol=1e-5)
    nrhs = 20
    us, T, W, G = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    from elphdynamics_amd import _lib
    _lib.check(_lib.load().elph_bench_wg_info(m._h, nrhs, C.byref(us), C.byref(T), C.byref(W), C.byref(G)))
    assert us.value == 1 and T.value == 2, (us.value, T.value)
    R, B = configs.rhs(m, nrhs)
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B)
    assert not fl.any() and (res < 1e-4).all()
    for i in (0, 9, 19):
        x = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x, m, np.ascontiguousarray(B[i]))
        assert abs(it1 - it[i]) <= 1 and rel(X[i], x) < 5e-5, i
    m.close()


def test_wg_resident_cg_ssh_two_slices_per_wave():
    """Config E (bond phonons): a batch beyond the 8 right-hand sides one round holds at 1 slice per wave runs 2 slices per wave
    (24 per round; three hopping-table sets per wave) — against single solves (1 slice per wave) of the same right-hand sides."""
    from elphdynamics_amd import configs, models, _lib
    m = configs.make_model("E", tol=1e-5)
    nrhs = 12
    us, T, W, G = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().elph_bench_wg_info(m._h, nrhs, C.byref(us), C.byref(T), C.byref(W), C.byref(G)))
    assert us.value == 1 and T.value == 2, (us.value, T.value)
    R, B = configs.rhs(m, nrhs)
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B)
    assert not fl.any() and (res < 1e-4).all()
    for i in (0, 5, 11):
        x = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x, m, np.ascontiguousarray(B[i]))
        assert abs(it1 - it[i]) <= 1 and rel(X[i], x) < 5e-5, i
    m.close()


@pytest.mark.parametrize("tag", ["B", "C", "D", "E"])
def test_wg_resident_cg_maxiter_history_and_initial_guess(oracle, tag):
    """Stop rule details through the resident kernel, every checkerboard form of it (lane program: B; DPP on the square lattice: C;
    honeycomb with mirror lanes: D; bond phonons with a table set per slice: E): maxiter exhaustion (flag 1), eps history against
    the oracle at 1e-10, non-zero initial guess."""
    from elphdynamics_amd import configs, models
    m = configs.make_model(tag, tol=1e-8)
    assert _wg_info(m)[0] == 1
    om = _oracle_model(oracle, m)
    R, B = configs.rhs(m, 1)
    b = np.ascontiguousarray(B[0])
    x = 0.1 * R[0].copy()
    it, hist = models.solve_(x, m, b, tol=1e-8, history=True)
    xo, ito, histo = oracle.cg_solve(om, b, tol=1e-8, maxiter=10000, history=True, x0=0.1 * R[0])
    assert abs(it - ito) <= 1 and rel(x, xo) < 1e-7
    n = min(41, it // 4 + 1)
    assert np.max(np.abs(hist[:n] - histo[:n]) / histo[:n]) < 1e-10
    x = np.zeros(m.Ndim)
    it2 = models.solve_(x, m, b, tol=1e-30, maxiter=17)
    assert it2 == 17
    m.close()
