"""CPU test of the host's Hessenberg QR iteration (kpm_host.cpp: elph_hess_eigvals, through elph_bench_hess_max_real with where = 0) against
the plain reference of tests/kpm_bounds_reference.py: the largest real part of the spectrum of every matrix of hessenberg_cases() within

    |got - ref| <= 32 n eps |H|_F kappa

— the backward error of a QR iteration times the first-order sensitivity of that eigenvalue.  tests/test_gpu_kpm_bounds.py holds the
device's iteration (kpm_dev.hip: hess_max_real) to the same matrices and the same bound.

The factor 32 was checked on the two existing implementations of the algorithm before the device saw it.  Largest |got - ref| / bound over
the list: host elph_hess_eigvals 0.012 (the 3 x 3 cyclic permutation; 0.004 on the Arnoldi matrices, below 1e-3 on the random ones), the
oracle's elpho_eigvals 0.012 (the same figures: on a Hessenberg matrix its reduction step does nothing and the iterations coincide).
"""
import ctypes as C

import numpy as np
import pytest

import kpm_bounds_reference as ref
from elphdynamics_amd import _lib


@pytest.fixture(scope="module")
def cases():
    return [(name, H, ref.hessenberg_top(H)) for name, H in ref.hessenberg_cases()]


def by_size(cases):
    """{n: [indices]}: one call of the hook per matrix size"""
    groups = {}
    for k, (_, H, _) in enumerate(cases):
        groups.setdefault(H.shape[0], []).append(k)
    return groups


def check_against_reference(cases, got, who):
    """the assertions the host and the device share; returns the largest |got - ref| / bound"""
    worst = 0.0
    for (name, H, top), g in zip(cases, got):
        bound = ref.qr_bound(H.shape[0], top["norm"], top["kappa"])
        err = abs(g - top["value"])
        print(f"{who} {name:14s} n {H.shape[0]:2d} kappa {top['kappa']:8.3g} |err| {err:9.3g} bound {bound:9.3g} ratio {err / bound:9.3g}")
        assert np.isfinite(g) and err <= bound, (who, name, g, top["value"], bound)
        worst = max(worst, err / bound)
    vals = {name: g for (name, _, _), g in zip(cases, got)}
    tops = {name: top for name, _, top in cases}
    # a power of two scales every operation of the iteration exactly: so does the result, within the bound
    for name, scale in (("scaled_up", 2.0 ** 300), ("scaled_down", 2.0 ** -300)):
        bound = ref.qr_bound(20, tops[name]["norm"], tops[name]["kappa"])
        assert abs(vals[name] - vals["scaled_base"] * scale) <= bound
    return worst


def test_the_reference_on_known_spectra(cases):
    """The matrices are what their names say, and the reference knows their analytic answers."""
    tops = {name: top for name, _, top in cases}
    assert tops["n1"]["value"] == -2.5
    assert abs(tops["real_pair"]["value"] - np.sqrt(2.0)) < 4 * ref.EPS and not tops["real_pair"]["complex"]
    assert abs(tops["complex_pair"]["value"] - 0.75) < 4 * ref.EPS and tops["complex_pair"]["complex"]
    assert abs(tops["cyclic3"]["value"] - 1.0) < 4 * ref.EPS
    assert abs(tops["triangular7"]["value"] - 3.5) < 8 * ref.EPS
    assert abs(tops["toeplitz64"]["value"] - (2.0 - 2.0 * np.cos(64 * np.pi / 65))) < 16 * ref.EPS
    rnd = [top for name, _, top in cases if name.startswith("random")]
    assert {H.shape[0] for name, H, _ in cases if name.startswith("random")} == {20, 33, 64}
    assert all(top["kappa"] <= 1e3 for top in rnd) and any(top["complex"] for top in rnd)
    assert tops["arnoldi_A"]["kappa"] < 1.01 and tops["arnoldi_Ainv"]["kappa"] < 1.01
    H = dict((name, H) for name, H, _ in cases)
    assert all(np.array_equal(h, np.triu(h, -1)) for h in H.values())
    assert H["blocks12"][3, 2] == 0.0 and H["blocks12"][7, 6] == 0.0 and np.count_nonzero(np.diag(H["blocks12"], -1)) == 9


def test_host_qr_against_the_reference(cases):
    got = np.zeros(len(cases))
    for n, idx in by_size(cases).items():
        got[idx] = _lib.hess_max_real([cases[k][1] for k in idx], where=0)
    worst = check_against_reference(cases, got, "host")
    assert worst <= 1.0


def test_oracle_qr_against_the_reference(cases, oracle):
    """The oracle's elpho_eigvals — the other implementation of the algorithm — meets the same bound."""
    got = []
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    for _, H, _ in cases:
        n = H.shape[0]
        a, wr, wi = np.ascontiguousarray(H.T), np.zeros(n), np.zeros(n)
        assert oracle.lib.elpho_eigvals(dp(a), n, dp(wr), dp(wi)) == 0
        got.append(wr.max())
    check_against_reference(cases, got, "oracle")


def test_hook_arguments():
    lib = _lib.load()
    a, out = np.eye(3), np.zeros(1)
    assert lib.elph_bench_hess_max_real(None, 0, 0, 3, _lib.dptr(a), _lib.dptr(out)) == _lib.ELPH_E_ARG
    assert lib.elph_bench_hess_max_real(None, 0, 1, 3, None, _lib.dptr(out)) == _lib.ELPH_E_ARG
    assert lib.elph_bench_hess_max_real(None, 2, 1, 3, _lib.dptr(a), _lib.dptr(out)) == _lib.ELPH_E_ARG
    assert lib.elph_bench_hess_max_real(None, 1, 1, 3, _lib.dptr(a), _lib.dptr(out)) == _lib.ELPH_E_ARG       # the device needs a handle
    assert lib.elph_bench_hess_max_real(None, 0, 1, 3, _lib.dptr(a), _lib.dptr(out)) == _lib.ELPH_OK and out[0] == 1.0
