"""CPU test of the KPM preconditioner's planning (kpm_host.cpp: elph_kpm_plan_chain, elph_kpm_tables) through the device-free probe
elph_bench_kpm_plan: the acceptance window, the buf hysteresis, the orders and coefficients of setup!(P) (KPMPreconditioners.jl:272-318),
the identity expansion of an inactive chain, the longest-first schedule and the order-1 fold weights of the tables."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from elphdynamics_amd import _lib


def rel_max(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


def chain_coeff(p, c):
    """chain c's coefficients (complex), from the flattened vector"""
    return p["coeff"][p["coff"][c, 0]:p["coff"][c, -1]]


@pytest.mark.parametrize("tag", ["sq4_L8", "sq4_L40"])
def test_golden(tag):
    k = golden(f"kpm_{tag}.npz")
    L = {"sq4_L8": 8, "sq4_L40": 40}[tag]
    p = _lib.kpm_plan(L, [[(float(k["e_min"]), float(k["e_max"]))]], float(k["buf"]), float(k["c1"]), float(k["c2"]))
    assert p["uploaded"] == [True] and p["active"] == [True]
    assert p["lam_lo"][0] == float(k["lam_lo"]) and p["lam_hi"][0] == float(k["lam_hi"])
    assert np.array_equal(p["order"][0], k["orders"])
    want = k["coeff_re"] + 1j * k["coeff_im"]
    assert rel_max(chain_coeff(p, 0), want) < 1e-12


def _oracle_kpm(oracle, L, e_min, e_max):
    """the oracle's setup!(P) with injected bounds, on a 2 x 2 Holstein lattice of Ltau = L"""
    tab = np.array([[1, 2], [3, 4], [1, 3], [2, 4]], dtype=np.int64)
    om = oracle.make_model(0, 4, L, tab, np.full(4, np.cosh(0.1)), np.full(4, np.sinh(0.1)), np.ones(4 * L))
    P = oracle.make_kpm(om, n=20, buf=0.05, c1=1.0, c2=1.0)
    oracle.kpm_setup(P, e_min=e_min, e_max=e_max)
    return P


@pytest.mark.parametrize("L", [7, 8, 21, 40])
@pytest.mark.parametrize("bounds", [(0.31, 1.72), (0.05, 1.9), (0.8, 1.1)])
def test_against_oracle(oracle, L, bounds):
    P = _oracle_kpm(oracle, L, *bounds)
    p = _lib.kpm_plan(L, [[bounds]])
    Lo2 = (L + 1) // 2
    assert P.active == 1 and p["active"] == [True]
    assert p["lam_lo"][0] == P.lam_lo and p["lam_hi"][0] == P.lam_hi
    assert p["lam_avg"][0] == P.lam_avg and p["lam_mag"][0] == P.lam_mag
    order = P._keep["order"][:Lo2]
    assert np.array_equal(p["order"][0], order)
    assert np.array_equal(p["coff"][0], P._keep["coff"][:Lo2 + 1])
    cz = P._keep["coeff"][:2 * int(order.sum())]
    assert rel_max(chain_coeff(p, 0), cz[0::2] + 1j * cz[1::2]) < 1e-12


def test_implausible_bounds_give_the_identity(oracle):
    P = _oracle_kpm(oracle, 8, 1.5, 1.2)
    p = _lib.kpm_plan(8, [[(1.5, 1.2)]])
    assert P.active == 0 and p["active"] == [False]
    assert np.all(p["order"] == 1) and np.all(p["coeff"] == 1.0) and np.all(p["c0"] == 1.0)
    assert p["lam_mag"][0] == -1.0
    assert np.array_equal(p["coff"][0], np.arange(5))
    assert np.all(p["fold"][0] == [1.0, 0.0])       # (an identity expansion hands over the r.r partial sums: no fold)


def test_mixed_chains():
    L, Lo2 = 10, 5
    bounds = [(0.3, 1.8), (1.5, 1.2), (0.6, 1.3), (-0.1, 1.5)]
    p = _lib.kpm_plan(L, [bounds])
    assert p["active"] == [True, False, True, False]
    for c, b in enumerate(bounds):
        solo = _lib.kpm_plan(L, [[b]])
        assert np.array_equal(p["order"][c], solo["order"][0])
        assert np.array_equal(p["coff"][c] - p["coff"][c, 0], solo["coff"][0])
        assert np.array_equal(chain_coeff(p, c), chain_coeff(solo, 0))
        assert p["lam_mag"][c] == solo["lam_mag"][0] and p["lam_avg"][c] == solo["lam_avg"][0]
    # the chains' coefficients follow one another in the flattened vector
    assert p["coff"][0, 0] == 0 and all(p["coff"][c, 0] == p["coff"][c - 1, -1] for c in range(1, 4))
    assert len(p["coeff"]) == p["coff"][-1, -1] and p["order"].shape == (4, Lo2)
    assert np.all(p["order"][[1, 3]] == 1) and np.all(p["lam_mag"][[1, 3]] == -1.0)


@pytest.mark.parametrize("L", [7, 8, 9, 40])
def test_schedule_and_fold(L):
    Lo2 = (L + 1) // 2
    # bounds that give order 1 at the high frequencies, so that both the ties of the schedule and the fold show
    p = _lib.kpm_plan(L, [[(0.5, 1.3), (0.3, 1.8), (1.5, 1.2)]], c2=0.5)
    for c in range(3):
        order, active = p["order"][c], p["active"][c]
        # frequency blocks by decreasing order, ties in frequency order (a stable sort)
        assert list(p["wsched"][c]) == sorted(range(Lo2), key=lambda w: -order[w])
        # the packed schedule's leading coefficients
        c0 = p["coeff"][p["coff"][c, :-1]]
        assert np.array_equal(p["c0"][c], c0[p["wsched"][c]])
        for w in range(Lo2):
            fold = active and order[w] == 1
            s1 = c0[w].real * c0[w].real + c0[w].imag * c0[w].imag if fold else 1.0      # |c0|^2: z_w = |c0|^2 r_w
            wgt = 1.0 if (L % 2 and w == Lo2 - 1) else 2.0       # (odd L: the last frequency is its own mirror image)
            assert p["fold"][c, w, 0] == s1
            assert p["fold"][c, w, 1] == (wgt * s1 / L if fold else 0.0)
    assert np.any(p["order"][0] == 1) and np.any(p["order"][0] > 1)       # (the case was chosen to have both)


def test_hysteresis():
    L = 20
    first = (0.3, 1.8)
    within = (0.3 * 1.02, 1.8 * 1.02)      # lam moves by 2 % < buf = 5 %
    beyond = (0.3 * 1.2, 1.8)
    p = _lib.kpm_plan(L, [[first], [within]])
    p0 = _lib.kpm_plan(L, [[first]])
    assert p["uploaded"] == [True, False]
    assert np.array_equal(p["order"], p0["order"]) and p["lam_lo"][0] == p0["lam_lo"][0] and p["lam_hi"][0] == p0["lam_hi"][0]
    assert np.array_equal(p["coeff"], p0["coeff"])
    q = _lib.kpm_plan(L, [[first], [beyond]])
    q1 = _lib.kpm_plan(L, [[beyond]])
    assert q["uploaded"] == [True, True]
    assert q["lam_lo"][0] == q1["lam_lo"][0] and np.array_equal(q["order"], q1["order"]) and np.array_equal(q["coeff"], q1["coeff"])
    # turning a chain off and on again is a change even when its window stays
    r = _lib.kpm_plan(L, [[first], [(1.5, 1.2)], [(1.5, 1.2)], [within]])
    assert r["uploaded"] == [True, True, False, True]
    assert np.array_equal(r["order"], p0["order"])


def test_probe_reports_a_short_coefficient_buffer():
    lib = _lib.load()
    eb = np.array([0.3, 1.8])
    n = C.c_int64()
    assert lib.elph_bench_kpm_plan(20, 0.05, 1.0, 1.0, 1, 1, _lib.dptr(eb), None, None, None, None, None, None, None, None, None, 0,
                                   C.byref(n)) == 0
    assert n.value > 2
    short = np.zeros(2)
    assert lib.elph_bench_kpm_plan(20, 0.05, 1.0, 1.0, 1, 1, _lib.dptr(eb), None, None, None, None, None, None, None, None,
                                   _lib.dptr(short), 2, C.byref(n)) != 0
