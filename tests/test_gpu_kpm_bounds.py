"""The device's eigenvalue bounds of the KPM set-up (kpm_dev.hip: k_kpm_bounds and its Hessenberg QR iteration hess_max_real) against the
plain references of tests/kpm_bounds_reference.py, through the hooks elph_bench_hess_max_real and elph_bench_kpm_bounds; the host path
(kpm_host.cpp) runs through the same hooks and meets the same bounds.

Why three kinds of Arnoldi cases: the largest Ritz value of a 20-step recursion moves by 1e-7 ... 3e-6 with the summation order of the dot
products alone (the error of column k of h grows about 5 x per column), so a tight tolerance is possible only where the recursion is short
(n <= 5: all summation orders agree with a long-double run to ~1e-13) or where it spans the whole space (N <= n: the Ritz values are the
spectrum).  There the tolerance is 32 x the reference's own spread of summation orders, never below 64 eps |e|; the full-depth cases keep the
2e-5 of test_kpm_vs_oracle.  Every case has three chains with different fields and different start vectors, and every chain is held to ITS
reference: a chain that read another chain's Ebar, hopping tables or start vector fails.

QR stage: the matrices and the bound |got - ref| <= 32 n eps |H|_F kappa of tests/test_kpm_hess_host.py, which records what the host's
and the oracle's iterations need of that bound (0.012 of it at most).
"""
import numpy as np
import pytest

import kpm_bounds_reference as ref
from test_kpm_hess_host import by_size, check_against_reference

pytestmark = pytest.mark.gpu

NCH = 3


@pytest.fixture(autouse=True)
def no_path_pins(monkeypatch):
    monkeypatch.delenv("ELPH_KPM_HOST", raising=False)
    monkeypatch.delenv("ELPH_KPM_DEVICE", raising=False)


def device_bounds(m, nch, n, bmax, bmin, where):
    from elphdynamics_amd import _lib
    _lib.check(m._lib.elph_kpm_create(m._h, int(n), 0.05, 1.0, 1.0))
    return _lib.kpm_bounds(m._h, nch, bmax, bmin, where)


def references(m, X, bmax, bmin, n):
    return [ref.bounds(m.neighbor_table, *ref.averaged_inputs(m, X[c]), bmax[c], bmin[c], n) for c in range(len(X))]


def check_tight(tag, n, who, got, refs, exact=False):
    """every chain against its own reference, at 32 x spread (floor 64 eps |e|); returns the largest |error| / tolerance"""
    worst = 0.0
    for c, r in enumerate(refs):
        want = r["dense"] if exact else (r["e_min"], r["e_max"])
        for k, what in enumerate(("e_min", "e_max")):
            tol = ref.tolerance(r["spread"][k], want[k])
            err = abs(got[c, k] - want[k])
            print(f"{tag} n {n} {who} chain {c} {what} {got[c, k]:.16g} ref {want[k]:.16g} spread {r['spread'][k]:.3g} |err| {err:.3g} "
                  f"tol {tol:.3g} ratio {err / tol:.3g}")
            assert err <= tol, (tag, n, who, c, what, got[c, k], want[k], tol)
            worst = max(worst, err / tol)
    # the chains are different problems: no two references coincide to the tolerance
    vals = [r["e_max"] for r in refs]
    assert min(abs(a - b) for i, a in enumerate(vals) for b in vals[i + 1:]) > 1e-6
    return worst


def make(tag, base=0.6, **kw):
    from elphdynamics_amd import configs, models
    m = configs.make_model(tag, **kw)
    X = ref.chain_fields(m, NCH, base=base)
    models.update_model_chains_(m, X)
    rng = np.random.default_rng(11)
    return m, X, rng.standard_normal((NCH, m.Nsites)), rng.standard_normal((NCH, m.Nsites))


# ------------------------------------------------------------------------------------------ the QR stage alone

def test_device_qr_against_the_reference():
    from elphdynamics_amd import _lib, configs
    cases = [(name, H, ref.hessenberg_top(H)) for name, H in ref.hessenberg_cases()]
    m = configs.make_model("b")
    try:
        dev, host = np.zeros(len(cases)), np.zeros(len(cases))
        for n, idx in by_size(cases).items():
            mats = [cases[k][1] for k in idx]
            dev[idx] = _lib.hess_max_real(mats, where=1, handle=m._h)          # one launch per size, one wave per matrix
            host[idx] = _lib.hess_max_real(mats, where=0)
        assert np.array_equal(np.isfinite(dev), np.isfinite(host))            # the same convergence class
        worst = check_against_reference(cases, dev, "device")
        print(f"QR stage: largest device |err| / bound = {worst:.3g}")
        a, out = 2.0 * np.eye(65) - np.eye(65, k=1) - np.eye(65, k=-1), np.zeros(1)      # one row more than the wave has lanes
        assert m._lib.elph_bench_hess_max_real(m._h, 1, 1, 65, _lib.dptr(a), _lib.dptr(out)) == _lib.ELPH_E_UNSUPPORTED
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ Arnoldi: exact spectrum, short and full recursions

@pytest.mark.parametrize("tag", ["b", "e"])           # 4 x 4 Holstein; 4 x 4 bond phonons: per-chain hopping tables (hop_stride != 0)
def test_exact_spectrum(tag):
    """N = 16 <= n = 20: the recursion spans the space and the Ritz values are the spectrum of A and of A^-1."""
    m, X, bmax, bmin = make(tag)
    try:
        refs = references(m, X, bmax, bmin, 20)
        dev, ran = device_bounds(m, NCH, 20, bmax, bmin, 1)
        host, ran0 = device_bounds(m, NCH, 20, bmax, bmin, 0)
        assert ran == 1 and ran0 == 0
        check_tight(tag, 20, "device", dev, refs, exact=True)
        check_tight(tag, 20, "host", host, refs, exact=True)
    finally:
        m.close()


# tag, model options, the depths.  s: N = 36 one register with dead lanes; B: N = 64 exactly one wave; q: N = 100 two registers, ragged;
# t12: 3 bonds per site and colour; C: N = 256, bond program in LDS; D: N = 288 honeycomb, bond program NOT in LDS; k: N = 400, 7 registers;
# l22: N = 484, 8 registers; e8: bond phonons; C with hopping disorder
LATTICES = [("s", {}, (1, 2, 5)), ("B", {}, (1, 2, 5)), ("q", {}, (1, 2, 5)), ("t12", {}, (1, 2, 5)), ("C", {}, (1, 2, 5, 20)),
            ("D", {}, (1, 2, 5, 20)), ("k", {}, (1, 2, 5)), ("l22", {}, (1, 2, 5, 20)), ("e8", {}, (1, 2, 5)),
            ("C", {"t_stddev": 0.1}, (1, 2, 5))]


@pytest.mark.parametrize("tag,opts,depths", LATTICES, ids=[t + ("_disorder" if o else "") for t, o, _ in LATTICES])
def test_short_and_full_recursions(tag, opts, depths):
    m, X, bmax, bmin = make(tag, **opts)
    try:
        if opts:
            # the hoppings really differ, from bond to bond and from direction to direction: make_model draws all of them from one generator
            assert len(set(np.round(m.cosht, 12))) == m.Nbonds == 2 * m.Nsites
        for n in depths:
            if n > 5:       # full depth: rougher fields, on which the reference's own summation orders agree to 3e-6 (chain_fields)
                from elphdynamics_amd import models
                X = ref.chain_fields(m, NCH, base=1.1)
                models.update_model_chains_(m, X)
            refs = references(m, X, bmax, bmin, n)
            dev, ran = device_bounds(m, NCH, n, bmax, bmin, 1)
            host, ran0 = device_bounds(m, NCH, n, bmax, bmin, 0)
            assert ran == 1 and ran0 == 0
            if n <= 5:
                wd = check_tight(tag, n, "device", dev, refs)
                wh = check_tight(tag, n, "host", host, refs)
                print(f"{tag} n {n}: largest |err| / tol device {wd:.3g} host {wh:.3g}")
            else:
                # the bound of test_kpm_vs_oracle: a coarse check, the short recursions carry the precision
                want = np.array([(r["e_min"], r["e_max"]) for r in refs])
                spread = max(max(r["spread"]) for r in refs)
                print(f"{tag} n {n}: |device - ref| {np.abs(dev - want).max():.3g} |host - ref| {np.abs(host - want).max():.3g} "
                      f"|device - host| {np.abs(dev - host).max():.3g} spread {spread:.3g}")
                assert spread < 3e-6                                           # the inputs can carry the bound
                assert np.abs(dev - want).max() < 2e-5 and np.abs(host - want).max() < 2e-5 and np.abs(dev - host).max() < 2e-5
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ breakdown of the recursion

def test_breakdown_in_the_first_step():
    """Uniform field, uniform hopping, constant start vector on 6 x 6: the start vector is an eigenvector, the Krylov space one-dimensional
    (l = 1, the n == 1 path of the QR iteration), and both bounds are that eigenvalue Ebar exp(4 dtau t)."""
    from elphdynamics_amd import configs, models
    m = configs.make_model("s")
    try:
        X = np.stack([np.full(m.Ndof, x) for x in (0.5, 1.0, 1.5)])
        models.update_model_chains_(m, X)
        ones = np.ones((NCH, m.Nsites))
        refs = references(m, X, ones, ones, 20)
        for c, r in enumerate(refs):
            lam = np.exp(-m.dtau * X[c, 0]) * np.exp(4 * m.dtau)
            assert abs(r["e_max"] - lam) < 1e-14 and abs(r["e_min"] - lam) < 1e-14
        dev, ran = device_bounds(m, NCH, 20, ones, ones, 1)
        host, _ = device_bounds(m, NCH, 20, ones, ones, 0)
        assert ran == 1
        check_tight("s uniform", 20, "device", dev, refs)
        check_tight("s uniform", 20, "host", host, refs)
        for c, r in enumerate(refs):
            assert np.all(np.abs(dev[c] - host[c]) <= [ref.tolerance(r["spread"][k], host[c, k]) for k in (0, 1)])
    finally:
        m.close()


def test_breakdown_in_the_third_step():
    """A start vector that is the sum of three eigenvectors of A (from the dense reference): the recursion stops at l = 3, e_max is the
    largest of the three eigenvalues and e_min the smallest."""
    m, X, _, _ = make("s")
    try:
        start, lams = [], []
        for c in range(NCH):
            # (the checkerboard product is not symmetric: A has a few complex pairs; LAPACK returns the real eigenvalues with real vectors)
            w, V = np.linalg.eig(ref.Operator(m.neighbor_table, *ref.averaged_inputs(m, X[c])).dense())
            real = np.flatnonzero(w.imag == 0.0)
            real = real[np.argsort(w.real[real])]
            pick = real[[0, len(real) // 2, -1]]
            start.append(sum(V[:, k].real / np.linalg.norm(V[:, k].real) for k in pick))
            lams.append(w.real[pick])
        start = np.ascontiguousarray(start)
        refs = references(m, X, start, start, 20)
        for r, lam in zip(refs, lams):
            assert abs(r["e_max"] - lam.max()) < 1e-11 and abs(r["e_min"] - lam.min()) < 1e-11
        dev, ran = device_bounds(m, NCH, 20, start, start, 1)
        host, _ = device_bounds(m, NCH, 20, start, start, 0)
        assert ran == 1
        check_tight("s 3 eigenvectors", 20, "device", dev, refs)
        check_tight("s 3 eigenvectors", 20, "host", host, refs)
        for c, r in enumerate(refs):
            assert np.all(np.abs(dev[c] - host[c]) <= [ref.tolerance(r["spread"][k], host[c, k]) for k in (0, 1)])
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ refusals, non-finite chains, dispatch

@pytest.mark.parametrize("tag,n", [("h", 20), ("q", 65), ("l22", 40)])      # N = 648 > 512; n > 64; 198 KB of LDS > 160 KB
def test_refusals_fall_back_to_the_host_and_say_so(tag, n):
    m, X, bmax, bmin = make(tag)
    try:
        dev, ran = device_bounds(m, NCH, n, bmax, bmin, 1)
        host, ran0 = device_bounds(m, NCH, n, bmax, bmin, 0)
        assert ran == 0 and ran0 == 0
        assert np.array_equal(dev, host) and np.all(np.isfinite(host))
    finally:
        m.close()


def test_non_finite_chain():
    """Chain 1 with a field so large that Ebar overflows to inf on the sites where it is negative and underflows to 0 where it is positive:
    A v is NaN and A^-1 v infinite, h is not finite, the QR iteration is skipped and the chain's bounds are (-inf, +inf) as in the
    reference (:890-895, :934-939).  Chains 0 and 2 are untouched, and setup!(P) turns chain 1's expansion off."""
    from elphdynamics_amd import models, preconditioners as pc
    m, X, bmax, bmin = make("b")
    try:
        dev0, _ = device_bounds(m, NCH, 20, bmax, bmin, 1)
        host0, _ = device_bounds(m, NCH, 20, bmax, bmin, 0)
        X[1] = 1e5 * np.repeat(np.where(np.arange(m.Nsites) % 2 == 0, 1.0, -1.0), m.Ltau)
        models.update_model_chains_(m, X)
        refs = references(m, X, bmax, bmin, 20)
        assert (refs[1]["e_min"], refs[1]["e_max"]) == (-np.inf, np.inf)
        dev, ran = device_bounds(m, NCH, 20, bmax, bmin, 1)
        host, _ = device_bounds(m, NCH, 20, bmax, bmin, 0)
        assert ran == 1
        for got, before in ((dev, dev0), (host, host0)):
            assert got[1, 0] == -np.inf and got[1, 1] == np.inf
            assert np.array_equal(got[[0, 2]], before[[0, 2]])
        P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
        act, _, _ = pc.setup_chains_(P, b_max=bmax, b_min=bmin)
        assert act.tolist() == [1, 0, 1]
    finally:
        m.close()


def test_dispatch_by_chain_count():
    """Without ELPH_KPM_HOST / ELPH_KPM_DEVICE setup!(P) takes the host for one and two chains and the device from three."""
    from elphdynamics_amd import configs, models
    m = configs.make_model("b")
    try:
        X = ref.chain_fields(m, NCH)
        rng = np.random.default_rng(11)
        bmax, bmin = rng.standard_normal((NCH, m.Nsites)), rng.standard_normal((NCH, m.Nsites))
        for nch, want in ((1, 0), (2, 0), (3, 1)):
            models.update_model_chains_(m, X[:nch])
            e, ran = device_bounds(m, nch, 20, bmax[:nch], bmin[:nch], 2)
            assert ran == want and np.all(np.isfinite(e))
    finally:
        m.close()
