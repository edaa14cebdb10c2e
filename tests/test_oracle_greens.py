"""Oracle (numpy restatement of GreensFunctions.jl setup!/convolve!) against the golden direct-sum correlations."""
import numpy as np
import pytest

from conftest import golden
from oracle.greens import EstimateGreensFunction

NAMES = ["GD0", "GD0_GD0", "GDD_G00", "GD0_G0D"]


def make(g):
    est = EstimateGreensFunction(int(g["Ltau"]), int(g["norb"]), int(g["L1"]), int(g["L2"]), 1, nv=g["R"].shape[0])
    est.R[:], est.MinvR[:] = g["R"], g["MinvR"]
    return est


@pytest.mark.parametrize("name", ["greens_sq4_L8.npz", "greens_hc3_L6.npz"])
def test_oracle_setup_matches_direct_correlations(name):
    g = golden(name)
    est = make(g)
    for (n1, n2) in [(1, 2), (1, 3), (2, 3)]:
        est.setup(n1, n2)
        for nm in NAMES:
            got = getattr(est, nm).reshape(-1, order="F")
            ref = g["%s_%d%d" % (nm, n1, n2)]
            scale = np.abs(ref).max()
            assert np.abs(got.imag).max() < 1e-14 * scale
            assert np.abs(got.real - ref).max() < 1e-13 * scale, (nm, n1, n2)


def test_oracle_measure_indexing_and_symmetries():
    g = golden("greens_hc3_L6.npz")
    est = make(g)
    est.setup(1, 2)
    L = est.L
    G = g["GD0_12"].reshape((2 * L, 2, 2, 3, 3, 1), order="F")
    # measure_GΔ0(l1,l2,l3,o1,o2,τ) = GΔ0[mod1(τ+1,2L), o2, o1, l1+1, l2+1, l3+1]  (GreensFunctions.jl:293-298)
    assert abs(est.measure_GD0(2, 1, 0, 1, 2, 3) - G[3, 1, 0, 2, 1, 0]) < 1e-13
    assert abs(est.measure_GD0(0, 0, 0, 2, 2, 2 * L) - G[0, 1, 1, 0, 0, 0]) < 1e-13
    # antiperiodic in τ → τ+L for G, periodic for the products
    assert np.allclose(est.GD0[L:], -est.GD0[:L], atol=1e-14)
    assert np.allclose(est.GD0_GD0[L:], est.GD0_GD0[:L], atol=1e-14)
    # estimate(): product of one solution element and one noise element (:334-346)
    assert est.estimate(2, 3, 4, 1, 1) == est.MinvR[0][(2 - 1) * L + 3] * est.R[0][(3 - 1) * L + 0]
    assert est.estimate(2, 3, 4, 1, 2) == est.MinvR[1][(2 - 1) * L + 3] * est.R[1][(3 - 1) * L + 0]


def direct_tables(L, ns, L1, L2, L3, x1, x2, r1, r2):
    """The four tables of setup! as plain cross-correlations over the doubled time axis, summed directly (no FFT): the formula of
    tests/golden/make_golden.py (gen_greens) with a third cell axis,
        ab[dt, s2, s1, d] = (1/V) sum_{t < 2L} sum_{cells l} a~[(t+dt) mod 2L, s2, l+d] * b~[t, s1, l],  V = 2L*Ncells."""
    shape = (L, ns, L1, L2, L3)
    grid = lambda v: v.reshape(shape, order="F")  # noqa: E731
    anti = lambda v: np.concatenate([grid(v), -grid(v)], axis=0)  # noqa: E731
    peri = lambda u, v: np.concatenate([grid(u) * grid(v)] * 2, axis=0)  # noqa: E731

    def corr(a2, b2):
        V = 2 * L * L1 * L2 * L3
        out = np.zeros((2 * L, ns, ns, L1, L2, L3))
        for dt in range(2 * L):
            for d1 in range(L1):
                for d2 in range(L2):
                    for d3 in range(L3):
                        ash = np.roll(a2, (-dt, -d1, -d2, -d3), axis=(0, 2, 3, 4))
                        out[dt, :, :, d1, d2, d3] = np.einsum("tsxyz,tuxyz->su", ash, b2) / V
        return out

    return dict(GD0=corr(anti((x1 + x2) / np.sqrt(2.0)), anti((r1 + r2) / np.sqrt(2.0))), GD0_GD0=corr(peri(x1, x2), peri(r1, r2)),
                GDD_G00=corr(peri(x2, r2), peri(x1, r1)), GD0_G0D=corr(peri(x1, r2), peri(x2, r1)))


# (norbits, L1, L2, L3, L): rectangular honeycomb cells with an odd time axis, a 3-D lattice, three orbitals, a chain, a rectangular square
# lattice, two orbitals on a 3-D lattice
SHAPES = [(2, 6, 4, 1, 7), (1, 3, 2, 2, 6), (3, 2, 3, 1, 5), (1, 5, 1, 1, 9), (1, 12, 6, 1, 8), (2, 3, 2, 2, 4)]


@pytest.mark.parametrize("ns,L1,L2,L3,L", SHAPES)
def test_oracle_setup_matches_direct_correlations_on_more_shapes(ns, L1, L2, L3, L):
    """The FFT restatement against the direct sum on shapes the fixtures do not cover: L1 != L2, L3 > 1, odd L, three orbitals.
    It is the reference the GPU tests compare against (tests/test_gpu_greens_shapes.py)."""
    est = EstimateGreensFunction(L, ns, L1, L2, L3, nv=3)
    rng = np.random.default_rng(1000 * ns + 100 * L1 + 10 * L2 + L3 + L)
    est.R[:] = rng.standard_normal(est.R.shape)
    est.MinvR[:] = rng.standard_normal(est.MinvR.shape)
    for (n1, n2) in [(1, 2), (3, 1)]:
        est.setup(n1, n2)
        ref = direct_tables(L, ns, L1, L2, L3, est.MinvR[n1 - 1], est.MinvR[n2 - 1], est.R[n1 - 1], est.R[n2 - 1])
        for nm in NAMES:
            got = getattr(est, nm)
            assert got.shape == ref[nm].shape
            scale = np.abs(ref[nm]).max()
            assert np.abs(got.imag).max() < 1e-13 * scale, (nm, n1, n2)
            assert np.abs(got.real - ref[nm]).max() < 1e-13 * scale, (nm, n1, n2)
