"""Direct-sum restatement of the Holstein bond correlations (measure_BondBond!, Measurements.jl:1663-1785; measure_BondPairGreens!,
:2390-2483; translational_average!, Utilities.jl:49-60), used by tests only.

With shift(f, r)[tau, i] = f[tau, i + r] on the periodic cell grid and
    f * g [dtau, dr] = 1 / (L ncells) sum_{tau, i} f[tau + dtau, i + dr] g[tau, i]          (periodic in L)
a listed pair p = (n'', n') of bond definitions, (d, c, r'') = (o1, o2, v) of n'' and (b, a, r') = (o1, o2, v) of n', gives
    BondBond        B = 4 (x1[b] shift(r1[a], r')) * (x2[d] shift(r2[c], r'')) - 2 (x1[b] shift(r2[a], r')) * (x2[d] shift(r1[c], r''))
                    + 2 G[D,0](l, c, b, tau = 0) at tau = 0, l = mod(-r' - r'', L), when a == d;   slice beta: B[0, -l]
    BondPairGreens  P = (shift(x1[a], r') x2[b]) * (shift(r1[c], r'') r2[d]);   slice beta: P[0, l] plus the three delta terms of :2466-2474
(r = noise vector, x = M^-1 r).  `star_direct` evaluates f * g by explicit sums over rolled arrays, one displacement at a time, no FFT;
`star_fft` is the second evaluation, written as translational_average! writes it (fft!, the reversed shifted copy, ifft!).  G[D,0] comes
from measurements_reference.setup_tables (direct sums on the doubled antiperiodic axis); nothing else of that file's tables is used.

Vectors are flat in the reference layout, index = site * Ltau + tau, site = norbits * cell + orbit, cell = l1 + L1 (l2 + L2 l3).  Fields
here are arrays [tau, l3, l2, l1]."""
import numpy as np

import measurements_reference as mref

CORRS = ("BondBond", "BondPairGreens")


def grid(v, L, ns, dims):
    """flat reference-layout vector -> [orbit][tau, l3, l2, l1]"""
    nc = dims[0] * dims[1] * dims[2]
    f = mref._field(v, L, ns, nc)                                           # [tau, orbit, cell]
    return [np.ascontiguousarray(f[:, o, :]).reshape(L, dims[2], dims[1], dims[0]) for o in range(ns)]


def shift(f, r):
    """shift(f, r)[tau, i] = f[tau, i + r]: circshift!(dest, src, (0, -r1, -r2, -r3))."""
    return np.roll(f, (-r[2], -r[1], -r[0]), axis=(1, 2, 3))


def star_direct(f, g, points=None):
    """f * g by direct sums.  points: the displacements (dtau, l3, l2, l1) to evaluate, all of them by default; the others are NaN."""
    out = np.full(f.shape, np.nan)
    if points is None:
        points = list(np.ndindex(*f.shape))
    for pt in points:
        out[tuple(pt)] = (np.roll(f, tuple(-k for k in pt), axis=(0, 1, 2, 3)) * g).sum() / f.size
    return out


def star_fft(f, g, points=None):
    """translational_average!(fg, f, g) (Utilities.jl:49-60) on complex copies, step by step as the reference writes it."""
    F, G = np.fft.fftn(f.astype(np.complex128)), np.fft.fftn(g.astype(np.complex128))
    N = f.size
    Gp = np.roll(G, tuple(s - 1 for s in G.shape), axis=(0, 1, 2, 3))      # circshift!(g', g, size - 1)
    Gp = Gp[::-1, ::-1, ::-1, ::-1]                                         # reverse!(g')
    fg = np.fft.ifftn(F * Gp / N)
    assert np.abs(fg.imag).max() <= 1e-13 * max(1.0, np.abs(fg.real).max())
    return fg.real


def _cell(l, dims):
    return (l[0] % dims[0]) + dims[0] * ((l[1] % dims[1]) + dims[1] * (l[2] % dims[2]))


def pair_terms(r1, x1, r2, x2, L, ns, dims, defs, request, star, GD0, points=None):
    """What one pair of vectors adds: {name: [L0, l3, l2, l1, np]}.  GD0: [2L, s2, s1, cell], measure_GD0(l, o1, o2, tau) =
    GD0[tau, o2 - 1, o1 - 1, cell(l)] (GreensFunctions.jl:293-298)."""
    R1, X1, R2, X2 = (grid(v, L, ns, dims) for v in (r1, x1, r2, x2))
    L1, L2, L3 = dims
    G = lambda l, o1, o2: GD0[0, o2 - 1, o1 - 1, _cell(l, dims)]  # noqa: E731
    out = {}
    for name, (L0, pairs) in request.items():
        res = np.zeros((L0, L3, L2, L1, pairs.shape[1]))
        for p in range(pairs.shape[1]):
            d, c, rpp = defs[pairs[0, p] - 1]                               # n'': d -> c displaced r''
            b, a, rp = defs[pairs[1, p] - 1]                                # n':  b -> a displaced r'
            if name == "BondBond":
                B = 4 * star(X1[b - 1] * shift(R1[a - 1], rp), X2[d - 1] * shift(R2[c - 1], rpp), points)
                B = B - 2 * star(X1[b - 1] * shift(R2[a - 1], rp), X2[d - 1] * shift(R1[c - 1], rpp), points)
                if a == d:
                    l = [(-rp[k] - rpp[k]) % dims[k] for k in range(3)]
                    B[0, l[2], l[1], l[0]] += 2 * G(l, c, b)
                res[:min(L0, L), ..., p] = B[:min(L0, L)]
                if L0 > 1:
                    for l3 in range(L3):
                        for l2 in range(L2):
                            for l1 in range(L1):
                                res[L, l3, l2, l1, p] = B[0, (-l3) % L3, (-l2) % L2, (-l1) % L1]
            elif name == "BondPairGreens":
                P = star(shift(X1[a - 1], rp) * X2[b - 1], shift(R1[c - 1], rpp) * R2[d - 1], points)
                res[:min(L0, L), ..., p] = P[:min(L0, L)]
                if L0 > 1:
                    d_ac, d_bd = float(a == c), float(b == d)
                    d_rr = float(tuple(rp) == tuple(rpp))
                    for l3 in range(L3):
                        for l2 in range(L2):
                            for l1 in range(L1):
                                l = (l1, l2, l3)
                                d_r0 = float(l == (0, 0, 0))
                                d_rl = float(all(rpp[k] == (rp[k] + l[k]) % dims[k] for k in range(3)))    # r'' as given, as the reference
                                val = P[0, l3, l2, l1]
                                val += d_ac * d_rr * d_bd * d_r0
                                val -= d_bd * d_r0 * G([(rp[k] + l[k] - rpp[k]) % dims[k] for k in range(3)], c, a)
                                val -= d_ac * d_rl * G(l, d, b)
                                res[L, l3, l2, l1, p] = val
            else:
                raise KeyError(name)
        out[name] = res
    return out


def measure(R, MinvR, L, ns, dims, defs, request, star=star_direct, points=None):
    """Everything accumulate adds for the vectors R, MinvR ((nv, Ndim)), summed over all pairs i < j.  defs: (o1, o2, (v1, v2, v3)) per
    bond definition, 1-based orbitals; request: {name: (L0, pairs (2, np) 1-based bond-definition indices)}.
    Returns {name: real [L0, L1, L2, L3, np]} (NaN where `points` left a displacement out)."""
    nv = R.shape[0]
    tot = {}
    for i in range(nv - 1):
        for j in range(i + 1, nv):
            GD0 = mref.setup_tables(R[i], MinvR[i], R[j], MinvR[j], L, ns, dims)[0]
            one = pair_terms(R[i], MinvR[i], R[j], MinvR[j], L, ns, dims, defs, request, star, GD0, points)
            for k, v in one.items():
                tot[k] = tot.get(k, 0.0) + v
    return {k: np.asfortranarray(v.transpose(0, 3, 2, 1, 4)) for k, v in tot.items()}


def sample_points(L, dims, n, seed):
    """Every cell displacement at dtau = 0 (it holds D = 0, every delta-term position and what the beta slices read) and n more
    displacements drawn without replacement from the rest, seeded."""
    L1, L2, L3 = dims
    pts = [(0, l3, l2, l1) for l3 in range(L3) for l2 in range(L2) for l1 in range(L1)]
    rng = np.random.default_rng(seed)
    nc = L1 * L2 * L3
    flat = rng.choice((L - 1) * nc, size=min(n, (L - 1) * nc), replace=False)
    for q in flat:
        dt, cell = 1 + q // nc, q % nc
        pts.append((int(dt), int(cell // (L1 * L2)), int((cell // L1) % L2), int(cell % L1)))
    return pts
