"""Direct-sum restatement of the Holstein measurements (Measurements.jl, GreensFunctions.jl:239-346, Utilities.jl:49-76), used by tests only.

Everything is computed from (R, MinvR, x, parameters, pairs) with explicit sums: a translation average is a sum over slices (np.roll
along the time axis) and over cells (a gather through the table of periodic cell sums) of the products, on the doubled antiperiodic
[a, -a] / periodic [a, a] time axis exactly as setup! builds it.  No FFT is used here; momentum() is the only transform and is
np.fft.fftn.  It therefore shares neither the transforms nor the half-axis storage of the device code.

For each reduced scalar `abs` holds the sum of the absolute values of its terms in the same normalisation: the yardstick of a
summation-order difference.  For products of sums (Nsqr's N1 N2) it is the product of the factors' yardsticks.

Vectors are flat in the reference layout, index = site * Ltau + tau, site = norbits * cell + orbit, cell = l1 + L1 (l2 + L2 l3).
"""
import numpy as np

GLOBAL_KEYS = ("density", "Nsqr", "mu")
ONSITE_KEYS = ("density", "double_occ", "x", "x2", "x4", "phonon_pe", "phonon_ke", "elph_energy", "mu")
CORRS = ("Greens", "DenDen", "SpinSpin", "PairGreens", "PhononGreens")


def cell_sum_table(L1, L2, L3):
    """idx[dc, c] = cell of (l(c) + l(dc)) with periodic wrap; neg[c] = cell of -l(c)."""
    nc = L1 * L2 * L3
    c = np.arange(nc)
    l1, l2, l3 = c % L1, (c // L1) % L2, c // (L1 * L2)
    idx = ((l1[None, :] + l1[:, None]) % L1) + L1 * (((l2[None, :] + l2[:, None]) % L2) + L2 * ((l3[None, :] + l3[:, None]) % L3))
    neg = ((-l1) % L1) + L1 * (((-l2) % L2) + L2 * ((-l3) % L3))
    return idx, neg


def _field(v, L, ns, nc):
    """flat reference-layout vector -> [tau, orbit, cell]"""
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(nc, ns, L).transpose(2, 1, 0))


def translation_average(a, b, idx):
    """out[dt, s2, s1, dc] = 1/(T nc) sum_{t, c} a[t + dt, s2, c + dc] * b[t, s1, c] for a, b of shape [T, ns, nc] (periodic in T):
    the sum over t is a product of the rolled array with b, the sum over c a gather along the table of cell sums."""
    T, ns, nc = a.shape
    out = np.zeros((T, ns, ns, nc))
    cols = np.arange(nc)[None, :]
    bm = b.reshape(T, ns * nc)
    for dt in range(T):
        ar = np.roll(a, -dt, axis=0).reshape(T, ns * nc)                    # ar[t] = a[t + dt]
        K = (ar.T @ bm).reshape(ns, nc, ns, nc)                             # K[s2, c', s1, c] = sum_t a[t + dt, s2, c'] b[t, s1, c]
        out[dt] = K[:, idx, :, cols].sum(axis=1).transpose(1, 2, 0)         # [dc, c, s2, s1] summed over c
    return out / (T * nc)


def setup_tables(r1, x1, r2, x2, L, ns, dims):
    """The four tables of setup!(estimator, n1, n2) (GreensFunctions.jl:239-288) as real arrays [2L, s2, s1, cell]; r = noise vector,
    x = M^-1 r.  Order: GD0, GD0_GD0, GDD_G00, GD0_G0D."""
    nc = dims[0] * dims[1] * dims[2]
    idx, _ = cell_sum_table(*dims)
    R1, X1, R2, X2 = (_field(v, L, ns, nc) for v in (r1, x1, r2, x2))
    anti = lambda v: np.concatenate([v, -v], axis=0)  # noqa: E731
    peri = lambda v: np.concatenate([v, v], axis=0)  # noqa: E731
    s2 = np.sqrt(2.0)
    return [translation_average(anti((X1 + X2) / s2), anti((R1 + R2) / s2), idx),
            translation_average(peri(X1 * X2), peri(R1 * R2), idx),
            translation_average(peri(X2 * R2), peri(X1 * R1), idx),
            translation_average(peri(X1 * R2), peri(X2 * R1), idx)]


def fold_correlation(name, T, o1, o2, L, L0, dims):
    """measure_<name>(model, Gr, l, o1, o2, tau) (Measurements.jl:1469-1552) for tau = 0..L0-1 and every cell -> [L0, nc]; o1, o2 1-based.
    T: the four tables; measure_X(l, o1, o2, tau) = X[mod1(tau + 1, 2L), o2, o1, l] (GreensFunctions.jl:293-329)."""
    nc = dims[0] * dims[1] * dims[2]
    _, neg = cell_sum_table(*dims)
    GD0, GD0_GD0, GDD_G00, GD0_G0D = T
    a, b = o2 - 1, o1 - 1
    delta = np.zeros(nc)
    delta[0] = 1.0 if o1 == o2 else 0.0
    out = np.zeros((L0, nc))
    for tau in range(L0):
        tm = tau % L
        if name == "Greens":
            g = GD0[tm, a, b, :]
            out[tau] = delta - g if tau == L else g
        elif name == "DenDen":
            G00, Grr = GD0[0, b, b, 0], GD0[0, a, a, 0]
            out[tau] = 4.0 * (1.0 - Grr - G00 + GDD_G00[tm, a, b, :] + 0.5 * (delta * (tm == 0) * GD0[tm, a, b, :] - GD0_G0D[tm, a, b, :]))
        elif name == "SpinSpin":
            if tau == L:                                                    # tau = 0, orbitals swapped, l -> -l
                dswap = np.zeros(nc)
                dswap[0] = 1.0 if o1 == o2 else 0.0
                out[tau] = (-2 * GD0_G0D[0, b, a, :] + 2 * dswap * GD0[0, b, a, :])[neg]
            else:
                out[tau] = -2 * GD0_G0D[tau, a, b, :] + 2 * delta * (tau == 0) * GD0[tau, a, b, :]
        elif name == "PairGreens":
            if tau == L:
                out[tau] = GD0_GD0[0, a, b, :] + delta * (1.0 - 2 * GD0[0, b, b, 0])
            else:
                out[tau] = GD0_GD0[tau, a, b, :]
        else:
            raise KeyError(name)
    return out


def phonon_greens(x, o1, o2, L, L0, ns, dims):
    """measure_PhononGreens! (Measurements.jl:1598-1650): translational_average!(x_o1, x_o2) = 1/(L nc) sum x_o1[. + D] x_o2[.]; slice L = slice 0."""
    nc = dims[0] * dims[1] * dims[2]
    idx, _ = cell_sum_table(*dims)
    X = _field(x, L, ns, nc)
    ta = translation_average(X[:, o1 - 1:o1, :], X[:, o2 - 1:o2, :], idx)[:, 0, 0, :]      # [L, nc]
    return ta[np.arange(L0) % L]


def measure(R, MinvR, x, par, request, tables=None, phonon=None):
    """Everything make_measurements! adds for the vectors R, MinvR ((nv, Ndim)) and the field x, summed over all pairs i < j.

    par: L, ns, dims = (L1, L2, L3), dtau, omega, omega4, lam, mu (per site), bonds = one (s1, s2, t) triple of arrays per bond
    definition (sites 1-based).  request: {name: (L0, pairs (2, np) 1-based)} for the measured correlations.
    tables / phonon: other evaluations of setup_tables / phonon_greens (the FFT forms that pin this file in tests/test_measurements_host.py).
    Returns dict(glob, onsite, el_ke: values; abs: {key: yardstick}; corr: {name: real [L0, L1, L2, L3, np]})."""
    L, ns, dims, dtau = par["L"], par["ns"], par["dims"], par["dtau"]
    nc = dims[0] * dims[1] * dims[2]
    N = ns * nc
    nv = R.shape[0]
    om, om4, lam, mu = (np.asarray(par[k], dtype=np.float64) for k in ("omega", "omega4", "lam", "mu"))
    xx = np.asarray(x, dtype=np.float64).reshape(N, L)
    glob = {k: 0.0 for k in GLOBAL_KEYS}
    onsite = {k: np.zeros(ns) for k in ONSITE_KEYS}
    el_ke = np.zeros(len(par["bonds"]))
    ab = {"glob": {k: 0.0 for k in GLOBAL_KEYS}, "onsite": {k: np.zeros(ns) for k in ONSITE_KEYS}, "el_ke": np.zeros(len(par["bonds"]))}
    corr = {name: np.zeros((L0, nc, pairs.shape[1])) for name, (L0, pairs) in request.items()}
    norm = nc * L
    ph = {}
    if "PhononGreens" in request:
        L0, pairs = request["PhononGreens"]
        for p in range(pairs.shape[1]):
            ph[p] = (phonon or phonon_greens)(x, int(pairs[0, p]), int(pairs[1, p]), L, L0, ns, dims)
    dx = np.roll(xx, -1, axis=1) - xx

    def add(key, o, terms):
        onsite[key][o] += terms.sum() / norm
        ab["onsite"][key][o] += np.abs(terms).sum() / norm

    for i in range(nv - 1):
        for j in range(i + 1, nv):
            r1, x1, r2, x2 = R[i], MinvR[i], R[j], MinvR[j]
            G1, G2 = (x1 * r1).reshape(N, L), (x2 * r2).reshape(N, L)
            T = (tables or setup_tables)(r1, x1, r2, x2, L, ns, dims)
            # global (Measurements.jl:845-861, :1283-1312)
            Tr1, Tr2 = G1.sum() / L, G2.sum() / L
            aT1, aT2 = np.abs(G1).sum() / L, np.abs(G2).sum() / L
            N1, N2 = 2 * (N - Tr1), 2 * (N - Tr2)
            aN1, aN2 = 2 * (N + aT1), 2 * (N + aT2)
            glob["density"] += (N1 + N2) / (2 * N)
            ab["glob"]["density"] += (aN1 + aN2) / (2 * N)
            g0 = T[3][0]
            glob["Nsqr"] += N1 * N2 + Tr1 + Tr2 - 2 * (N / ns) * g0.sum()
            ab["glob"]["Nsqr"] += aN1 * aN2 + aT1 + aT2 + 2 * (N / ns) * np.abs(g0).sum()
            glob["mu"] += mu.mean()
            ab["glob"]["mu"] += np.abs(mu).mean()
            # on-site (:916-976)
            for o in range(ns):
                s = slice(o, N, ns)
                g1, g2, xo = G1[s], G2[s], xx[s]
                add("density", o, (1.0 - g1) + (1.0 - g2))
                add("double_occ", o, (1.0 - g1) * (1.0 - g2))
                add("phonon_ke", o, 0.5 / dtau - dx[s] ** 2 / dtau ** 2 / 2)
                add("phonon_pe", o, om[s, None] ** 2 * xo ** 2 / 2 + om4[s, None] * xo ** 4)
                add("elph_energy", o, lam[s, None] * xo * (2.0 - g1 - g2))
                add("x", o, xo)
                add("x2", o, xo ** 2)
                add("x4", o, xo ** 4)
                add("mu", o, np.repeat(mu[s, None], L, axis=1))
            # inter-site (:1029-1070)
            X1, R1, X2, R2 = (v.reshape(N, L) for v in (x1, r1, x2, r2))
            for d, (s1, s2, t) in enumerate(par["bonds"]):
                s1, s2 = np.asarray(s1) - 1, np.asarray(s2) - 1
                terms = np.asarray(t)[:, None] * np.stack([X1[s1] * R1[s2], X1[s2] * R1[s1], X2[s1] * R2[s2], X2[s2] * R2[s1]])
                el_ke[d] += terms.sum() / norm
                ab["el_ke"][d] += np.abs(terms).sum() / norm
            # correlations (:1469-1650)
            for name, (L0, pairs) in request.items():
                for p in range(pairs.shape[1]):
                    if name == "PhononGreens":
                        corr[name][:, :, p] += ph[p]
                    else:
                        corr[name][:, :, p] += fold_correlation(name, T, int(pairs[0, p]), int(pairs[1, p]), L, L0, dims)
    shaped = {name: a.reshape((a.shape[0],) + tuple(dims) + (a.shape[2],), order="F") for name, a in corr.items()}
    return dict(glob=glob, onsite=onsite, el_ke=el_ke, abs=ab, corr=shaped)


def momentum(position):
    """fourier_transform_correlations! (Measurements.jl:1160-1170): fft over the three cell axes."""
    return np.fft.fftn(position, axes=(1, 2, 3))


def simpson(f, dx):
    """Utilities.jl:65-76 along the first axis."""
    n = f.shape[0]
    F = 0.0 * f[0]
    for i in range(2, n, 2):                                                # 1-based i = 2, 4, ... <= n - 1
        F = F + dx * (f[i - 2] / 3 + 4 * f[i - 1] / 3 + f[i] / 3)
    if n % 2 == 0:
        F = F + dx * (5 * f[n - 1] / 12 + 2 * f[n - 2] / 3 - f[n - 3] / 12)
    return F
