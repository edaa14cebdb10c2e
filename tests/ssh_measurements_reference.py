"""Direct-sum restatement of the SSH branch of Measurements.jl (:845-861, :978-1024, :1072-1155, :1283-1312, :1469-1596, :2488-2541), used
by tests only.  Everything is computed from (R, MinvR, x, parameters, pairs) with explicit sums; no FFT is used (the estimator's tables
and the folds are those of tests/measurements_reference.py, the phonon translation average its translation_average).

`abs` holds for each reduced scalar the sum of the absolute values of its terms in the same normalisation, as in measurements_reference.

Vectors are flat in the reference layout, index = site * Ltau + tau; the field is x[phonon * Ltau + tau] and, for PhononGreens,
phonon = cell + ncells * type (the reference's reshape to (Ltau, L1, L2, L3, nph)).
"""
import numpy as np

import measurements_reference as mref

GLOBAL_KEYS = mref.GLOBAL_KEYS
ONSITE_KEYS = ("density", "double_occ", "mu")
INTERSITE_KEYS = ("x", "x2", "x4", "phonon_pe", "phonon_ke", "elph_energy", "el_ke", "sign_switch")
CORRS = ("Greens", "DenDen", "SpinSpin", "PairGreens", "PhononGreens")


def modulated_hopping(t, alpha, alpha2, x):
    """t' = t - (alpha x + sign(x) alpha2 x^2) (SSHModels.jl:531-533); x: [bonds, tau]."""
    return t[:, None] - (alpha[:, None] * x + np.sign(x) * alpha2[:, None] * x ** 2)


def phonon_greens(x, b1, b2, L, L0, nph, dims):
    """measure_PhononGreens!(ssh) (:2488-2541): translational_average!(x2x1, x_b2, x_b1) = 1/(L nc) sum x_b2[. + D] x_b1[.]; slice L = slice 0."""
    nc = dims[0] * dims[1] * dims[2]
    x = np.asarray(x, dtype=np.float64)
    if x.size != L * nc * nph:
        raise ValueError("DimensionMismatch: %d fields cannot be reshaped to (%d, %d, %d, %d, %d)" % ((x.size, L) + tuple(dims) + (nph,)))
    idx, _ = mref.cell_sum_table(*dims)
    X = np.ascontiguousarray(x.reshape(nph, nc, L).transpose(2, 0, 1))      # [tau, type, cell]
    ta = mref.translation_average(X[:, b2 - 1:b2, :], X[:, b1 - 1:b1, :], idx)[:, 0, 0, :]
    return ta[np.arange(L0) % L]


def measure(R, MinvR, x, par, request, tables=None, phonon=None):
    """Everything make_measurements! adds on an SSH model for the vectors R, MinvR ((nv, Ndim)) and the field x, summed over all pairs i < j.

    par: L, ns, dims, dtau, mu (per site), nph (phonon types), omega, alpha, alpha2 (per phonon), bonds = one (s1, s2, t, phonon) tuple
    of arrays per bond definition (sites 1-based; phonon: the 0-based phonon of every bond, or None for a definition of bare bonds).
    request: {name: (L0, pairs (2, np) 1-based)}.  tables / phonon: other evaluations of setup_tables / phonon_greens.
    Returns dict(glob, onsite, inter: values; abs: {group: {key: yardstick}}; corr: {name: real [L0, L1, L2, L3, np]})."""
    L, ns, dims, dtau = par["L"], par["ns"], par["dims"], par["dtau"]
    nc = dims[0] * dims[1] * dims[2]
    N = ns * nc
    nv = R.shape[0]
    mu = np.asarray(par["mu"], dtype=np.float64)
    om, al, al2 = (np.asarray(par[k], dtype=np.float64) for k in ("omega", "alpha", "alpha2"))
    ndef = len(par["bonds"])
    Nbonds = sum(len(b[0]) for b in par["bonds"])
    V = (Nbonds // ndef) * L if ndef else 1                                 # :1094
    xx = np.asarray(x, dtype=np.float64).reshape(-1, L)                     # [phonon, tau]
    glob = {k: 0.0 for k in GLOBAL_KEYS}
    onsite = {k: np.zeros(ns) for k in ONSITE_KEYS}
    inter = {k: np.zeros(ndef) for k in INTERSITE_KEYS}
    ab = {"glob": {k: 0.0 for k in GLOBAL_KEYS}, "onsite": {k: np.zeros(ns) for k in ONSITE_KEYS}, "inter": {k: np.zeros(ndef) for k in INTERSITE_KEYS}}
    corr = {name: np.zeros((L0, nc, pairs.shape[1])) for name, (L0, pairs) in request.items()}
    norm = nc * L
    ph = {}
    if "PhononGreens" in request:
        L0, pairs = request["PhononGreens"]
        for p in range(pairs.shape[1]):
            ph[p] = (phonon or phonon_greens)(x, int(pairs[0, p]), int(pairs[1, p]), L, L0, par["nph"], dims)

    def add(group, key, k, terms, n):
        {"onsite": onsite, "inter": inter}[group][key][k] += terms.sum() / n
        ab[group][key][k] += np.abs(terms).sum() / n

    for i in range(nv - 1):
        for j in range(i + 1, nv):
            r1, x1, r2, x2 = R[i], MinvR[i], R[j], MinvR[j]
            G1, G2 = (x1 * r1).reshape(N, L), (x2 * r2).reshape(N, L)
            T = (tables or mref.setup_tables)(r1, x1, r2, x2, L, ns, dims)
            # global (:845-861, :1283-1312)
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
            # on-site (:978-1024)
            for o in range(ns):
                s = slice(o, N, ns)
                g1, g2 = G1[s], G2[s]
                add("onsite", "density", o, (1.0 - g1) + (1.0 - g2), norm)
                add("onsite", "double_occ", o, (1.0 - g1) * (1.0 - g2), norm)
                add("onsite", "mu", o, np.repeat(mu[s, None], L, axis=1), norm)
            # inter-site (:1072-1155)
            X1, R1, X2, R2 = (v.reshape(N, L) for v in (x1, r1, x2, r2))
            for d, (s1, s2, t, phn) in enumerate(par["bonds"]):
                s1, s2, t = np.asarray(s1) - 1, np.asarray(s2) - 1, np.asarray(t, dtype=np.float64)
                h = -(X1[s1] * R1[s2] + X1[s2] * R1[s1] + X2[s1] * R2[s2] + X2[s2] * R2[s1])          # [bond, tau]
                tp = np.repeat(t[:, None], L, axis=1)
                if phn is not None:
                    phn = np.asarray(phn)
                    xb = xx[phn]
                    dx = np.roll(xb, -1, axis=1) - xb
                    tp = modulated_hopping(t, al[phn], al2[phn], xb)
                    add("inter", "phonon_pe", d, om[phn, None] ** 2 * xb ** 2 / 2, V)
                    add("inter", "phonon_ke", d, 0.5 / dtau - dx ** 2 / dtau ** 2 / 2, V)
                    add("inter", "elph_energy", d, al[phn, None] * h * xb, V)
                    add("inter", "x", d, xb, V)
                    add("inter", "x2", d, xb ** 2, V)
                    add("inter", "x4", d, xb ** 4, V)
                    add("inter", "sign_switch", d, (np.sign(t)[:, None] != np.sign(tp)).astype(np.float64), V)
                add("inter", "el_ke", d, -tp * h, V)
            # correlations (:1469-1596, :2488-2541)
            for name, (L0, pairs) in request.items():
                for p in range(pairs.shape[1]):
                    if name == "PhononGreens":
                        corr[name][:, :, p] += ph[p]
                    else:
                        corr[name][:, :, p] += mref.fold_correlation(name, T, int(pairs[0, p]), int(pairs[1, p]), L, L0, dims)
    shaped = {name: a.reshape((a.shape[0],) + tuple(dims) + (a.shape[2],), order="F") for name, a in corr.items()}
    return dict(glob=glob, onsite=onsite, inter=inter, abs=ab, corr=shaped)


momentum = mref.momentum
simpson = mref.simpson
