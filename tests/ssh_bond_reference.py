"""The yardstick of the SSH model's inter-site correlations (csrc/ssh_bondcorr.hip), in numpy, used by tests only.

BondBond and BondPairGreens are bond_reference.measure, unchanged: the reference's methods read model.bond_definitions alone.
CurrentCurrent (measure_CurrentCurrent!(..., model::SSHModel, ...), Measurements.jl:2100-2384) has two independent evaluations here:

  current_transcript   the reference's text operation by operation: circshift! is np.roll, the buffer aliasing is kept (R1', R1'',
                       M^-1R1', M^-1R1'' ARE G1; R2', R2'', M^-1R2', M^-1R2'' ARE G2), translational_average! is written as
                       Utilities.jl:49-60 writes it with np.fft.  Arrays are indexed [tau, l1, l2, l3] as the reference's.
  current_direct       direct sums over (tau, cell) from the written-out formula, no FFT, arrays [tau, l3, l2, l1] as bond_reference's:
      A0 = t' x1[s] sh(r1[e])   A1 = t' sh(x1[e]) r1[s]   A2 = t' sh(x2[e]) r2[s]   A3 = t' x2[s] sh(r2[e])
      A4 = t' x1[s] sh(r2[e])   A5 = t' sh(x2[e]) r1[s]   A6 = t' sh(r1[e]) x2[s]   A7 = t' sh(x1[e]) r2[s]
      J = 4 A0[n']*A2[n''] - 4 A0[n']*A3[n''] - 4 A1[n']*A2[n''] - 4 A1[n']*A3[n'']
        - 2 A4[n']*A5[n''] + 2 A6[n'']*A4[n'] + 2 A7[n']*A5[n''] - 2 A7[n']*A6[n'']
      and at tau = 0, with u = t'[n'], w = t'[n''], <.> the mean over (tau, i), sh_l(f)[i] = f[i + l]:
      a == c: + 2 <u x1[b] sh_l(w r1[d])>            at l = mod(r'' - r', L)
      a == d: - 2 <u x1[b] sh_l(w sh_r''(r1[c]))>    at l = mod(-r', L)
      b == c: - 2 <u sh_r'(x1[b]) sh_l(w r1[d])>     at l = mod(r'', L)      (the reference indexes with r'' unreduced and throws)
      b == d: + 2 <u sh_r'(x1[a]) w sh_r''(r1[c])>   at l = 0
      slice beta: J[0, -l], delta terms included.
  (x = M^-1 r; n'' = pairs[0, p] with (d, c, r'') = (o1, o2, v), n' = pairs[1, p] with (b, a, r'); s = o1, e = o2, sh = shift by v;
  f * g as in bond_reference.)

t'[tau, cell, n] is model.t' (Ltau, Nbonds) reshaped to (Ltau, L1, L2, L3, n_def): bond = cell + ncells n, t' = t - (alpha x + sign(x)
alpha2 x^2), t' = t on a bare bond; it is built from ssh_measurement_cases.ref_par.  Vectors are flat in the reference layout,
index = site * Ltau + tau, site = norbits * cell + orbit, cell = l1 + L1 (l2 + L2 l3)."""
import numpy as np

import bond_reference as bref
import ssh_measurements_reference as sref

CORRS = ("BondBond", "CurrentCurrent", "BondPairGreens")


def definitions(model):
    """(o1, o2, (v1, v2, v3)) per bond definition of an SSH model."""
    return [(int(d["o1"]), int(d["o2"]), tuple(int(k) for k in d["v"])) for d in model.bond_definitions]


def hopping(x, par):
    """model.t' as [bond, tau] in the reference's bond order (SSHModels.jl:531-533; bare bonds keep t)."""
    L = par["L"]
    xx = np.asarray(x, dtype=np.float64).reshape(-1, L)
    al, al2 = np.asarray(par["alpha"], dtype=np.float64), np.asarray(par["alpha2"], dtype=np.float64)
    rows = []
    for (_, _, t, phn) in par["bonds"]:
        t = np.asarray(t, dtype=np.float64)
        if phn is None:
            rows.append(np.repeat(t[:, None], L, axis=1))
        else:
            phn = np.asarray(phn)
            rows.append(sref.modulated_hopping(t, al[phn], al2[phn], xx[phn]))
    return np.concatenate(rows, axis=0)


def _reshape_hopping(tp, L, dims, ndef):
    nc = dims[0] * dims[1] * dims[2]
    if tp.shape[0] != ndef * nc:
        raise ValueError("DimensionMismatch: t' of %d bonds cannot be reshaped to (%d, %d, %d, %d, %d)" % ((tp.shape[0], L) + tuple(dims) + (ndef,)))
    return tp.reshape(ndef, dims[2], dims[1], dims[0], L)                   # [n, l3, l2, l1, tau]


# ---------------------------------------------------------------------------------------------- (a) the transcript

def translational_average_(fg, f, g):
    """translational_average!(fg, f, g) (Utilities.jl:49-60); f and g are left modified, as there."""
    f[...] = np.fft.fftn(f)
    g[...] = np.fft.fftn(g)
    N = f.size
    gp = fg
    gp[...] = np.roll(g, tuple(s - 1 for s in fg.shape), axis=(0, 1, 2, 3))
    gp[...] = gp[::-1, ::-1, ::-1, ::-1].copy()
    fg[...] = f * gp / N
    fg[...] = np.fft.ifftn(fg)


def current_transcript(r1, x1, r2, x2, tp, L, ns, dims, defs, L0, pairs):
    """One call of measure_CurrentCurrent! (:2100-2384) on a zeroed container: complex (L0, L1, L2, L3, n_p)."""
    L1, L2, L3 = dims
    nv = len(defs)
    shaped = lambda v: np.asarray(v, dtype=np.complex128).reshape(L3, L2, L1, ns, L).transpose(4, 3, 2, 1, 0)  # noqa: E731  (L, n_o, L1, L2, L3)
    r1, Mr1, r2, Mr2 = shaped(r1), shaped(x1), shaped(r2), shaped(x2)
    crntcrnt, G1G2, G1, G2 = (np.zeros((L, L1, L2, L3), dtype=np.complex128) for _ in range(4))
    t = _reshape_hopping(tp, L, dims, nv).transpose(4, 3, 2, 1, 0)          # (L, L1, L2, L3, n_v)
    container = np.zeros((L0, L1, L2, L3, pairs.shape[1]), dtype=np.complex128)

    def circshift_(dest, src, shifts):
        dest[...] = np.roll(src, shifts, axis=(0, 1, 2, 3))

    for p in range(pairs.shape[1]):
        crntcrnt[...] = 0.0
        n1 = pairs[1, p]
        n2 = pairs[0, p]
        b, a, rp = defs[n1 - 1]
        t1 = t[..., n1 - 1]
        d, c, rpp = defs[n2 - 1]
        t2 = t[..., n2 - 1]
        sp, spp = (0, -rp[0], -rp[1], -rp[2]), (0, -rpp[0], -rpp[1], -rpp[2])
        o = lambda arr, k: arr[:, k - 1]  # noqa: E731
        # :2170-2183
        MR1, R1, MR2, R2 = o(Mr1, b), o(r1, a), o(Mr2, c), o(r2, d)
        circshift_(G1, R1, sp)
        circshift_(G2, MR2, spp)
        G1[...] = MR1 * G1
        G2[...] = G2 * R2
        G1 *= t1
        G2 *= t2
        translational_average_(G1G2, G1, G2)
        crntcrnt += 4 * G1G2
        # :2186-2199
        MR1, R1, MR2, R2 = o(Mr1, b), o(r1, a), o(Mr2, d), o(r2, c)
        circshift_(G1, R1, sp)
        circshift_(G2, R2, spp)
        G1[...] = MR1 * G1
        G2[...] = MR2 * G2
        G1 *= t1
        G2 *= t2
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 4 * G1G2
        # :2202-2215
        MR1, R1, MR2, R2 = o(Mr1, a), o(r1, b), o(Mr2, c), o(r2, d)
        circshift_(G1, MR1, sp)
        circshift_(G2, MR2, spp)
        G1[...] = G1 * R1
        G2[...] = G2 * R2
        G1 *= t1
        G2 *= t2
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 4 * G1G2
        # :2218-2231 (the comment says J +=; the statement subtracts)
        MR1, R1, MR2, R2 = o(Mr1, a), o(r1, b), o(Mr2, d), o(r2, c)
        circshift_(G1, MR1, sp)
        circshift_(G2, R2, spp)
        G1[...] = G1 * R1
        G2[...] = MR2 * G2
        G1 *= t1
        G2 *= t2
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 4 * G1G2
        # :2234-2247
        MR1, R1, MR2, R2 = o(Mr1, b), o(r1, d), o(Mr2, c), o(r2, a)
        circshift_(G2, MR2, spp)
        circshift_(G1, R2, sp)
        G1[...] = MR1 * G1
        G2[...] = G2 * R1
        G1 *= t1
        G2 *= t2
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 2 * G1G2
        # :2250-2263 (G1 carries the n'' field and t'', G2 the n' field and t')
        MR1, R1, MR2, R2 = o(Mr1, b), o(r1, c), o(Mr2, d), o(r2, a)
        circshift_(G1, R1, spp)
        circshift_(G2, R2, sp)
        G1[...] = G1 * MR2
        G2[...] = MR1 * G2
        G1 *= t2
        G2 *= t1
        translational_average_(G1G2, G1, G2)
        crntcrnt += 2 * G1G2
        # :2266-2279
        MR1, R1, MR2, R2 = o(Mr1, a), o(r1, d), o(Mr2, c), o(r2, b)
        circshift_(G1, MR1, sp)
        circshift_(G2, MR2, spp)
        G1[...] = G1 * R2
        G2[...] = R1 * G2
        G1 *= t1
        G2 *= t2
        translational_average_(G1G2, G1, G2)
        crntcrnt += 2 * G1G2
        # :2282-2295
        MR1, R1, MR2, R2 = o(Mr1, a), o(r1, c), o(Mr2, d), o(r2, b)
        circshift_(G1, MR1, sp)
        circshift_(G2, R1, spp)
        G1[...] = G1 * R2
        G2[...] = G2 * MR2
        G1 *= t1
        G2 *= t2
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 2 * G1G2
        # :2298-2313
        if a == c:
            l1, l2, l3 = (rpp[0] - rp[0]) % L1, (rpp[1] - rp[1]) % L2, (rpp[2] - rp[2]) % L3
            MR1, R1 = o(Mr1, b), o(r1, d)
            G1[...] = MR1
            G2[...] = R1
            G1 *= t1
            G2 *= t2
            circshift_(G1G2, G1, (0, l1, l2, l3))
            G1G2 *= G2
            crntcrnt[0, l1, l2, l3] += 2 * G1G2.sum() / G1G2.size
        # :2316-2331
        if a == d:
            l1, l2, l3 = (-rp[0]) % L1, (-rp[1]) % L2, (-rp[2]) % L3
            MR1, R1 = o(Mr1, b), o(r1, c)
            G1[...] = MR1
            circshift_(G2, R1, spp)
            G1 *= t1
            G2 *= t2
            circshift_(G1G2, G1, (0, l1, l2, l3))
            G1G2 *= G2
            crntcrnt[0, l1, l2, l3] -= 2 * G1G2.sum() / G1G2.size
        # :2334-2349 (reads M^-1 r1[:, b]; l = r'' is reduced mod L here, the reference's index throws otherwise)
        if b == c:
            l1, l2, l3 = rpp[0], rpp[1], rpp[2]
            MR1, R1 = o(Mr1, b), o(r1, d)
            circshift_(G1, MR1, sp)
            G2[...] = R1
            G1 *= t1
            G2 *= t2
            circshift_(G1G2, G1, (0, l1, l2, l3))
            G1G2 *= G2
            crntcrnt[0, l1 % L1, l2 % L2, l3 % L3] -= 2 * G1G2.sum() / G1G2.size
        # :2352-2361
        if b == d:
            MR1, R1 = o(Mr1, a), o(r1, c)
            circshift_(G1, MR1, sp)
            circshift_(G2, R1, spp)
            G1 *= t1
            G2 *= t2
            G1G2[...] = G1 * G2
            crntcrnt[0, 0, 0, 0] += 2 * G1G2.sum() / G1G2.size
        # :2364-2380
        if L0 == 1:
            container[:, :, :, :, p] += crntcrnt[0:1]
        else:
            container[0:L, :, :, :, p] += crntcrnt
            for l3 in range(L3):
                for l2 in range(L2):
                    for l1 in range(L1):
                        container[L, l1, l2, l3, p] += crntcrnt[0, (-l1) % L1, (-l2) % L2, (-l3) % L3]
    return container


# ---------------------------------------------------------------------------------------------- (b) direct sums

def current_direct(r1, x1, r2, x2, tp, L, ns, dims, defs, L0, pairs):
    """What one pair of vectors adds to CurrentCurrent, from the module docstring's formula: real (L0, L1, L2, L3, n_p)."""
    L1, L2, L3 = dims
    R1, X1, R2, X2 = (bref.grid(v, L, ns, dims) for v in (r1, x1, r2, x2))   # [orbit][tau, l3, l2, l1]
    T = _reshape_hopping(tp, L, dims, len(defs)).transpose(0, 4, 1, 2, 3)     # [n][tau, l3, l2, l1]
    sh = bref.shift
    A = []
    for n, (s, e, v) in enumerate(defs):
        s, e, t = s - 1, e - 1, T[n]
        A.append([t * X1[s] * sh(R1[e], v), t * sh(X1[e], v) * R1[s], t * sh(X2[e], v) * R2[s], t * X2[s] * sh(R2[e], v),
                  t * X1[s] * sh(R2[e], v), t * sh(X2[e], v) * R1[s], t * sh(R1[e], v) * X2[s], t * sh(X1[e], v) * R2[s]])
    star = bref.star_direct
    res = np.zeros((L0, L3, L2, L1, pairs.shape[1]))
    for p in range(pairs.shape[1]):
        n2, n1 = pairs[0, p] - 1, pairs[1, p] - 1
        d, c, rpp = defs[n2]
        b, a, rp = defs[n1]
        F, G = A[n1], A[n2]                                                 # the fields of n', n''
        J = (4 * star(F[0], G[2]) - 4 * star(F[0], G[3]) - 4 * star(F[1], G[2]) - 4 * star(F[1], G[3])
             - 2 * star(F[4], G[5]) + 2 * star(G[6], F[4]) + 2 * star(F[7], G[5]) - 2 * star(F[7], G[6]))
        u, w = T[n1], T[n2]
        mean = lambda f: f.sum() / f.size  # noqa: E731
        at = lambda l: (0, l[2] % L3, l[1] % L2, l[0] % L1)  # noqa: E731
        if a == c:
            l = [rpp[k] - rp[k] for k in range(3)]
            J[at(l)] += 2 * mean(u * X1[b - 1] * sh(w * R1[d - 1], l))
        if a == d:
            l = [-rp[k] for k in range(3)]
            J[at(l)] -= 2 * mean(u * X1[b - 1] * sh(w * sh(R1[c - 1], rpp), l))
        if b == c:
            l = list(rpp)
            J[at(l)] -= 2 * mean(u * sh(X1[b - 1], rp) * sh(w * R1[d - 1], l))
        if b == d:
            J[0, 0, 0, 0] += 2 * mean(u * sh(X1[a - 1], rp) * w * sh(R1[c - 1], rpp))
        res[:min(L0, L), ..., p] = J[:min(L0, L)]
        if L0 > 1:
            for l3 in range(L3):
                for l2 in range(L2):
                    for l1 in range(L1):
                        res[L, l3, l2, l1, p] = J[0, (-l3) % L3, (-l2) % L2, (-l1) % L1]
    return res.transpose(0, 3, 2, 1, 4)


def measure_current(R, MinvR, x, par, defs, L0, pairs, one=current_direct):
    """CurrentCurrent summed over all pairs i < j of the vectors R, MinvR ((nv, Ndim)): real [L0, L1, L2, L3, np], Fortran order."""
    tp = hopping(x, par)
    nv = R.shape[0]
    tot = 0.0
    for i in range(nv - 1):
        for j in range(i + 1, nv):
            got = one(R[i], MinvR[i], R[j], MinvR[j], tp, par["L"], par["ns"], par["dims"], defs, L0, pairs)
            if np.iscomplexobj(got):
                assert np.abs(got.imag).max() <= 1e-13 * max(1.0, np.abs(got.real).max())
                got = got.real
            tot = tot + got
    return np.asfortranarray(tot)


def measure(R, MinvR, x, par, defs, request, one=current_direct):
    """Everything accumulate_ssh_bonds_ adds: {name: real [L0, L1, L2, L3, np]} for the requested names of CORRS.
    request: {name: (L0, pairs (2, np) 1-based bond-definition indices)}; par: ssh_measurement_cases.ref_par(model)."""
    out = {}
    both = {k: v for k, v in request.items() if k in bref.CORRS}
    if both:
        out.update(bref.measure(R, MinvR, par["L"], par["ns"], par["dims"], defs, both))
    if "CurrentCurrent" in request:
        L0, pairs = request["CurrentCurrent"]
        out["CurrentCurrent"] = measure_current(R, MinvR, x, par, defs, L0, pairs, one)
    return out
