"""The yardstick of the Holstein model's CurrentCurrent (csrc/currcorr.hip), in numpy, used by tests only: two independent evaluations
of measure_CurrentCurrent!(..., model::HolsteinModel, ...) (Measurements.jl:1790-2098) as it executes.

  current_transcript   (a) the reference's text operation by operation: circshift! is np.roll, the buffer aliasing is kept (R1', R1'',
                       M^-1R1', M^-1R1'' ARE G1; R2', R2'', M^-1R2', M^-1R2'' ARE G2), translational_average! is
                       ssh_bond_reference.translational_average_ (Utilities.jl:49-60 written with np.fft).  `for tau in L_t` iterates
                       over the NUMBER L_t, so its body runs once, with tau = L_t: `last_slice_` below scales the last slice alone.
                       t is model.t reshaped to (L1, L2, L3, n_def) (:1835).  Arrays are indexed [tau, l1, l2, l3] as the reference's.
  current_direct       (b) ssh_bond_reference.current_direct, imported and not edited: direct sums over (tau, cell) from the written-out
                       formula of that module's docstring, fed the weight table tp[bond, tau] of `weights`: 1 on slices 0 .. L - 2 and
                       t[bond] on slice L - 1.

`weights(t, L, everywhere=True)` is the OTHER reading (t on every slice, what the reference's comments describe), for the test that
tells the two apart.  model.t is in definition order, bond = cell + ncells (n - 1).  Vectors are flat in the reference layout,
index = site * Ltau + tau, site = norbits * cell + orbit, cell = l1 + L1 (l2 + L2 l3)."""
import numpy as np

import ssh_bond_reference as sbref

translational_average_ = sbref.translational_average_


def weights(t, L, everywhere=False):
    """tp[bond, tau]: the hopping that weights a factor of bond `bond` on slice tau, as the reference executes it (or, everywhere=True,
    as its comments read)."""
    t = np.asarray(t, dtype=np.float64)
    tp = np.ones((t.shape[0], L))
    if everywhere:
        tp[:] = t[:, None]
    else:
        tp[:, L - 1] = t
    return tp


def current_direct(r1, x1, r2, x2, t, L, ns, dims, defs, L0, pairs, everywhere=False):
    """(b): the direct sums with the last-slice weight table."""
    return sbref.current_direct(r1, x1, r2, x2, weights(t, L, everywhere), L, ns, dims, defs, L0, pairs)


def current_transcript(r1, x1, r2, x2, t0, L, ns, dims, defs, L0, pairs):
    """(a): one call of measure_CurrentCurrent! (:1790-2098) on a zeroed container: complex (L0, L1, L2, L3, n_p)."""
    L1, L2, L3 = dims
    nv = len(defs)
    shaped = lambda v: np.asarray(v, dtype=np.complex128).reshape(L3, L2, L1, ns, L).transpose(4, 3, 2, 1, 0)  # noqa: E731  (L, n_o, L1, L2, L3)
    r1, Mr1, r2, Mr2 = shaped(r1), shaped(x1), shaped(r2), shaped(x2)       # :1803-1806
    crntcrnt, G1G2, G1, G2 = (np.zeros((L, L1, L2, L3), dtype=np.complex128) for _ in range(4))     # :1809-1812
    t0 = np.asarray(t0, dtype=np.float64)
    if t0.shape[0] != L1 * L2 * L3 * nv:
        raise ValueError("DimensionMismatch: t of %d bonds cannot be reshaped to (%d, %d, %d, %d)" % (t0.shape[0], L1, L2, L3, nv))
    t = t0.reshape(nv, L3, L2, L1).transpose(3, 2, 1, 0)                    # :1835  (L1, L2, L3, n_v), first index fastest
    container = np.zeros((L0, L1, L2, L3, pairs.shape[1]), dtype=np.complex128)

    def circshift_(dest, src, shifts):
        dest[...] = np.roll(src, shifts, axis=(0, 1, 2, 3))

    def last_slice_(Ga, ta, Gb, tb):
        """@views for tau in L_t; @. Ga[tau,:,:,:] *= ta; @. Gb[tau,:,:,:] *= tb; end -- the one iteration, tau = L_t"""
        for tau in (L,):
            Ga[tau - 1] *= ta
            Gb[tau - 1] *= tb

    for p in range(pairs.shape[1]):
        crntcrnt[...] = 0.0                                                 # :1841
        n1 = pairs[1, p]                                                    # n'
        n2 = pairs[0, p]                                                    # n''
        d, c, rpp = defs[n2 - 1]
        t2 = t[..., n2 - 1]
        b, a, rp = defs[n1 - 1]
        t1 = t[..., n1 - 1]
        sp, spp = (0, -rp[0], -rp[1], -rp[2]), (0, -rpp[0], -rpp[1], -rpp[2])
        o = lambda arr, k: arr[:, k - 1]  # noqa: E731
        # :1860-1875
        MR1, R1, MR2, R2 = o(Mr1, b), o(r1, a), o(Mr2, c), o(r2, d)
        circshift_(G1, R1, sp)
        circshift_(G2, MR2, spp)
        G1[...] = MR1 * G1
        G2[...] = G2 * R2
        last_slice_(G1, t1, G2, t2)
        translational_average_(G1G2, G1, G2)
        crntcrnt += 4 * G1G2
        # :1878-1893
        MR1, R1, MR2, R2 = o(Mr1, b), o(r1, a), o(Mr2, d), o(r2, c)
        circshift_(G1, R1, sp)
        circshift_(G2, R2, spp)
        G1[...] = MR1 * G1
        G2[...] = MR2 * G2
        last_slice_(G1, t1, G2, t2)
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 4 * G1G2
        # :1896-1911
        MR1, R1, MR2, R2 = o(Mr1, a), o(r1, b), o(Mr2, c), o(r2, d)
        circshift_(G1, MR1, sp)
        circshift_(G2, MR2, spp)
        G1[...] = G1 * R1
        G2[...] = G2 * R2
        last_slice_(G1, t1, G2, t2)
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 4 * G1G2
        # :1914-1929 (the comment says J +=; the statement subtracts)
        MR1, R1, MR2, R2 = o(Mr1, a), o(r1, b), o(Mr2, d), o(r2, c)
        circshift_(G1, MR1, sp)
        circshift_(G2, R2, spp)
        G1[...] = G1 * R1
        G2[...] = MR2 * G2
        last_slice_(G1, t1, G2, t2)
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 4 * G1G2
        # :1932-1947
        MR1, R1, MR2, R2 = o(Mr1, b), o(r1, d), o(Mr2, c), o(r2, a)
        circshift_(G2, MR2, spp)
        circshift_(G1, R2, sp)
        G1[...] = MR1 * G1
        G2[...] = G2 * R1
        last_slice_(G1, t1, G2, t2)
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 2 * G1G2
        # :1950-1965 (G1 carries the n'' field and t'', G2 the n' field and t')
        MR1, R1, MR2, R2 = o(Mr1, b), o(r1, c), o(Mr2, d), o(r2, a)
        circshift_(G1, R1, spp)
        circshift_(G2, R2, sp)
        G1[...] = G1 * MR2
        G2[...] = MR1 * G2
        last_slice_(G1, t2, G2, t1)
        translational_average_(G1G2, G1, G2)
        crntcrnt += 2 * G1G2
        # :1968-1983
        MR1, R1, MR2, R2 = o(Mr1, a), o(r1, d), o(Mr2, c), o(r2, b)
        circshift_(G1, MR1, sp)
        circshift_(G2, MR2, spp)
        G1[...] = G1 * R2
        G2[...] = R1 * G2
        last_slice_(G1, t1, G2, t2)
        translational_average_(G1G2, G1, G2)
        crntcrnt += 2 * G1G2
        # :1986-2001
        MR1, R1, MR2, R2 = o(Mr1, a), o(r1, c), o(Mr2, d), o(r2, b)
        circshift_(G1, MR1, sp)
        circshift_(G2, R1, spp)
        G1[...] = G1 * R2
        G2[...] = G2 * MR2
        last_slice_(G1, t1, G2, t2)
        translational_average_(G1G2, G1, G2)
        crntcrnt -= 2 * G1G2
        # :2004-2021
        if a == c:
            l1, l2, l3 = (rpp[0] - rp[0]) % L1, (rpp[1] - rp[1]) % L2, (rpp[2] - rp[2]) % L3
            MR1, R1 = o(Mr1, b), o(r1, d)
            G1[...] = MR1
            G2[...] = R1
            last_slice_(G1, t1, G2, t2)
            circshift_(G1G2, G1, (0, l1, l2, l3))
            G1G2 *= G2
            crntcrnt[0, l1, l2, l3] += 2 * G1G2.sum() / G1G2.size
        # :2024-2041
        if a == d:
            l1, l2, l3 = (-rp[0]) % L1, (-rp[1]) % L2, (-rp[2]) % L3
            MR1, R1 = o(Mr1, b), o(r1, c)
            G1[...] = MR1
            circshift_(G2, R1, spp)
            last_slice_(G1, t1, G2, t2)
            circshift_(G1G2, G1, (0, l1, l2, l3))
            G1G2 *= G2
            crntcrnt[0, l1, l2, l3] -= 2 * G1G2.sum() / G1G2.size
        # :2044-2061 (reads M^-1 r1[:, b]; l = r'' is reduced mod L here, the reference's index throws otherwise)
        if b == c:
            l1, l2, l3 = rpp[0], rpp[1], rpp[2]
            MR1, R1 = o(Mr1, b), o(r1, d)
            circshift_(G1, MR1, sp)
            G2[...] = R1
            last_slice_(G1, t1, G2, t2)
            circshift_(G1G2, G1, (0, l1, l2, l3))
            G1G2 *= G2
            crntcrnt[0, l1 % L1, l2 % L2, l3 % L3] -= 2 * G1G2.sum() / G1G2.size
        # :2064-2075
        if b == d:
            MR1, R1 = o(Mr1, a), o(r1, c)
            circshift_(G1, MR1, sp)
            circshift_(G2, R1, spp)
            last_slice_(G1, t1, G2, t2)
            G1G2[...] = G1 * G2
            crntcrnt[0, 0, 0, 0] += 2 * G1G2.sum() / G1G2.size
        # :2078-2094
        if L0 == 1:
            container[:, :, :, :, p] += crntcrnt[0:1]
        else:
            container[0:L, :, :, :, p] += crntcrnt
            for l3 in range(L3):
                for l2 in range(L2):
                    for l1 in range(L1):
                        container[L, l1, l2, l3, p] += crntcrnt[0, (-l1) % L1, (-l2) % L2, (-l3) % L3]
    return container


def measure(R, MinvR, t, L, ns, dims, defs, L0, pairs, one=current_direct):
    """CurrentCurrent summed over all pairs i < j of the vectors R, MinvR ((nv, Ndim)): real [L0, L1, L2, L3, np], Fortran order."""
    nv = R.shape[0]
    tot = 0.0
    for i in range(nv - 1):
        for j in range(i + 1, nv):
            got = one(R[i], MinvR[i], R[j], MinvR[j], t, L, ns, dims, defs, L0, pairs)
            if np.iscomplexobj(got):
                assert np.abs(got.imag).max() <= 1e-13 * max(1.0, np.abs(got.real).max())
                got = got.real
            tot = tot + got
    return np.asfortranarray(tot)
