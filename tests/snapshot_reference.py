"""A numpy restatement of the reference's three snapshot measurements (take_density_snapshot!, take_double_occupancy_snapshot!,
take_phonon_position_snapshot!, Measurements.jl:1351-1460) for the snapshot tests.  The loops over the vectors are written out with the
reference's own ranges, 1-based as there, never through a factorised form: the double occupancy runs n over 1..n_v - 1 and m over
2..n_v, which for n_v > 2 holds n = m terms and both orders of some pairs.  The loops over sites and slices are array operations.

R, MinvR: one chain's vectors, (n_v, Nsites * Ltau) in the reference's layout (tau fastest: Julia's (Ltau, Nsites, n_v) view);
x: one field, Nph * Ltau, tau fastest."""
from math import comb

import numpy as np

NAMES = ("density", "double_occupancy", "phonon_position")


def _d(R, MinvR, N, L):
    """d[n, i, tau] = 1 - MinvR[tau, i, n] R[tau, i, n]"""
    nv = R.shape[0]
    return 1.0 - np.asarray(MinvR, dtype=np.float64).reshape(nv, N, L) * np.asarray(R, dtype=np.float64).reshape(nv, N, L)


def density(R, MinvR, N, L):
    d = _d(R, MinvR, N, L)
    nv = d.shape[0]
    val = np.zeros(N)
    for tau in range(1, L + 1):
        for n in range(1, nv + 1):
            val += 2 * d[n - 1, :, tau - 1]
    return val / (nv * L)


def double_occupancy(R, MinvR, N, L):
    d = _d(R, MinvR, N, L)
    nv = d.shape[0]
    val = np.zeros(N)
    for tau in range(1, L + 1):
        for n in range(1, nv - 1 + 1):                  # for n in 1:nv-1
            for m in range(2, nv + 1):                  # for m in 2:nv
                val += d[n - 1, :, tau - 1] * d[m - 1, :, tau - 1]
    return val / (comb(nv, 2) * L)


def phonon_position(x, Nph, L):
    return np.array([np.mean(np.asarray(x, dtype=np.float64).reshape(Nph, L)[i]) for i in range(Nph)])


def snapshots(R, MinvR, x, N, Nph, L):
    """All three of one chain: name -> profile."""
    return {"density": density(R, MinvR, N, L), "double_occupancy": double_occupancy(R, MinvR, N, L), "phonon_position": phonon_position(x, Nph, L)}
