"""The cases of tests/test_msolver_sizes_host.py (CPU) and tests/test_gpu_msolver_sizes.py (GPU): BiCGStab, GMRES and the one-sided KPM apply
on the smallest lattices that reach each launch class of that route.

Two launches pick their shape by size.  The solver kernels of msolve.hip run one workgroup per right-hand side with a wave per 256 unknowns,
1 ... 16 waves (ms_block), and every scalar of a solve is a sum over those waves.  The one-sided Chebyshev kernel k_kpm_cheb_side<NPL,
TRANSPOSED> runs cbs = 64 ... 1024 threads (a thread per bond of the largest colour), NPL = ceil(N / cbs) = 1 ... 6 sites per thread, and
keeps the bond program in LDS where it fits next to the slab (lds_tables); beyond 6 sites per thread the launcher refuses the lattice.
LATTICES lists, per configuration, what the launchers must choose there — computed on the host from
kpm_bounds_reference.colour_runs and the launchers' arithmetic (launch_shape() below; the host test holds the table to it), and asserted on
the device against the library's own probe (_lib.kpm_side_info), so that a changed colouring or crossover cannot turn a case into another
class unnoticed.
"""
import numpy as np

from elphdynamics_amd import lattice as lat
from kpm_bounds_reference import LOCAL_CONFIGS, colour_runs, config_row

# The lattices on their short time axes, written like the rows of elphdynamics_amd.configs.CONFIGS (kind, orbitals, Lspatial, bonds, beta,
# dtau) and with the same parameters and fields; s (6 x 6, 20 slices) and l64 (64 x 64, 4 slices) are rows of that table.  They live here, not
# there: the tables of tests/test_lattice_shape.py and tests/test_wg_plan.py hold a recorded row per configuration of the package.
LOCAL_CONFIGS.update({
    "q8": ("holstein", 1, 10, lat.SQUARE_BONDS, 0.8, 0.1),
    "y8": ("holstein", 2, 6, lat.HONEYCOMB_BONDS, 0.8, 0.1),
    "t13": ("holstein", 1, 13, lat.TRIANGULAR_BONDS, 0.8, 0.1),
    "e12s": ("ssh", 1, 12, lat.SQUARE_BONDS, 0.4, 0.05),
    "S9": ("holstein", 1, 12, lat.SQUARE_BONDS, 0.9, 0.1),
    "C8": ("holstein", 1, 16, lat.SQUARE_BONDS, 0.8, 0.1),
    "m36": ("holstein", 1, 36, lat.SQUARE_BONDS, 0.4, 0.1),
    "m48": ("holstein", 1, 48, lat.SQUARE_BONDS, 0.4, 0.1),
    "m70": ("holstein", 1, 70, lat.SQUARE_BONDS, 0.4, 0.1),
    "m72": ("holstein", 1, 72, lat.SQUARE_BONDS, 0.4, 0.1),
    "m80": ("holstein", 1, 80, lat.SQUARE_BONDS, 0.4, 0.1),
    "b300": ("holstein", 1, 4, lat.SQUARE_BONDS, 30.0, 0.1),
})
row = config_row         # tag -> the row configs.make_model() takes

# tag -> (N, Ltau, waves of ms_block, cbs, NPL, lds_tables); NPL 7: refused (cbs, lds_tables as the probe still reports them)
LATTICES = {
    "s":    (36, 20, 3, 64, 1, 1),            # square 6 x 6
    "q8":   (100, 8, 4, 64, 2, 1),            # square 10 x 10
    "y8":   (72, 8, 3, 64, 2, 1),             # honeycomb 6 x 6 cells
    "t13":  (169, 8, 6, 128, 2, 1),           # triangular 13 x 13: 8 ragged colours
    "e12s": (144, 8, 5, 128, 2, 1),           # bond phonons, square 12 x 12
    "S9":   (144, 9, 6, 128, 2, 1),           # square 12 x 12 on an odd time axis (the direct transform)
    "C8":   (256, 8, 8, 128, 2, 1),           # square 16 x 16
    "m36":  (1296, 4, 16, 704, 2, 0),         # square 36 x 36
    "m48":  (2304, 4, 16, 1024, 3, 0),
    "l64":  (4096, 4, 16, 1024, 4, 0),
    "m70":  (4900, 4, 16, 1024, 5, 0),
    "m72":  (5184, 4, 16, 1024, 6, 0),
    "m80":  (6400, 4, 16, 1024, 7, 0),        # refused
    "b300": (16, 300, 16, 64, 1, 1),          # square 4 x 4, 300 slices: the scalar transform (no one-tile table beyond 256 slices)
}
NPL_MAX = 6
REFUSED = "m80"
APPLY_TAGS = tuple(t for t in LATTICES if t != REFUSED)
TWO_CHAIN_TAGS = ("q8", "m48")


def launch_shape(m):
    """(waves, cbs, NPL, lds_tables) of a host model by the launchers' arithmetic (kernels.hip: elph_kpm_slab_shape, msolve.hip: ms_block)."""
    N, nb = m.Nsites, len(m.neighbor_table)
    maxcol = max([hi - lo for lo, hi in colour_runs(m.neighbor_table)] + [1])
    gen = 64 if N <= 512 else min(1024, 64 * ((N // 2 + 63) // 64))
    cbs = min(1024, max(gen, 64 * ((maxcol + 63) // 64)))
    lds = int(N <= 65535 and 16 * N + 20 * nb <= 64 * 1024)
    return min(16, max(1, (m.Ndim + 255) // 256)), cbs, (N + cbs - 1) // cbs, lds


# The transform forms of the one-sided apply: (tag, vectors, form of _lib.DFT_FORMS).  The twisted pair of a batch takes the scalar kernels where
# no one-tile table exists (beyond 256 slices) and the batch is below the split's crossover, one tile per wave below the matrix-core
# crossovers, the even/odd split from 448 column-tile waves on an even axis of 8 slices or more (12 x 12: 9 column tiles x 50 vectors), and
# the direct matrix-core form where there is no split: an odd axis (S9: 9 tiles x 1 row group x 64 vectors >= 512) or fewer than 8 slices
# (m48: 144 tiles x 4 vectors).
FORM_CASES = (("b300", 3, "SCALAR"), ("e12s", 5, "ONE_TILE"), ("e12s", 50, "SPLIT_LDS"), ("S9", 64, "DIRECT"), ("m48", 4, "DIRECT"),
              ("m48", 3, "ONE_TILE"))

# Preconditioned solves from the zero guess: (tag, operator, solver, restart, tol, maxiter), tol of msolver_reference.TOLS — 1e-5, 1e-8 for
# GMRES(4) (which then crosses a restart), and the next of TOLS where a float64 summation order leaves a log-margin below MARGIN (SOLVE_TOL:
# the host test asserts the margin of the value written here for every case).
SOLVE_TAGS = ("s", "e12s", "t13", "C8", "m48", "m72")         # 3, 5, 6, 8, 16 and 16 waves
SOLVERS = (("bicgstab", 0), ("gmres", 20), ("gmres", 4))
SOLVER_MAXITER = 40
SOLVE_TOL = {}


def _tol(tag, op, solver, restart):
    return SOLVE_TOL.get((tag, op, solver, restart), 1e-8 if restart == 4 else 1e-5)


SOLVE_CASES = tuple((tag, op, solver, restart, _tol(tag, op, solver, restart), SOLVER_MAXITER)
                    for tag in SOLVE_TAGS for op in ("M", "MT") for solver, restart in SOLVERS)

# ldiv! of a batch of stop_rule_cases.BATCH guesses: (tag, operator, solver, restart), tol 1e-5, maxiter 40
BATCH_TAGS = ("C8", "m48")
BATCH_TOL = 1e-5
BATCH_CASES = tuple((tag, op, solver, restart) for tag in BATCH_TAGS for op in ("M", "MT") for solver, restart in SOLVERS)
# ... and with solver.maxiter = 20 and a call maxiter of 2 (BiCGStab: two iterations; GMRES(4): the whole first cycle, four), which no guess
# converges in: the near guess ends below sqrt(tol) and is kept (flag 0), the zero and far guesses end above it, are solved again from zero
# without the expansion, run out of those 20 iterations too and come back zeroed with flag 1.  tol = FLAG_TOL[tag] puts sqrt(tol) between the
# two groups (their residuals: 2e-5 against 1e-3 on C8, 9e-7 against 2e-4 on m48; the host test asserts the log-margin of every one).  GMRES(20)
# runs its whole first cycle whatever the call's maxiter and converges in it, so it is not among these.
FLAG_CASES = tuple((tag, op, solver, restart) for tag in BATCH_TAGS for op in ("M", "MT") for solver, restart in (("bicgstab", 0), ("gmres", 4)))
FLAG_SOLVER_MAXITER, FLAG_CALL_MAXITER = 20, 2
FLAG_TOL = {"C8": 1e-8, "m48": 1e-10}

# the bare iterations on 48 x 48: 5 steps of BiCGStab, one full cycle of GMRES(20)
BARE_TAG = "m48"


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def spread(xs):
    """The largest relative difference between any two of the vectors xs."""
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    return max(rel(a, b) for i, a in enumerate(xs) for b in xs[i + 1:])


def bound(project, spread_):
    """The project's figure where the reference's own spread over its float64 summation orders is at least 100 times smaller, else 100 x that
    spread."""
    return project if 100.0 * spread_ <= project else 100.0 * spread_
