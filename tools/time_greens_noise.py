"""Time of one update of the Green's-function estimator with its noise vectors drawn on the device (est.device_rng_, one
elph_greens_update_rng: no vector crosses the bus) next to today's greens.update_ with a numpy generator, which draws n_v nchains Ndim
normals on the host, uploads them, solves, and copies M^-1 R back.  Config C (16 x 16, L = 160), tol = 1e-5, no preconditioner, n_v = 10
vectors per chain as the decks have it (`time_greens_noise.py [chain counts, default 2,16,64] [repetitions] [n_v]`).  One handle and one
estimator serve both sides (the flag est.device_rng is switched between them), the sides alternate within a repetition, every call
synchronises before it returns; medians after one warm-up.  The host path is also replayed in its three parts, each timed alone: the
draw (rng.standard_normal), upload + solve (elph_greens_update) and the copy of M^-1 R (elph_greens_get_vectors).  The solve is the same
work on both sides up to the iteration counts of different vectors, which are printed.
The generator alone is timed through the private hook elph_bench_greens_noise (HIP events around 20 launches back to back into a buffer of
the estimator's shape) in both mappings of Box-Muller pairs to threads: 0 = pair k on thread k (the HMC generator's mapping), 1 = site
fastest across the lanes (what the estimator ships for even L); 5 rounds of `repetitions` alternating measurements after one warm-up each,
the median of every round, and the spread of those medians from round to round (max - min) beside the difference of the two mappings."""
import ctypes as C
import os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
from elphdynamics_amd import configs, greens, models, synth
from elphdynamics_amd._lib import P_i64, P_int, check, dptr
counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
nv = int(sys.argv[3]) if len(sys.argv) > 3 else 10
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731
LAUNCHES, ROUNDS = 20, 5

for nch in counts:
    m = configs.make_model("C", tol=1e-5)
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=70 + c) for c in range(nch)])
    models.update_model_chains_(m, X)
    nvt = nv * nch
    est = greens.EstimateGreensFunction(m, nv=nvt)
    check(m._lib.elph_greens_set_rng(m._h, C.c_uint64(20261019)))      # (est.device_rng_ without the flag: the loop below switches it)
    rng = np.random.default_rng(nch)
    it, res, fl = np.zeros(nvt, dtype=np.int64), np.zeros(nvt), np.zeros(nvt, dtype=np.int32)
    A, B, B1, B2, B3, itA, itB = [], [], [], [], [], [], []
    for rep in range(reps + 1):         # the first repetition warms up (allocations, first launches) and is not reported
        est.device_rng = True
        t0 = time.perf_counter()
        ia, _, fa = greens.update_(est, m)
        t1 = time.perf_counter()
        est.device_rng = False
        ib, _, fb = greens.update_(est, m, rng=rng)
        t2 = time.perf_counter()
        R = rng.standard_normal((nvt, m.Ndim))
        t3 = time.perf_counter()
        check(m._lib.elph_greens_update(m._h, dptr(R), 0, it.ctypes.data_as(P_i64), dptr(res), fl.ctypes.data_as(P_int)))
        t4 = time.perf_counter()
        check(m._lib.elph_greens_get_vectors(m._h, None, dptr(est.MinvR)))
        t5 = time.perf_counter()
        assert not fa.any() and not fb.any() and not fl.any()
        if rep:
            A.append(t1 - t0); B.append(t2 - t1); B1.append(t3 - t2); B2.append(t4 - t3); B3.append(t5 - t4)
            itA.append(ia.mean()); itB.append(ib.mean())
    print(f"{nch} chains, n_v = {nv} ({nvt * m.Ndim / 1e6:.2f} M normals, {nvt * m.Ndim * 8 / 1e6:.1f} MB per direction): medians of {reps} repetitions (ms): "
          f"device-drawn update {med(A):.1f} [min {1e3 * min(A):.1f}] ({np.mean(itA):.0f} iterations per vector)  greens.update_ with a numpy rng "
          f"{med(B):.1f} [min {1e3 * min(B):.1f}] ({np.mean(itB):.0f} iterations)  its parts alone: draw {med(B1):.1f} [min {1e3 * min(B1):.1f}] + "
          f"upload and solve {med(B2):.1f} [min {1e3 * min(B2):.1f}] + copy of M^-1 R {med(B3):.2f} [min {1e3 * min(B3):.2f}]  "
          f"host-drawn / device-drawn {med(B) / med(A):.2f}")
    ms = C.c_double()
    M0, M1 = [], []                     # the median of each round, per mapping
    for rnd in range(ROUNDS):
        G = {0: [], 1: []}
        for rep in range(reps + 1):
            for mapping in (0, 1):
                check(m._lib.elph_bench_greens_noise(m._h, mapping, nvt, 7 + rep, LAUNCHES, C.byref(ms), 0, 0, None))
                if rep:
                    G[mapping].append(ms.value / LAUNCHES)
        M0.append(float(np.median(G[0]))); M1.append(float(np.median(G[1])))
    g0, g1 = float(np.median(M0)), float(np.median(M1))
    spread = max(max(M0) - min(M0), max(M1) - min(M1))
    print(f"{nch} chains: the generator alone, {nvt * m.Ndim * 8 / 1e6:.1f} MB written, {ROUNDS} rounds of {reps} x {LAUNCHES} launches, ms per launch: "
          f"pair-indexed {g0:.4f} (round medians {min(M0):.4f} .. {max(M0):.4f})  site-fastest {g1:.4f} ({min(M1):.4f} .. {max(M1):.4f})  "
          f"pair-indexed - site-fastest {g0 - g1:.4f}, round-to-round spread of the medians {spread:.4f}, ratio {g0 / g1:.2f}  "
          f"({nvt * m.Ndim * 8 / 1e9 / g1:.2f} TB/s written by the site-fastest one)")
    m.close()
