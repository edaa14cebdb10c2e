"""Inputs and runs shared by tests/test_gpu_wg_t4_chain.py and tools/record_wg_t4_bits.py: the 4-slice shape of the workgroup-resident CG
kernel (csrc/cg_wg.hip, ELPH_WG_T=4) on config C, from x0 = 0 and from a non-zero initial guess, for a fixed number of iterations.

  * x0 = 0: elph_bench_prepare / elph_bench_run(what = 9) / elph_bench_get_x — the instantiation that does not read x0 (the benchmark's).
  * the non-zero guess: the measurement hooks know no initial guess (elph_bench_prepare zeroes x), so every right-hand side takes ITERS
    iterations of elph_cg_solve with maxiter = ITERS and a tolerance that is never reached — the instantiation that reads x0.
Both leave x after exactly ITERS iterations; digest() is what tests/golden/wg_t4_bits.json records of it."""
import ctypes as C
import hashlib

import numpy as np

NRHS, ITERS = 3, 25
GUESS_SEED, GUESS_SCALE = 9100, 0.3
NSAMPLES = 12


def guess(ndim, n):
    """The non-zero initial guess of right-hand sides 0 .. n-1."""
    from elphdynamics_amd import synth
    return np.stack([GUESS_SCALE * synth.randn(GUESS_SEED + i, ndim) for i in range(n)])


def wg_shape(m, nrhs):
    from elphdynamics_amd import _lib
    us, T, W, G = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().elph_bench_wg_info(m._h, nrhs, C.byref(us), C.byref(T), C.byref(W), C.byref(G)))
    return us.value, T.value, W.value, G.value


def wg_fallbacks(m):
    from elphdynamics_amd import _lib
    cd, fb = C.c_int(), C.c_int64()
    _lib.check(_lib.load().elph_wg_status(m._h, C.byref(cd), C.byref(fb)))
    return cd.value, fb.value


def fixed_iterations_from_zero(m, B, iters=ITERS):
    """x of every row of B after `iters` iterations of the resident kernel from x0 = 0 (the measurement hooks)."""
    from elphdynamics_amd import _lib
    lib = _lib.load()
    Bc = np.ascontiguousarray(B)
    ms = C.c_double()
    _lib.check(lib.elph_bench_prepare(m._h, 1, Bc.shape[0], _lib.dptr(Bc)))
    _lib.check(lib.elph_bench_run(m._h, 9, Bc.shape[0], iters, 0, C.byref(ms)))
    X = np.empty_like(Bc)
    _lib.check(lib.elph_bench_get_x(m._h, Bc.shape[0], _lib.dptr(X)))
    return X


def resident_plan(m, nrhs):
    """The launch record (cg_wg.hip: WgPlan, through the device-free probe) a solve of nrhs right-hand sides on this model reads under the
    switches now in the environment: elph_wg_cg launches the resident kernel exactly when it says `resident` — its only other ways out
    are a preconditioned solve and a handle cooling down after a time-out (wg_fallbacks)."""
    from elphdynamics_amd import _lib
    return _lib.wg_plan(m.kind, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, nrhs=nrhs)


def fixed_iterations_from_guess(m, B, X0, iters=ITERS):
    """x of every row of B after `iters` iterations of the resident kernel from the rows of X0 (one solve per row, stopped by maxiter).
    That the solves run in the resident kernel and not in the two-kernel iteration is asserted on the plan every launch reads: the cost
    rule takes the resident kernel for one right-hand side, at 4 slices per wave, and the launch table holds that kernel; no solve may
    leave the handle cooling down."""
    from elphdynamics_amd import models
    plan = resident_plan(m, 1)
    assert (plan["resident"], plan["has_kernel"], plan["T"]) == (1, 1, 4), plan
    assert wg_fallbacks(m) == (0, 0)
    X = np.array(X0, dtype=np.float64, order="C")
    for i in range(B.shape[0]):
        it = models.solve_(X[i], m, np.ascontiguousarray(B[i]), maxiter=iters, tol=1e-300)
        assert it == iters, (i, it)
        assert wg_fallbacks(m) == (0, 0), i
    return X


def digest(X):
    """What the fixture keeps of a block x: the SHA-256 of its bytes and a dozen evenly spaced values as hex floats."""
    flat = np.ascontiguousarray(X, dtype=np.float64).ravel()
    idx = np.linspace(0, flat.size - 1, NSAMPLES).astype(np.int64)
    return {"sha256": hashlib.sha256(flat.tobytes()).hexdigest(), "samples": [[int(i), float(flat[i]).hex()] for i in idx]}
