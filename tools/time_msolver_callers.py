"""Time of the callers of the solve under each solver kind: one HMC update (Nt = 20 leapfrog steps, 22 force / action evaluations) and one
update of the Green's-function estimator (n_v = 10 noise vectors per chain), by CG on MtM with the symmetric KPM preconditioner and by
BiCGStab and GMRES(20) on Mt and M with the LeftRight one.  Config C (16 x 16, L = 160), tol = 1e-5, expansion n = 20, buf = 0.05,
c1 = c2 = 1, at 1 / 16 / 64 chains in lockstep (`time_msolver_callers.py [chain counts, default 1,16,64] [repetitions, default 5]`).
One process; every call synchronises before it returns; medians after one warm-up.  The fields start from the configuration's own field
(chain c: synth.phonon_field(seed = 900 + c)) and the random numbers of repetition r are the same for every kind; every repetition of the
HMC update starts from that same state (the state is pushed again; the push is not timed).
Also the pair solve alone (elph_bench_msolve_pair: the 2 x chains right-hand sides the last evaluation left on the device) with and
without the zero-guess start of its stages — the same bits, one mat-vec per stage apart."""
import ctypes as C
import os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
from elphdynamics_amd import _lib, configs, greens, hmc, models, preconditioners as prec, synth
chains = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
TOL, NT, DT, NV = 1e-5, 20, 0.01, 10
KINDS = (("CG", -1), ("BiCGStab", -1), ("GMRES", 20))
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731


def make(kind, restart, nch):
    m = configs.make_model("C", tol=TOL)
    m.solver, m.mul_by_M = models.make_solver(kind, m.Ndim, TOL, 10000, restart)
    fa = prec.FourierAccelerator(m)
    prec.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
    H = hmc.HybridMonteCarlo(m, fa, DT, NT * DT, alpha=0.0, Nb=1, nchains=nch)
    P = (prec.LeftRightKPMPreconditioner if m.mul_by_M else prec.SymmetricKPMPreconditioner)(m, n=20, buf=0.05, c1=1.0, c2=1.0)
    return m, fa, H, P


def randoms(m, nch, rep):
    s = 7000 + 10 * rep
    r = dict(R=synth.randn(s, nch * m.Ndof).reshape(nch, -1), Rp=synth.randn(s + 1, nch * m.Ndim).reshape(nch, -1),
             Rm=synth.randn(s + 2, nch * m.Ndim).reshape(nch, -1),
             kpm_randn=synth.randn(s + 3, (NT + 2) * 2 * nch * m.Nsites).reshape(NT + 2, 2, nch, m.Nsites), u=np.zeros(nch))
    if nch == 1:
        r = {k: (v[0] if k != "kpm_randn" else np.ascontiguousarray(v[:, :, 0, :])) for k, v in r.items()}
        r["u"] = 0.0
    return r


for nch in chains:
    print(f"{nch} chain{'s' if nch > 1 else ''}:")
    for kind, restart in KINDS:
        m, fa, H, P = make(kind, restart, nch)
        X0 = np.stack([m.x.copy() if c == 0 else synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=900 + c) for c in range(nch)])
        T, its, flags = [], None, None
        for rep in range(reps + 1):          # the first repetition warms up (allocations, first launches) and is not reported
            if nch > 1:
                H.X[:], H.V[:] = X0, 0.0
            else:
                m.x[:], H.v[:] = X0[0], 0.0
            H.push_()
            rnd = randoms(m, nch, 0)
            t0 = time.perf_counter()
            if nch > 1:
                acc, its = hmc.update_chains_(m, H, fa, P, randoms=rnd)
                flags = H.flags
            else:
                acc, its = hmc.update_(m, H, fa, P, randoms=rnd, pull=False)
                flags = np.array([H.flag])
            if rep:
                T.append(time.perf_counter() - t0)
        assert not np.any(flags), flags
        line = [f"  {kind}{'(20)' if restart > 0 else ''}: HMC update {med(T):.1f} ms [min {1e3 * min(T):.1f}], iterations per evaluation {float(np.max(its)):.1f};"]
        if m.mul_by_M:                       # the pair solve alone on what the last evaluation left in work.b
            for zero in (1, 0):
                Tz, ms, it4 = [], C.c_double(), np.zeros(4 * nch, dtype=np.int64)
                for rep in range(reps + 1):
                    _lib.check(m._lib.elph_bench_msolve_pair(m._h, 2 * nch, 1, zero, 1, C.byref(ms), _lib.iptr(it4)))
                    if rep:
                        Tz.append(ms.value)
                line.append(f"pair solve of {2 * nch} {'with' if zero else 'without'} the zero-guess start {float(np.median(Tz)):.2f} ms "
                            f"[min {min(Tz):.2f}] ({int(it4[:2 * nch].max())} + {int(it4[2 * nch:].max())} iterations);")
        est = greens.EstimateGreensFunction(m, NV * nch)
        R = synth.randn(7900, est.nv * m.Ndim).reshape(est.nv, m.Ndim)
        if nch > 1:
            H.pull_()
            models.update_model_chains_(m, H.X)
        T, it = [], None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            it, res, fl = greens.update_(est, m, P, R=R, rng=np.random.default_rng(11))
            if rep:
                T.append(time.perf_counter() - t0)
        assert not fl.any()
        line.append(f"estimator update of {est.nv} vectors {med(T):.1f} ms [min {1e3 * min(T):.1f}], {int(it.max())} iterations")
        print(" ".join(line))
        m.close()
