"""Time of the special updates with the moves drawn and decided on the device (draw="device": ONE elph_hmc_special_update_chains
for all moves of all chains) next to the host route of the same commit (draw="host": a numpy generator draws the sites / bonds /
phonon pairs, one elph_hmc_special_move[_chains] per move; the SSH swap of chains copies every field back before every move).
Both routes run in one process on the same handle, from the same fields (pushed again before every timed call, outside the clock),
with the handle's generator on, so that Rp, Rm, kpm_randn and u are drawn by the library on both sides and only the draw of the
columns, the per-chain launches and the host-side Metropolis test differ.  The routes alternate within a repetition; every call
synchronises before it returns; medians after one warm-up.

Cases: reflection and Holstein swap at config C (16 x 16, L = 160), SSH swap at config E; 8 moves; tol = 1e-5; without and with the
KPM preconditioner; `time_special_updates.py [chain counts, default 1,2,16,64] [repetitions] [moves] [cases, default refl,swap,ssh]`.
For the host route the part that is not the library's move is timed alone as well, replayed on the same fields: hmc.pull_() plus
the Python draw of the SSH swap (the comparison of world lines chain by chain); the integer draws of the other two."""
import os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
from elphdynamics_amd import configs, hmc, models, preconditioners as pc, synth
counts = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1, 2, 16, 64]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
moves = int(sys.argv[3]) if len(sys.argv) > 3 else 8
cases = sys.argv[4].split(",") if len(sys.argv) > 4 else ["refl", "swap", "ssh"]
med = lambda v: 1e3 * float(np.median(v))  # noqa: E731
CASES = {"refl": ("C", hmc.reflection_update_, "reflection, config C"), "swap": ("C", hmc.swap_update_, "Holstein swap, config C"),
         "ssh": ("E", hmc.swap_update_, "SSH swap, config E")}


def host_draw_alone(m, H, rng, name):
    """What the host route does per call besides the library's moves, on the fields as they stand."""
    nch = H.nchains
    t0 = time.perf_counter()
    for _ in range(moves):
        if name != "ssh":
            rng.integers(0, m.Nph if name == "refl" else m.Nbonds, size=nch)
            continue
        H.pull_()
        X = H.X if nch > 1 else m.x.reshape(1, -1)
        for c in range(nch):
            x = X[c].reshape(m.Nph, m.Ltau)
            i = int(rng.integers(0, m.Nph))
            if not np.allclose(x, x[0], rtol=1e-8, atol=0):
                j = int(rng.integers(0, m.Nph))
                while hmc._isapprox(x[i], x[j]):
                    j = int(rng.integers(0, m.Nph))
    return time.perf_counter() - t0


for name in cases:
    tag, helper, title = CASES[name]
    for nch in counts:
        m = configs.make_model(tag, tol=1e-5, maxiter=20000)
        if m.kind == models.SSH:
            m.omega4 = np.zeros(m.Nph)
            X0 = np.stack([m.x * (0.8 + 0.1 * (c % 5)) * (1.0 + 0.1 * synth.randn(700 + c, m.Ndof)) for c in range(nch)])
        else:
            X0 = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=100 + 17 * c) for c in range(nch)])
        fa = pc.FourierAccelerator(m)
        pc.update_M_(fa, m, 0.0, np.inf, 1.0, 0.1)
        H = hmc.HybridMonteCarlo(m, fa, dt=0.01, tr=0.1, alpha=0.0, Nb=1, nchains=nch)
        H.device_rng_(20261019)
        rng = np.random.default_rng(nch)

        def push():
            if nch > 1:
                H.X[:] = X0
            else:
                m.x[:] = X0[0]
            H.push_()

        for P in (None, pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)):
            A, B, D, fA, fB = [], [], [], [], []
            for rep in range(reps + 1):         # the first repetition warms up (allocations, first launches) and is not reported
                push()
                t0 = time.perf_counter()
                fa_ = helper(m, H, moves, P, draw="device")
                t1 = time.perf_counter()
                push()
                t2 = time.perf_counter()
                fb_ = helper(m, H, moves, P, rng=rng)       # (hmc.device_rng is on: only the columns come from rng)
                t3 = time.perf_counter()
                push()
                d = host_draw_alone(m, H, rng, name)
                if rep:
                    A.append(t1 - t0); B.append(t3 - t2); D.append(d); fA.append(fa_); fB.append(fb_)
            print(f"{title}, {nch} chain(s), {moves} moves, {'KPM preconditioner' if P is not None else 'no preconditioner'}: medians of {reps} "
                  f"repetitions (ms per call): draw on the device {med(A):.1f} [min {1e3 * min(A):.1f}]  draw on the host {med(B):.1f} "
                  f"[min {1e3 * min(B):.1f}]  of which pull_ + Python draw alone {med(D):.2f} ({100 * med(D) / med(B):.1f} %)  "
                  f"host / device {med(B) / med(A):.2f}  accepted {np.mean(fA):.2f} / {np.mean(fB):.2f}  "
                  f"(fields: {X0.nbytes / 1e6:.1f} MB, copied back per move by the host route of the SSH swap only)", flush=True)
        m.close()
