"""The 2 x 2 x 2 patch kernels of a simple-cubic Holstein lattice (pgrid::Cu) against the kernels the lattice had before them (ELPH_NO_PG=1,
read per call), in ONE process on one handle:  time_cubic.py L [nrhs ...]   (L = 6, 8, 10, 12; Ltau = 40; default batches 1 16 64)
Per batch: the preconditioned CG iteration (elph_bench_run unit 3) and the MtM mat-vec (unit 0), each the median of 5 windows per form, the two
forms alternating window by window after a warm-up of both; then a solve of the batch in both forms (iteration counts, largest difference)."""
import sys, os, ctypes as C
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from elphdynamics_amd import lattice as lat, models, preconditioners as pc, synth
from elphdynamics_amd._lib import check, dptr
L, Lt = int(sys.argv[1]), 40
m = models.HolsteinModel(lat.Lattice(1, L, L, L), Lt * 0.1, 0.1, tol=1e-5, maxiter=20000)
for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
    m.assign_t_(1.0, 1, 1, d)
m.assign_omega_(1.0); m.assign_lambda_(1.0); m.assign_mu_(0.0)
m.initialize_model_()
m.x[:] = synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau)
models.update_model_(m)
P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
pc.setup_(P, rng=np.random.default_rng(1))
lib = m._lib
v = [C.c_int() for _ in range(5)]
check(lib.elph_bench_pg_info(m._h, *[C.byref(x) for x in v]))
print("L", L, "N", m.Nsites, "Ltau", Lt, "orders sum", int(P.orders.sum()), "max", int(P.orders.max()), "patch (kind, px, py, nw, tables)", tuple(x.value for x in v))
ms, fused = C.c_double(), C.c_int()
FORMS = (("patch", "0"), ("before", "1"))


def window(what, nrhs, reps):
    check(lib.elph_bench_prepare(m._h, what, nrhs, None))
    check(lib.elph_bench_run(m._h, what, nrhs, reps, 0, C.byref(ms)))
    return ms.value * 1e3 / reps


for nrhs in [int(a) for a in sys.argv[2:]] or [1, 16, 64]:
    B = np.ascontiguousarray(np.stack([synth.randn(100 + r, m.Ndim) for r in range(nrhs)]))
    line = f"L={L:2d} nrhs={nrhs:3d}"
    for what, name, reps in ((3, "pcg_iter", 1000), (0, "MtM", 2000)):
        t, px = {f: [] for f, _ in FORMS}, {}
        for f, e in FORMS:      # warm-up of both forms: code objects, caches
            os.environ["ELPH_NO_PG"] = e
            check(lib.elph_bench_prepare(m._h, what, nrhs, dptr(B)))
            check(lib.elph_bench_run(m._h, what, nrhs, 50, 0, C.byref(ms)))
            check(lib.elph_bench_px_info(m._h, C.byref(fused)))
            px[f] = fused.value
        for _ in range(5):
            for f, e in FORMS:
                os.environ["ELPH_NO_PG"] = e
                t[f].append(window(what, nrhs, reps))
        a, b = np.median(t["patch"]), np.median(t["before"])
        line += f" | {name} patch {a:8.1f} us (min {min(t['patch']):.1f} max {max(t['patch']):.1f}) before {b:8.1f} us (min {min(t['before']):.1f} max {max(t['before']):.1f}) ratio {b / a:.2f}"
        if what == 3:
            line += f" fused {px['patch']}/{px['before']}"
    sol = {}
    for f, e in FORMS:
        os.environ["ELPH_NO_PG"] = e
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B, P=P)
        sol[f] = (X, it, fl)
    same = np.array_equal(sol["patch"][1], sol["before"][1]) and not sol["patch"][2].any()
    diff = np.abs(sol["patch"][0] - sol["before"][0]).max() / np.abs(sol["before"][0]).max()
    print(line + f" | solves: iterations {int(sol['patch'][1].max())} equal {same} max diff {diff:.1e}", flush=True)
os.environ.pop("ELPH_NO_PG", None)
m.close()
