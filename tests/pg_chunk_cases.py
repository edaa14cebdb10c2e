"""The time-axis walk of the patch mat-vec kernels k_mul_pg and k_cg_ap_pg (csrc/pgrid.hip) — the cases, held once, for tests/test_pg_chunk_host.py
(CPU: the rule, the pin, the probes, the oracle's stop margins) and tests/test_gpu_pg_chunks.py (GPU: every case against the oracle).

A workgroup of these kernels takes a chunk of T consecutive time slices of one vector.  elph_pg_chunks (pgrid.hip) chooses T for a launch; ELPH_PG_T=n
pins it.  parent_rule() restates the two loops the launchers carried before that function existed; alias_of() restates the ladder of pg_dispatch.

RULE: part (a), the rule as it stands — one lattice per slots class, batches large enough for T >= 2 without the pin.
PIN:  part (b), every instantiation pg_dispatch can hand to k_mul_pg / k_cg_ap_pg on a handle, at Ltau = 7 with two or three vectors and ELPH_PG_T in
      PIN_T: last chunks of 1 and of T - 1 slices, the whole axis in one chunk, the clamp.  LONG: some of them at Ltau = 11 for T = 5, 8, 10.
FUSED: the p/x-fused k_cg_ap_pg<PX> at the smallest shapes whose transform plan fuses, at T = 1 and one ragged T.
UNREACHED: the aliases of pg_dispatch no case reaches, with the reason.

Inputs, all from seeds on the CPU: the field synth.phonon_field(seed = FIELD_SEED), right-hand sides b_r = M^T randn(RHS_SEED + r), guesses
x0_r = 0.1 randn(GUESS_SEED + r), the mat-vec vector randn(MATVEC_SEED).  The seeds were chosen on the oracle so that every solve case keeps the margin of
test_gpu_cubic.oracle_solves at the stop test (SEEDS holds the cases that needed another draw); test_pg_chunk_host.py asserts it for every case."""
import os
import re

import numpy as np

DTAU = 0.1
FIELD_SEED, RHS_SEED, GUESS_SEED, MATVEC_SEED, KPM_SEED = 4343, 100, 300, 77, 11
TOL = 1e-5
SEEDS = {"sq64": (4344, 100)}          # case name -> (field seed, right-hand-side seed) where the default pair left a knife edge at the stop test

SQUARE_BONDS = [(1, 1, (1, 0, 0)), (1, 1, (0, 1, 0))]
CUBIC_BONDS = [(1, 1, (1, 0, 0)), (1, 1, (0, 1, 0)), (1, 1, (0, 0, 1))]

# ------------------------------------------------------------------------------------------ the rule, restated

CG_LENGTHS = (1, 2, 4, 5, 8, 10, 16, 20, 32, 40)
MUL_LENGTHS = (1, 2, 4, 5, 8, 10, 16, 20)
KERNELS = ("mul", "cg_ap", "cg_ap_px")


def slots_of(px, py, nw, honeycomb):
    """Workgroups of k_cg_ap_pg the chip holds in one round: 1024 SIMDs, two waves each for 8 registers per vector, nw wavefronts per slice."""
    return 1024 * (2 if (not honeycomb and px * py <= 8) else 1) // nw


def parent_choice(kernel, px, py, nw, honeycomb, nvec, L):
    """(the chunk length the loop of a launcher chose before the clamp, whether it fell through to 20)."""
    lengths, room = (MUL_LENGTHS, 2048) if kernel == "mul" else (CG_LENGTHS, slots_of(px, py, nw, honeycomb))
    for c in lengths:
        if nvec * ((L + c - 1) // c) <= room:
            return c, False
    return 20, True


def parent_rule(kernel, px, py, nw, honeycomb, nvec, L):
    """(T, chunks, last) as the two launchers chose them before elph_pg_chunks: the shortest listed chunk whose workgroups fit, else 20, clamped
    to [1, L]."""
    T = max(1, min(parent_choice(kernel, px, py, nw, honeycomb, nvec, L)[0], L))
    nch = (L + T - 1) // T
    return T, nch, L - (nch - 1) * T


def pinned(n, L):
    """(T, chunks, last) under ELPH_PG_T=n."""
    T = max(1, min(int(n), L))
    nch = (L + T - 1) // T
    return T, nch, L - (nch - 1) * T


# one launch shape per slots class (px, py, nw, honeycomb): 2048, 1024, 682, 512, 409, 341, 256 — and the honeycomb shapes, which hold one wave per SIMD
# whatever their patch
SLOT_SHAPES = {2048: [(2, 4, 1, False), (2, 2, 1, False)], 1024: [(2, 6, 1, False), (4, 4, 1, False), (2, 2, 2, False), (3, 2, 1, True), (2, 2, 1, True)],
               682: [(2, 2, 3, False)], 512: [(2, 2, 4, False), (4, 4, 2, False), (2, 2, 2, True), (3, 3, 2, True)], 409: [(2, 2, 5, False)],
               341: [(2, 2, 6, False), (4, 4, 3, False), (3, 3, 3, True)], 256: [(4, 4, 4, False), (2, 2, 4, True)]}

# ------------------------------------------------------------------------------------------ pg_dispatch, restated


def alias_of(kind, px, py, nw, tables):
    """The alias pg_dispatch (pgrid.hip) launches for a patch kind (1 square, 2 honeycomb, 3 triangular, 4 cubic), a launch shape and the
    disorder-table flag; None where it has no instantiation."""
    if tables:
        return {2: "M22_2D", 3: "M22_3D", 4: "M22_4D", 5: "M22_5D"}.get(nw) or ("SQ44D" if px == 4 else "SQ26D" if py == 6 else "SQ24D")
    if kind == 1 and (px, py) == (2, 2) and 2 <= nw <= 6:
        return f"M22_{nw}"
    if kind == 1 and (px, py) == (4, 4) and 2 <= nw <= 4:
        return f"M44_{nw}"
    if kind == 2 and px in (2, 3) and 2 <= nw <= 4:
        return f"H{px}{px}_{nw}"
    if kind == 4 and nw in (1, 2, 4):
        return f"CU_{nw}"
    if kind != 3 and nw > 1:
        return None
    return {(1, 4, 4): "SQ44", (1, 2, 6): "SQ26", (1, 2, 4): "SQ24", (1, 2, 10): "SQ2A", (1, 4, 6): "SQ46", (2, 3, 2): "HC32", (2, 4, 2): "HC42",
            (2, 3, 3): "HC33", (3, 2, 2): "TR22", (3, 2, 4): "TR24", (3, 2, 6): "TR26", (3, 4, 4): "TR44"}.get((kind, px, py))


def dispatch_aliases():
    """The aliases pg_dispatch launches, read from its source (one `launch(Tag<NAME>{})` per rung)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "elphdynamics_amd", "csrc", "pgrid.hip")
    with open(path) as f:
        text = f.read()
    body = text[text.index("static int pg_dispatch("):text.index("static void pg_launch_shape(")]
    return re.findall(r"launch\(Tag<(\w+)>\{\}\)", body)


# ------------------------------------------------------------------------------------------ the cases

NO_FAST = {"ELPH_NO_FAST": "1"}       # no lane program on the handle (lattices up to 512 sites have one): its mat-vecs and k_cg_ap are the patch kernels (read at elph_create)
ONE_WAVE = {"ELPH_PG_MW": "0"}        # patch shapes of one wavefront per slice only: the disordered 28 x 28 keeps its 4 x 4 patches (SQ44D)
PIN_LTAU, LONG_LTAU = 7, 11
PIN_T = (1, 2, 3, 4, 6, 7, 40)        # Ltau = 7: chunks 7x1 | 2+2+2+1 | 3+3+1 | 4+3 | 6+1 | 7 | 7 (clamped)
LONG_T = (5, 8, 10)                   # Ltau = 11: 5+5+1 | 8+3 | 10+1

# name: (family, side, environment, t_stddev, alias, vectors)
PIN = {
    "sq20": ("sq", 20, NO_FAST, 0.0, "SQ24", 2), "sq24": ("sq", 24, {}, 0.0, "SQ26", 3), "sq28": ("sq", 28, {}, 0.0, "SQ44", 2),
    "sq30": ("sq", 30, {}, 0.0, "SQ2A", 2), "sq36": ("sq", 36, {}, 0.0, "SQ46", 2),
    "sq22": ("sq", 22, NO_FAST, 0.0, "M22_2", 3), "sq26": ("sq", 26, {}, 0.0, "M22_3", 2), "sq34": ("sq", 34, {}, 0.0, "M22_5", 2),
    "sq38": ("sq", 38, {}, 0.0, "M22_6", 2),
    "sq40": ("sq", 40, {}, 0.0, "M44_2", 3), "sq48": ("sq", 48, {}, 0.0, "M44_3", 2), "sq64": ("sq", 64, {}, 0.0, "M44_4", 2),
    "hc18": ("hc", 18, {}, 0.0, "HC32", 3), "hc20": ("hc", 20, {}, 0.0, "HC42", 2), "hc21": ("hc", 21, {}, 0.0, "HC33", 2),
    "hc22": ("hc", 22, {}, 0.0, "H22_2", 3), "hc26": ("hc", 26, {}, 0.0, "H22_3", 2), "hc28": ("hc", 28, {}, 0.0, "H22_4", 2),
    "hc27": ("hc", 27, {}, 0.0, "H33_2", 2), "hc36": ("hc", 36, {}, 0.0, "H33_3", 2), "hc42": ("hc", 42, {}, 0.0, "H33_4", 2),
    "tri12": ("tri", 12, NO_FAST, 0.0, "TR22", 3), "tri20": ("tri", 20, NO_FAST, 0.0, "TR24", 2), "tri24": ("tri", 24, {}, 0.0, "TR26", 2),
    "tri32": ("tri", 32, {}, 0.0, "TR44", 2),
    "cu6": ("cu", 6, NO_FAST, 0.0, "CU_1", 3), "cu8": ("cu", 8, NO_FAST, 0.0, "CU_1", 2), "cu10": ("cu", 10, {}, 0.0, "CU_2", 3),
    "cu12": ("cu", 12, {}, 0.0, "CU_4", 2),
    "sq20d": ("sq", 20, NO_FAST, 0.1, "SQ24D", 2), "sq24d": ("sq", 24, {}, 0.1, "SQ26D", 2), "sq28d1": ("sq", 28, ONE_WAVE, 0.1, "SQ44D", 2),
    "sq22d": ("sq", 22, NO_FAST, 0.1, "M22_2D", 2), "sq26d": ("sq", 26, {}, 0.1, "M22_3D", 3), "sq28d": ("sq", 28, {}, 0.1, "M22_4D", 2),
    "sq34d": ("sq", 34, {}, 0.1, "M22_5D", 2),
}
# several wavefronts per slice (the exchange buffers between sweeps) and one single-wavefront shape at the chunk lengths Ltau = 7 cannot hold
LONG = ("cu10", "cu12", "sq26", "sq40", "hc22", "hc27", "sq24", "sq26d")

# the aliases of pg_dispatch no handle reaches with k_mul_pg / k_cg_ap_pg in these tests
UNREACHED = {
    "M22_4": "uniform 2 x 2 patches on four wavefronts exist only as pg_launch_shape's re-shaping of 28 x 28, 30 x 30 and 32 x 32 from 48 right-hand "
             "sides, for k_kpm_cheb_pg and the fused k_cg_ap_pg<PX>; FUSED['sq28x48'] runs the latter, no handle runs k_mul_pg or the un-fused "
             "k_cg_ap_pg in it (the same template on four wavefronts with tables is M22_4D, on 2, 3, 5, 6 wavefronts M22_2 ... M22_6)",
}

# part (a).  name: (family, side, Ltau, right-hand sides, k_cg_ap_pg's (T, chunks, last), the batched k_mul_pg's (T, chunks, last)).
# RULE_DTAU: these models take dtau = 1/30 (beta = 0.7 at 21 slices).  At dtau = 0.1 the un-preconditioned solves of 10^3 x 21 stop after 101 ... 103
# iterations, far beyond the 40 over which two summation orders of CG agree to 1e-10 (header of tests/test_gpu_parity.py): measured on the device,
# the patch kernels at the rule's T = 4, the same at T = 1 and the generic kernels (ELPH_NO_PG=1) ALL stop one iteration from the oracle on the same 8
# of the 100 right-hand sides (oracle margins up to 3e-2) and hold x to 2e-6 on the others — the drift of CG, not of a kernel.  At dtau = 1/30 the
# same batches stop after 32 ... 74 iterations with x within 2e-15 of the oracle's in all three forms.
RULE_DTAU = 1.0 / 30.0
RULE = {
    "sq24": ("sq", 24, 21, 100, (4, 6, 1), (2, 11, 1)),          # 2 x 6 patches, 1024 slots
    "cu10": ("cu", 10, 21, 100, (4, 6, 1), (2, 11, 1)),          # Cu<2>, 1024 slots
    "cu12": ("cu", 12, 9, 60, (2, 5, 1), (1, 9, 1)),             # Cu<4>, 512 slots
    "hc18": ("hc", 18, 23, 90, (4, 6, 3), (2, 12, 1)),           # 3 x 2 cells, 1024 slots: a last chunk of T - 1 slices
}

# the p/x-fused iteration.  name: (PIN lattice, Ltau, right-hand sides, the alias k_cg_ap_pg<PX> launches): the smallest even time axis and batch at
# which the transform plan fuses (found with _lib.dft_plan; the cubic rows are test_gpu_cubic.FUSED); run at T = 1 and at ragged_T(Ltau)
FUSED = {
    "cu6": ("cu6", 8, 32, "CU_1"), "cu8": ("cu8", 8, 16, "CU_1"), "cu10": ("cu10", 16, 8, "CU_2"), "cu12": ("cu12", 28, 6, "CU_4"),
    "sq20": ("sq20", 8, 24, "SQ24"), "sq24": ("sq24", 10, 16, "SQ26"), "sq28": ("sq28", 14, 12, "SQ44"), "sq30": ("sq30", 16, 8, "SQ2A"),
    "sq36": ("sq36", 22, 6, "SQ46"), "sq22": ("sq22", 8, 16, "M22_2"), "sq26": ("sq26", 12, 12, "M22_3"), "sq34": ("sq34", 20, 8, "M22_5"),
    "sq38": ("sq38", 24, 6, "M22_6"), "sq40": ("sq40", 26, 6, "M44_2"), "sq48": ("sq48", 36, 4, "M44_3"),
    "hc18": ("hc18", 12, 12, "HC32"), "hc20": ("hc20", 14, 12, "HC42"), "hc21": ("hc21", 14, 8, "HC33"), "hc22": ("hc22", 16, 8, "H22_2"),
    "hc26": ("hc26", 22, 6, "H22_3"), "hc28": ("hc28", 26, 6, "H22_4"), "hc27": ("hc27", 24, 6, "H33_2"),
    "tri20": ("tri20", 8, 24, "TR24"), "tri24": ("tri24", 10, 16, "TR26"), "tri32": ("tri32", 16, 8, "TR44"),
    # pg_launch_shape's re-shaping from 48 right-hand sides: 28 x 28 as 2 x 2 patches on four wavefronts
    "sq28x48": ("sq28", 14, 48, "M22_4"),
}
# (no fused case: 64 x 64, honeycomb 36 x 36 and 42 x 42 — no time axis up to 40 slices fuses below 48 right-hand sides; triangular 12 x 12 — 9 column
#  tiles never make the streaming transform; the disorder-table variants — their walk is that of the aliases above, PIN runs their un-fused kernels)


def ragged_T(ltau):
    """The first of 3, 5, 4 that does not divide the time axis: the pinned chunk length of a fused case."""
    return next(T for T in (3, 5, 4) if ltau % T)


def family(name):
    from elphdynamics_amd import lattice as lat
    return {"sq": (1, 2, SQUARE_BONDS, 1), "hc": (2, 2, lat.HONEYCOMB_BONDS, 2), "tri": (1, 2, lat.TRIANGULAR_BONDS, 3), "cu": (1, 3, CUBIC_BONDS, 4)}[name]


def seeds(case):
    return SEEDS.get(case, (FIELD_SEED, RHS_SEED))


def make_model(fam, side, ltau, t_stddev=0.0, field_seed=FIELD_SEED, host=False, dtau=DTAU):
    """The Holstein model (t = omega = lambda = 1, mu = 0, dtau = 0.1; t_stddev: hopping disorder) on the side^d lattice of a family with ltau time
    slices; host: without a device handle — the same lattice, tables and field."""
    from elphdynamics_amd import lattice as lat, models, synth
    from kpm_bounds_reference import _HostHolstein
    norb, dim, bonds, _ = family(fam)
    la = lat.Lattice(norb, side, side, side if dim == 3 else 1)
    beta = ltau * dtau
    m = _HostHolstein(la, beta, dtau) if host else models.HolsteinModel(la, beta, dtau, tol=TOL, maxiter=20000)
    rng = np.random.default_rng(field_seed + 991)
    for (o1, o2, d) in bonds:
        m.assign_t_(1.0, o1, o2, d, stddev=t_stddev, rng=rng)
    m.assign_omega_(1.0)
    m.assign_lambda_(1.0)
    m.assign_mu_(0.0)
    m.initialize_model_()
    assert m.Ltau == ltau
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, beta, dtau, omega=1.0, lam=1.0, seed=field_seed)
    if not host:
        models.update_model_(m)
    return m


def oracle_model(orc, m):
    E = orc.update_model_holstein(m.Nsites, m.Ltau, m.dtau, m.x, m.lam, m.lam2, m.mu)
    return orc.make_model(0, m.Nsites, m.Ltau, m.neighbor_table, m.cosht, m.sinht, E)


def shape_of(m):
    """(patch kind, px, py, nw, tables) the library recognises in a model's bond table, without a device (reads ELPH_PG_MW)."""
    from elphdynamics_amd import _lib
    v = _lib.lattice_shape(0, m.Nsites, m.neighbor_table, m.cosht, m.sinht)
    return v["patch_kind"], v["patch_PX"], v["patch_PY"], v["patch_NW"], not v["hop_uniform"]


def inputs(orc, om, ndim, nvec, rhs_seed=RHS_SEED):
    """(B, X0): b_r = M^T randn(rhs_seed + r) by the oracle, x0_r = 0.1 randn(GUESS_SEED + r)."""
    from elphdynamics_amd import synth
    B = np.stack([orc.mulMT(om, synth.randn(rhs_seed + r, ndim)) for r in range(nvec)])
    X0 = np.stack([0.1 * synth.randn(GUESS_SEED + r, ndim) for r in range(nvec)])
    return B, X0


def oracle_solves(orc, om, B, X0=None, oP=None, tol=TOL):
    """[(x, iterations)] of the oracle per right-hand side.  tol = TOL: with the condition on the inputs — the oracle's eps at its last iteration and
    at the one before differ from the tolerance by more than 1e-6 relative, so that an equal iteration count is no coin toss."""
    out = []
    for r in range(B.shape[0]):
        b = np.ascontiguousarray(B[r])
        x0 = None if X0 is None else np.ascontiguousarray(X0[r])
        xo, ito, histo = orc.cg_solve(om, b, x0=x0, tol=tol, maxiter=20000, P=oP, history=True)
        if tol == TOL:
            assert abs(histo[-1] / tol - 1) > 1e-6 and abs(histo[-2] / tol - 1) > 1e-6, (r, histo[-2:])
        assert histo[-1] < tol <= histo[-2], (r, histo[-2:])
        out.append((xo, int(ito)))
    return out


def oracle_kpm(orc, om, nsites):
    """The oracle's expansion (n = 20, as test_kpm_vs_oracle) and its Arnoldi bounds."""
    oP = orc.make_kpm(om, n=20, buf=0.05, c1=1.0, c2=1.0)
    rng = np.random.default_rng(KPM_SEED)
    e_min, e_max = orc.kpm_setup(oP, b_max=rng.standard_normal(nsites), b_min=rng.standard_normal(nsites))
    assert oP.active == 1
    return oP, e_min, e_max
