"""The time-axis walk of the patch mat-vec kernels k_mul_pg and k_cg_ap_pg (csrc/pgrid.hip) at every chunk length, against the CPU oracle (run with
-m gpu on an MI355X).

A workgroup of these kernels walks T consecutive time slices of one vector with the previous slice in registers.  Production batches run T = 4 ... 20;
the batches of the other test modules almost all stay at T = 1, and where they reach T = 2 they compare the patch kernels with themselves.  Here the
reference is the oracle, on the same tables and field, every input made on the CPU from seeds (tests/pg_chunk_cases.py holds the cases;
tests/test_pg_chunk_host.py asserts on the CPU that each reaches the chunking it was designed for and that the oracle's solves stop with a margin):

  (a) test_rule_case — the rule as it stands, no pin: one lattice per slots class with a batch large enough that elph_pg_chunks itself gives k_cg_ap_pg
      T = 4 / 2 and the batched k_mul_pg T = 2, every one with a short last chunk.  An un-preconditioned batch from non-zero guesses (k_mul_pg<2>
      computes A x0 and the true residuals, k_cg_ap_pg iterates) and a KPM-preconditioned batch on the oracle's Arnoldi bounds: the oracle's
      iteration count and solution per right-hand side, the returned residual against the oracle's mat-vec on the returned x.
  (b) test_pin_matvecs, test_pin_solves — every alias of pg_dispatch a handle reaches with these kernels (PIN: 35 of the 36; the one listed below
      under "not reached"), at Ltau = 7 with two or three vectors under ELPH_PG_T = 1, 2, 3, 4, 6, 7, 40 — last chunks of 1 and of T - 1 slices, the
      whole axis in one chunk, the clamp — and, for the shapes of several wavefronts and two others, at Ltau = 11 under 5, 8, 10.
      test_pin_fused — k_cg_ap_pg<PX> in the p/x-fused preconditioned iteration at the smallest shape whose transform plan fuses, T = 1 and one ragged
      T; 28 x 28 with 48 right-hand sides runs it re-shaped to 2 x 2 patches on four wavefronts (M22_4).

Bounds.  Mat-vecs 1e-13 against the oracle (the suite's bound), and BIT-EQUAL to the same call at T = 1: each element sees the same operations in the
same order whatever the chunk — the slice loop is `#pragma unroll 1`, the halo slice is loaded, not recomputed.  Solves: the oracle's iteration
counts at tol = 1e-5 and x within 1e-8 at that count; at tol = 1e-13 x within 1e-10 and the returned residual within 1e-12 absolute (the bounds of
tests/test_gpu_cubic.py for the same quantities); against T = 1 on the same handle equal counts at tol = 1e-5 — where the host test holds the stop to
a margin; at 1e-13 eps ends at the round-off of the residual recursion and a count may differ by one, 64 x 64: 98 against 97 — and x within 1e-10
at both tolerances (the p.z partial sums of a chunk are added in another order than those of its slices, so no bit-equality).  Fused: the oracle's counts at 1e-5, its solutions of tol = 1e-13
within 1e-10, as test_gpu_cubic.check_batched_solves.

Which kernels ran is asserted before anything is compared: elph_bench_pg_chunk_info (the launch shape and chunking the handle takes now, and that its
mat-vecs and streaming iteration take the patch kernels at all), elph_bench_pg_info (kind, tables), elph_bench_px_info (fused or not),
elph_bench_wg_info and elph_bench_slabs_info (neither resident form: ELPH_SLABS=0 keeps the slab form out, and it accepts x0 = 0 only),
elph_wg_status (no fallback).  No case is skipped; a case whose probe does not show the designed T fails.

pg_dispatch aliases not reached (pg_chunk_cases.UNREACHED; the host test holds covered + listed to the count of pg_dispatch):
  M22_4   uniform 2 x 2 patches on four wavefronts exist only as pg_launch_shape's re-shaping of 28 x 28, 30 x 30 and 32 x 32 from 48 right-hand
          sides, for k_kpm_cheb_pg and the fused k_cg_ap_pg<PX> — test_pin_fused[sq28x48] runs the latter; no handle runs k_mul_pg or the un-fused
          k_cg_ap_pg in it (the same template with tables is M22_4D, on 2, 3, 5, 6 wavefronts M22_2 ... M22_6: all in PIN).

Every test prints its largest errors (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest

import pg_chunk_cases as pc
from test_gpu_parity import _pg_info, _px_fused, rel

pytestmark = pytest.mark.gpu

ENV = ("ELPH_PG_T", "ELPH_NO_FAST", "ELPH_PG_MW", "ELPH_PG_2X2_FROM", "ELPH_NO_PG", "ELPH_PG_PX", "ELPH_PG_DIS", "ELPH_SLABS", "ELPH_NO_WG")


@pytest.fixture
def env(monkeypatch):
    """Clears the switches that choose among these kernels, keeps the slab form out, and sets a case's own (some are read when the handle is made)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ELPH_SLABS", "0")

    def use(d):
        for k, v in d.items():
            monkeypatch.setenv(k, v)
    return use


def assert_patch_kernels(m, kernel, nvec, fam, alias, chunks, fused=None):
    """The handle would launch `kernel` for nvec vectors in the alias's shape with the chunking (T, chunks, last), its streaming iteration takes the
    patch kernels, and no resident form ran or applies."""
    from elphdynamics_amd import _lib
    lib = m._lib
    info = _lib.pg_chunk_info(m._h, kernel, nvec)
    kind, _, _, _, tables = _pg_info(m)
    assert kind == pc.family(fam)[3] and info["taken"] == 1, (info, kind)
    assert pc.alias_of(kind, info["px"], info["py"], info["nw"], bool(tables)) == alias, (info, tables, alias)
    assert (info["T"], info["chunks"], info["last"]) == tuple(chunks), (kernel, nvec, info, chunks)
    v = [C.c_int() for _ in range(4)]
    _lib.check(lib.elph_bench_wg_info(m._h, nvec, *[C.byref(x) for x in v]))
    assert v[0].value == 0, "the workgroup-resident solve applies"
    _lib.check(lib.elph_bench_slabs_info(m._h, min(nvec, 8), *[C.byref(x) for x in v]))
    assert v[0].value == 0, "the slab form applies"
    cd, fb = C.c_int(), C.c_int64()
    _lib.check(lib.elph_wg_status(m._h, C.byref(cd), C.byref(fb)))
    assert cd.value == 0 and fb.value == 0
    if fused is not None:
        assert _px_fused(m) is fused


def open_case(orc, env, lattice, ltau, seed_key=None):
    fam, side, e, sd, alias, nvec = pc.PIN[lattice]
    env(e)
    fs, rs = pc.seeds(seed_key or lattice)
    m = pc.make_model(fam, side, ltau, sd, fs)
    return m, pc.oracle_model(orc, m), fam, alias, nvec, rs


def gpu_kpm(m, e_min, e_max, oP):
    from elphdynamics_amd import preconditioners as pcn
    P = pcn.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pcn.setup_(P, e_min=e_min, e_max=e_max)
    assert P.active and P.lam_lo == oP.lam_lo and P.lam_hi == oP.lam_hi
    return P


def true_residual(orc, om, b, x):
    return np.linalg.norm(b - orc.mulMTM(om, np.ascontiguousarray(x))) / np.linalg.norm(b)


WALKS = [(name, pc.PIN_LTAU) for name in pc.PIN] + [(name, pc.LONG_LTAU) for name in pc.LONG]
WALK_IDS = [f"{name}-L{ltau}" for name, ltau in WALKS]


def pins(ltau):
    return pc.PIN_T if ltau == pc.PIN_LTAU else (1,) + pc.LONG_T


# ------------------------------------------------------------------------------------------ (b) the mat-vecs

@pytest.mark.parametrize("name,ltau", WALKS, ids=WALK_IDS)
def test_pin_matvecs(oracle, env, name, ltau):
    """mulM!, mulMT!, mulMTM! of one vector at every pinned T: the oracle's at 1e-13, and the bits of T = 1."""
    from elphdynamics_amd import models, synth
    m, om, fam, alias, _, _ = open_case(oracle, env, name, ltau)
    try:
        v = synth.randn(pc.MATVEC_SEED, m.Ndim)
        fns = ((models.mulM_, oracle.mulM(om, v)), (models.mulMt_, oracle.mulMT(om, v)), (models.mulMtM_, oracle.mulMTM(om, v)))
        first, worst = None, 0.0
        for T in pins(ltau):
            env({"ELPH_PG_T": str(T)})
            assert_patch_kernels(m, "mul", 1, fam, alias, pc.pinned(T, ltau))
            ys = []
            for fn, ref in fns:
                y = np.full(m.Ndim, np.nan)
                fn(y, m, v)
                err = rel(y, ref)
                worst = max(worst, err)
                assert err < 1e-13, (T, fn.__name__, err)
                ys.append(y)
            if first is None:
                assert T == 1
                first = ys
            for y, y1, (fn, _) in zip(ys, first, fns):
                assert np.array_equal(y, y1), (T, fn.__name__, rel(y, y1))
        print(f"pg-chunks matvec {name} Ltau={ltau} {alias}: largest error against the oracle {worst:.2e}, bit-equal across T = {pins(ltau)}")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ (b) the un-preconditioned batch

@pytest.mark.parametrize("name,ltau", WALKS, ids=WALK_IDS)
def test_pin_solves(oracle, env, name, ltau):
    """An un-preconditioned batch from non-zero guesses at every pinned T (k_mul_pg<2>: A x0 and the true residuals; k_cg_ap_pg: the iterations)."""
    from elphdynamics_amd import models
    m, om, fam, alias, nvec, rs = open_case(oracle, env, name, ltau)
    try:
        nvec = nvec if ltau == pc.PIN_LTAU else 2
        B, X0 = pc.inputs(oracle, om, m.Ndim, nvec, rs)
        ref = {tol: pc.oracle_solves(oracle, om, B, X0, tol=tol) for tol in (pc.TOL, 1e-13)}
        first, worst = None, {pc.TOL: 0.0, 1e-13: 0.0, "res": 0.0, "T1": 0.0}
        for T in pins(ltau):
            env({"ELPH_PG_T": str(T)})
            got = {}
            for tol, bound in ((pc.TOL, 1e-8), (1e-13, 1e-10)):
                m.solver.tol = tol
                X = X0.copy()
                it, res, fl = models.ldiv_batched_(X, m, B)
                assert_patch_kernels(m, "cg_ap", nvec, fam, alias, pc.pinned(T, ltau))
                assert_patch_kernels(m, "mul", nvec, fam, alias, pc.pinned(T, ltau))
                assert not fl.any()
                if tol == pc.TOL:
                    assert [int(i) for i in it] == [r[1] for r in ref[tol]], (T, it, [r[1] for r in ref[tol]])
                for r in range(nvec):
                    err = rel(X[r], ref[tol][r][0])
                    worst[tol] = max(worst[tol], err)
                    assert err < bound, (T, tol, r, err)
                    if tol == 1e-13:
                        d = abs(res[r] - true_residual(oracle, om, B[r], X[r]))
                        worst["res"] = max(worst["res"], d)
                        assert d < 1e-12, (T, r, d)
                got[tol] = (X, it.copy())
            if first is None:
                assert T == 1
                first = got
            for tol in got:
                if tol == pc.TOL:          # (the counts of tol = 1e-13 carry no margin: eps ends at the round-off of the recursion)
                    assert np.array_equal(got[tol][1], first[tol][1]), (T, tol, got[tol][1], first[tol][1])
                err = rel(got[tol][0], first[tol][0])
                worst["T1"] = max(worst["T1"], err)
                assert err < 1e-10, (T, tol, err)
        print(f"pg-chunks solve {name} Ltau={ltau} {alias} x{nvec}: counts {[r[1] for r in ref[pc.TOL]]}; x against the oracle {worst[pc.TOL]:.2e} "
              f"(1e-5) {worst[1e-13]:.2e} (1e-13); residual {worst['res']:.2e}; against T = 1 {worst['T1']:.2e}")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ (b) the p/x-fused iteration

@pytest.mark.parametrize("name", sorted(pc.FUSED))
def test_pin_fused(oracle, env, name):
    """k_cg_ap_pg<PX> (it reads the ready p with two halo slices and writes z and the p.z partials) at T = 1 and at one ragged T."""
    from elphdynamics_amd import models
    lattice, ltau, nrhs, alias = pc.FUSED[name]
    m, om, fam, _, _, rs = open_case(oracle, env, lattice, ltau, seed_key="fused-" + name)
    try:
        oP, e_min, e_max = pc.oracle_kpm(oracle, om, m.Nsites)
        P = gpu_kpm(m, e_min, e_max, oP)
        B, _ = pc.inputs(oracle, om, m.Ndim, nrhs, rs)
        ref = {tol: pc.oracle_solves(oracle, om, B, None, oP, tol=tol) for tol in (pc.TOL, 1e-13)}
        worst = {pc.TOL: 0.0, 1e-13: 0.0}
        for T in (1, pc.ragged_T(ltau)):
            env({"ELPH_PG_T": str(T)})
            for tol, bound in ((pc.TOL, 1e-8), (1e-13, 1e-10)):
                m.solver.tol = tol
                X = np.zeros_like(B)
                it, res, fl = models.ldiv_batched_(X, m, B, P=P)
                assert_patch_kernels(m, "cg_ap_px", nrhs, fam, alias, pc.pinned(T, ltau), fused=True)
                assert not fl.any()
                if tol == pc.TOL:
                    assert [int(i) for i in it] == [r[1] for r in ref[tol]], (T, it, [r[1] for r in ref[tol]])
                for r in range(nrhs):
                    err = rel(X[r], ref[tol][r][0])
                    worst[tol] = max(worst[tol], err)
                    assert err < bound, (T, tol, r, err)
        print(f"pg-chunks fused {name} Ltau={ltau} {alias} x{nrhs} T=1,{pc.ragged_T(ltau)}: counts {sorted(set(r[1] for r in ref[pc.TOL]))}; x against "
              f"the oracle {worst[pc.TOL]:.2e} (1e-5) {worst[1e-13]:.2e} (1e-13)")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ (a) the rule as it stands

@pytest.mark.parametrize("name", sorted(pc.RULE))
def test_rule_case(oracle, env, name):
    """No pin: the batch itself reaches T >= 2 in k_cg_ap_pg and (but for 12^3) in the batched k_mul_pg, each with a short last chunk."""
    from elphdynamics_amd import models
    fam, side, ltau, nrhs, cg, mul = pc.RULE[name]
    fs, rs = pc.seeds("rule-" + name)
    m = pc.make_model(fam, side, ltau, 0.0, fs, dtau=pc.RULE_DTAU)
    try:
        om = pc.oracle_model(oracle, m)
        kind, px, py, nw, tables = _pg_info(m)
        alias = pc.alias_of(kind, px, py, nw, bool(tables))
        B, X0 = pc.inputs(oracle, om, m.Ndim, nrhs, rs)
        worst = {}
        for label, guess, oP in (("plain", X0, None), ("kpm", None, pc.oracle_kpm(oracle, om, m.Nsites))):
            P = None if oP is None else gpu_kpm(m, oP[1], oP[2], oP[0])
            ref = pc.oracle_solves(oracle, om, B, guess, None if oP is None else oP[0])
            X = np.zeros_like(B) if guess is None else guess.copy()
            it, res, fl = models.ldiv_batched_(X, m, B, P=P)
            assert_patch_kernels(m, "cg_ap", nrhs, fam, alias, cg, fused=None if oP is None else False)
            assert_patch_kernels(m, "mul", nrhs, fam, alias, mul)
            assert not fl.any() and [int(i) for i in it] == [r[1] for r in ref], (label, it, [r[1] for r in ref])
            ex = max(rel(X[r], ref[r][0]) for r in range(nrhs))
            er = max(abs(res[r] - true_residual(oracle, om, B[r], X[r])) for r in range(nrhs))
            worst[label] = (ex, er)
            assert ex < 1e-8 and er < 1e-12, (label, ex, er)
        print(f"pg-chunks rule {name} Ltau={ltau} {alias} x{nrhs}: k_cg_ap_pg {cg}, k_mul_pg {mul}; (x, residual) against the oracle: plain "
              f"{worst['plain'][0]:.2e} {worst['plain'][1]:.2e}, preconditioned {worst['kpm'][0]:.2e} {worst['kpm'][1]:.2e}")
    finally:
        m.close()
