"""Every CG form's stop rules and the vector it stops with, against the CPU oracle (run with -m gpu on an MI355X).

The cases — models, guesses, parameter sets, the helper that restates the rule — are those of tests/stop_rule_cases.py;
tests/test_stop_rules_host.py holds every one of them to its preconditions on the oracle alone (designed reasons, log-margins >= 1e-3,
stops within 40 iterations, neighbouring iterates 1e-4 apart).  On that ground this module asks every form for

  * the oracle's iteration count, exactly;
  * rel(x, x_oracle) < 1e-10 at every stop, converged or not (the project's figure for the first 40 iterations, header of
    tests/test_gpu_parity.py): a form that returns x_{j-1} or x_{j+1} misses it by six orders;
  * the same count and the same bits with and without a residual history (history=True switches the screening comparisons of the stop
    test off: the only place the screened and the exact path of one kernel meet), the history within 1e-10 of the oracle's;
  * in a batch of six right-hand sides that end for three different reasons (set P: flags 0; set F: flags 0 / 2 / 1), the oracle's
    (iters, flag, residual_error) per right-hand side, flagged solutions exactly zero, the others within 1e-10 of the oracle's and equal
    to the same solve done alone — a finished right-hand side stays frozen while the others go on;
  * the same with two chains resident, each right-hand side against the oracle model of its own chain;
  * inside a preconditioned batch, the retry of flagged right-hand sides other than the first, with the parked slot 0 intact.

Which form ran is asserted before anything is compared, from the probes elph_bench_wg_info, elph_wg_status, elph_bench_px_info,
elph_bench_pg_info, elph_bench_slabs_info and elph_bench_info (the plan's slices per wave).  The two-stream split has no probe of its
own: it is told from the one-stream solve by the plan it leaves behind — elph_choose_T_px gives 64 right-hand sides of the 16 x 16 x 160
model 5 slices per wave when two halves are in flight on two streams (1536 ... 2048 waves) and 4 on one stream (>= 2560 waves), and a
batch the split declines keeps the one-stream plan.  k_pcg_wg has no probe and rests on ELPH_PCG_WG=1 and a healthy elph_wg_status, as
its own tests do.  The REASON of a stop is inferred from the oracle: the device's CgState.done is not exported.

Parts a form leaves out (FORMS below): the p/x-fused iteration is planned from 48 (16 x 16) or 64 right-hand sides on, so those forms
run the batches only; the slab form accepts x0 = 0 only, so its reasons and the two coincidences at j = maxiter come from parameter
sets on the zero guess, it has no mixed batch, and no case engages the kappa side of its stop screen (0.17 sqrt(kmax) > 1 needs
kmax > 35, K_j of the 18 x 18 x 6 model stays below); k_pcg_wg takes up to eight right-hand sides: its batches have three, one of
each kind, and the kappa side of ITS screen is engaged by the big-kappa case on the right-hand side whose residual grows at first.
"""
import ctypes as C
import os

import numpy as np
import pytest

import stop_rule_cases as src

pytestmark = pytest.mark.gpu

X_BOUND = 1e-10          # x and the residual histories against the oracle's (north star: the first 40 iterations)
RESID_BOUND = 1e-8       # residual_error against the oracle's true residual, relative
RETRY_BOUND = 1e-6       # a retried right-hand side carries the un-preconditioned solution (test_kpm_fallback_to_unpreconditioned)
ENV = ("ELPH_NO_WG", "ELPH_WG_NO_DPP", "ELPH_WG_T", "ELPH_NO_FAST", "ELPH_CHUNK_T", "ELPH_SQ16_AP", "ELPH_SPLIT_STREAMS", "ELPH_PCG_WG",
       "ELPH_SLABS", "ELPH_SLABS_P", "ELPH_FUSE_PX", "ELPH_FUSE_XR")


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture
def form_env():
    """Sets a form's environment switches (some are read when the handle is created) and puts the old values back."""
    old = {k: os.environ.get(k) for k in ENV}

    def use(env):
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(env)

    yield use
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


# ------------------------------------------------------------------------------------------ probes

def _ints(fn, m, *lead, n):
    out = [C.c_int() for _ in range(n)]
    from elphdynamics_amd._lib import check
    check(fn(m._h, *lead, *[C.byref(o) for o in out]))
    return [o.value for o in out]


def probe(m, nrhs, keys):
    """What the probes say about the handle after its last solve: only the keys asked for (elph_bench_slabs_info builds the slabs of a
    handle that may have them) and the health of the resident kernels."""
    lib = m._lib
    cd, fb = C.c_int(), C.c_int64()
    lib.elph_wg_status(m._h, C.byref(cd), C.byref(fb))
    read = {"wg": lambda: _ints(lib.elph_bench_wg_info, m, nrhs, n=4)[0], "wg_T": lambda: _ints(lib.elph_bench_wg_info, m, nrhs, n=4)[1],
            "px": lambda: _ints(lib.elph_bench_px_info, m, n=1)[0], "pg": lambda: _ints(lib.elph_bench_pg_info, m, n=5)[0],
            "plan_T": lambda: _ints(lib.elph_bench_info, m, nrhs, n=1)[0], "slabs": lambda: _ints(lib.elph_bench_slabs_info, m, min(nrhs, 8), n=4)[0]}
    out = {k: read[k]() for k in keys}
    out.update(cooling=cd.value, fallbacks=fb.value)
    return out


class Form:
    """One CG form: the model, the environment that reaches it and what the probes must say after a solve of `nrhs` right-hand sides.
    expect: probe key -> value (or a predicate).  parts: "singles", "batch", "chains".  batch: right-hand sides per batch."""

    def __init__(self, name, model, env, expect, prec=False, parts=("singles", "batch"), batch=6):
        self.name, self.model, self.env, self.expect, self.prec, self.parts, self.batch = name, model, env, expect, prec, parts, batch
        self.key = (model, prec)

    def assert_ran(self, m, nrhs, plan=True):
        """plan=False: the health of the resident kernels only — after a preconditioned batch with flagged right-hand sides the plan the
        probes read is that of the last retry, an un-preconditioned solve of one right-hand side."""
        got = probe(m, nrhs, self.expect if plan else ())
        for k, want in (self.expect.items() if plan else ()):
            assert want(got[k]) if callable(want) else got[k] == want, (self.name, "another form ran", k, got)
        assert got["cooling"] == 0 and got["fallbacks"] == 0, (self.name, "a resident launch gave up and the streaming iteration redid it", got)


RESIDENT = {"wg": 1}
STREAM = {"wg": 0}
FORMS = [
    # the whole un-preconditioned solve in one launch (cg_wg.hip: k_cg_wg)
    Form("wg-b", "b", {}, RESIDENT, parts=("singles", "batch", "chains")),               # lane program, 4 x 4 x 20
    Form("wg-y", "y", {}, RESIDENT),                                                      # honeycomb 6 x 6, one cell per lane
    Form("wg-e", "e", {}, RESIDENT, parts=("singles", "batch", "chains")),               # bond phonons 4 x 4
    Form("wg-C-dpp", "C", {}, RESIDENT, parts=("singles", "batch", "chains")),           # the DPP form with the 16 x 16 sweep order
    Form("wg-C-lane", "C", {"ELPH_WG_NO_DPP": "1"}, RESIDENT),
    Form("wg-E", "E", {}, RESIDENT),                                                      # bond phonons 16 x 16, a table set per slice
    # the same kernel on slabs of rows (slabs.hip); x0 = 0 only
    Form("slabs-i", "i", {"ELPH_SLABS": "1"}, {"wg": 0, "slabs": 1}, parts=("singles",)),
    # the streaming iteration, un-preconditioned
    Form("fast-b", "b", {"ELPH_NO_WG": "1"}, dict(STREAM, plan_T=1, pg=0)),              # k_cg_ap_fast
    Form("chunk-b", "b", {"ELPH_NO_WG": "1", "ELPH_CHUNK_T": "4"}, dict(STREAM, plan_T=4), parts=("singles", "batch", "chains")),
    Form("chunk-C", "C", {"ELPH_NO_WG": "1", "ELPH_CHUNK_T": "4"}, dict(STREAM, plan_T=4), parts=("singles", "batch", "chains")),
    Form("chunk-rt-C-7", "C", {"ELPH_NO_WG": "1", "ELPH_CHUNK_T": "7"}, dict(STREAM, plan_T=7)),      # k_cg_ap_chunk_rt, ragged last chunk
    Form("chunk-rt-C-6", "C", {"ELPH_NO_WG": "1", "ELPH_CHUNK_T": "6"}, dict(STREAM, plan_T=6)),
    Form("chunk-C-3", "C", {"ELPH_NO_WG": "1", "ELPH_CHUNK_T": "3"}, dict(STREAM, plan_T=4)),      # 160 = 53 x 3 + 1: elph_choose_T lengthens the chunks until the last holds two slices — 4, a template length
    Form("gen-t", "t", {}, dict(STREAM, plan_T=1, pg=0)),                                # k_cg_ap of kernels.hip, natively (nine ragged colours)
    Form("gen-b", "b", {"ELPH_NO_FAST": "1"}, dict(STREAM, plan_T=1, pg=0)),
    Form("pg-k", "k", {"ELPH_NO_FAST": "1"}, dict(STREAM, pg=1)),                        # k_cg_ap_pg: 2 x 4 patches
    Form("pg-t12", "t12", {"ELPH_NO_FAST": "1"}, dict(STREAM, pg=3)),                    # triangular patches
    Form("stream-e", "e", {"ELPH_NO_WG": "1"}, dict(STREAM, plan_T=1), parts=("singles", "batch", "chains")),
    # the streaming iteration, KPM-preconditioned
    Form("kpm-b", "b", {"ELPH_PCG_WG": "0"}, {"px": 0}, prec=True),                      # the five-kernel form
    Form("px-C-sq16", "C", {"ELPH_PCG_WG": "0", "ELPH_SPLIT_STREAMS": "0"}, {"px": 2}, prec=True, parts=("batch",), batch=48),
    Form("px-C-lane", "C", {"ELPH_PCG_WG": "0", "ELPH_SPLIT_STREAMS": "0", "ELPH_SQ16_AP": "0"}, {"px": 1}, prec=True, parts=("batch",), batch=48),
    Form("px-k40", "k40", {}, {"px": 1, "pg": 1}, prec=True, parts=("batch",), batch=64),           # the fused patch form
    Form("px-l22", "l22", {}, {"px": 1}, prec=True, parts=("batch",), batch=64),                     # the fused generic form
    # two half-batches on two streams: 64 right-hand sides (halves of 32: the fused plan needs 28), told by the two-stream plan's 5 slices per
    # wave; the same batch on one stream, 4 slices per wave, next to it
    Form("split-C", "C", {"ELPH_PCG_WG": "0", "ELPH_SPLIT_STREAMS": "1"}, {"px": 2, "plan_T": 5}, prec=True, parts=("batch",), batch=64),
    Form("px-C-64", "C", {"ELPH_PCG_WG": "0", "ELPH_SPLIT_STREAMS": "0"}, {"px": 2, "plan_T": 4}, prec=True, parts=("batch",), batch=64),
    # the whole preconditioned solve in one launch (pcg_wg.hip: k_pcg_wg)
    Form("pcg-wg-C", "C", {"ELPH_PCG_WG": "1"}, {"px": 0}, prec=True, batch=3),
    Form("pcg-wg-C80", "C80", {"ELPH_PCG_WG": "1"}, {"px": 0}, prec=True, batch=3),
]
IDS = [f.name for f in FORMS]


# ------------------------------------------------------------------------------------------ the checker

def _open(form, use_env, oracle, nchains=1, bounds=None):
    """(GPU model, expansion or None, the oracle's setup) of a form; with nchains > 1 the chains of stop_rule_cases.chain_fields resident."""
    from elphdynamics_amd import models, preconditioners as pc
    use_env(form.env)
    S = src.setup(oracle, form.model, form.prec, nchains, bounds)
    m = src.gpu_model(form.model)
    if nchains > 1:
        models.update_model_chains_(m, S.fields)
    P = None
    if form.prec:
        P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
        if nchains > 1:
            act, _, _ = pc.setup_chains_(P, e_min=np.array([b[0] for b in S.bounds]), e_max=np.array([b[1] for b in S.bounds]))
            assert act.all()
        else:
            pc.setup_(P, e_min=S.bounds[0][0], e_max=S.bounds[0][1])
    return m, P, S


def _set_solver(m, tol, kmax, maxiter):
    m.solver.tol, m.solver.kmax, m.solver.maxiter = float(tol), float(kmax), int(maxiter)


def check_singles(form, m, P, S):
    """Every single right-hand side of the form's model: solve_ with and without a history, then ldiv_."""
    from elphdynamics_amd import models
    for label, kind, c, tol, kmax, call, solver_mi, reason, _ in src.singles(form.key):
        xo, ito, histo = S.solve(kind, c, 0, tol, kmax, call)
        x0, b = S.guess(kind, c, 0), S.rhs(kind, 0)
        _set_solver(m, tol, kmax, solver_mi)
        x = x0.copy()
        it = models.solve_(x, m, b, P=P, tol=tol, kmax=kmax, maxiter=call)
        form.assert_ran(m, 1)
        xh = x0.copy()
        ith, hist = models.solve_(xh, m, b, P=P, tol=tol, kmax=kmax, maxiter=call, history=True)
        form.assert_ran(m, 1)
        d, dh = rel(x, xo), float(np.max(np.abs(hist[:ito + 1] - histo) / histo)) if len(hist) == len(histo) else np.inf
        print(f"{form.name} {label}: {reason} stop, iterations {it} (history on: {ith}, oracle {ito}), |x - x_oracle| / |x_oracle| = {d:.2e}, history {dh:.2e}")
        assert it == ito, (form.name, label, "screened path", it, ito)
        assert ith == ito, (form.name, label, "with a history", ith, ito)
        assert d < X_BOUND, (form.name, label, d)
        assert np.array_equal(x, xh), (form.name, label, "history on / off", rel(x, xh))
        assert dh < X_BOUND, (form.name, label, dh)
        # ldiv!: the flag logic on top (a call maxiter only where it differs from solver.maxiter)
        xl = x0.copy()
        itl, resl, fll = models.ldiv_(xl, m, b, P=P, maxiter=0 if call == solver_mi else call)
        xr, itr, resr, flr = S.ldiv(kind, c, 0, tol, kmax, solver_mi, 0 if call == solver_mi else call)
        assert (itl, fll) == (itr, flr), (form.name, label, "ldiv", itl, fll, itr, flr)
        assert abs(resl - resr) <= RESID_BOUND * resr, (form.name, label, resl, resr)
        if flr:
            assert not xl.any(), (form.name, label, "a flagged solution is zero-filled")
        elif form.prec and itr != ito:         # came back from the un-preconditioned retry
            assert rel(xl, xr) < RETRY_BOUND, (form.name, label, rel(xl, xr))
        else:
            assert np.array_equal(xl, x), (form.name, label, "ldiv_ and solve_ run the same solve")


def _kinds(n):
    """The kinds of a batch of n right-hand sides: stop_rule_cases.BATCH (an early tolerance stop first and last), tiled for the large
    batches of the fused forms, one of each kind for three."""
    if n == 3:
        return ("near", "zero", "far")
    k = [src.BATCH[r % 6] for r in range(n)]
    k[-1] = "near"
    return tuple(k)


def check_batch(form, m, P, S, which, nchains=1, alone=True):
    """One batch under parameter set `which` ("P" / "F"): right-hand side r on chain r % nchains, X carrying the guesses."""
    from elphdynamics_amd import models
    tol, kmax, mi, c = src.PARAMS[form.key][which]
    kinds = _kinds(form.batch)
    n = len(kinds)
    B = np.ascontiguousarray(np.tile(S.b, (n, 1)))
    X = np.ascontiguousarray(np.stack([S.guess(kinds[r], c, r % nchains) for r in range(n)]))
    X0 = X.copy()
    _set_solver(m, tol, kmax, mi)
    it, res, fl = models.ldiv_batched_(X, m, B, P=P)
    form.assert_ran(m, n, plan=not (form.prec and which == "F"))      # (set P ran first: the same handle, batch size and plan)
    same_variant = form.expect.get("wg") == 1 and probe(m, n, ("wg_T",))["wg_T"] == probe(m, 1, ("wg_T",))["wg_T"]
    for r in range(n):
        ch = r % nchains
        xo, ito, reso, flo = S.ldiv(kinds[r], c, ch, tol, kmax, mi)
        x1, it1, _ = S.solve(kinds[r], c, ch, tol, kmax, mi)
        retried = form.prec and ito != it1
        d = 0.0 if flo else rel(X[r], xo)
        print(f"{form.name} set {which} rhs {r} ({kinds[r]}, chain {ch}): iterations {it[r]} (oracle {ito}), flag {fl[r]} ({flo}), "
              f"residual {res[r]:.6e} ({reso:.6e}), |x - x_oracle| / |x_oracle| = {d:.2e}")
        assert (it[r], fl[r]) == (ito, flo), (form.name, which, r, kinds[r], it[r], fl[r], ito, flo)
        assert abs(res[r] - reso) <= RESID_BOUND * reso, (form.name, which, r, res[r], reso)
        if which == "P":
            assert flo == 0
        if flo:
            assert not X[r].any(), (form.name, which, r, "a flagged solution is zero-filled")
        else:
            assert d < (RETRY_BOUND if retried else X_BOUND), (form.name, which, r, kinds[r], d)
        if alone and nchains == 1 and r < 6:      # the same solve alone on the same handle: the others of the batch changed nothing
            xa = X0[r].copy()
            ita, resa, fla = models.ldiv_(xa, m, S.b, P=P)
            assert (ita, fla) == (it[r], fl[r]), (form.name, which, r, "alone", ita, fla)
            if same_variant:
                assert np.array_equal(xa, X[r]), (form.name, which, r, "alone: the same kernel variant gives the same bits", rel(xa, X[r]))
            elif not fla:
                assert rel(xa, X[r]) < (RETRY_BOUND if retried else X_BOUND), (form.name, which, r, "alone", rel(xa, X[r]))
    if which == "F" and not form.prec:
        assert sorted(set(fl.tolist())) == [0, 1, 2]


@pytest.mark.parametrize("form", FORMS, ids=IDS)
def test_stops_and_stopping_vectors(oracle, form_env, form):
    m, P, S = _open(form, form_env, oracle)
    try:
        if "singles" in form.parts:
            check_singles(form, m, P, S)
        if "batch" in form.parts:
            check_batch(form, m, P, S, "P")
            check_batch(form, m, P, S, "F")
    finally:
        m.close()


@pytest.mark.parametrize("form", [f for f in FORMS if "chains" in f.parts], ids=[f.name for f in FORMS if "chains" in f.parts])
def test_batch_with_two_chains(oracle, form_env, form):
    """The set P batch with two chains resident: right-hand side r on chain r % 2, every one against the oracle model of its chain."""
    assert form.key in src.CHAINS
    m, P, S = _open(form, form_env, oracle, nchains=2)
    try:
        check_batch(form, m, P, S, "P", nchains=2)
        check_batch(form, m, P, S, "F", nchains=2)
    finally:
        m.close()


@pytest.mark.parametrize("name", list(src.RETRY))
def test_retry_of_flagged_right_hand_sides_inside_a_preconditioned_batch(oracle, form_env, name):
    """ldiv_core's retry (Models.jl:129-133) with two chains resident under a deliberately weak expansion: right-hand sides 1 and 3 are
    flagged in the preconditioned pass and solved again alone, un-preconditioned, from zero, on THEIR chain (solo_chain), through the
    park / restore shuffle of slot 0; right-hand sides 0 and 2 keep their preconditioned solutions."""
    from elphdynamics_amd import models
    # the first pass: the five-kernel streaming form (four right-hand sides are below what the fused iteration is planned for)
    form = Form("retry-" + name, name, {"ELPH_PCG_WG": "0"}, {"px": 0, "plan_T": 1}, prec=True)
    tol, call = src.RETRY[name]
    m, P, S = _open(form, form_env, oracle, nchains=2, bounds=src.WEAK_BOUNDS)
    try:
        n = len(src.RETRY_SLOTS)
        B = np.ascontiguousarray(np.tile(S.b, (n, 1)))
        X = np.ascontiguousarray(np.stack([S.guess(kind, c, r % 2) for r, (kind, c) in enumerate(src.RETRY_SLOTS)]))
        _set_solver(m, tol, 1e12, src.RETRY_SOLVER_MAXITER)
        # which form runs a preconditioned pass of this batch shape: asked of a batch nothing of which is flagged (the probes read the plan of
        # the LAST solve, and a retry is an un-preconditioned solve of one right-hand side)
        Xn = np.ascontiguousarray(np.stack([S.guess("near", 1.0, r % 2) for r in range(n)]))
        _, _, fln = models.ldiv_batched_(Xn, m, B, P=P, maxiter=call)
        assert not fln.any()
        form.assert_ran(m, n)
        it, res, fl = models.ldiv_batched_(X, m, B, P=P, maxiter=call)
        form.assert_ran(m, n, plan=False)
        for r, (kind, c) in enumerate(src.RETRY_SLOTS):
            xo, ito, reso, flo = S.ldiv(kind, c, r % 2, tol, 1e12, src.RETRY_SOLVER_MAXITER, call)
            d = rel(X[r], xo)
            print(f"retry {name} rhs {r} ({kind}): iterations {it[r]} (oracle {ito}), flag {fl[r]} ({flo}), residual {res[r]:.6e} ({reso:.6e}), x {d:.2e}")
            assert (it[r], fl[r]) == (ito, flo) and flo == 0, (name, r, it[r], fl[r], ito, flo)
            assert abs(res[r] - reso) <= RESID_BOUND * reso, (name, r, res[r], reso)
            assert (ito > call) == (r in (1, 3))
            assert d < (RETRY_BOUND if r in (1, 3) else X_BOUND), (name, r, d)
    finally:
        m.close()
