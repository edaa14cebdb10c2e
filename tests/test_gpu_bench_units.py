"""The timed units of elph_bench_run (csrc/bench_hooks.hip) — the code bench.py measures — on handles of Ltau = 16: what every unit leaves
in x (elph_bench_get_x), that every unit returns a positive time, and the codes of the calls it refuses.

  * what = 1 (8 x 8, 4 right-hand sides) and what = 3 (16 x 16, KPM set up, 8 right-hand sides): the repetitions of one call continue where
    the last call stopped — 32 in one call leave the bits of 16 + 16.  (Counts in multiples of ELPH_CG_CHUNK: the ping-pong parity.)
  * what = 11: the batch as two half-batches on two streams (cg_solve.hip: SplitRun) leaves the bits of what = 3 — with ELPH_CHUNK_T
    pinned, as test_preconditioned_batch_as_two_half_batches_on_two_streams asserts it of whole solves.  The batch is of 56 right-hand
    sides, not 8: split_legal wants the halves p/x-fused, and at Ltau = 16 the tau-transforms carry the fused updates from 28 vectors on
    (dft_mfma.hip: elph_plan_dft) — 56 is the smallest batch it accepts on this handle, 54 is refused; elph_bench_px_info reports the
    iteration fused.
  * what = 9, 10, 12: the resident forms, each at the smallest shape its probe accepts — 8 x 8 (elph_bench_wg_info); 18 x 18, the smallest
    lattice of test_gpu_slabs.py (elph_bench_slabs_info under ELPH_SLABS=1); and for what = 10 the 16 x 16 lattice with one right-hand side
    at Ltau = 160, not 16: pcg_wg.hip (pcg_shape) takes the time axes whose transform tables have 20 or 40 tiles, of which 160 slices are the
    shortest, and one right-hand side only under ELPH_PCG_WG=1 (by default from six); it has no probe of its own, the call itself answers
    ELPH_E_UNSUPPORTED elsewhere — as it does on the Ltau = 16 handle.  After 16 repetitions x is the streaming form's x of the same handle
    after 16 repetitions up to RESIDENT_BOUND.  The resident forms group their partial sums differently, and the streaming forms apply
    x += alpha p one iteration late (elph_bench.h), so the two differ by more than round-off; the bound is measured, not guessed: on the
    library of the commit before these units were split out of elph_api.hip the relative differences |x_res - x_str| / |x_str| were
        what = 9:  3.436e-02      what = 10: 1.331e-03      what = 12: 3.683e-02
    and RESIDENT_BOUND is ten times the largest of them.
  * what = 0, 2, 4 - 8: ELPH_OK and a positive time.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RESIDENT_BOUND = 3.7e-01
REPS = 16


def _row(L):
    from elphdynamics_amd import lattice as lat
    return ("holstein", 1, L, lat.SQUARE_BONDS, 1.6, 0.1)      # Ltau = 16


def _rhs(m, n, seed):
    from elphdynamics_amd import synth
    return np.ascontiguousarray(np.stack([synth.randn(seed + r, m.Ndim) for r in range(n)]))


def _prepare(m, what, B):
    from elphdynamics_amd import _lib
    _lib.check(_lib.load().elph_bench_prepare(m._h, what, B.shape[0], _lib.dptr(B)))


def _run(m, what, nrhs, reps, use_graph=0):
    """(return code, ms) of one elph_bench_run"""
    from elphdynamics_amd import _lib
    ms = C.c_double(-1.0)
    return _lib.load().elph_bench_run(m._h, what, nrhs, reps, use_graph, C.byref(ms)), ms.value


def _timed(m, what, nrhs, reps):
    from elphdynamics_amd import _lib
    rc, ms = _run(m, what, nrhs, reps)
    _lib.check(rc)
    assert ms > 0.0, (what, ms)
    return ms


def _x(m, nrhs):
    from elphdynamics_amd import _lib
    X = np.empty((nrhs, m.Ndim))
    _lib.check(_lib.load().elph_bench_get_x(m._h, nrhs, _lib.dptr(X)))
    return X


def _after(m, prep, B, runs):
    """x after elph_bench_prepare(prep) and the (what, reps) calls of `runs`"""
    _prepare(m, prep, B)
    for what, reps in runs:
        _timed(m, what, B.shape[0], reps)
    return _x(m, B.shape[0])


def _not_cooling(m):
    from elphdynamics_amd import _lib
    cd, fb = C.c_int(), C.c_int64()
    _lib.check(_lib.load().elph_wg_status(m._h, C.byref(cd), C.byref(fb)))
    assert (cd.value, fb.value) == (0, 0)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _resident_vs_streaming(m, what, prep, stream, B):
    """the relative difference of x after REPS repetitions of a resident form (prepared as `prep`) and of the streaming form of the same handle"""
    xs = _after(m, stream, B, [(stream, REPS)])
    _not_cooling(m)
    xr = _after(m, prep, B, [(what, REPS)])
    _not_cooling(m)
    d = _rel(xr, xs)
    print(f"what = {what}: |x_res - x_str| / |x_str| = {d:.3e} after {REPS} repetitions")
    assert np.isfinite(xr).all() and np.linalg.norm(xs) > 0.0
    return d


@pytest.fixture(scope="module")
def sq8():
    from elphdynamics_amd import configs
    m = configs.make_model(_row(8), tol=1e-8)
    assert m.Ltau == 16
    yield m, _rhs(m, 4, 8600)
    m.close()


@pytest.fixture(scope="module")
def sq16():
    """16 x 16 with the chunk length pinned (read at elph_create) and the preconditioner set up"""
    from elphdynamics_amd import configs, preconditioners as pc, synth
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ELPH_CHUNK_T", "4")
        m = configs.make_model(_row(16), tol=1e-8)
    assert m.Ltau == 16
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, b_max=synth.randn(1, m.Nsites), b_min=synth.randn(2, m.Nsites))
    yield m, _rhs(m, 8, 8700)
    m.close()


def test_streaming_iteration_continues_across_calls(sq8):
    m, B = sq8
    assert np.array_equal(_after(m, 1, B, [(1, 32)]), _after(m, 1, B, [(1, 16), (1, 16)]))


def test_preconditioned_iteration_continues_across_calls(sq16):
    m, B = sq16
    assert np.array_equal(_after(m, 3, B, [(3, 32)]), _after(m, 3, B, [(3, 16), (3, 16)]))


def test_two_streams_leave_the_bits_of_one(sq16):
    from elphdynamics_amd import _lib
    m, _ = sq16
    B = _rhs(m, 56, 8900)
    x3 = _after(m, 3, B, [(3, REPS)])
    fused = C.c_int()
    _lib.check(_lib.load().elph_bench_px_info(m._h, C.byref(fused)))
    assert fused.value != 0
    x11 = _after(m, 3, B, [(11, REPS)])
    assert np.array_equal(x11, x3) and np.abs(x3).max() > 0.0
    assert _run(m, 11, 54, REPS)[0] == _lib.ELPH_E_UNSUPPORTED


def test_resident_cg_against_streaming(sq8):
    from elphdynamics_amd import _lib
    m, B = sq8
    v = [C.c_int() for _ in range(4)]
    _lib.check(_lib.load().elph_bench_wg_info(m._h, B.shape[0], *[C.byref(x) for x in v]))
    assert v[0].value == 1
    assert _resident_vs_streaming(m, 9, 1, 1, B) <= RESIDENT_BOUND


def test_resident_preconditioned_cg_against_streaming(sq16, monkeypatch):
    from elphdynamics_amd import _lib, configs, preconditioners as pc, synth
    monkeypatch.setenv("ELPH_PCG_WG", "1")
    m16, B16 = sq16
    _prepare(m16, 10, B16[:1])
    assert _run(m16, 10, 1, REPS)[0] == _lib.ELPH_E_UNSUPPORTED      # Ltau = 16: two tiles
    m = configs.make_model("C", tol=1e-8)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_(P, b_max=synth.randn(1, m.Nsites), b_min=synth.randn(2, m.Nsites))
    d = _resident_vs_streaming(m, 10, 10, 3, _rhs(m, 1, 9000))
    m.close()
    assert d <= RESIDENT_BOUND


def test_slab_form_against_streaming(monkeypatch):
    from elphdynamics_amd import _lib, configs
    monkeypatch.setenv("ELPH_SLABS", "1")
    m = configs.make_model(_row(18), tol=1e-8)
    assert m.Ltau == 16
    v = [C.c_int() for _ in range(4)]
    _lib.check(_lib.load().elph_bench_slabs_info(m._h, 1, *[C.byref(x) for x in v]))
    assert v[0].value == 1
    d = _resident_vs_streaming(m, 12, 1, 1, _rhs(m, 1, 8800))
    m.close()
    assert d <= RESIDENT_BOUND


@pytest.mark.parametrize("what", [0, 2, 4, 5, 6, 7, 8])
def test_single_kernel_units_return_a_time(sq16, what):
    m, B = sq16
    _prepare(m, what, B)
    _timed(m, what, B.shape[0], REPS)


def test_refused_calls(sq16):
    from elphdynamics_amd import _lib
    m, B = sq16
    _prepare(m, 3, B)
    assert _run(m, 3, 1 << 20, REPS)[0] == _lib.ELPH_E_ARG                         # beyond the reserved capacity
    assert _run(m, 11, 3, REPS)[0] == _lib.ELPH_E_UNSUPPORTED                       # split_legal: no two whole halves
    assert _run(m, 3, B.shape[0], REPS, use_graph=1)[0] == _lib.ELPH_E_UNSUPPORTED
    # a refused call launches nothing: the batch goes on as if it had not been made
    x = _after(m, 3, B, [(3, REPS)])
    _prepare(m, 3, B)
    assert _run(m, 11, 3, REPS)[0] == _lib.ELPH_E_UNSUPPORTED
    _timed(m, 3, B.shape[0], REPS)
    assert np.array_equal(_x(m, B.shape[0]), x)
