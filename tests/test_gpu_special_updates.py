"""GPU (-m gpu): elph_hmc_special_update_chains / hmc.special_update_ — the special updates of every resident chain in one library
call, the columns drawn on the device (include/elph_gpu.h; SpecialUpdates.jl:97-366).

The draw is checked against its numpy restatement (tests/special_update_reference.py), the decisions and actions against the explicit
replay of the same batches through special_move_chains_ on a second handle that has no generator.  S0 and S1 of the two routes are
held to 1e-8 relative, the bound test_gpu_hmc.py::test_device_rng_equals_explicit_batches uses for them; the fields must agree bit
for bit, because the moves only permute or negate elements."""
import ctypes as C

import numpy as np
import pytest

import special_update_reference as sur

pytestmark = pytest.mark.gpu

SEED = 0x5EED5


def _dynamics(m, nch, with_kpm):
    from elphdynamics_amd import hmc, models, preconditioners as pc
    if m.kind == models.SSH:
        m.omega4 = np.zeros(m.Nph)
    fa = pc.FourierAccelerator(m)
    pc.update_M_(fa, m, 0.0, np.inf, 1.0, 0.3)
    H = hmc.HybridMonteCarlo(m, fa, dt=0.05, tr=0.1, alpha=0.0, Nb=1, nchains=nch)
    P = pc.SymmetricKPMPreconditioner(m, 16, 0.05, 1.0, 1.0) if with_kpm else None
    return H, P


def _make(tag, nch, with_kpm=False, prepare=None):
    """prepare(m): called on the model before anything reads its parameter arrays."""
    from elphdynamics_amd import configs
    m = configs.make_model(tag, tol=1e-9, maxiter=20000)
    if prepare is not None:
        prepare(m)
    H, P = _dynamics(m, nch, with_kpm)
    return m, H, P


def _fields(m, nch):
    """(nch, Ndof): a different rough field per chain, world lines all distinct."""
    from elphdynamics_amd import models, synth
    if m.kind == models.SSH:
        return np.stack([m.x * (0.8 + 0.1 * c) * (1.0 + 0.1 * synth.randn(700 + c, m.Ndof)) for c in range(nch)])
    return np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=900 + c) for c in range(nch)])


def _push(m, H, X):
    if H.nchains > 1:
        H.X[:] = X
    else:
        m.x[:] = X[0]
    H.push_()


def _pull(m, H):
    H.pull_()
    return (H.X if H.nchains > 1 else m.x.reshape(1, -1)).copy()


def _batches(m):
    n = C.c_uint64()
    assert m._lib.elph_hmc_rng_batches(m._h, C.byref(n)) == 0
    return n.value


def _assert_parity(a, b):
    """a: the namespace of special_update_; b: the dict of sur.replay of the same batches."""
    assert np.array_equal(a.col_i, b["col_i"]) and np.array_equal(a.col_j, b["col_j"])
    assert np.all(np.abs(b["u"] - b["P"]) > 1e-6), "a decision sits on the edge: pick another seed"
    assert not a.flags.any() and not b["flags"].any()
    print("accepted:", a.accepted.astype(int).tolist(), " least |u - P|:", np.min(np.abs(b["u"] - b["P"])))
    assert np.array_equal(a.accepted, b["accepted"].astype(bool))
    for x, y in ((a.S0, b["S0"]), (a.S1, b["S1"])):
        print("max relative difference of the actions:", np.max(np.abs(x - y) / np.abs(y)))
        assert np.all(np.abs(x - y) <= 1e-8 * np.abs(y))


PARITY = [("b", k, nch, kpm) for k in (sur.REFLECT, sur.SWAP) for nch in (1, 3) for kpm in (False, True)] + [("e", sur.SWAP, 3, False)]


@pytest.mark.parametrize("tag,kind,nch,with_kpm", PARITY)
def test_device_drawn_moves_equal_their_explicit_replay(tag, kind, nch, with_kpm):
    """Three moves drawn and decided on the device against the same three moves handed to special_move_chains_ one by one, with the
    columns of the restated draw and Rp, Rm, kpm_randn, u of the batch numbers the order draw, Rp, Rm, [kpm_randn], u gives."""
    check_device_drawn_moves_equal_their_explicit_replay(tag, kind, nch, with_kpm)


def check_device_drawn_moves_equal_their_explicit_replay(tag, kind, nch, with_kpm, prepare=None):
    from elphdynamics_amd import hmc
    nmoves = 3
    m, H, P = _make(tag, nch, with_kpm, prepare)
    X0 = _fields(m, nch)
    _push(m, H, X0)
    H.device_rng_(SEED)
    a = hmc.special_update_(m, H, kind, nmoves, P=P)
    assert a.accepted.shape == (nmoves, nch) and a.accepted.dtype == bool
    Xa, nb = _pull(m, H), _batches(m)
    m.close()
    m, H, P = _make(tag, nch, with_kpm, prepare)
    _push(m, H, X0)
    b = sur.replay(m, H, kind, nmoves, SEED, with_kpm, P, X0)
    Xb = _pull(m, H)
    m.close()
    _assert_parity(a, b)
    assert nb == b["batches"] == nmoves * (5 if with_kpm else 4)
    assert np.array_equal(Xa, Xb) and np.array_equal(Xa, b["fields"])


def _track(X, kind, res, nf):
    """The fields after the moves of `res` (columns and decisions as the device reported them), applied to X on the host."""
    X = np.array(X)
    for k in range(res.accepted.shape[0]):
        for c in range(X.shape[0]):
            if res.accepted[k, c]:
                X[c] = sur.apply_move(X[c], kind, res.col_i[k, c], res.col_j[k, c], nf)
    return X


def test_ssh_swap_on_crafted_world_lines():
    """Config e, three chains: all world lines distinct / all equal / all equal but one (exact copies or O(1) apart: ≈ is never near
    its threshold).  Equal lines: i == j, the field stays, the move is still evaluated and reported.  One odd line: j is the odd
    column, or one of the others when i is the odd one.  Columns against the restatement move by move, fields against the exchange."""
    from elphdynamics_amd import hmc, synth
    nch, nmoves, odd = 3, 4, 7
    m, H, P = _make("e", nch)
    nf, L = m.Nph, m.Ltau
    line = 0.3 * np.sin(2 * np.pi * np.arange(L) / L) + 0.2
    X0 = np.zeros((nch, nf, L))
    X0[0] = line[None, :] + 0.05 * np.arange(nf)[:, None]
    X0[1] = line
    X0[2] = line
    X0[2, odd] = 0.1 - line
    X0 = X0.reshape(nch, -1)
    _push(m, H, X0)
    H.device_rng_(SEED + 1)
    a = hmc.special_update_(m, H, sur.SWAP, nmoves)
    Xa = _pull(m, H)
    m.close()
    assert not a.flags.any() and np.all(a.iters > 0) and np.all(np.isfinite(a.S0)) and np.all(a.S0 != 0.0) and np.all(np.isfinite(a.S1))
    X = X0.copy()
    for k in range(nmoves):
        u = synth.uniform01(synth.batch_seed(SEED + 1, 4 * k + 1), 2 * nch)
        ci, cj = sur.draw(sur.SWAP, True, u, nf, fields=X)
        assert np.array_equal(a.col_i[k], ci) and np.array_equal(a.col_j[k], cj)
        assert ci[0] != cj[0] and ci[1] == cj[1]
        lines = X[2].reshape(nf, L)
        here, = [q for q in range(nf) if sum(np.array_equal(lines[q], lines[p]) for p in range(nf)) == 1]      # where the odd line is now
        assert (cj[2] == here) if ci[2] != here else (cj[2] != here)
        assert a.S0[k, 1] == a.S1[k, 1] or abs(a.S0[k, 1] - a.S1[k, 1]) < 1e-8 * abs(a.S0[k, 1])      # the identity: the same action, solved twice
        for c in range(nch):
            if a.accepted[k, c]:
                X[c] = sur.apply_move(X[c], sur.SWAP, ci[c], cj[c], nf)
    assert np.array_equal(Xa, X) and np.array_equal(Xa[1], X0[1])


def _ssh_square(L1, L2, ltau, nch):
    from elphdynamics_amd import lattice as lat, models, synth
    dtau = 0.05
    m = models.SSHModel(lat.Lattice(1, L1, L2, 1), ltau * dtau, dtau, tol=1e-9, maxiter=20000)
    for (o1, o2, d) in lat.SQUARE_BONDS:
        m.assign_hopping_(1.0, 0.1, 0.0, 0.1, o1, o2, d, name="xyz"[d.index(1)])
    m.initialize_model_()
    assert m.Ltau == ltau and m.Nph == 2 * L1 * L2
    m.x[:] = 0.25 * synth.phonon_field(m.Nph, m.Ltau, m.beta, dtau, omega=0.1, lam=0.0, seed=4242)
    models.update_model_(m)
    H, P = _dynamics(m, nch, False)
    return m, H


def test_ssh_draw_beyond_one_workgroup_of_columns():
    """A 12 x 12 square lattice with two bond definitions and Ltau = 5: 288 phonon columns — more than one workgroup's 256, no
    multiple of the wave size — on an odd, short time axis.  Chain 1 carries copies of its column i scattered over the columns
    (every third one and the last 40), so that D has gaps in every part of the selection.  One move; columns against the restatement.
    (The draw kernel walks the whole time axis per lane: there is no tile of tau to exceed.)"""
    from elphdynamics_amd import hmc, synth
    nch = 2
    m, H = _ssh_square(12, 12, 5, nch)
    nf, L = m.Nph, m.Ltau
    assert nf == 288 and L == 5
    u = synth.uniform01(synth.batch_seed(SEED + 2, 1), 2 * nch)
    X0 = np.stack([m.x * (1.0 + 0.1 * c) for c in range(nch)]).reshape(nch, nf, L)
    i1 = sur.pick(u[2], nf)
    copies = [q for q in range(nf) if q % 3 == 0 or q >= nf - 40]
    X0[1, copies] = X0[1, i1]
    X0 = X0.reshape(nch, -1)
    _push(m, H, X0)
    H.device_rng_(SEED + 2)
    a = hmc.special_update_(m, H, sur.SWAP, 1)
    Xa = _pull(m, H)
    m.close()
    ci, cj = sur.draw(sur.SWAP, True, u, nf, fields=X0)
    D1 = sur.different_columns(X0[1].reshape(nf, L), i1)
    assert len(D1) == nf - len(set(copies) | {i1}) and len(sur.different_columns(X0[0].reshape(nf, L), ci[0])) == nf - 1
    assert np.array_equal(a.col_i[0], ci) and np.array_equal(a.col_j[0], cj) and cj[1] in D1
    assert not a.flags.any() and np.array_equal(Xa, _track(X0, sur.SWAP, a, nf))


@pytest.mark.parametrize("kind", [sur.REFLECT, sur.SWAP])
def test_a_chain_of_three_decides_as_the_single_chain(kind):
    """Chain c of a 3-chain call decides and ends as the 1-chain move on that chain's field with that chain's columns and numbers
    (explicit replay on a single-chain handle without a generator)."""
    from elphdynamics_amd import hmc, synth
    nch, nmoves = 3, 2
    m, H, P = _make("b", nch)
    X0 = _fields(m, nch)
    _push(m, H, X0)
    H.device_rng_(SEED + 3)
    a = hmc.special_update_(m, H, kind, nmoves)
    Xa = _pull(m, H)
    ndim = m.Ndim
    m.close()
    assert not a.flags.any()
    for c in range(nch):
        m1, H1, P1 = _make("b", 1)
        _push(m1, H1, X0[c:c + 1])
        for k in range(nmoves):
            B = sur.Batches(SEED + 3, 4 * k + 1)                   # past the move's draw batch
            Rp, Rm, u = B.randn(nch * ndim).reshape(nch, ndim), B.randn(nch * ndim).reshape(nch, ndim), B.uniform(nch)
            acc, s0, s1, it, fl = hmc.special_move_chains_(m1, H1, kind, a.col_i[k, c:c + 1], a.col_j[k, c:c + 1],
                                                           randoms=dict(Rp=Rp[c], Rm=Rm[c], kpm_randn=None, u=u[c:c + 1]))
            Pacc = min(1.0, np.exp(-(s1[0] - s0[0])))
            assert abs(u[c] - Pacc) > 1e-6, "a decision sits on the edge: pick another seed"
            assert fl[0] == 0 and bool(acc[0]) == a.accepted[k, c]
            assert abs(s0[0] - a.S0[k, c]) <= 1e-8 * abs(s0[0]) and abs(s1[0] - a.S1[k, c]) <= 1e-8 * abs(s1[0])
        assert np.array_equal(_pull(m1, H1)[0], Xa[c])
        m1.close()


@pytest.mark.parametrize("kind", [sur.SWAP, sur.REFLECT])
def test_explicit_moves_of_three_chains_move_and_undo_per_chain(kind):
    """special_move_chains_ on a three-chain handle without a generator and without a preconditioner: the columns are uploaded, all chains
    move in one masked launch and the rejected ones are undone by the mask.  u = 0 accepts whenever the flag is 0 (chain 0), u = 1 can
    never lie below min(1, ·) (chain 2 is rejected and must come back bit for bit); chain 1 of the swap gets i == j, the identity:
    its field stays whatever its decision and S0 = S1, solved twice, to the 1e-8 this file holds an identity move to."""
    from elphdynamics_amd import hmc, synth
    nch = 3
    m, H, P = _make("b", nch)
    nf, ndim = m.Nph, m.Ndim
    assert (m.Nsites, m.Ltau) == (16, 20)
    X0 = _fields(m, nch)
    _push(m, H, X0)
    ci, cj = np.array([2, 5, 11]), np.array([9, 5, 4])
    r = dict(Rp=synth.randn(31, nch * ndim).reshape(nch, ndim), Rm=synth.randn(32, nch * ndim).reshape(nch, ndim), kpm_randn=None,
             u=np.array([0.0, 0.5, 1.0]))
    acc, s0, s1, it, fl = hmc.special_move_chains_(m, H, kind, ci, cj, randoms=r)
    X = _pull(m, H)
    m.close()
    print("accepted:", acc.astype(int).tolist(), " S0:", s0.tolist(), " S1:", s1.tolist(), " flags:", fl.tolist())
    assert not fl.any()
    assert acc[0] and np.array_equal(X[0], sur.apply_move(X0[0], kind, ci[0], cj[0], nf)) and not np.array_equal(X[0], X0[0])
    assert not acc[2] and np.array_equal(X[2], X0[2])
    if kind == sur.SWAP:
        assert np.array_equal(X[1], X0[1])
        assert abs(s0[1] - s1[1]) <= 1e-8 * abs(s0[1])
    else:                       # a reflection has no identity: chain 1's field follows its own decision
        assert np.array_equal(X[1], sur.apply_move(X0[1], kind, ci[1], cj[1], nf) if acc[1] else X0[1])


@pytest.mark.parametrize("tag,kind,with_kpm", [("e", sur.SWAP, False), ("b", sur.REFLECT, True)])
def test_the_same_seed_gives_the_same_run(tag, kind, with_kpm):
    """Deterministic reductions, no floating-point atomics: fields and every output repeat bit for bit."""
    from elphdynamics_amd import hmc
    runs = []
    for _ in range(2):
        m, H, P = _make(tag, 3, with_kpm)
        _push(m, H, _fields(m, 3))
        H.device_rng_(SEED + 4)
        a = hmc.special_update_(m, H, kind, 2, P=P)
        runs.append((a, _pull(m, H)))
        m.close()
    (a, Xa), (b, Xb) = runs
    assert np.array_equal(Xa, Xb)
    for k in ("accepted", "col_i", "col_j", "S0", "S1", "iters", "flags"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def _raw(m, kind, nmoves, nch):
    from elphdynamics_amd._lib import P_int
    acc = np.zeros((max(nmoves, 1), nch), dtype=np.int32)
    rc = m._lib.elph_hmc_special_update_chains(m._h, kind, nmoves, 0, acc.ctypes.data_as(P_int), None, None, None, None, None, None)
    return rc, m._lib.elph_last_error().decode()


def test_refusals_leave_the_handle_usable():
    from elphdynamics_amd import _lib, hmc
    from test_gpu_hmc import _ssh_golden_model
    from elphdynamics_amd import preconditioners as pc
    m, H, P = _make("b", 2)
    _push(m, H, _fields(m, 2))
    rc, msg = _raw(m, sur.REFLECT, 1, 2)
    assert rc == _lib.ELPH_E_STATE and "elph_hmc_set_rng" in msg              # no generator
    H.device_rng_(SEED)
    assert _raw(m, sur.REFLECT, 0, 2)[0] == _lib.ELPH_E_ARG                   # nmoves < 1
    assert _raw(m, 2, 1, 2)[0] == _lib.ELPH_E_ARG
    assert _batches(m) == 0                                                  # a refused call draws nothing
    # the same handle as the one rank of a sharded lattice
    N = m.Nsites
    gs, key = np.arange(N, dtype=np.int64), (C.c_ubyte * 64)()
    _lib.check(m._lib.elph_shard_create(m._h, 0, 1, 0, N, 0, 0, 0, N, 0, _lib.iptr(gs), C.cast(key, C.c_void_p)))
    assert _raw(m, sur.REFLECT, 1, 2)[0] == _lib.ELPH_E_UNSUPPORTED
    _lib.check(m._lib.elph_shard_destroy(m._h))
    a = hmc.special_update_(m, H, sur.REFLECT, 1)
    assert a.accepted.shape == (1, 2) and not a.flags.any() and _batches(m) == 4
    m.close()
    # shared fields
    g, hgold, ms = _ssh_golden_model(1, shared=True)
    fa = pc.FourierAccelerator(ms)
    fa.M[:] = g["faM"]
    Hs = hmc.HybridMonteCarlo(ms, fa, float(g["dt"]), int(g["nt"]) * float(g["dt"]), alpha=0.0, Nb=1)
    Hs.device_rng_(SEED)
    assert _raw(ms, sur.SWAP, 1, 1)[0] == _lib.ELPH_E_UNSUPPORTED
    acc, its = hmc.update_(ms, Hs, fa, None)                                  # still usable
    assert Hs.flag == 0
    ms.close()


def test_frequency_driven_helpers_with_the_device_draw():
    """reflection_update_ / swap_update_ with draw="device": one library call each, the mean accepted fraction of that call."""
    from elphdynamics_amd import hmc
    nch = 3
    for tag, helper, kind, count, want in (("b", hmc.reflection_update_, sur.REFLECT, 2, 2), ("b", hmc.swap_update_, sur.SWAP, 3, 3),
                                           ("e", hmc.swap_update_, sur.SWAP, 2, 2)):
        m, H, P = _make(tag, nch)
        X0 = _fields(m, nch)
        _push(m, H, X0)
        H.device_rng_(SEED + 5)
        frac = helper(m, H, count, None, draw="device")
        assert 0.0 <= frac <= 1.0 and _batches(m) == 4 * want
        _push(m, H, X0)
        H.device_rng_(SEED + 5)
        assert frac == float(hmc.special_update_(m, H, kind, want).accepted.mean())
        if tag == "e":
            assert hmc.reflection_update_(m, H, 2, None, draw="device") == 0.0 and _batches(m) == 4 * want      # not a Holstein model: nothing drawn
        m.close()
