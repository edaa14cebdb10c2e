"""No GPU: the numpy restatement of the device draw of the special updates (tests/special_update_reference.py) on crafted fields,
the argument checks and early returns of the draw="device" helpers (hmc.reflection_update_ / swap_update_) on a stub dynamics
object — none of them may reach the library — and the declaration and binding of elph_hmc_special_update_chains."""
import os
import re
import types

import numpy as np
import pytest

import special_update_reference as sur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pick_clamps_the_uniform_that_rounds_to_one():
    assert sur.pick(1.0, 7) == 6 and sur.pick(0.0, 7) == 0 and sur.pick(1.0, 1) == 0
    assert sur.pick(np.nextafter(1.0, 0.0), 7) == 6 and sur.pick(3.0 / 7.0, 7) in (2, 3)
    assert [sur.pick(u, 4) for u in (0.1, 0.3, 0.6, 0.9)] == [0, 1, 2, 3]


def test_isapprox_is_julias():
    a = np.array([1.0, 2.0, 3.0])
    assert sur.isapprox(a, a.copy()) and sur.isapprox(a, a * (1 + 1e-9)) and not sur.isapprox(a, a * (1 + 1e-7))
    assert sur.isapprox(np.zeros(3), np.zeros(3)) and not sur.isapprox(np.zeros(3), 1e-100 * np.ones(3))      # no absolute tolerance


def _crafted(nf=6, L=5):
    line = 0.3 * np.sin(2 * np.pi * np.arange(L) / L) + 0.2
    distinct = line[None, :] + 0.05 * np.arange(nf)[:, None]
    equal = np.tile(line, (nf, 1))
    one_odd = equal.copy()
    one_odd[4] = 0.1 - line
    return distinct, equal, one_odd


def test_different_columns_and_the_empty_set():
    distinct, equal, one_odd = _crafted()
    nf = distinct.shape[0]
    for i in range(nf):
        assert sur.different_columns(distinct, i) == [q for q in range(nf) if q != i]
        assert sur.different_columns(equal, i) == []
        assert sur.different_columns(one_odd, i) == ([4] if i != 4 else [0, 1, 2, 3, 5])
    # D empty: the identity, whatever u1 says
    for u1 in (0.0, 0.5, 1.0):
        assert sur.ssh_pair(equal, 0.4, u1) == (2, 2)
    # one odd line: j is forced to it, or ranges over the others when i is the odd one
    assert sur.ssh_pair(one_odd, 0.0, 0.99) == (0, 4)
    assert [sur.ssh_pair(one_odd, 4.5 / 6, u1)[1] for u1 in (0.0, 0.21, 0.41, 0.61, 0.81, 1.0)] == [0, 1, 2, 3, 5, 5]
    # all distinct: j = the r-th column other than i, in increasing order
    assert sur.ssh_pair(distinct, 2.5 / 6, 0.0) == (2, 0) and sur.ssh_pair(distinct, 2.5 / 6, 0.5) == (2, 3) and sur.ssh_pair(distinct, 2.5 / 6, 1.0) == (2, 5)


def test_draw_uses_two_uniforms_per_chain():
    from elphdynamics_amd import synth
    distinct, equal, one_odd = _crafted()
    nf = distinct.shape[0]
    u = synth.uniform01(synth.batch_seed(11, 1), 6)
    ci, cj = sur.draw(sur.SWAP, True, u, nf, fields=np.stack([distinct.reshape(-1), equal.reshape(-1), one_odd.reshape(-1)]))
    assert [int(c) for c in ci] == [sur.pick(u[0], nf), sur.pick(u[2], nf), sur.pick(u[4], nf)]
    assert ci[0] != cj[0] and ci[1] == cj[1] and ((cj[2] == 4) if ci[2] != 4 else (cj[2] != 4))
    ri, rj = sur.draw(sur.REFLECT, False, u, nf)
    assert np.array_equal(ri, ci) and np.array_equal(rj, ri)
    table = np.array([[1, 2], [2, 3], [3, 1], [1, 4]])
    bi, bj = sur.draw(sur.SWAP, False, u, nf, table=table)
    assert [(int(a), int(b)) for a, b in zip(bi, bj)] == [tuple(table[sur.pick(u[2 * c], 4)] - 1) for c in range(3)]
    X = sur.apply_move(one_odd.reshape(-1), sur.SWAP, 0, 4, nf).reshape(nf, -1)
    assert np.array_equal(X[0], one_odd[4]) and np.array_equal(X[4], one_odd[0]) and np.array_equal(X[1], one_odd[1])
    assert np.array_equal(sur.apply_move(distinct.reshape(-1), sur.REFLECT, 3, 3, nf).reshape(nf, -1)[3], -distinct[3])


class _NoLibrary:
    """A model whose library must not be touched: any attribute of the handle or the library raises."""

    def __init__(self, kind, Nph=8, Nbonds=16):
        self.kind, self.Nph, self.Nbonds, self.Ltau = kind, Nph, Nbonds, 4

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached: model.{name}")


def _stub(device_rng, nchains=2):
    return types.SimpleNamespace(device_rng=device_rng, nchains=nchains)


def test_device_draw_wants_the_generator_and_no_host_rng():
    from elphdynamics_amd import hmc, models
    for kind in (models.HOLSTEIN, models.SSH):
        m = _NoLibrary(kind)
        for helper in (hmc.reflection_update_, hmc.swap_update_):
            with pytest.raises(ValueError, match="device_rng_"):
                helper(m, _stub(False), 2, None, draw="device")
            with pytest.raises(ValueError, match="rng"):
                helper(m, _stub(True), 2, None, rng=np.random.default_rng(1), draw="device")
            with pytest.raises(ValueError, match="draw"):
                helper(m, _stub(True), 2, None, draw="gpu")


def test_device_draw_keeps_the_early_returns():
    from elphdynamics_amd import hmc, models
    on = _stub(True)
    assert hmc.reflection_update_(_NoLibrary(models.SSH), on, 3, None, draw="device") == 0.0          # not a Holstein model
    assert hmc.reflection_update_(_NoLibrary(models.HOLSTEIN), on, 0, None, draw="device") == 0.0
    assert hmc.swap_update_(_NoLibrary(models.HOLSTEIN), on, 0, None, draw="device") == 0.0
    assert hmc.swap_update_(_NoLibrary(models.HOLSTEIN, Nbonds=0), on, 2, None, draw="device") == 0.0
    assert hmc.swap_update_(_NoLibrary(models.SSH, Nph=1, Nbonds=1), on, 2, None, draw="device") == 0.0
    # the host route's early returns are what they were
    assert hmc.reflection_update_(_NoLibrary(models.SSH), _stub(False), 3, None) == 0.0
    assert hmc.swap_update_(_NoLibrary(models.HOLSTEIN), _stub(False), 0, None) == 0.0


def test_device_draw_is_one_call_with_the_clamped_count(monkeypatch):
    """min(Nph, nsites) reflections, min(Nbonds, nbonds) swaps, the mean of `accepted` of that one call."""
    from elphdynamics_amd import hmc, models
    calls = []

    def fake(model, H, kind, nmoves, P=None):
        calls.append((kind, nmoves, P))
        acc = np.zeros((nmoves, H.nchains), dtype=bool)
        acc[0, 0] = True
        return types.SimpleNamespace(accepted=acc)

    monkeypatch.setattr(hmc, "special_update_", fake)
    on = _stub(True, nchains=2)
    assert hmc.reflection_update_(_NoLibrary(models.HOLSTEIN, Nph=8), on, 20, "P", draw="device") == 1 / 16
    assert hmc.swap_update_(_NoLibrary(models.HOLSTEIN, Nbonds=16), on, 3, None, draw="device") == 1 / 6
    assert hmc.swap_update_(_NoLibrary(models.SSH, Nph=8, Nbonds=4), on, 9, None, draw="device") == 1 / 8
    assert calls == [(hmc.REFLECT, 8, "P"), (hmc.SWAP, 3, None), (hmc.SWAP, 4, None)]


def test_the_entry_is_declared_and_bound():
    import ctypes as C
    from elphdynamics_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "elph_gpu.h")).read()
    proto = re.search(r"^int elph_hmc_special_update_chains\(([^;]*)\);", hdr, re.M | re.S)
    assert proto, "include/elph_gpu.h does not declare elph_hmc_special_update_chains"
    args = [a.strip() for a in proto.group(1).replace("\n", " ").split(",")]
    assert len(args) == 11 and args[0] == "elph_handle h" and args[2] == "int64_t nmoves"
    assert "SpecialUpdates.jl:97-366" in hdr and ":113" in hdr and ":248-258" in hdr and ":324-328" in hdr
    assert re.search(r"^#define ELPH_ABI_VERSION 2$", hdr, re.M) and _lib.ABI_VERSION == 2
    res, argtypes = _lib.SIGNATURES["elph_hmc_special_update_chains"]
    assert res is C.c_int and len(argtypes) == 11
    assert argtypes == [_lib.Handle, C.c_int, C.c_int64, C.c_int, _lib.P_int, _lib.P_i64, _lib.P_i64, _lib.P_dbl, _lib.P_dbl, _lib.P_i64, _lib.P_int]
    assert hasattr(_lib.load(), "elph_hmc_special_update_chains")
