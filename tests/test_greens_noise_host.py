"""greens.update_'s choice between the host-drawn and the device-drawn update (no GPU: the library calls are recorded by a stub).

Precedence: an explicit R takes elph_greens_update whatever the flag says; est.device_rng alone takes elph_greens_update_rng and copies no
vector; neither takes elph_greens_update with vectors from `rng`."""
from types import SimpleNamespace

import numpy as np


class StubLib:
    """Every entry point succeeds and is recorded as (name, args)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("elph_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call

    def names(self):
        return [n for n, _ in self.calls]


def stub_estimator(nv=3):
    from elphdynamics_amd import greens
    lib = StubLib()
    model = SimpleNamespace(_lib=lib, _h=None, _nchains=1, Ndim=8, Ltau=2, Nsites=4, lattice=SimpleNamespace(L1=2, L2=2, L3=1, norbits=1))
    est = greens.EstimateGreensFunction(model, nv=nv)
    assert lib.names() == ["elph_greens_create"] and est.device_rng is False
    lib.calls.clear()
    return lib, model, est


def test_device_rng_sets_the_flag_through_the_library_and_pull_fetches_both_arrays():
    lib, model, est = stub_estimator()
    est.device_rng_(2 ** 64 + 7)                                            # seeds are taken mod 2^64
    assert est.device_rng is True
    (name, (h, seed)), = lib.calls
    assert name == "elph_greens_set_rng" and h is None and seed.value == 7
    lib.calls.clear()
    est.pull_()
    (name, (h, R, X)), = lib.calls
    assert name == "elph_greens_get_vectors" and R is not None and X is not None


def test_an_explicit_R_takes_the_old_path_even_with_the_flag_set():
    from elphdynamics_amd import greens
    lib, model, est = stub_estimator()
    est.device_rng_(1)
    lib.calls.clear()
    R = np.arange(24.0).reshape(3, 8)
    it, res, fl = greens.update_(est, model, R=R)
    assert lib.names() == ["elph_greens_update", "elph_greens_get_vectors"]
    assert np.array_equal(est.R, R) and it.shape == res.shape == fl.shape == (3,)
    assert lib.calls[1][1][1] is None                                       # only M^-1 R is copied back, as before


def test_the_flag_alone_takes_the_device_drawn_update_and_copies_nothing():
    from elphdynamics_amd import greens

    class NoDraws:
        def standard_normal(self, *a, **k):
            raise AssertionError("rng must not be asked for noise vectors on the device-drawn path")

    lib, model, est = stub_estimator()
    est.device_rng_(1)
    lib.calls.clear()
    it, res, fl = greens.update_(est, model, rng=NoDraws())
    assert lib.names() == ["elph_greens_update_rng"]
    name, (h, use_prec, *outs) = lib.calls[0]
    assert use_prec == 0 and len(outs) == 3 and all(o is not None for o in outs)
    assert not est.R.any() and not est.MinvR.any()                          # the host mirrors stay as they were (stale until pull_)
    assert it.shape == res.shape == fl.shape == (3,)


def test_neither_takes_the_old_path_with_vectors_from_rng():
    from elphdynamics_amd import greens
    lib, model, est = stub_estimator()
    greens.update_(est, model, rng=np.random.default_rng(4))
    assert lib.names() == ["elph_greens_update", "elph_greens_get_vectors"]
    assert np.array_equal(est.R, np.random.default_rng(4).standard_normal((3, 8)))
