"""What the nine measurement modules share above the library (measurements.py's docstring has the table of who measures what): the
container of resident chains with its host checks and device-side guards, written once, and the two implementations the four chain
modules are instances of, one for the on-site families (chain_measurements.py, ssh_chain_measurements.py) and one for the bond families
(chain_bond_measurements.py, ssh_chain_bond_measurements.py).  current_measurements.py uses the container, the checks and the guards;
the single-configuration modules use the guards, the bond-definition packing and the fetch pointers; snapshots.py and mu_tuner.py make
their folder, chain-count and row checks with the functions here.

A family is a small record.  Its `single` is the single-configuration module it delegates to, one container of which it keeps per chain;
an on-site one provides _new_container, initialize_measurement_folders_, _create_args(container, model, mu), _fetch_buffers,
_store_scalars, _process_fetched, write_measurements_ and _zero_container, a bond one _create_args(container, model), _process_fetched
and _zero_groups.  The library's functions are looked up by name, `prefix` + create / set_mu / accumulate / fetch / reset, where they
are called and not before: a model without a library passes every host check.

This module imports none of the measurement modules, so each of them may import it.
"""
import os
from collections import namedtuple

import numpy as np

from . import greens as _greens
from ._lib import P_dbl, check, dptr


class ChainContainer:
    """One single-configuration container per resident chain, and which device side holds their sums."""

    def __init__(self, chains, n_rand_vecs):
        self.chains = chains                 # one container of the family's single-configuration module per chain
        self.nchains = len(chains)
        self.n_rand_vecs = n_rand_vecs       # per chain
        self._device_of = None               # the model whose handle holds the device side ...
        self._device_est = None              # ... and the estimator it was shaped by: a newer one on the model has dropped it


def chain_folders(model, datafolders):
    """One data folder per chain resident in the model, as a list; a single name (str, PathLike) is the one folder of one chain."""
    nchains = int(getattr(model, "_nchains", 1))
    datafolders = [datafolders] if isinstance(datafolders, (str, os.PathLike)) else list(datafolders)
    if len(datafolders) != nchains:
        raise ValueError("%d data folders for the %d chains resident in the model" % (len(datafolders), nchains))
    return datafolders


def check_chains(c, model):
    if int(getattr(model, "_nchains", 1)) != c.nchains:
        raise ValueError("the container was made for %d chains, %d are resident in the model" % (c.nchains, getattr(model, "_nchains", 1)))


def check_vectors(c, Gr):
    if Gr.nv != c.n_rand_vecs * c.nchains:
        raise ValueError("the estimator holds %d vectors, the container normalises for num_random_vectors = %d for each of %d chains"
                         % (Gr.nv, c.n_rand_vecs, c.nchains))


def chain_rows(a, nchains, width, what):
    """`a` as float64 rows, one per chain; what: "X" (width Ndof) or "mu" (width Nsites)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (nchains, width):
        raise ValueError("%s has shape %s, not (nchains, %s) = (%d, %d)" % (what, a.shape, "Ndof" if what == "X" else "Nsites", nchains, width))
    return a


def device_current(c, model, Gr):
    """Whether the device side the container made is still the model's: same handle, and no newer estimator has dropped it."""
    return c._device_of is model and c._device_est is Gr


def require_device(c, model, what="nothing"):
    """In front of a fetch; what: "nothing", or "no" and the family's noun."""
    if c._device_of is not model:
        raise RuntimeError("%s has been measured on this model yet" % what)


def reset_device(c, model, name):
    """The tail of every reset: the device's accumulators to zero by the library's `name`, where the container has a device side."""
    if c._device_of is model and model is not None and getattr(model, "_h", None):
        check(getattr(model._lib, name)(model._h))


def pack_bond_definitions(defs):
    """(o1, o2, v) int32 arrays of a *_create call from [(o1, o2, (v1, v2, v3))]; one zero entry where there is no definition."""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    return i32([d[0] for d in defs] or [0]), i32([d[1] for d in defs] or [0]), i32([k for d in defs for k in d[2]] or [0, 0, 0])


def position_pointers(group, names):
    """The position arrays of `group` in the order of `names` for a *_fetch call, None for a correlation that is not measured."""
    return [group[name].position.ctypes.data_as(P_dbl) if name in group else None for name in names]


# refuse(model) raises for the model the family does not measure.  check_refuses: whether the host check in front of every accumulate
# repeats it; chain_measurements.py alone does not, and a caller sees the library's refusal there (kept as it is, not decided).
OnsiteFamily = namedtuple("OnsiteFamily", "single refuse check_refuses prefix")


def onsite_check(fam, cm, model, Gr, X, mu):
    """Everything that can be wrong on the host, before any library call."""
    assert Gr.model is model
    if fam.check_refuses:
        fam.refuse(model)
    check_chains(cm, model)
    check_vectors(cm, Gr)
    X = chain_rows(X, cm.nchains, model.Ndof, "X")
    if mu is not None:
        mu = chain_rows(mu, cm.nchains, model.Nsites, "mu")
    return X, mu


def onsite_accumulate(fam, cm, model, Gr, X, mu):
    X, mu = onsite_check(fam, cm, model, Gr, X, mu)
    if not device_current(cm, model, Gr):
        mu = np.ascontiguousarray(np.tile(model.mu, (cm.nchains, 1)), dtype=np.float64) if mu is None else mu
        args, keep = fam.single._create_args(cm.chains[0], model, mu)
        check(getattr(model._lib, fam.prefix + "create")(model._h, cm.nchains, *args))
        cm._device_of, cm._device_est = model, Gr
    elif mu is not None:                    # the tuners moved it since: the device's rows follow (a small copy), the sums so far are kept
        check(getattr(model._lib, fam.prefix + "set_mu")(model._h, dptr(mu)))
    check(getattr(model._lib, fam.prefix + "accumulate")(model._h, dptr(X)))


def onsite_make(fam, cm, model, Gr, X, P, R, rng, mu):
    X, mu = onsite_check(fam, cm, model, Gr, X, mu)
    out = _greens.update_(Gr, model, P, rng=rng, R=R)
    onsite_accumulate(fam, cm, model, Gr, X, mu)
    return out


def onsite_fetch(fam, cm, model):
    require_device(cm, model)
    for chain, c in enumerate(cm.chains):
        scal, ptrs = fam.single._fetch_buffers(c)
        check(getattr(model._lib, fam.prefix + "fetch")(model._h, chain, dptr(scal), *ptrs))
        fam.single._store_scalars(c, scal)


def onsite_reset(fam, cm, model):
    for c in cm.chains:
        fam.single._zero_container(c)
    reset_device(cm, model, fam.prefix + "reset")


# corr: the correlations in the order of the library's request and fetch arrays; takes_X: whether accumulate is given the chains'
# fields; noun: what a fetch before the first accumulate says has not been measured.
BondFamily = namedtuple("BondFamily", "single refuse prefix corr takes_X noun")


def bond_accumulate(fam, cb, model, Gr, X=None):
    assert Gr.model is model                # everything that can be wrong on the host, before any library call
    fam.refuse(model)
    check_chains(cb, model)
    check_vectors(cb, Gr)
    X = chain_rows(X, cb.nchains, model.Ndof, "X") if fam.takes_X else None
    if not cb.chains[0].intersite_corr:     # nothing requested: nothing to set up or fold
        return
    if not device_current(cb, model, Gr):
        args, keep = fam.single._create_args(cb.chains[0], model)
        check(getattr(model._lib, fam.prefix + "create")(model._h, cb.nchains, *args))
        cb._device_of, cb._device_est = model, Gr
    check(getattr(model._lib, fam.prefix + "accumulate")(model._h, *([dptr(X)] if fam.takes_X else [])))


def bond_fetch(fam, cb, model):
    require_device(cb, model, "no " + fam.noun)
    for chain, c in enumerate(cb.chains):
        check(getattr(model._lib, fam.prefix + "fetch")(model._h, chain, *position_pointers(c.intersite_corr, fam.corr)))


def bond_reset(fam, cb, model):
    for c in cb.chains:
        fam.single._zero_groups(c.intersite_corr, c.intersite_susc)
    reset_device(cb, model, fam.prefix + "reset")
