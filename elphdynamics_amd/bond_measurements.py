"""Host-side mirror of the inter-site correlation group of Measurements.jl for the Holstein model: BondBond, BondPairGreens and the
susceptibility BondPairSusc, accumulated on the device (csrc/bondcorr.hip) with the reference's per-bin processing and files.

    c = initialize_bond_container(model, info, datafolder, bond_definitions=None)   init_corr_container! / init_susc_container!, :156-175, :767-819
    initialize_bond_folders_(c)                                                     the inter-site parts of :420-540
    accumulate_bonds_(c, model, Gr)                                                 measure_BondBond! (:1663-1785), measure_BondPairGreens! (:2390-2483)
    fetch_bonds_(c, model)
    process_bond_measurements_(c, bin_size, model)                                  the inter-site parts of :574-676, BondPairSusc :666-672
    write_bond_measurements_(c, model, bin)                                         :681-693
    reset_bond_measurements_(c, model)                                              :698-758

It stands beside measurements.MeasurementsContainer (whose constructor keeps refusing the inter-site correlations by name) and is used
next to one on the same model and estimator, in either order.  `info` is the same `[measurements]` table; `bond_definitions` is a list of
(o1, o2, (v1, v2, v3)) (Bond.o1, Bond.o2, Bond.v of the reference's model.bond_definitions), by default what model.assign_t_ recorded.  The
constructor makes no library call; the device side (elph_bond_create) is made by the first accumulate_bonds_.

Arrays as in measurements.py: `position` and `momentum` complex128 (L0, L1, L2, L3, n_p) in Fortran order, `pairs` int (2, n_p) of 1-based
bond-definition indices: pairs[0, p] is the bond at the origin (n'' of the reference), pairs[1, p] the displaced one (n').

Scope.  CurrentCurrent with measure = true is refused with UnsupportedMeasurement: the reference's Holstein method scales its fields by
the hopping inside `for tau in L_tau`, which visits the last time slice alone, and whether to mirror that is undecided.  So are a request
on a model without bond definitions, the SSH model and several chains resident; sharded and slab handles are refused by the library.
"""
import os
from math import comb

import numpy as np

from ._lib import P_dbl, P_int, check
from .measurements import Correlation, UnsupportedMeasurement, _key_file, _pairs, _write_correlation, simpson

BOND_CORR = ("BondBond", "BondPairGreens")                 # the order of elph_bond_create's request arrays
BOND_SUSC_OF = (("BondPairSusc", "BondPairGreens"),)       # :156-175


class BondContainer:
    def __init__(self):
        self.intersite_corr, self.intersite_susc = {}, {}
        self.bond_definitions = []
        self.n_rand_vecs = 1
        self.datafolder = ""
        self._device_of = None           # the model whose handle holds the device side


def _refuse_model(model):
    if getattr(model, "kind", None) != 0:
        raise UnsupportedMeasurement("bond correlations of the SSH model are not supported (Holstein only)")
    if getattr(model, "_nchains", 1) > 1:
        raise UnsupportedMeasurement("bond correlations with several chains resident (model._nchains = %d) are not supported" % model._nchains)


def initialize_bond_container(model, info, datafolder, bond_definitions=None):
    """The inter-site group of initialize_measurements_container(holstein, info, datafolder) (:156-175)."""
    _refuse_model(model)
    info = info or {}
    if info.get("CurrentCurrent", {}).get("measure", False) is True:
        raise UnsupportedMeasurement("[measurements.CurrentCurrent] measure = true: not supported; the reference's Holstein method scales "
                                     "its fields by the hopping on the last time slice only (`for tau in L_tau`), and whether to mirror "
                                     "that is undecided")
    defs = bond_definitions if bond_definitions is not None else getattr(model, "bond_definitions", [])
    defs = [(int(o1), int(o2), tuple(int(k) for k in v)) for o1, o2, v in defs]
    lat = model.lattice
    L, L1, L2, L3 = model.Ltau, lat.L1, lat.L2, lat.L3
    c = BondContainer()
    c.n_rand_vecs = int(info.get("num_random_vectors", 1))                  # :36-40
    c.datafolder = datafolder
    c.bond_definitions = defs
    for name in BOND_CORR:                                                  # init_corr_container!, :767-796
        entry = info.get(name)
        if entry is None or entry.get("measure", False) is not True:
            continue
        if not defs:
            raise UnsupportedMeasurement("[measurements.%s] measure = true: the model has no bond definitions (none recorded by assign_t_, "
                                         "none passed)" % name)
        pairs = _pairs(entry, len(defs))
        L0 = L + 1 if entry.get("time_dependent", False) is True else 1
        c.intersite_corr[name] = Correlation((L0, L1, L2, L3, pairs.shape[1]), pairs)
    for susc, corr in BOND_SUSC_OF:                                         # init_susc_container!, :801-819
        if corr in c.intersite_corr and c.intersite_corr[corr].position.shape[0] > 1:
            pairs = c.intersite_corr[corr].pairs
            c.intersite_susc[susc] = Correlation((L1, L2, L3, pairs.shape[1]), pairs)
    return c


def initialize_bond_folders_(container):
    """The inter-site parts of initialize_measurement_folders!(container) (:420-540)."""
    d = container.datafolder
    for group, cols in ((container.intersite_corr, " tau"), (container.intersite_susc, "")):
        for k, corr in group.items():
            for space, letter in (("position", "r"), ("momentum", "k")):
                folder = os.path.join(d, "%s_%s_f" % (k, space))
                os.mkdir(folder)
                header = "index bond1 bond2 %s3 %s2 %s1%s" % (letter, letter, letter, cols)
                _key_file(os.path.join(folder, "%s_%s_key.out" % (k, space)), header, getattr(corr, space), corr.pairs)


def _ensure_device(container, model, Gr):
    if container._device_of is model:
        return
    _refuse_model(model)
    assert Gr.model is model
    if Gr.nv != container.n_rand_vecs:
        raise ValueError("the estimator holds %d vectors, the container normalises for num_random_vectors = %d" % (Gr.nv, container.n_rand_vecs))
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(P_int)  # noqa: E731
    defs, corr = container.bond_definitions, container.intersite_corr
    o1, o2 = i32([d[0] for d in defs] or [0]), i32([d[1] for d in defs] or [0])
    v = i32([k for d in defs for k in d[2]] or [0, 0, 0])
    measure = i32([name in corr for name in BOND_CORR])
    timedep = i32([name in corr and corr[name].position.shape[0] > 1 for name in BOND_CORR])
    npairs = i32([corr[name].pairs.shape[1] if name in corr else 0 for name in BOND_CORR])
    plist = [corr[name].pairs.T.reshape(-1) for name in BOND_CORR if name in corr]
    pairs = i32(np.concatenate(plist)) if plist else i32([0, 0])
    check(model._lib.elph_bond_create(model._h, len(defs), ip(o1), ip(o2), ip(v), ip(measure), ip(timedep), ip(npairs), ip(pairs)))
    container._device_of = model


def accumulate_bonds_(container, model, Gr):
    """measure_BondBond! and measure_BondPairGreens! for every pair i < j of the estimator's vectors (the loop of make_measurements!,
    :550-560), folded into the device's accumulators; nothing comes back to the host."""
    _refuse_model(model)
    if not container.intersite_corr:                                        # nothing requested: nothing to set up or fold
        return
    _ensure_device(container, model, Gr)
    check(model._lib.elph_bond_accumulate(model._h))
    Gr.n1, Gr.n2 = Gr.nv - 1, Gr.nv                                         # the estimator's device tables are the last pair's now


def fetch_bonds_(container, model):
    """The device's un-normalised sums into the container's position arrays; the momentum arrays are not touched."""
    if container._device_of is not model:
        raise RuntimeError("no bond correlation has been measured on this model yet")
    corr = container.intersite_corr
    ptrs = [corr[name].position.ctypes.data_as(P_dbl) if name in corr else None for name in BOND_CORR]
    check(model._lib.elph_bond_fetch(model._h, *ptrs))


def process_bond_measurements_(container, bin_size, model):
    """The inter-site parts of process_measurements!(container, sim_params, model) (:574-676): fetch, momentum = fft over the cell axes,
    division by bin_size * binomial(n_rand_vecs, 2), Simpson's rule over tau for BondPairSusc (:666-672)."""
    fetch_bonds_(container, model)
    V = int(bin_size) * comb(container.n_rand_vecs, 2)
    if V == 0:
        raise ValueError("bin_size * binomial(num_random_vectors = %d, 2) is zero" % container.n_rand_vecs)
    for corr in container.intersite_corr.values():
        corr.momentum[...] = np.fft.fftn(corr.position, axes=(1, 2, 3))
        corr.position /= V
        corr.momentum /= V
    for susc, name in BOND_SUSC_OF:
        if susc in container.intersite_susc:
            container.intersite_susc[susc].position[...] = simpson(container.intersite_corr[name].position, model.dtau)
            container.intersite_susc[susc].momentum[...] = simpson(container.intersite_corr[name].momentum, model.dtau)


def write_bond_measurements_(container, model, bin):
    """The inter-site correlations and susceptibilities of write_measurements!(container, model, bin) (:681-693, :1258-1274)."""
    for group in (container.intersite_corr, container.intersite_susc):
        for name, corr in group.items():
            _write_correlation(corr.position, name, "position", container.datafolder, bin)
            _write_correlation(corr.momentum, name, "momentum", container.datafolder, bin)


def reset_bond_measurements_(container, model):
    """reset_measurements!(container, model) (:698-758) for the inter-site correlations: the container's arrays and the device's
    accumulators to zero."""
    for group in (container.intersite_corr, container.intersite_susc):
        for corr in group.values():
            corr.position[...] = 0
            corr.momentum[...] = 0
    if container._device_of is model and model is not None and getattr(model, "_h", None):
        check(model._lib.elph_bond_reset(model._h))
