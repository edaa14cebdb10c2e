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

Scope: the table in measurements.py's docstring has what each of the nine modules measures and refuses, this one included.  The message
that refuses CurrentCurrent here is from before the question it names was settled: current_measurements.py measures it, mirroring the
reference's Holstein method as it executes.
"""
from ._chain_unit import pack_bond_definitions, position_pointers, require_device, reset_device
from ._lib import check
from .measurements import (UnsupportedMeasurement, _bin_volume, _check_estimator, _corr_group, _group_folders, _i32, _ip, _process_group,
                           _refuse_model, _request_arrays, _requested, _susc_group, _write_groups, _zero_groups, simpson)  # noqa: F401

BOND_CORR = ("BondBond", "BondPairGreens")                 # the order of elph_bond_create's request arrays
BOND_SUSC_OF = (("BondPairSusc", "BondPairGreens"),)       # :156-175


class BondContainer:
    def __init__(self):
        self.intersite_corr, self.intersite_susc = {}, {}
        self.bond_definitions = []
        self.n_rand_vecs = 1
        self.datafolder = ""
        self._device_of = None           # the model whose handle holds the device side


SUBJECT = "bond correlations"


def _new_bond_container(model, info, datafolder, bond_definitions=None):
    """The container of one configuration for the request `info`, after the caller has decided that the model is measured: the requests
    neither path measures are refused here."""
    info = info or {}
    if info.get("CurrentCurrent", {}).get("measure", False) is True:
        raise UnsupportedMeasurement("[measurements.CurrentCurrent] measure = true: not supported; the reference's Holstein method scales "
                                     "its fields by the hopping on the last time slice only (`for tau in L_tau`), and whether to mirror "
                                     "that is undecided")
    defs = bond_definitions if bond_definitions is not None else getattr(model, "bond_definitions", [])
    defs = [(int(o1), int(o2), tuple(int(k) for k in v)) for o1, o2, v in defs]
    dims = (model.lattice.L1, model.lattice.L2, model.lattice.L3)
    c = BondContainer()
    c.n_rand_vecs = int(info.get("num_random_vectors", 1))                  # :36-40
    c.datafolder = datafolder
    c.bond_definitions = defs
    if not defs and _requested(info, BOND_CORR):
        raise UnsupportedMeasurement("[measurements.%s] measure = true: the model has no bond definitions (none recorded by assign_t_, "
                                     "none passed)" % _requested(info, BOND_CORR)[0])
    c.intersite_corr = _corr_group(info, BOND_CORR, len(defs), model.Ltau, dims)
    c.intersite_susc = _susc_group(c.intersite_corr, BOND_SUSC_OF, dims)
    return c


def initialize_bond_container(model, info, datafolder, bond_definitions=None):
    """The inter-site group of initialize_measurements_container(holstein, info, datafolder) (:156-175)."""
    _refuse_model(model, SUBJECT)
    return _new_bond_container(model, info, datafolder, bond_definitions)


def initialize_bond_folders_(container):
    """The inter-site parts of initialize_measurement_folders!(container) (:420-540)."""
    _group_folders(container.datafolder, container.intersite_corr, container.intersite_susc, "bond1", "bond2")


def _create_args(container, model):
    """The arguments of elph_bond_create after the handle and of elph_bond_chains_create after nchains: the bond definitions and the
    request (nothing of the model).  Second value: the arrays the pointers refer to, to be kept alive across the call."""
    arrays = pack_bond_definitions(container.bond_definitions) + _request_arrays(container.intersite_corr, BOND_CORR)
    return [len(container.bond_definitions), *map(_ip, arrays)], arrays


def _ensure_device(container, model, Gr):
    if container._device_of is model:
        return
    _refuse_model(model, SUBJECT)
    _check_estimator(container, model, Gr)
    args, keep = _create_args(container, model)
    check(model._lib.elph_bond_create(model._h, *args))
    container._device_of = model


def accumulate_bonds_(container, model, Gr):
    """measure_BondBond! and measure_BondPairGreens! for every pair i < j of the estimator's vectors (the loop of make_measurements!,
    :550-560), folded into the device's accumulators; nothing comes back to the host."""
    _refuse_model(model, SUBJECT)
    if not container.intersite_corr:                                        # nothing requested: nothing to set up or fold
        return
    _ensure_device(container, model, Gr)
    check(model._lib.elph_bond_accumulate(model._h))
    Gr.n1, Gr.n2 = Gr.nv - 1, Gr.nv                                         # the estimator's device tables are the last pair's now


def fetch_bonds_(container, model):
    """The device's un-normalised sums into the container's position arrays; the momentum arrays are not touched."""
    require_device(container, model, "no bond correlation")
    check(model._lib.elph_bond_fetch(model._h, *position_pointers(container.intersite_corr, BOND_CORR)))


def process_bond_measurements_(container, bin_size, model):
    """The inter-site parts of process_measurements!(container, sim_params, model) (:574-676): fetch, momentum = fft over the cell axes,
    division by bin_size * binomial(n_rand_vecs, 2), Simpson's rule over tau for BondPairSusc (:666-672)."""
    fetch_bonds_(container, model)
    _process_fetched(container, bin_size, model.dtau)


def _process_fetched(container, bin_size, dtau):
    _process_group(container.intersite_corr, container.intersite_susc, BOND_SUSC_OF, _bin_volume(container, bin_size), dtau)


def write_bond_measurements_(container, model, bin):
    """The inter-site correlations and susceptibilities of write_measurements!(container, model, bin) (:681-693, :1258-1274)."""
    _write_groups(container.datafolder, bin, container.intersite_corr, container.intersite_susc)


def reset_bond_measurements_(container, model):
    """reset_measurements!(container, model) (:698-758) for the inter-site correlations: the container's arrays and the device's
    accumulators to zero."""
    _zero_groups(container.intersite_corr, container.intersite_susc)
    reset_device(container, model, "elph_bond_reset")
