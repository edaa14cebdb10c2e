"""Host-side mirror of the inter-site correlation group of Measurements.jl for the bond-phonon (SSH) model: BondBond, CurrentCurrent,
BondPairGreens and the susceptibility BondPairSusc (:295-302, :322), accumulated on the device (csrc/ssh_bondcorr.hip) with the
reference's per-bin processing and files.  It stands beside ssh_measurements.py as bond_measurements.py stands beside measurements.py.

    c = initialize_ssh_bond_container(model, info, datafolder)       init_corr_container! / init_susc_container!, :295-302, :322, :767-819
    initialize_ssh_bond_folders_(c)                                  the inter-site parts of :420-540
    accumulate_ssh_bonds_(c, model, Gr)                              measure_BondBond! (:1663-1785), measure_CurrentCurrent!(ssh) (:2100-2384),
                                                                     measure_BondPairGreens! (:2390-2483)
    fetch_ssh_bonds_(c, model)
    process_ssh_bond_measurements_(c, bin_size, model)               the inter-site parts of :574-676, BondPairSusc :666-672
    write_ssh_bond_measurements_(c, model, bin)                      :681-693
    reset_ssh_bond_measurements_(c, model)                           :698-758

It is used next to an SSHMeasurementsContainer (whose constructor keeps refusing the three names) on the same model and estimator, in
either order.  `info` is the same `[measurements]` table; the bond definitions are model.bond_definitions (what assign_hopping_
recorded), pairs default to all n_def^2.  The constructor makes no library call; the device side (elph_ssh_bond_create) is made by the
first accumulate_ssh_bonds_.  Arrays as in bond_measurements.py: pairs[0, p] is the bond at the origin (n'' of the reference),
pairs[1, p] the displaced one (n').  CurrentCurrent has no susceptibility.

measure_CurrentCurrent! is mirrored as it executes, which differs from its comments in three places.  The fourth of its eight terms is
subtracted (:2231) under a comment that says `J +=`.  The sixth term averages the field of n'' against the field of n', in that order
(:2256-2260), unlike the other seven.  The b == c delta term reads M^-1 r1[:, b] (:2340) where its comment names a.
Where the reference throws: the b == c term indexes with r'' unreduced (:2336-2348), a BoundsError for a negative or >= L displacement;
here r'' is reduced mod L.  The reshape of t' to (Ltau, L1, L2, L3, n_def) (:2145) throws unless Nbonds = n_def * ncells; the library
refuses a CurrentCurrent request there (ELPH_E_UNSUPPORTED naming both counts), BondBond and BondPairGreens stay available.

Scope: the table in measurements.py's docstring has what each of the nine modules measures and refuses, this one included.
"""
import numpy as np

from ._chain_unit import pack_bond_definitions, position_pointers, require_device, reset_device
from ._lib import check, dptr, iptr
from .bond_measurements import BondContainer
from .measurements import (INTERSITE_CORR, UnsupportedMeasurement, _bin_volume, _check_estimator, _corr_group, _group_folders, _i32, _ip,  # noqa: F401
                           _process_group, _refuse_chains, _refuse_holstein, _request_arrays, _requested, _susc_group, _write_groups, _zero_groups, simpson)

SSH_BOND_CORR = INTERSITE_CORR                                 # BondBond, CurrentCurrent, BondPairGreens: elph_ssh_bond_create's request order
SSH_BOND_SUSC_OF = (("BondPairSusc", "BondPairGreens"),)       # :322
SUBJECT = "SSH bond correlations"


class SSHBondContainer(BondContainer):
    """The same fields."""


def _refuse_model(model):
    _refuse_holstein(model, SUBJECT)
    _refuse_chains(model, SUBJECT)


def _new_ssh_bond_container(model, info, datafolder):
    """The container of one configuration for the request `info`, after the caller has decided that the model is measured."""
    info = info or {}
    defs = [(int(d["o1"]), int(d["o2"]), tuple(int(k) for k in d["v"])) for d in getattr(model, "bond_definitions", [])]
    dims = (model.lattice.L1, model.lattice.L2, model.lattice.L3)
    c = SSHBondContainer()
    c.n_rand_vecs = int(info.get("num_random_vectors", 1))                  # :189-193
    c.datafolder = datafolder
    c.bond_definitions = defs
    if not defs and _requested(info, SSH_BOND_CORR):
        raise UnsupportedMeasurement("[measurements.%s] measure = true: the model has no bond definitions (none recorded by assign_hopping_)"
                                     % _requested(info, SSH_BOND_CORR)[0])
    c.intersite_corr = _corr_group(info, SSH_BOND_CORR, len(defs), model.Ltau, dims)
    c.intersite_susc = _susc_group(c.intersite_corr, SSH_BOND_SUSC_OF, dims)
    return c


def initialize_ssh_bond_container(model, info, datafolder):
    """The BondBond, CurrentCurrent, BondPairGreens and BondPairSusc part of initialize_measurements_container(ssh, info, datafolder)
    (:295-302, :322)."""
    _refuse_model(model)
    return _new_ssh_bond_container(model, info, datafolder)


def initialize_ssh_bond_folders_(container):
    """The inter-site parts of initialize_measurement_folders!(container) (:420-540)."""
    _group_folders(container.datafolder, container.intersite_corr, container.intersite_susc, "bond1", "bond2")


def _create_args(container, model):
    """The arguments of elph_ssh_bond_create after the handle and of elph_ssh_bond_chains_create after nchains: the bond definitions, the
    bonds and phonons of the model, the request.  Second value: the arrays the pointers refer to, to be kept alive across the call."""
    defs = container.bond_definitions
    o1, o2, v = pack_bond_definitions(defs)
    request = _request_arrays(container.intersite_corr, SSH_BOND_CORR)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)  # noqa: E731
    nb, nph_tot = int(model.Nbonds), int(model.Nph)
    t, b2d, b2p = f64(model.t), i64(model.bond_to_definition), i64(model.bond_to_phonon)
    al, al2 = f64(model.alpha), f64(model.alpha2)
    args = [len(defs), _ip(o1), _ip(o2), _ip(v), nb, dptr(t) if nb else None, iptr(b2d) if nb else None, iptr(b2p) if nb else None, nph_tot,
            dptr(al) if nph_tot else None, dptr(al2) if nph_tot else None] + [_ip(a) for a in request]
    return args, (o1, o2, v, t, b2d, b2p, al, al2, request)


def _ensure_device(container, model, Gr):
    if container._device_of is model:
        return
    _refuse_model(model)
    _check_estimator(container, model, Gr)
    args, keep = _create_args(container, model)
    check(model._lib.elph_ssh_bond_create(model._h, *args))
    container._device_of = model


def accumulate_ssh_bonds_(container, model, Gr):
    """measure_BondBond!, measure_CurrentCurrent! and measure_BondPairGreens! for every pair i < j of the estimator's vectors (the loop of
    make_measurements!, :550-560), folded into the device's accumulators; nothing comes back to the host."""
    _refuse_model(model)
    if not container.intersite_corr:                                        # nothing requested: nothing to set up or fold
        return
    _ensure_device(container, model, Gr)
    check(model._lib.elph_ssh_bond_accumulate(model._h, dptr(np.ascontiguousarray(model.x, dtype=np.float64))))
    Gr.n1, Gr.n2 = Gr.nv - 1, Gr.nv                                         # the estimator's device tables are the last pair's now


def fetch_ssh_bonds_(container, model):
    """The device's un-normalised sums into the container's position arrays; the momentum arrays are not touched."""
    require_device(container, model, "no SSH bond correlation")
    check(model._lib.elph_ssh_bond_fetch(model._h, *position_pointers(container.intersite_corr, SSH_BOND_CORR)))


def process_ssh_bond_measurements_(container, bin_size, model):
    """The inter-site parts of process_measurements!(container, sim_params, model) (:574-676): fetch, momentum = fft over the cell axes,
    division by bin_size * binomial(n_rand_vecs, 2), Simpson's rule over tau for BondPairSusc (:666-672)."""
    fetch_ssh_bonds_(container, model)
    _process_fetched(container, bin_size, model.dtau)


def _process_fetched(container, bin_size, dtau):
    _process_group(container.intersite_corr, container.intersite_susc, SSH_BOND_SUSC_OF, _bin_volume(container, bin_size), dtau)


def write_ssh_bond_measurements_(container, model, bin):
    """The inter-site correlations and susceptibilities of write_measurements!(container, model, bin) (:681-693, :1258-1274)."""
    _write_groups(container.datafolder, bin, container.intersite_corr, container.intersite_susc)


def reset_ssh_bond_measurements_(container, model):
    """reset_measurements!(container, model) (:698-758) for the three correlations: the container's arrays and the device's accumulators
    to zero."""
    _zero_groups(container.intersite_corr, container.intersite_susc)
    reset_device(container, model, "elph_ssh_bond_reset")
