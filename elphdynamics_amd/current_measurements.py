"""CurrentCurrent of the Holstein model (measure_CurrentCurrent!(..., model::HolsteinModel, ...), Measurements.jl:1790-2098), accumulated
on the device (csrc/currcorr.hip) for one configuration or for every chain resident in a handle (a lockstep run), with the reference's
per-bin processing and files.  A container of its own beside the bond containers (bond_measurements.py, chain_bond_measurements.py) and
the on-site ones, on the precedent of snapshots.py: those keep refusing a true [measurements.CurrentCurrent] entry, and split_info hands
each kind of container its part of one deck's [measurements] table.

    rest, cur = split_info(info)                                                        info without its CurrentCurrent entry; that entry with num_random_vectors
    c = initialize_current_container(model, info, datafolders, bond_definitions=None)   init_corr_container! (:157-162, :767-796) per chain
    initialize_current_folders_(c)                                                      CurrentCurrent's part of :420-540 per chain
    accumulate_current_(c, model, Gr)                                                   measure_CurrentCurrent! (:1790-2098): every pair of a chain's vectors, all chains at once
    fetch_current_(c, model)                                                            the device's sums into the chains' position arrays
    process_current_measurements_(c, bin_size, model)                                   CurrentCurrent's part of :574-676 per chain
    write_current_measurements_(c, model, bin)                                          :681-693 per chain, into the chain's folder
    reset_current_measurements_(c, model)                                               :698-758

The reference is mirrored as it executes.  Its Holstein method builds the fields, translation averages, delta terms and tau = beta slice
of the SSH method (ssh_bond_measurements.py) and weights every factor by the static hopping model.t inside `for tau in L_tau`, a loop
that visits the last time slice alone: the weight of a bond is 1 on slices 1 .. L_tau - 1 and its t on slice L_tau.  With t = 1
everywhere the number is the physical one; otherwise it is what the reference produces (csrc/currcorr.hip's header has the lines).

datafolders is one string (one configuration) or one folder per resident chain; c.chains holds one CurrentChain per chain, each with
the `intersite_corr` group {"CurrentCurrent": Correlation} of measurements.py (position and momentum complex128 (L0, L1, L2, L3, n_p) in
Fortran order, pairs int (2, n_p) of 1-based bond-definition indices, pairs[0, p] the bond at the origin).  `info` is the [measurements]
table (or split_info's second part); `bond_definitions` as bond_measurements.py takes them, by default what model.assign_t_ recorded.
The constructor makes no library call; the device side (elph_current_create, given model.t and model.Nbonds) is made by the first
accumulate_current_, and again after a new EstimateGreensFunction on the model has dropped it.  The method reads the estimator's vectors
and nothing setup_ makes: Gr.n1 and Gr.n2 are left alone.  The estimator serves the chains with n_rand_vecs * nchains vectors, vector v
of chain c at index v * nchains + c; a bin is normalised by bin_size * binomial(n_rand_vecs, 2) with the vectors PER CHAIN.
CurrentCurrent has no susceptibility (:157-162).

Scope: the table in measurements.py's docstring has what each of the nine modules measures and refuses, this one included; the container,
its host checks and its device-side guards are _chain_unit.py's.  Refused by the library besides sharded and slab handles: a model whose
Nbonds is not n_def * ncells (the reference's reshape of t fails).
"""
import os

import numpy as np

from . import _chain_unit as _cu
from ._lib import check, dptr
from .measurements import (UnsupportedMeasurement, _bin_volume, _check_estimator, _corr_group, _group_folders, _ip, _process_group,
                           _refuse_ssh, _request_arrays, _write_groups, _zero_groups)

CURRENT_CORR = ("CurrentCurrent",)
SUBJECT = "CurrentCurrent measurements"


class CurrentChain:
    """One chain's part: the group the helpers of measurements.py work on, its folder, and the vectors per chain."""

    def __init__(self, intersite_corr, datafolder, n_rand_vecs):
        self.intersite_corr = intersite_corr
        self.datafolder = datafolder
        self.n_rand_vecs = n_rand_vecs


class CurrentContainer(_cu.ChainContainer):
    """chains: one CurrentChain per chain."""

    def __init__(self, chains, bond_definitions, n_rand_vecs):
        super().__init__(chains, n_rand_vecs)
        self.bond_definitions = bond_definitions


def split_info(info):
    """(info without its CurrentCurrent entry, {"CurrentCurrent": that entry, "num_random_vectors": ...}): one [measurements] table for
    all containers."""
    rest = dict(info or {})
    cur = {}
    if "CurrentCurrent" in rest:
        cur["CurrentCurrent"] = rest.pop("CurrentCurrent")
    if "num_random_vectors" in rest:
        cur["num_random_vectors"] = rest["num_random_vectors"]
    return rest, cur


def initialize_current_container(model, info, datafolders, bond_definitions=None):
    """CurrentCurrent's part of initialize_measurements_container(holstein, info, datafolder) (:157-162) for every resident chain."""
    _refuse_ssh(model, SUBJECT)
    info = info or {}
    datafolders = _cu.chain_folders(model, datafolders)
    defs = bond_definitions if bond_definitions is not None else getattr(model, "bond_definitions", [])
    defs = [(int(o1), int(o2), tuple(int(k) for k in v)) for o1, o2, v in defs]
    requested = (info.get("CurrentCurrent") or {}).get("measure", False) is True
    if requested and not defs:
        raise UnsupportedMeasurement("[measurements.CurrentCurrent] measure = true: the model has no bond definitions (none recorded by "
                                     "assign_t_, none passed)")
    dims = (model.lattice.L1, model.lattice.L2, model.lattice.L3)
    nv = int(info.get("num_random_vectors", 1))                             # :36-40
    chains = [CurrentChain(_corr_group(info, CURRENT_CORR, len(defs), model.Ltau, dims), os.fspath(f), nv) for f in datafolders]
    return CurrentContainer(chains, defs, nv)


def initialize_current_folders_(c):
    """CurrentCurrent's parts of initialize_measurement_folders!(container) (:420-540), in every chain's folder."""
    for ch in c.chains:
        _group_folders(ch.datafolder, ch.intersite_corr, {}, "bond1", "bond2")


def _check(c, model, Gr):
    """Everything that can be wrong on the host, before any library call."""
    _refuse_ssh(model, SUBJECT)
    _cu.check_chains(c, model)
    if c.nchains == 1:
        _check_estimator(c, model, Gr)
    else:
        assert Gr.model is model
        _cu.check_vectors(c, Gr)


def _ensure_device(c, model, Gr):
    if _cu.device_current(c, model, Gr):
        return
    defs = c.bond_definitions
    o1, o2, v = _cu.pack_bond_definitions(defs)
    measure, td, npairs, pairs = _request_arrays(c.chains[0].intersite_corr, CURRENT_CORR)
    t = np.ascontiguousarray(model.t, dtype=np.float64)
    check(model._lib.elph_current_create(model._h, c.nchains, len(defs), _ip(o1), _ip(o2), _ip(v), int(model.Nbonds), dptr(t) if t.size else None,
                                         int(measure[0]), int(td[0]), int(npairs[0]), _ip(pairs)))
    c._device_of, c._device_est = model, Gr


def accumulate_current_(c, model, Gr):
    """measure_CurrentCurrent! for every pair v1 < v2 of a chain's vectors (the loop of make_measurements!, :550-560), folded into the
    device's accumulators for all chains at once; nothing comes back to the host, and the estimator's own tables (Gr.n1, Gr.n2) are not
    touched."""
    _check(c, model, Gr)
    if not c.chains[0].intersite_corr:                                      # nothing requested: nothing to set up or fold
        return
    _ensure_device(c, model, Gr)
    check(model._lib.elph_current_accumulate(model._h))


def fetch_current_(c, model):
    """The device's un-normalised sums into every chain's position array; the momentum arrays are not touched."""
    _cu.require_device(c, model, "no CurrentCurrent")
    for chain, ch in enumerate(c.chains):
        check(model._lib.elph_current_fetch(model._h, chain, *_cu.position_pointers(ch.intersite_corr, CURRENT_CORR)))


def _process_fetched(c, bin_size, dtau):
    for ch in c.chains:
        _process_group(ch.intersite_corr, {}, (), _bin_volume(ch, bin_size), dtau)


def process_current_measurements_(c, bin_size, model):
    """CurrentCurrent's part of process_measurements!(container, sim_params, model) (:574-676) per chain: fetch, momentum = fft over the
    cell axes, division by bin_size * binomial(n_rand_vecs, 2)."""
    fetch_current_(c, model)
    _process_fetched(c, bin_size, model.dtau)


def write_current_measurements_(c, model, bin):
    """CurrentCurrent_position_f / CurrentCurrent_momentum_f of write_measurements!(container, model, bin) (:681-693, :1258-1274), into
    every chain's folder."""
    for ch in c.chains:
        _write_groups(ch.datafolder, bin, ch.intersite_corr)


def reset_current_measurements_(c, model):
    """reset_measurements!(container, model) (:698-758) for CurrentCurrent: every chain's arrays and the device's accumulators to zero."""
    for ch in c.chains:
        _zero_groups(ch.intersite_corr)
    _cu.reset_device(c, model, "elph_current_reset")
