"""Bond correlations of every chain resident in a handle (a lockstep run: hmc.update_chains_, langevin.evolve_): the chain-aware twin
of bond_measurements.py, beside chain_measurements.py the way bond_measurements.py stands beside measurements.py.  One BondContainer per
chain, each with its own data folder; on the device all chains are accumulated by the same launches (elph_bond_chains_*,
csrc/bondcorr.hip), the chain a grid axis.

    cb = initialize_chain_bond_container(model, info, datafolders, bond_definitions=None)   one container per chain (:156-175, :767-819 each)
    initialize_bond_folders_(cb)                                                            the inter-site parts of :420-540 per chain
    accumulate_bonds_(cb, model, Gr)                                                        measure_BondBond! (:1663-1785), measure_BondPairGreens!
                                                                                            (:2390-2483): every pair of a chain's vectors, all chains at once
    fetch_bonds_(cb, model)                                                                 the device's sums into the chains' containers
    process_bond_measurements_(cb, bin_size, model)                                         the inter-site parts of :574-676, BondPairSusc :666-672, per chain
    write_bond_measurements_(cb, model, bin)                                                :681-693 per chain, into the chain's folder
    reset_bond_measurements_(cb, model)                                                     :698-758

The correlations read the estimator's vectors and neither the field nor mu, so accumulate_bonds_ takes no X.  The estimator serves the
chains with n_rand_vecs * nchains vectors, vector v of chain c at index v * nchains + c (greens.chain_vector), as
process_input_file(deck, nchains=n) builds it; a bin is normalised by bin_size * binomial(n_rand_vecs, 2) with the vectors PER CHAIN.  A
chain's folder holds exactly the files bond_measurements.py writes for one configuration, BondPairSusc included.

It is used next to a chain_measurements.ChainMeasurementsContainer (whose constructor keeps refusing the inter-site requests by name) on
the same model and estimator, in either order: the two device sides are separate, and neither touches the estimator's own tables, so
Gr.n1 and Gr.n2 are left alone.

The device side is shaped by the estimator and dropped by the library when a new EstimateGreensFunction is made on the model (with the
sums it held): the next accumulate_bonds_ with the new estimator makes it again.

Scope: what bond_measurements.py measures for one configuration.  Refused with UnsupportedMeasurement naming the request:
CurrentCurrent with measure = true (current_measurements.py measures it for every resident chain, in a container of its own beside this
one; its split_info hands this constructor the table without that entry), the SSH model, a request on a model without bond definitions.  bond_measurements.py itself keeps
refusing resident chains; sharded and slab handles are refused by the library.
"""
from . import bond_measurements as _bm
from .measurements import _i32, _ip, _refuse_ssh, _request_arrays
from ._lib import P_dbl, check

UnsupportedMeasurement = _bm.UnsupportedMeasurement
SUBJECT = "chain bond correlations"


class ChainBondContainer:
    def __init__(self, chains, n_rand_vecs):
        self.chains = chains                 # one BondContainer per chain
        self.nchains = len(chains)
        self.n_rand_vecs = n_rand_vecs       # per chain
        self._device_of = None               # the model whose handle holds the device side ...
        self._device_est = None              # ... and the estimator it was shaped by: a newer one on the model has dropped it


def initialize_chain_bond_container(model, info, datafolders, bond_definitions=None):
    """One BondContainer per resident chain of `model` for the request `info`; datafolders: one folder per chain."""
    _refuse_ssh(model, SUBJECT)
    nchains = int(getattr(model, "_nchains", 1))
    datafolders = list(datafolders)
    if len(datafolders) != nchains:
        raise ValueError("%d data folders for the %d chains resident in the model" % (len(datafolders), nchains))
    chains = [_bm._new_bond_container(model, info, folder, bond_definitions) for folder in datafolders]
    return ChainBondContainer(chains, chains[0].n_rand_vecs)


def initialize_bond_folders_(cb):
    for c in cb.chains:
        _bm.initialize_bond_folders_(c)


def _check(cb, model, Gr):
    """Everything that can be wrong on the host, before any library call."""
    assert Gr.model is model
    _refuse_ssh(model, SUBJECT)
    if int(getattr(model, "_nchains", 1)) != cb.nchains:
        raise ValueError("the container was made for %d chains, %d are resident in the model" % (cb.nchains, getattr(model, "_nchains", 1)))
    if Gr.nv != cb.n_rand_vecs * cb.nchains:
        raise ValueError("the estimator holds %d vectors, the container normalises for num_random_vectors = %d for each of %d chains"
                         % (Gr.nv, cb.n_rand_vecs, cb.nchains))


def _ensure_device(cb, model, Gr):
    if cb._device_of is model and cb._device_est is Gr:
        return
    first = cb.chains[0]
    defs = first.bond_definitions
    o1, o2 = _i32([d[0] for d in defs] or [0]), _i32([d[1] for d in defs] or [0])
    v = _i32([k for d in defs for k in d[2]] or [0, 0, 0])
    request = _request_arrays(first.intersite_corr, _bm.BOND_CORR)
    check(model._lib.elph_bond_chains_create(model._h, cb.nchains, len(defs), _ip(o1), _ip(o2), _ip(v), *map(_ip, request)))
    cb._device_of, cb._device_est = model, Gr


def accumulate_bonds_(cb, model, Gr):
    """measure_BondBond! and measure_BondPairGreens! for every pair v1 < v2 of a chain's vectors, folded into the device's accumulators
    for all chains at once; nothing comes back to the host, and the estimator's own tables (Gr.n1, Gr.n2) are not touched."""
    _check(cb, model, Gr)
    if not cb.chains[0].intersite_corr:                                     # nothing requested: nothing to set up or fold
        return
    _ensure_device(cb, model, Gr)
    check(model._lib.elph_bond_chains_accumulate(model._h))


def fetch_bonds_(cb, model):
    """The device's un-normalised sums into every chain's position arrays; the momentum arrays are not touched."""
    if cb._device_of is not model:
        raise RuntimeError("no bond correlation has been measured on this model yet")
    for chain, c in enumerate(cb.chains):
        corr = c.intersite_corr
        ptrs = [corr[name].position.ctypes.data_as(P_dbl) if name in corr else None for name in _bm.BOND_CORR]
        check(model._lib.elph_bond_chains_fetch(model._h, chain, *ptrs))


def process_bond_measurements_(cb, bin_size, model):
    """The inter-site parts of process_measurements! (:574-676) per chain; every chain's sums run over binomial(n_rand_vecs, 2) pairs of
    ITS vectors."""
    fetch_bonds_(cb, model)
    for c in cb.chains:
        _bm._process_fetched(c, bin_size, model.dtau)


def write_bond_measurements_(cb, model, bin):
    """write_measurements! (:681-693) for the inter-site group per chain, into the chain's folder."""
    for c in cb.chains:
        _bm.write_bond_measurements_(c, model, bin)


def reset_bond_measurements_(cb, model):
    """reset_measurements! (:698-758): every chain's arrays and the device's accumulators to zero."""
    for c in cb.chains:
        _bm._zero_groups(c.intersite_corr, c.intersite_susc)
    if cb._device_of is model and model is not None and getattr(model, "_h", None):
        check(model._lib.elph_bond_chains_reset(model._h))
