"""Inter-site correlations of every chain of the bond-phonon (SSH) model resident in a handle (a lockstep run: langevin.evolve_,
hmc.update_chains_): the chain-aware twin of ssh_bond_measurements.py, beside ssh_chain_measurements.py the way ssh_bond_measurements.py
stands beside ssh_measurements.py.  One SSHBondContainer per chain, each with its own data folder; on the device all chains are
accumulated by the same launches (elph_ssh_bond_chains_*, csrc/ssh_bondcorr.hip), the chain a grid axis.

    cb = initialize_ssh_chain_bond_container(model, info, datafolders)   one container per chain (:295-302, :322, :767-819 each)
    initialize_ssh_bond_folders_(cb)                                     the inter-site parts of :420-540 per chain
    accumulate_ssh_bonds_(cb, model, Gr, X)                              measure_BondBond! (:1663-1785), measure_CurrentCurrent!(ssh)
                                                                         (:2100-2384), measure_BondPairGreens! (:2390-2483): every pair of
                                                                         a chain's vectors, all chains at once
    fetch_ssh_bonds_(cb, model)                                          the device's sums into the chains' containers
    process_ssh_bond_measurements_(cb, bin_size, model)                  the inter-site parts of :574-676, BondPairSusc :666-672, per chain
    write_ssh_bond_measurements_(cb, model, bin)                         :681-693 per chain, into the chain's folder
    reset_ssh_bond_measurements_(cb, model)                              :698-758

X is (nchains, Ndof): chain c's field (the dynamics' X after pull_()), from which CurrentCurrent recomputes chain c's modulated hopping.
The estimator serves the chains with n_rand_vecs * nchains vectors, vector v of chain c at index v * nchains + c (greens.chain_vector),
as process_input_file(deck, nchains=n) builds it; a bin is normalised by bin_size * binomial(n_rand_vecs, 2) with the vectors PER CHAIN.
A chain's folder holds exactly the files ssh_bond_measurements.py writes for one configuration, BondPairSusc included.

It is used next to an ssh_chain_measurements.SSHChainMeasurementsContainer (whose constructor keeps refusing the three names) on the
same model and estimator, in either order: the two device sides are separate, and neither touches the estimator's own tables, so Gr.n1
and Gr.n2 are left alone.

The device side is shaped by the estimator and dropped by the library when a new EstimateGreensFunction is made on the model (with the
sums it held): the next accumulate_ssh_bonds_ with the new estimator makes it again.

Scope: what ssh_bond_measurements.py measures for one configuration, with its departures from the reference's comments.  Refused with
UnsupportedMeasurement naming the request: the Holstein model (chain_bond_measurements.py measures it), a request on a model without
bond definitions.  ssh_bond_measurements.py itself keeps refusing resident chains; sharded and slab handles, and CurrentCurrent where
Nbonds != n_def * ncells, are refused by the library.
"""
import numpy as np

from . import ssh_bond_measurements as _sb
from ._lib import P_dbl, check, dptr

UnsupportedMeasurement = _sb.UnsupportedMeasurement
SUBJECT = "SSH chain bond correlations"


class SSHChainBondContainer:
    def __init__(self, chains, n_rand_vecs):
        self.chains = chains                 # one SSHBondContainer per chain
        self.nchains = len(chains)
        self.n_rand_vecs = n_rand_vecs       # per chain
        self._device_of = None               # the model whose handle holds the device side ...
        self._device_est = None              # ... and the estimator it was shaped by: a newer one on the model has dropped it


def initialize_ssh_chain_bond_container(model, info, datafolders):
    """One SSHBondContainer per resident chain of `model` for the request `info`; datafolders: one folder per chain."""
    _sb._refuse_holstein(model)
    nchains = int(getattr(model, "_nchains", 1))
    datafolders = list(datafolders)
    if len(datafolders) != nchains:
        raise ValueError("%d data folders for the %d chains resident in the model" % (len(datafolders), nchains))
    chains = [_sb._new_ssh_bond_container(model, info, folder) for folder in datafolders]
    return SSHChainBondContainer(chains, chains[0].n_rand_vecs)


def initialize_ssh_bond_folders_(cb):
    for c in cb.chains:
        _sb.initialize_ssh_bond_folders_(c)


def _check(cb, model, Gr, X):
    """Everything that can be wrong on the host, before any library call."""
    assert Gr.model is model
    _sb._refuse_holstein(model)
    if int(getattr(model, "_nchains", 1)) != cb.nchains:
        raise ValueError("the container was made for %d chains, %d are resident in the model" % (cb.nchains, getattr(model, "_nchains", 1)))
    if Gr.nv != cb.n_rand_vecs * cb.nchains:
        raise ValueError("the estimator holds %d vectors, the container normalises for num_random_vectors = %d for each of %d chains"
                         % (Gr.nv, cb.n_rand_vecs, cb.nchains))
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.shape != (cb.nchains, model.Ndof):
        raise ValueError("X has shape %s, not (nchains, Ndof) = (%d, %d)" % (X.shape, cb.nchains, model.Ndof))
    return X


def _ensure_device(cb, model, Gr):
    if cb._device_of is model and cb._device_est is Gr:
        return
    args, keep = _sb._create_args(cb.chains[0], model)
    check(model._lib.elph_ssh_bond_chains_create(model._h, cb.nchains, *args))
    cb._device_of, cb._device_est = model, Gr


def accumulate_ssh_bonds_(cb, model, Gr, X):
    """measure_BondBond!, measure_CurrentCurrent! and measure_BondPairGreens! for every pair v1 < v2 of a chain's vectors, folded into the
    device's accumulators for all chains at once; nothing comes back to the host, and the estimator's own tables (Gr.n1, Gr.n2) are not
    touched."""
    X = _check(cb, model, Gr, X)
    if not cb.chains[0].intersite_corr:                                     # nothing requested: nothing to set up or fold
        return
    _ensure_device(cb, model, Gr)
    check(model._lib.elph_ssh_bond_chains_accumulate(model._h, dptr(X)))


def fetch_ssh_bonds_(cb, model):
    """The device's un-normalised sums into every chain's position arrays; the momentum arrays are not touched."""
    if cb._device_of is not model:
        raise RuntimeError("no SSH bond correlation has been measured on this model yet")
    for chain, c in enumerate(cb.chains):
        corr = c.intersite_corr
        ptrs = [corr[name].position.ctypes.data_as(P_dbl) if name in corr else None for name in _sb.SSH_BOND_CORR]
        check(model._lib.elph_ssh_bond_chains_fetch(model._h, chain, *ptrs))


def process_ssh_bond_measurements_(cb, bin_size, model):
    """The inter-site parts of process_measurements! (:574-676) per chain; every chain's sums run over binomial(n_rand_vecs, 2) pairs of
    ITS vectors."""
    fetch_ssh_bonds_(cb, model)
    for c in cb.chains:
        _sb._process_fetched(c, bin_size, model.dtau)


def write_ssh_bond_measurements_(cb, model, bin):
    """write_measurements! (:681-693) for the three correlations and BondPairSusc per chain, into the chain's folder."""
    for c in cb.chains:
        _sb.write_ssh_bond_measurements_(c, model, bin)


def reset_ssh_bond_measurements_(cb, model):
    """reset_measurements! (:698-758): every chain's arrays and the device's accumulators to zero."""
    for c in cb.chains:
        _sb._zero_groups(c.intersite_corr, c.intersite_susc)
    if cb._device_of is model and model is not None and getattr(model, "_h", None):
        check(model._lib.elph_ssh_bond_chains_reset(model._h))
