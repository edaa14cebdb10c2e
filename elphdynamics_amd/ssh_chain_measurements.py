"""Measurements of every chain of the bond-phonon (SSH) model resident in a handle (a lockstep run: langevin.evolve_, hmc.update_chains_):
the chain-aware twin of ssh_measurements.py, as chain_measurements.py is of measurements.py.  One SSHMeasurementsContainer per chain, each
with its own data folder; on the device all chains are accumulated by the same launches (elph_ssh_meas_chains_*,
csrc/ssh_measure.hip), the chain a grid axis.

    cm = initialize_ssh_chain_measurements_container(model, info, datafolders)   one container per chain (Measurements.jl:180-338 each)
    initialize_measurement_folders_(cm)                                          :343-540 per chain
    make_measurements_(cm, model, Gr, X, nmeas, P=None, R=None, rng=None, mu=None)      :545-566: update! of all chains' vectors as one
                                                                                  batched solve, then accumulate_
    accumulate_(cm, model, Gr, X, mu=None)                                       every pair of a chain's vectors, all chains at once
    fetch_(cm, model)                                                            the device's sums into the chains' containers
    process_measurements_(cm, bin_size, model)                                   :574-676 per chain
    write_measurements_(cm, model, bin)                                          :681-693 per chain, into the chain's folder
    reset_measurements_(cm, model)                                               :698-758

X, mu, the estimator's vectors per chain, the normalisation of a bin and the life of the device side are chain_measurements.py's, word
for word; the field is the dynamics' X after pull_().  A chain's folder holds exactly the files of a single-configuration run.

Scope: what ssh_measurements.py measures for one configuration, and its refusals but the resident chains; the table in
measurements.py's docstring has the module for everything else.  The functions below are the on-site family of _chain_unit.py with
this module's record.
"""
from . import _chain_unit as _cu
from . import ssh_measurements as _sm

UnsupportedMeasurement = _sm.UnsupportedMeasurement
SUBJECT = "SSH chain measurements"
FAMILY = _cu.OnsiteFamily(single=_sm, refuse=lambda model: _sm._refuse_holstein(model, _sm.SUBJECT), check_refuses=True,
                          prefix="elph_ssh_meas_chains_")


class SSHChainMeasurementsContainer(_cu.ChainContainer):
    """chains: one SSHMeasurementsContainer per chain."""


def initialize_ssh_chain_measurements_container(model, info, datafolders):
    """One container per resident chain of `model` for the request `info`; datafolders: one folder per chain."""
    FAMILY.refuse(model)
    chains = [_sm._new_container(model, info, folder) for folder in _cu.chain_folders(model, datafolders)]
    return SSHChainMeasurementsContainer(chains, chains[0].n_rand_vecs)


def initialize_measurement_folders_(cm):
    for c in cm.chains:
        _sm.initialize_measurement_folders_(c)


def accumulate_(cm, model, Gr, X, mu=None):
    """make_measurements! without its update! for every chain: each pair v1 < v2 of a chain's vectors is set up and folded into the
    device's accumulators for all chains at once; nothing comes back to the host."""
    _cu.onsite_accumulate(FAMILY, cm, model, Gr, X, mu)


def make_measurements_(cm, model, Gr, X, nmeas, P=None, R=None, rng=None, mu=None):
    """make_measurements!(container, model, Gr, nmeas, preconditioner) (:545-566) for every chain: one batched solve for all chains'
    vectors (greens.update_, which sets the preconditioner up per chain), then accumulate_.  Returns update_'s (iters, residual_error,
    flag), entry v * nchains + c for vector v of chain c."""
    return _cu.onsite_make(FAMILY, cm, model, Gr, X, P, R, rng, mu)


def fetch_(cm, model):
    """The device's un-normalised sums into every chain's container (position arrays and scalars)."""
    _cu.onsite_fetch(FAMILY, cm, model)


def process_measurements_(cm, bin_size, model):
    """process_measurements! (:574-676) per chain; every chain's sums run over binomial(n_rand_vecs, 2) pairs of ITS vectors."""
    fetch_(cm, model)
    for c in cm.chains:
        _sm._process_fetched(c, bin_size, model.dtau)


def write_measurements_(cm, model, bin):
    """write_measurements! (:681-693) per chain, into the chain's folder."""
    for c in cm.chains:
        _sm.write_measurements_(c, model, bin)


def reset_measurements_(cm, model):
    """reset_measurements! (:698-758): every chain's arrays and the device's accumulators to zero."""
    _cu.onsite_reset(FAMILY, cm, model)
