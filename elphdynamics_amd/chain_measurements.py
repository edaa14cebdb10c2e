"""Measurements of every chain resident in a handle (a lockstep run: hmc.update_chains_, langevin.evolve_): the chain-aware twin of
measurements.py.  One MeasurementsContainer per chain, each with its own data folder; on the device all chains are accumulated by the
same launches (elph_meas_chains_*, csrc/measure.hip), the chain a grid axis.

    cm = initialize_chain_measurements_container(model, info, datafolders)     one container per chain (Measurements.jl:27-178 each)
    initialize_measurement_folders_(cm)                                        :343-540 per chain
    make_measurements_(cm, model, Gr, X, nmeas, P=None, R=None, rng=None, mu=None)      :545-566: update! of all chains' vectors as one
                                                                                batched solve, then accumulate_
    accumulate_(cm, model, Gr, X, mu=None)                                     every pair of a chain's vectors, all chains at once
    fetch_(cm, model)                                                          the device's sums into the chains' containers
    process_measurements_(cm, bin_size, model)                                 :574-676 per chain
    write_measurements_(cm, model, bin)                                        :681-693 per chain, into the chain's folder
    reset_measurements_(cm, model)                                             :698-758

X is (nchains, Ndof): chain c's field (the HybridMonteCarlo's X after pull_()).  mu is (nchains, Nsites), a row per chain, for a run
whose tuners move the chains' chemical potentials apart (hmc.set_mu_).  Given, it replaces the rows the device side holds, for this and
every later accumulate; None keeps them (model.mu for every chain when the device side is made, by the first accumulate_).  The
estimator serves the chains with n_rand_vecs * nchains vectors, vector v of chain c at index v * nchains + c (greens.chain_vector), as
process_input_file(deck, nchains=n) builds it; a bin is normalised by bin_size * binomial(n_rand_vecs, 2) with the vectors PER CHAIN.
A chain's folder holds exactly the files of a single-configuration run.

The device side is shaped by the estimator and dropped by the library when a new EstimateGreensFunction is made on the model (with the
sums it held): the next accumulate_ with the new estimator makes it again, with the mu given then (or model.mu).

Scope: what measurements.py measures for one configuration, and its refusals but the resident chains; the table in measurements.py's
docstring has the module for everything else.  The functions below are the on-site family of _chain_unit.py with this module's record.
"""
from . import _chain_unit as _cu
from . import measurements as _ms

UnsupportedMeasurement = _ms.UnsupportedMeasurement
FAMILY = _cu.OnsiteFamily(single=_ms, refuse=lambda model: _ms._refuse_ssh(model, "chain measurements"), check_refuses=False,
                          prefix="elph_meas_chains_")


class ChainMeasurementsContainer(_cu.ChainContainer):
    """chains: one MeasurementsContainer per chain."""


def initialize_chain_measurements_container(model, info, datafolders):
    """One container per resident chain of `model` for the request `info`; datafolders: one folder per chain."""
    FAMILY.refuse(model)
    chains = [_ms._new_container(model, info, folder) for folder in _cu.chain_folders(model, datafolders)]
    return ChainMeasurementsContainer(chains, chains[0].n_rand_vecs)


def initialize_measurement_folders_(cm):
    for c in cm.chains:
        _ms.initialize_measurement_folders_(c)


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
        _ms._process_fetched(c, bin_size, model.dtau)


def write_measurements_(cm, model, bin):
    """write_measurements! (:681-693) per chain, into the chain's folder."""
    for c in cm.chains:
        _ms.write_measurements_(c, model, bin)


def reset_measurements_(cm, model):
    """reset_measurements! (:698-758): every chain's arrays and the device's accumulators to zero."""
    _cu.onsite_reset(FAMILY, cm, model)
