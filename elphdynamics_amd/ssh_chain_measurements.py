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

X is (nchains, Ndof): chain c's field (the dynamics' X after pull_()).  mu is (nchains, Nsites), a row per chain, for a run whose tuners
move the chains' chemical potentials apart (hmc.set_mu_).  Given, it replaces the rows the device side holds, for this and every later
accumulate; None keeps them (model.mu for every chain when the device side is made, by the first accumulate_).  The estimator serves the
chains with n_rand_vecs * nchains vectors, vector v of chain c at index v * nchains + c (greens.chain_vector), as
process_input_file(deck, nchains=n) builds it; a bin is normalised by bin_size * binomial(n_rand_vecs, 2) with the vectors PER CHAIN.
A chain's folder holds exactly the files of a single-configuration run.

The device side is shaped by the estimator and dropped by the library when a new EstimateGreensFunction is made on the model (with the
sums it held): the next accumulate_ with the new estimator makes it again, with the mu given then (or model.mu).

Scope: what ssh_measurements.py measures for one configuration.  Refused with UnsupportedMeasurement naming the request: the Holstein
model (chain_measurements.py measures it), BondBond, CurrentCurrent, BondPairGreens with measure = true, a [measurements.Snapshots] entry
set to true (snapshots.py takes them for every chain, in a container of its own).  The SSH bond correlations over chains live in a container of their own beside this one (ssh_chain_bond_measurements.py,
csrc/ssh_bondcorr.hip), used on the same model and estimator, in either order.  ssh_measurements.py itself keeps refusing
resident chains.
"""
import numpy as np

from . import greens as _greens
from . import ssh_measurements as _sm
from ._lib import check, dptr

UnsupportedMeasurement = _sm.UnsupportedMeasurement
SUBJECT = "SSH chain measurements"


class SSHChainMeasurementsContainer:
    def __init__(self, chains, n_rand_vecs):
        self.chains = chains                 # one SSHMeasurementsContainer per chain
        self.nchains = len(chains)
        self.n_rand_vecs = n_rand_vecs       # per chain
        self._device_of = None               # the model whose handle holds the device side ...
        self._device_est = None              # ... and the estimator it was shaped by: a newer one on the model has dropped it


def initialize_ssh_chain_measurements_container(model, info, datafolders):
    """One container per resident chain of `model` for the request `info`; datafolders: one folder per chain."""
    _sm._refuse_holstein(model)
    nchains = int(getattr(model, "_nchains", 1))
    datafolders = list(datafolders)
    if len(datafolders) != nchains:
        raise ValueError("%d data folders for the %d chains resident in the model" % (len(datafolders), nchains))
    chains = [_sm._new_container(model, info, folder) for folder in datafolders]
    return SSHChainMeasurementsContainer(chains, chains[0].n_rand_vecs)


def initialize_measurement_folders_(cm):
    for c in cm.chains:
        _sm.initialize_measurement_folders_(c)


def _chain_rows(a, cm, width, what):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (cm.nchains, width):
        raise ValueError("%s has shape %s, not (nchains, %s) = (%d, %d)" % (what, a.shape, "Ndof" if what == "X" else "Nsites", cm.nchains, width))
    return a


def _check(cm, model, Gr, X, mu):
    """Everything that can be wrong on the host, before any library call."""
    assert Gr.model is model
    _sm._refuse_holstein(model)
    if int(getattr(model, "_nchains", 1)) != cm.nchains:
        raise ValueError("the container was made for %d chains, %d are resident in the model" % (cm.nchains, getattr(model, "_nchains", 1)))
    if Gr.nv != cm.n_rand_vecs * cm.nchains:
        raise ValueError("the estimator holds %d vectors, the container normalises for num_random_vectors = %d for each of %d chains"
                         % (Gr.nv, cm.n_rand_vecs, cm.nchains))
    X = _chain_rows(X, cm, model.Ndof, "X")
    if mu is not None:
        mu = _chain_rows(mu, cm, model.Nsites, "mu")
    return X, mu


def _ensure_device(cm, model, Gr, mu):
    if cm._device_of is model and cm._device_est is Gr:
        if mu is not None:              # the tuners moved it since: the device's rows follow (a small copy), the sums so far are kept
            check(model._lib.elph_ssh_meas_chains_set_mu(model._h, dptr(mu)))
        return
    mu = np.ascontiguousarray(np.tile(model.mu, (cm.nchains, 1)), dtype=np.float64) if mu is None else mu
    args, keep = _sm._create_args(cm.chains[0], model)
    check(model._lib.elph_ssh_meas_chains_create(model._h, cm.nchains, dptr(mu), *args))
    cm._device_of, cm._device_est = model, Gr


def accumulate_(cm, model, Gr, X, mu=None):
    """make_measurements! without its update! for every chain: each pair v1 < v2 of a chain's vectors is set up and folded into the
    device's accumulators for all chains at once; nothing comes back to the host."""
    X, mu = _check(cm, model, Gr, X, mu)
    _ensure_device(cm, model, Gr, mu)
    check(model._lib.elph_ssh_meas_chains_accumulate(model._h, dptr(X)))


def make_measurements_(cm, model, Gr, X, nmeas, P=None, R=None, rng=None, mu=None):
    """make_measurements!(container, model, Gr, nmeas, preconditioner) (:545-566) for every chain: one batched solve for all chains'
    vectors (greens.update_, which sets the preconditioner up per chain), then accumulate_.  Returns update_'s (iters, residual_error,
    flag), entry v * nchains + c for vector v of chain c."""
    X, mu = _check(cm, model, Gr, X, mu)
    out = _greens.update_(Gr, model, P, rng=rng, R=R)
    accumulate_(cm, model, Gr, X, mu)
    return out


def fetch_(cm, model):
    """The device's un-normalised sums into every chain's container (position arrays and scalars)."""
    if cm._device_of is not model:
        raise RuntimeError("nothing has been measured on this model yet")
    for chain, c in enumerate(cm.chains):
        scal, ptrs = _sm._fetch_buffers(c)
        check(model._lib.elph_ssh_meas_chains_fetch(model._h, chain, dptr(scal), *ptrs))
        _sm._store_scalars(c, scal)


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
    for c in cm.chains:
        _sm._zero_container(c)
    if cm._device_of is model and model is not None and getattr(model, "_h", None):
        check(model._lib.elph_ssh_meas_chains_reset(model._h))
