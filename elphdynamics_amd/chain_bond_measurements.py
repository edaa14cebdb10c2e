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

Scope: what bond_measurements.py measures for one configuration, and its refusals but the resident chains; the table in
measurements.py's docstring has the module for everything else.  The functions below are the bond family of _chain_unit.py with this
module's record.
"""
from . import _chain_unit as _cu
from . import bond_measurements as _bm
from .measurements import _refuse_ssh

UnsupportedMeasurement = _bm.UnsupportedMeasurement
SUBJECT = "chain bond correlations"
FAMILY = _cu.BondFamily(single=_bm, refuse=lambda model: _refuse_ssh(model, SUBJECT), prefix="elph_bond_chains_", corr=_bm.BOND_CORR,
                        takes_X=False, noun="bond correlation")


class ChainBondContainer(_cu.ChainContainer):
    """chains: one BondContainer per chain."""


def initialize_chain_bond_container(model, info, datafolders, bond_definitions=None):
    """One BondContainer per resident chain of `model` for the request `info`; datafolders: one folder per chain."""
    FAMILY.refuse(model)
    chains = [_bm._new_bond_container(model, info, folder, bond_definitions) for folder in _cu.chain_folders(model, datafolders)]
    return ChainBondContainer(chains, chains[0].n_rand_vecs)


def initialize_bond_folders_(cb):
    for c in cb.chains:
        _bm.initialize_bond_folders_(c)


def accumulate_bonds_(cb, model, Gr):
    """measure_BondBond! and measure_BondPairGreens! for every pair v1 < v2 of a chain's vectors, folded into the device's accumulators
    for all chains at once; nothing comes back to the host, and the estimator's own tables (Gr.n1, Gr.n2) are not touched."""
    _cu.bond_accumulate(FAMILY, cb, model, Gr)


def fetch_bonds_(cb, model):
    """The device's un-normalised sums into every chain's position arrays; the momentum arrays are not touched."""
    _cu.bond_fetch(FAMILY, cb, model)


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
    _cu.bond_reset(FAMILY, cb, model)
