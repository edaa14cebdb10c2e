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
The estimator's vectors per chain, the normalisation of a bin, the life of the device side and the use beside the on-site chain
container (here an ssh_chain_measurements.SSHChainMeasurementsContainer) are chain_bond_measurements.py's.  A chain's folder holds
exactly the files ssh_bond_measurements.py writes for one configuration, BondPairSusc included.

Scope: what ssh_bond_measurements.py measures for one configuration, with its departures from the reference's comments, and its
refusals but the resident chains (the library's of CurrentCurrent where Nbonds != n_def * ncells included); the table in
measurements.py's docstring has the module for everything else.  The functions below are the bond family of _chain_unit.py with this
module's record.
"""
from . import _chain_unit as _cu
from . import ssh_bond_measurements as _sb

UnsupportedMeasurement = _sb.UnsupportedMeasurement
SUBJECT = "SSH chain bond correlations"
FAMILY = _cu.BondFamily(single=_sb, refuse=lambda model: _sb._refuse_holstein(model, _sb.SUBJECT), prefix="elph_ssh_bond_chains_",
                        corr=_sb.SSH_BOND_CORR, takes_X=True, noun="SSH bond correlation")


class SSHChainBondContainer(_cu.ChainContainer):
    """chains: one SSHBondContainer per chain."""


def initialize_ssh_chain_bond_container(model, info, datafolders):
    """One SSHBondContainer per resident chain of `model` for the request `info`; datafolders: one folder per chain."""
    FAMILY.refuse(model)
    chains = [_sb._new_ssh_bond_container(model, info, folder) for folder in _cu.chain_folders(model, datafolders)]
    return SSHChainBondContainer(chains, chains[0].n_rand_vecs)


def initialize_ssh_bond_folders_(cb):
    for c in cb.chains:
        _sb.initialize_ssh_bond_folders_(c)


def accumulate_ssh_bonds_(cb, model, Gr, X):
    """measure_BondBond!, measure_CurrentCurrent! and measure_BondPairGreens! for every pair v1 < v2 of a chain's vectors, folded into the
    device's accumulators for all chains at once; nothing comes back to the host, and the estimator's own tables (Gr.n1, Gr.n2) are not
    touched."""
    _cu.bond_accumulate(FAMILY, cb, model, Gr, X)


def fetch_ssh_bonds_(cb, model):
    """The device's un-normalised sums into every chain's position arrays; the momentum arrays are not touched."""
    _cu.bond_fetch(FAMILY, cb, model)


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
    _cu.bond_reset(FAMILY, cb, model)
