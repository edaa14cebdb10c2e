"""Host-side mirror of Measurements.jl for the bond-phonon (SSH) model: the measurement container, its accumulation on the device
(csrc/ssh_measure.hip), and the per-bin processing and files.  It stands beside measurements.py (Holstein) and bond_measurements.py.

    c = initialize_ssh_measurements_container(model, info, datafolder)   Measurements.jl:180-338
    initialize_measurement_folders_(c)                                   :343-540
    make_measurements_(c, model, Gr, nmeas, P=None, R=None, rng=None)    :545-566   update! then every pair of vectors, on the device
    process_measurements_(c, bin_size, model)                            :574-676   fetch, momentum copy, normalise, susceptibilities
    write_measurements_(c, model, bin)                                   :681-693
    reset_measurements_(c, model)                                        :698-758

`info` is the `[measurements]` table of an input deck.  The constructor reads host attributes of the model only and makes no library
call; the device side (elph_ssh_meas_create) is made by the first make_measurements_ / accumulate_.  Arrays as in measurements.py.

What the SSH branch measures: the global scalars density, Nsqr, mu; per orbital density, double_occ, mu (:978-1024); per bond definition
x, x2, x4, phonon_pe, phonon_ke, elph_energy, el_ke, sign_switch (:1072-1155), normalised by (Nbonds // nbonds) * Ltau; the on-site
correlations Greens, DenDen, SpinSpin, PairGreens over orbital pairs with the susceptibilities PairSusc, ChargeSusc, SpinSusc; and the
inter-site PhononGreens over pairs of phonon types 1..nph (:2488-2541; all nph^2 by default), present only when the model has phonons
(:291-293).  pairs[0, p] = b1, pairs[1, p] = b2: PhononGreens[D] = 1/(L Nc) sum x_b2[. + D] x_b1[.].

Scope: the table in measurements.py's docstring has what each of the nine modules measures and refuses, this one included.  Refused by
the library besides sharded and slab handles: PhononGreens on a lattice where Nph != nph * ncells (the reference's reshape of the field
throws).

Line order in the scalar files (the reference's is the unspecified order of a Julia Dict), extending the one of measurements.py:
density, Nsqr, mu / density, double_occ, mu / x, x2, x4, phonon_pe, phonon_ke, elph_energy, el_ke, sign_switch.
"""
import os

import numpy as np

from . import greens as _greens
from . import measurements as _ms
from ._chain_unit import position_pointers, require_device, reset_device
from ._lib import check, dptr, iptr
from .measurements import (GLOBAL_KEYS, INTERSITE_CORR, SUSC_OF, MeasurementsContainer, UnsupportedMeasurement, _bin_volume,  # noqa: F401
                           _check_estimator, _corr_group, _divide_scalars, _group_folders, _ip, _process_group, _refuse_chains,
                           _refuse_holstein, _request_arrays, _susc_group, _write_groups, _zero_container, _zero_groups, simpson)

ONSITE_KEYS = ("density", "double_occ", "mu")
INTERSITE_KEYS = ("x", "x2", "x4", "phonon_pe", "phonon_ke", "elph_energy", "el_ke", "sign_switch")
KEYS = (GLOBAL_KEYS, ONSITE_KEYS, INTERSITE_KEYS)
ONSITE_CORR = ("Greens", "DenDen", "SpinSpin", "PairGreens")
CREATE_ORDER = ONSITE_CORR + ("PhononGreens",)              # the order of elph_ssh_meas_create's request arrays
SUBJECT = "SSH measurements"


class SSHMeasurementsContainer(MeasurementsContainer):
    """The same fields; the inter-site scalars and PhononGreens (intersite_corr) are filled here."""


def _new_container(model, info, datafolder):
    """The container of one configuration of an SSH model for the request `info`, after the caller has decided that the model is measured
    (ssh_chain_measurements.py makes one per resident chain): the requests neither path measures are refused here."""
    info = info or {}
    for name in INTERSITE_CORR:
        if info.get(name, {}).get("measure", False) is True:
            what = name + (" (and BondPairSusc)" if name == "BondPairGreens" else "")
            raise UnsupportedMeasurement("[measurements.%s] measure = true: the inter-site correlation %s of the SSH model is not supported by this container; "
                                         "ssh_bond_measurements.initialize_ssh_bond_container measures it" % (name, what))
    for key, val in info.get("Snapshots", {}).items():
        if val is True:
            raise UnsupportedMeasurement("[measurements.Snapshots] %s = true: snapshots are not supported" % key)
    lat = model.lattice
    dims, no, nb = (lat.L1, lat.L2, lat.L3), lat.norbits, int(model.nbonds)
    c = SSHMeasurementsContainer()
    c.n_rand_vecs = int(info.get("num_random_vectors", 1))                  # :189-193
    c.datafolder = datafolder
    c.global_meas = {k: 0j for k in GLOBAL_KEYS}
    c.onsite_meas = {k: np.zeros(no, dtype=np.complex128) for k in ONSITE_KEYS}
    c.intersite_meas = {k: np.zeros(nb, dtype=np.complex128) for k in INTERSITE_KEYS}
    c.onsite_corr = _corr_group(info, ONSITE_CORR, no, model.Ltau, dims)
    if model.nph > 0:                                                       # :291-293
        c.intersite_corr = _corr_group(info, ("PhononGreens",), int(model.nph), model.Ltau, dims)
    c.onsite_susc = _susc_group(c.onsite_corr, SUSC_OF, dims)
    return c


def initialize_ssh_measurements_container(model, info, datafolder):
    """initialize_measurements_container(ssh, info, datafolder) (:180-338)."""
    _refuse_holstein(model, SUBJECT)
    _refuse_chains(model, SUBJECT)
    return _new_container(model, info, datafolder)


def initialize_measurement_folders_(container):
    """initialize_measurement_folders!(container) (:343-540): the on-site groups' key files name orbit1, orbit2, the inter-site ones bond1, bond2."""
    d = container.datafolder
    for name in ("global_measurements_f", "onsite_measurements_f", "intersite_measurements_f"):
        os.mkdir(os.path.join(d, name))
    _group_folders(d, container.onsite_corr, container.onsite_susc, "orbit1", "orbit2")
    _group_folders(d, container.intersite_corr, container.intersite_susc, "bond1", "bond2")


def bond_arrays(model):
    """(sites (Nbonds, 2) 1-based, t) in the reference's bond order (:1103-1107): neighbor_table[:, checkerboard_perm[bond]] and t[bond]."""
    nb = int(model.Nbonds)
    if nb == 0:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    rows = np.asarray(model.checkerboard_perm, dtype=np.int64) - 1
    return np.ascontiguousarray(model.neighbor_table[rows], dtype=np.int64), np.ascontiguousarray(model.t, dtype=np.float64)


def _all_corr(container):
    return dict(container.onsite_corr, **container.intersite_corr)


def _create_args(container, model, mu):
    """The arguments of elph_ssh_meas_create after the handle and of elph_ssh_meas_chains_create after nchains: `mu` (float64: Nsites, or a
    row per chain), dtau, the bonds, the phonons and the container's requests.  The second value keeps the arrays alive for the call."""
    sites, t = bond_arrays(model)
    request = _request_arrays(_all_corr(container), CREATE_ORDER)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)  # noqa: E731
    nph_tot, nb = int(model.Nph), int(model.Nbonds)
    b2d, b2p = i64(model.bond_to_definition), i64(model.bond_to_phonon)
    par = [f64(a) for a in (model.omega, model.alpha, model.alpha2)]
    args = [dptr(mu), float(model.dtau), nb, int(model.nbonds), iptr(sites) if nb else None, dptr(t) if nb else None, iptr(b2d) if nb else None,
            iptr(b2p) if nb else None, nph_tot, int(model.nph), *[dptr(a) if nph_tot else None for a in par], *map(_ip, request)]
    return args, (mu, sites, t, b2d, b2p, par, request)


def _ensure_device(container, model, Gr):
    if container._device_of is model:
        return
    _refuse_holstein(model, SUBJECT)
    _check_estimator(container, model, Gr)
    args, keep = _create_args(container, model, np.ascontiguousarray(model.mu, dtype=np.float64))
    check(model._lib.elph_ssh_meas_create(model._h, *args))
    container._device_of = model


def accumulate_(container, model, Gr):
    """make_measurements! without its update! (:550-560): every pair i < j of the estimator's vectors is set up and folded into the device's
    accumulators; nothing comes back to the host."""
    _refuse_chains(model, SUBJECT)
    _ensure_device(container, model, Gr)
    check(model._lib.elph_ssh_meas_accumulate(model._h, dptr(np.ascontiguousarray(model.x, dtype=np.float64))))
    Gr.n1, Gr.n2 = Gr.nv - 1, Gr.nv                                         # the estimator's device tables are the last pair's now


def make_measurements_(container, model, Gr, nmeas, P=None, R=None, rng=None):
    """make_measurements!(container, model, Gr, nmeas, preconditioner) (:545-566).  R / rng: the noise vectors of update_ (greens.py).
    Returns update_'s (iters, residual_error, flag).  nmeas numbers the snapshots of the reference; none are taken here."""
    out = _greens.update_(Gr, model, P, rng=rng, R=R)
    accumulate_(container, model, Gr)
    return out


def _fetch_buffers(container):
    """(scalars, the position arrays' pointers in CREATE_ORDER) for a *_fetch call into the container."""
    return _ms._scalar_buffer(container, KEYS), position_pointers(_all_corr(container), CREATE_ORDER)


def _store_scalars(container, scal):
    _ms._store_scalars(container, scal, KEYS)


def fetch_(container, model):
    """The device's un-normalised sums into the container (position arrays and scalars); the momentum arrays are not touched."""
    require_device(container, model)
    scal, ptrs = _fetch_buffers(container)
    check(model._lib.elph_ssh_meas_fetch(model._h, dptr(scal), *ptrs))
    _store_scalars(container, scal)


def _process_fetched(container, bin_size, dtau):
    """process_measurements! after the fetch: momentum copy, normalisation, susceptibilities."""
    V = _bin_volume(container, bin_size)
    _divide_scalars(container, V)
    _process_group(container.onsite_corr, container.onsite_susc, SUSC_OF, V, dtau)
    _process_group(container.intersite_corr, container.intersite_susc, (), V, dtau)


def process_measurements_(container, bin_size, model):
    """process_measurements!(container, sim_params, model) (:574-676); bin_size is sim_params.bin_size."""
    fetch_(container, model)
    _process_fetched(container, bin_size, model.dtau)


def write_measurements_(container, model, bin):
    """write_measurements!(container, model, bin) (:681-693, :1175-1274)."""
    _ms.write_measurements_(container, model, bin, KEYS)


def reset_measurements_(container, model):
    """reset_measurements!(container, model) (:698-758): the container's arrays and the device's accumulators to zero."""
    _zero_container(container)
    reset_device(container, model, "elph_ssh_meas_reset")
