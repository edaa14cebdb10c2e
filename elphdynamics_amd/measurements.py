"""Host-side mirror of Measurements.jl for the Holstein model: the measurement container, its accumulation on the device, and the
per-bin processing and files.

    c = initialize_measurements_container(model, info, datafolder)     Measurements.jl:27-178
    initialize_measurement_folders_(c)                                 :343-540
    make_measurements_(c, model, Gr, nmeas, P=None, R=None, rng=None)  :545-566   update! then every pair of vectors, on the device
    process_measurements_(c, bin_size, model)                          :574-676   fetch, momentum copy, normalise, susceptibilities
    write_measurements_(c, model, bin)                                 :681-693
    reset_measurements_(c, model)                                      :698-758

`info` is the `[measurements]` table of an input deck (process_input keeps it as sim.input["measurements"]).  The constructor reads host
attributes of the model only and makes no library call; the device side (elph_meas_create, csrc/measure.hip) is made by the first
make_measurements_ / accumulate_.  Between two process_measurements_ the sums live on the device: the container's arrays are filled by
process_measurements_ (or fetch_), one small copy per bin.

Arrays keep the reference's shapes in Fortran order (Julia's memory image): a correlation's `position` and `momentum` are complex128
(L0, L1, L2, L3, n_p) with L0 = Ltau + 1 (time-dependent, tau = beta included) or 1 (equal-time), `pairs` is int (2, n_p), 1-based; a
susceptibility's are (L1, L2, L3, n_p).

Who measures what.  Nine modules, one container each, used beside one another on the same model and estimator, in any order.  What a
module does not measure it refuses with UnsupportedMeasurement naming the request, never skips; sharded and slab handles are refused by
the library.  "scalars": the global, on-site and inter-site numbers of the three scalar files.  The chain modules measure every chain
resident in a handle (a lockstep run) in the same launches, one single-configuration container per chain; what they share is written
once in _chain_unit.py.

    module                          model     configurations  correlations (their susceptibilities)             device unit
    measurements.py                 Holstein  one             scalars; Greens, DenDen, SpinSpin, PairGreens,    csrc/measure.hip
                                                              PhononGreens (PairSusc, ChargeSusc, SpinSusc)
    chain_measurements.py           Holstein  chains          as measurements.py                                csrc/measure.hip
    bond_measurements.py            Holstein  one             BondBond, BondPairGreens (BondPairSusc)           csrc/bondcorr.hip
    chain_bond_measurements.py      Holstein  chains          as bond_measurements.py                           csrc/bondcorr.hip
    current_measurements.py         Holstein  one or chains   CurrentCurrent                                    csrc/currcorr.hip
    ssh_measurements.py             SSH       one             scalars; Greens, DenDen, SpinSpin, PairGreens     csrc/ssh_measure.hip
                                                              (PairSusc, ChargeSusc, SpinSusc), PhononGreens
    ssh_chain_measurements.py       SSH       chains          as ssh_measurements.py                            csrc/ssh_measure.hip
    ssh_bond_measurements.py        SSH       one             BondBond, CurrentCurrent, BondPairGreens          csrc/ssh_bondcorr.hip
                                                              (BondPairSusc)
    ssh_chain_bond_measurements.py  SSH       chains          as ssh_bond_measurements.py                       csrc/ssh_bondcorr.hip

Refused by every module: the other model.  By the one-configuration modules: several chains resident in the handle (model._nchains
> 1); current_measurements.py takes either.  By the four on-site modules: BondBond, CurrentCurrent, BondPairGreens (and with it
BondPairSusc) with measure = true, and a [measurements.Snapshots] entry set to true (snapshots.py takes them for one configuration or
every chain, in a container of its own: snapshots.split_info splits the table).  By bond_measurements.py and
chain_bond_measurements.py: CurrentCurrent with measure = true (current_measurements.split_info hands them the table without it).  By the
five bond and current modules: a request on a model without bond definitions.

One thing is not the reference's: the line order inside the global_measurements, onsite_measurements and intersite_measurements files.
The reference writes them in the iteration order of a Julia Dict, which is unspecified; here it is density, Nsqr, mu / density,
double_occ, x, x2, x4, phonon_pe, phonon_ke, elph_energy, mu / el_ke.  Readers key on the name column.
"""
import os
from math import comb

import numpy as np

from . import greens as _greens
from ._chain_unit import position_pointers, require_device, reset_device
from ._lib import P_int, check, dptr, iptr

GLOBAL_KEYS = ("density", "Nsqr", "mu")
ONSITE_KEYS = ("density", "double_occ", "x", "x2", "x4", "phonon_pe", "phonon_ke", "elph_energy", "mu")
INTERSITE_KEYS = ("el_ke",)
KEYS = (GLOBAL_KEYS, ONSITE_KEYS, INTERSITE_KEYS)           # a model's scalars in the order of its device unit's buffer and of its files
ONSITE_CORR = ("Greens", "DenDen", "SpinSpin", "PairGreens", "PhononGreens")        # the order of elph_meas_create's request arrays
INTERSITE_CORR = ("BondBond", "CurrentCurrent", "BondPairGreens")
SUSC_OF = (("PairSusc", "PairGreens"), ("ChargeSusc", "DenDen"), ("SpinSusc", "SpinSpin"))      # :148-155


class UnsupportedMeasurement(NotImplementedError):
    """A request of the [measurements] table, or a model, that this port does not measure."""


class Correlation:
    """(position, momentum, pairs) of one correlation function or susceptibility (:792, :814)."""

    def __init__(self, shape, pairs):
        self.position = np.zeros(shape, dtype=np.complex128, order="F")
        self.momentum = np.zeros(shape, dtype=np.complex128, order="F")
        self.pairs = pairs


class MeasurementsContainer:
    def __init__(self):
        self.global_meas, self.onsite_meas, self.intersite_meas = {}, {}, {}
        self.onsite_corr, self.intersite_corr, self.onsite_susc, self.intersite_susc = {}, {}, {}, {}
        self.snapshots = []
        self.n_rand_vecs = 1
        self.datafolder = ""
        self._device_of = None           # the model whose handle holds the device side


def _pairs(entry, n):
    """:776-782: the listed pairs sorted (lexicographically, as sort! of a Vector{Vector{Int}}), or all n^2 with the first index slowest."""
    if "pairs" in entry:
        pairs = sorted([int(p[0]), int(p[1])] for p in entry["pairs"])
    else:
        pairs = [[i, j] for i in range(1, n + 1) for j in range(1, n + 1)]
    return np.array(pairs, dtype=np.int64).reshape(-1, 2).T.copy()


def _refuse_ssh(model, subject):
    if getattr(model, "kind", None) != 0:
        raise UnsupportedMeasurement("%s of the SSH model are not supported (Holstein only)" % subject)


def _refuse_holstein(model, subject):
    """subject: "SSH measurements" / "SSH bond correlations"; the module named is the Holstein one for the same correlations."""
    if getattr(model, "kind", None) != 1:
        raise UnsupportedMeasurement("%s of the Holstein model are not supported (SSH only; see %smeasurements.py)"
                                     % (subject, "bond_" if "bond" in subject else ""))


def _refuse_chains(model, subject):
    if getattr(model, "_nchains", 1) > 1:
        raise UnsupportedMeasurement("%s with several chains resident (model._nchains = %d) are not supported" % (subject, model._nchains))


def _refuse_model(model, subject):
    """The models neither container measures; subject: "measurements" / "bond correlations"."""
    _refuse_ssh(model, subject)
    _refuse_chains(model, subject)


def _requested(info, names):
    return [name for name in names if (info.get(name) or {}).get("measure", False) is True]


def _corr_group(info, names, n, L, dims):
    """init_corr_container! (:767-796) for every requested name; n: what a pair's indices count (orbitals, bond definitions)."""
    group = {}
    for name in _requested(info, names):
        pairs = _pairs(info[name], n)
        L0 = L + 1 if info[name].get("time_dependent", False) is True else 1
        group[name] = Correlation((L0,) + dims + (pairs.shape[1],), pairs)
    return group


def _susc_group(corr_group, table, dims):
    """init_susc_container! (:801-819): one susceptibility per time-dependent correlation of `table`, on the same pairs."""
    return {susc: Correlation(dims + (corr_group[corr].pairs.shape[1],), corr_group[corr].pairs)
            for susc, corr in table if corr in corr_group and corr_group[corr].position.shape[0] > 1}


def _new_container(model, info, datafolder):
    """The container of one configuration for the request `info`, after the caller has decided that the model is measured: the requests
    neither path measures are refused here."""
    info = info or {}
    for name in INTERSITE_CORR:
        if info.get(name, {}).get("measure", False) is True:
            what = name + (" (and BondPairSusc)" if name == "BondPairGreens" else "")
            raise UnsupportedMeasurement("[measurements.%s] measure = true: the inter-site correlation %s is not supported" % (name, what))
    for key, val in info.get("Snapshots", {}).items():
        if val is True:
            raise UnsupportedMeasurement("[measurements.Snapshots] %s = true: snapshots are not supported" % key)
    lat = model.lattice
    dims, no = (lat.L1, lat.L2, lat.L3), lat.norbits
    c = MeasurementsContainer()
    c.n_rand_vecs = int(info.get("num_random_vectors", 1))                  # :36-40
    c.datafolder = datafolder
    c.global_meas = {k: 0j for k in GLOBAL_KEYS}
    c.onsite_meas = {k: np.zeros(no, dtype=np.complex128) for k in ONSITE_KEYS}
    c.intersite_meas = {k: np.zeros(int(model.nbonds), dtype=np.complex128) for k in INTERSITE_KEYS}
    c.onsite_corr = _corr_group(info, ONSITE_CORR, no, model.Ltau, dims)
    c.onsite_susc = _susc_group(c.onsite_corr, SUSC_OF, dims)
    return c


def initialize_measurements_container(model, info, datafolder):
    """initialize_measurements_container(holstein, info, datafolder) (:27-178)."""
    _refuse_model(model, "measurements")
    return _new_container(model, info, datafolder)


def _key_file(path, header, arr, pairs):
    """The key of one array (:391-416, :471-496): 1-based index in memory order, the pair's orbitals, 0-based displacements, last
    axis first."""
    with open(path, "w") as f:
        f.write(header + "\n")
        nd = arr.ndim
        for i, idx in enumerate(np.ndindex(*arr.shape[::-1])):
            cidx = idx[::-1]                                                 # first index fastest
            p = cidx[-1]
            f.write(" ".join(["%d" % (i + 1), "%d" % pairs[0, p], "%d" % pairs[1, p]] + ["%d" % cidx[k] for k in range(nd - 2, -1, -1)]) + "\n")


def _group_folders(datafolder, corr_group, susc_group, col1, col2):
    """The folders and key files of a group's correlations and susceptibilities (:420-540); col1, col2: what a pair's columns are called."""
    for group, cols in ((corr_group, " tau"), (susc_group, "")):
        for k, corr in group.items():
            for space, letter in (("position", "r"), ("momentum", "k")):
                folder = os.path.join(datafolder, "%s_%s_f" % (k, space))
                os.mkdir(folder)
                header = "index %s %s %s3 %s2 %s1%s" % (col1, col2, letter, letter, letter, cols)
                _key_file(os.path.join(folder, "%s_%s_key.out" % (k, space)), header, getattr(corr, space), corr.pairs)


def initialize_measurement_folders_(container):
    """initialize_measurement_folders!(container) (:343-540)."""
    d = container.datafolder
    for name in ("global_measurements_f", "onsite_measurements_f", "intersite_measurements_f"):
        os.mkdir(os.path.join(d, name))
    _group_folders(d, container.onsite_corr, container.onsite_susc, "orbit1", "orbit2")


def bond_arrays(model):
    """(sites (nbonds_total, 2) 1-based, t) in the reference's bond order bond = (definition - 1) * ncells + cell (:1044-1054):
    neighbor_table[:, checkerboard_perm[bond]] and t[bond].  initialize_model_ sorts model.neighbor_table into checkerboard order and
    leaves model.t in definition order; checkerboard_perm maps a definition-ordered bond to its row of the sorted table."""
    nb = int(model.Nbonds)
    if nb != int(model.nbonds) * model.lattice.ncells:
        raise ValueError("el_ke: %d bonds are not %d definitions x %d cells (duplicate bonds were removed on a short axis): the "
                         "reference's bond -> definition map does not hold" % (nb, model.nbonds, model.lattice.ncells))
    if nb == 0:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    rows = np.asarray(model.checkerboard_perm, dtype=np.int64) - 1
    return np.ascontiguousarray(model.neighbor_table[rows], dtype=np.int64), np.ascontiguousarray(model.t, dtype=np.float64)


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _ip(a):
    return a.ctypes.data_as(P_int)


def _request_arrays(group, names):
    """measure / time_dependent / npairs / pairs of a *_create call (int32; the requests' pair lists one after another)."""
    plist = [group[name].pairs.T.reshape(-1) for name in names if name in group]
    return (_i32([name in group for name in names]), _i32([name in group and group[name].position.shape[0] > 1 for name in names]),
            _i32([group[name].pairs.shape[1] if name in group else 0 for name in names]), _i32(np.concatenate(plist)) if plist else _i32([0, 0]))


def _check_estimator(container, model, Gr):
    assert Gr.model is model
    if Gr.nv != container.n_rand_vecs:
        raise ValueError("the estimator holds %d vectors, the container normalises for num_random_vectors = %d" % (Gr.nv, container.n_rand_vecs))


def _create_args(container, model, mu):
    """The arguments of elph_meas_create after the handle and of elph_meas_chains_create after nchains: the model's parameters with `mu`
    (float64: Nsites, or a row per chain), the bonds and the container's requests.  The second value keeps the arrays alive for the call."""
    sites, t = bond_arrays(model)
    request = _request_arrays(container.onsite_corr, ONSITE_CORR)
    par = [np.ascontiguousarray(a, dtype=np.float64) for a in (model.omega, model.omega4, model.lam)]
    args = [*map(dptr, par), dptr(mu), float(model.dtau), sites.shape[0], int(model.nbonds), iptr(sites) if sites.size else None,
            dptr(t) if t.size else None, *map(_ip, request)]
    return args, (sites, t, request, par, mu)


def _ensure_device(container, model, Gr):
    if container._device_of is model:
        return
    _refuse_ssh(model, "measurements")
    _check_estimator(container, model, Gr)
    args, keep = _create_args(container, model, np.ascontiguousarray(model.mu, dtype=np.float64))
    check(model._lib.elph_meas_create(model._h, *args))
    container._device_of = model


def accumulate_(container, model, Gr):
    """make_measurements! without its update! (:550-560): every pair i < j of the estimator's vectors is set up and folded into the device's
    accumulators; nothing comes back to the host."""
    _refuse_chains(model, "measurements")
    _ensure_device(container, model, Gr)
    check(model._lib.elph_meas_accumulate(model._h, dptr(np.ascontiguousarray(model.x, dtype=np.float64))))
    Gr.n1, Gr.n2 = Gr.nv - 1, Gr.nv                                         # the estimator's device tables are the last pair's now


def make_measurements_(container, model, Gr, nmeas, P=None, R=None, rng=None):
    """make_measurements!(container, model, Gr, nmeas, preconditioner) (:545-566).  R / rng: the noise vectors of update_ (greens.py).
    Returns update_'s (iters, residual_error, flag).  nmeas numbers the snapshots of the reference; none are taken here."""
    out = _greens.update_(Gr, model, P, rng=rng, R=R)
    accumulate_(container, model, Gr)
    return out


def _scalar_buffer(container, keys=KEYS):
    """The buffer a *_fetch call fills: the global scalars, every on-site key per orbital, every inter-site key per bond definition."""
    no, nb = len(container.onsite_meas["density"]), len(container.intersite_meas["el_ke"])
    return np.zeros(len(keys[0]) + len(keys[1]) * no + len(keys[2]) * nb)


def _store_scalars(container, scal, keys=KEYS):
    no, nb = len(container.onsite_meas["density"]), len(container.intersite_meas["el_ke"])
    for i, k in enumerate(keys[0]):
        container.global_meas[k] = complex(scal[i])
    at = len(keys[0])
    for i, k in enumerate(keys[1]):
        container.onsite_meas[k][:] = scal[at + i * no:at + (i + 1) * no]
    at += len(keys[1]) * no
    for i, k in enumerate(keys[2]):
        container.intersite_meas[k][:] = scal[at + i * nb:at + (i + 1) * nb]


def _fetch_buffers(container):
    """(scalars, the position arrays' pointers in ONSITE_CORR order) for a *_fetch call into the container."""
    return _scalar_buffer(container), position_pointers(container.onsite_corr, ONSITE_CORR)


def fetch_(container, model):
    """The device's un-normalised sums into the container (position arrays and scalars); the momentum arrays are not touched."""
    require_device(container, model)
    scal, ptrs = _fetch_buffers(container)
    check(model._lib.elph_meas_fetch(model._h, dptr(scal), *ptrs))
    _store_scalars(container, scal)


def simpson(f, dx):
    """simpson(f, dx) (Utilities.jl:65-76) along the first axis: composite Simpson over pairs of intervals and, for an even number of
    points, the reference's end correction over the last interval."""
    f = np.asarray(f)
    n = f.shape[0]
    F = np.zeros(f.shape[1:], dtype=f.dtype)
    for i in range(1, n - 1, 2):                                            # Julia's i = 2, 4, ..., <= n - 1
        F = F + dx * (1 / 3 * f[i - 1] + 4 / 3 * f[i] + 1 / 3 * f[i + 1])
    if n % 2 == 0:
        F = F + dx * (5 / 12 * f[n - 1] + 2 / 3 * f[n - 2] - 1 / 12 * f[n - 3])
    return F


def fourier_transform_correlations_(group):
    """fourier_transform_correlations! (:1160-1170): momentum = fft of position over the three cell axes."""
    for corr in group.values():
        corr.momentum[...] = np.fft.fftn(corr.position, axes=(1, 2, 3))


def _bin_volume(container, bin_size):
    """bin_size * binomial(n_rand_vecs, 2): the pairs of vectors a bin's sums run over (:590-592)."""
    V = int(bin_size) * comb(container.n_rand_vecs, 2)
    if V == 0:
        raise ValueError("bin_size * binomial(num_random_vectors = %d, 2) is zero" % container.n_rand_vecs)
    return V


def _divide_group(group, V):
    for corr in group.values():
        corr.position /= V
        corr.momentum /= V


def _simpson_group(susc_group, corr_group, table, dtau):
    """measure_susceptibility! (:2550-2572) for the susceptibilities of `table` that are measured."""
    for susc, corr in table:
        if susc in susc_group:
            susc_group[susc].position[...] = simpson(corr_group[corr].position, dtau)
            susc_group[susc].momentum[...] = simpson(corr_group[corr].momentum, dtau)


def _process_group(corr_group, susc_group, table, V, dtau):
    """A group's part of process_measurements! (:574-676): momentum = fft over the cell axes, both divided by V, Simpson's rule over tau."""
    fourier_transform_correlations_(corr_group)
    _divide_group(corr_group, V)
    _simpson_group(susc_group, corr_group, table, dtau)


def _divide_scalars(container, V):
    for k in container.global_meas:
        container.global_meas[k] /= V
    for group in (container.onsite_meas, container.intersite_meas):
        for k in group:
            group[k] /= V


def normalize_(container, bin_size):
    """:590-629: everything divided by bin_size * binomial(n_rand_vecs, 2)."""
    V = _bin_volume(container, bin_size)
    _divide_scalars(container, V)
    _divide_group(container.onsite_corr, V)


def measure_susceptibilities_(container, dtau):
    """:636-663 with measure_susceptibility! (:2550-2572): Simpson's rule over tau of the normalised correlations."""
    _simpson_group(container.onsite_susc, container.onsite_corr, SUSC_OF, dtau)


def _process_fetched(container, bin_size, dtau):
    """process_measurements! after the fetch: momentum copy, normalisation, susceptibilities."""
    fourier_transform_correlations_(container.onsite_corr)
    normalize_(container, bin_size)
    measure_susceptibilities_(container, dtau)


def process_measurements_(container, bin_size, model):
    """process_measurements!(container, sim_params, model) (:574-676); bin_size is sim_params.bin_size."""
    fetch_(container, model)
    _process_fetched(container, bin_size, model.dtau)


def _write_correlation(arr, name, space, datafolder, bin):
    """write_correlation! (:1258-1274)."""
    meas = "%s_%s" % (name, space)
    with open(os.path.join(datafolder, meas + "_f", "%s_%.5d.out" % (meas, bin)), "w") as f:
        f.write("index %s_real %s_imag\n" % (meas, meas))
        flat = arr.reshape(-1, order="F")
        f.writelines("%d %.8f %.8f\n" % (i + 1, v.real, v.imag) for i, v in enumerate(flat))


def _write_groups(datafolder, bin, *groups):
    for group in groups:
        for name, corr in group.items():
            _write_correlation(corr.position, name, "position", datafolder, bin)
            _write_correlation(corr.momentum, name, "momentum", datafolder, bin)


def _zero_groups(*groups):
    for group in groups:
        for corr in group.values():
            corr.position[...] = 0
            corr.momentum[...] = 0


def write_measurements_(container, model, bin, keys=KEYS):
    """write_measurements!(container, model, bin) (:681-693, :1175-1274); keys: the scalars' line order (the model's KEYS)."""
    d = container.datafolder
    with open(os.path.join(d, "global_measurements_f", "global_measurements_%.5d.out" % bin), "w") as f:
        for k in keys[0]:
            f.write("%s %.8f\n" % (k, container.global_meas[k].real))
    with open(os.path.join(d, "onsite_measurements_f", "onsite_measurements_%.5d.out" % bin), "w") as f:
        f.write("measurement orbit value\n")
        for k in keys[1]:
            for o, v in enumerate(container.onsite_meas[k]):
                f.write("%s %d %.8f\n" % (k, o + 1, v.real))
    with open(os.path.join(d, "intersite_measurements_f", "intersite_measurements_%.5d.out" % bin), "w") as f:
        f.write("measurement bond value\n")
        for k in keys[2]:
            for b, v in enumerate(container.intersite_meas[k]):
                f.write("%s %d %.8f\n" % (k, b + 1, v.real))
    _write_groups(d, bin, container.onsite_corr, container.intersite_corr, container.onsite_susc, container.intersite_susc)


def _zero_container(container):
    for k in container.global_meas:
        container.global_meas[k] = 0j
    for group in (container.onsite_meas, container.intersite_meas):
        for k in group:
            group[k][:] = 0
    _zero_groups(container.onsite_corr, container.intersite_corr, container.onsite_susc, container.intersite_susc)


def reset_measurements_(container, model):
    """reset_measurements!(container, model) (:698-758): the container's arrays and the device's accumulators to zero."""
    _zero_container(container)
    reset_device(container, model, "elph_meas_reset")
