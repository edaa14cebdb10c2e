"""Snapshot measurements of Measurements.jl: per-site profiles of one configuration, one file per measurement, for one configuration
or every chain resident in a handle (a lockstep run), Holstein and SSH models alike.  A container of its own beside the on-site ones
(measurements.py, chain_measurements.py, ssh_measurements.py, ssh_chain_measurements.py), which keep refusing a true
[measurements.Snapshots] entry: split_info hands each kind of container its part of one deck's [measurements] table.

    rest, snap = split_info(info)                                      info without its Snapshots table, the Snapshots table
    sc = initialize_snapshots_container(model, info, datafolders)      Measurements.jl:57-82; info: the [measurements] table
    initialize_snapshot_folders_(sc)                                   :352-359   <name>_snapshots_f in every chain's folder
    arrays = snapshot_arrays_(sc, model, Gr, X=None)                   :1351-1460 name -> (nchains, Nsites) or (nchains, Nph)
    write_snapshots_(sc, arrays, nmeas)                                the files, pure host code
    take_snapshots_(sc, model, Gr, nmeas, X=None)                      make_snapshot_measurements! (:822-838): the two above

datafolders is one string (one configuration) or one folder per resident chain.  sc.snapshots lists the requested names in the
reference's order: density, double_occupancy, phonon_position.  density and double_occupancy come from one device call for all chains
(elph_snapshots, csrc/snapshots.hip) over the vectors the estimator holds after greens.update_ (or greens.set_vectors_), vector v of
chain c at row v * nchains + c; only what is requested is copied back.  phonon_position is the tau-mean of the field: of X
((nchains, Ndof), the HybridMonteCarlo's X after pull_()), or of model.x for one configuration when X is not given.  The double
occupancy keeps the reference's ranges (n = 1..n_v - 1, m = 2..n_v: for n_v > 2 they hold n = m terms), see csrc/snapshots.hip.

A file is <folder>/<name>_snapshots_f/<name>_snapshot_%.6d.out: the bare name on the first line, then one "%.8f" line per site or
phonon.  take_snapshots_ goes where the reference's make_measurements! ends: after the container's accumulate_, with the same nmeas.
Sharded and slab handles are refused by the library.
"""
import os

import numpy as np

from ._chain_unit import chain_folders, chain_rows, check_chains
from ._lib import check, dptr
from .measurements import UnsupportedMeasurement

SNAPSHOTS = ("density", "double_occupancy", "phonon_position")          # the reference's order (:57-82)


class SnapshotsContainer:
    def __init__(self, snapshots, datafolders, nchains):
        self.snapshots = snapshots           # the requested names, in the order of SNAPSHOTS
        self.datafolders = datafolders       # one folder per chain
        self.nchains = nchains


def split_info(info):
    """(info without its Snapshots table, the Snapshots table): one [measurements] table for both kinds of container."""
    info = dict(info or {})
    snap = dict(info.pop("Snapshots", None) or {})
    return info, snap


def initialize_snapshots_container(model, info, datafolders):
    """The snapshot part of initialize_measurements_container (:57-82) for the [measurements] table `info`; datafolders: one string for
    one configuration, or one folder per resident chain."""
    datafolders = chain_folders(model, datafolders)
    _, snap = split_info(info)
    for key, val in snap.items():
        if val is True and key not in SNAPSHOTS:
            raise UnsupportedMeasurement("[measurements.Snapshots] %s = true: there is no such snapshot (%s)" % (key, ", ".join(SNAPSHOTS)))
    return SnapshotsContainer([name for name in SNAPSHOTS if snap.get(name, False) is True], [os.fspath(f) for f in datafolders], len(datafolders))


def initialize_snapshot_folders_(sc):
    """The snapshot part of initialize_measurement_folders! (:352-359), in every chain's folder."""
    for folder in sc.datafolders:
        for name in sc.snapshots:
            os.mkdir(os.path.join(folder, "%s_snapshots_f" % name))


def snapshot_arrays_(sc, model, Gr, X=None):
    """name -> array for every requested snapshot: density and double_occupancy (nchains, Nsites) from one elph_snapshots call that
    asks for what is requested only, phonon_position (nchains, Nph) from X or, for one configuration, model.x."""
    if Gr.model is not model:
        raise ValueError("the estimator was made for another model")
    check_chains(sc, model)
    nch = sc.nchains
    out = {}
    if "phonon_position" in sc.snapshots:
        if X is None:
            if nch != 1:
                raise ValueError("phonon_position of %d resident chains needs X, (nchains, Ndof)" % nch)
            X = model.x
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim == 1 and nch == 1:
            X = X[None]
        X = chain_rows(X, nch, model.Ndof, "X")
    device = [name for name in sc.snapshots if name != "phonon_position"]
    if device:
        for name in device:
            out[name] = np.zeros((nch, model.Nsites))
        ptr = lambda name: dptr(out[name]) if name in out else None  # noqa: E731
        check(model._lib.elph_snapshots(model._h, nch, ptr("density"), ptr("double_occupancy")))
    if "phonon_position" in sc.snapshots:
        # x viewed as (Ltau, Nph) in the reference, tau fastest: mean(x[:, p]) (:1441-1456)
        out["phonon_position"] = X.reshape(nch, model.Nph, model.Ltau).mean(axis=2)
    return {name: out[name] for name in sc.snapshots}


def write_snapshots_(sc, arrays, nmeas):
    """One file per requested snapshot and chain (:1362, :1400, :1445): the name, then "%.8f" per site or phonon."""
    for name in sc.snapshots:
        a = np.asarray(arrays[name], dtype=np.float64)
        if a.ndim != 2 or a.shape[0] != sc.nchains:
            raise ValueError("%s has shape %s, not (nchains, n) with nchains = %d" % (name, a.shape, sc.nchains))
        for folder, row in zip(sc.datafolders, a):
            path = os.path.join(folder, "%s_snapshots_f" % name, "%s_snapshot_%.6d.out" % (name, nmeas))
            with open(path, "w") as f:
                f.write(name + "\n")
                f.write("".join("%.8f\n" % v for v in row))


def take_snapshots_(sc, model, Gr, nmeas, X=None):
    """make_snapshot_measurements!(container, model, Gr, nmeas) (:822-838) for every chain; returns the arrays it wrote."""
    arrays = snapshot_arrays_(sc, model, Gr, X) if sc.snapshots else {}
    write_snapshots_(sc, arrays, nmeas)
    return arrays
