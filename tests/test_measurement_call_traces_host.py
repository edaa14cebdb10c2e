"""The library calls of the nine measurement modules, written out: each module is driven through its lifecycle (constructor, folders,
accumulate twice, fetch, process, write, reset) on a host model whose `_lib` is a stand-in that records every call and returns 0, and
the recorded sequence is compared with the literal one below.  None of this needs a device.

A recorded call is (name, the scalar arguments in order, one letter per argument: "s" a scalar, "p" a pointer, "0" None).  The chain
families run on two chains, get their second accumulate with `mu` where they take one, and a third with a fresh estimator object, after
which the device side is made again.  The texts of the checks the families share are pinned verbatim, and the scalar files of the
Holstein and the SSH single containers are compared byte for byte where their keys coincide."""
import os

import numpy as np
import pytest

from test_bond_measurements_host import HONEYCOMB, TD
from test_measurements_host import host_model
from test_ssh_measurements_host import host_case

NV, NCH = 2, 2
ONSITE = {"num_random_vectors": NV, "Greens": TD, "DenDen": {"measure": True, "time_dependent": False}, "PairGreens": TD}
SSH_ONSITE = dict(ONSITE, PhononGreens=TD)
BONDS = {"num_random_vectors": NV, "BondBond": TD, "BondPairGreens": TD}
SSH_BONDS = dict(BONDS, CurrentCurrent={"measure": True, "time_dependent": False})
CURRENT = {"num_random_vectors": NV, "CurrentCurrent": TD}


class Recorder:
    """model._lib: every attribute is a function that records its call and returns 0 (ELPH_OK)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            scalar = [isinstance(a, (int, float, np.integer, np.floating)) for a in args]
            self.calls.append((name, tuple(a for a, s in zip(args, scalar) if s),
                               "".join("s" if s else "0" if a is None else "p" for a, s in zip(args, scalar))))
            return 0
        return call


class FakeEstimator:
    def __init__(self, model, nv):
        self.model, self.nv = model, nv


def holstein(nchains=1):
    m = host_model(ns=2, dims=(3, 2, 1), L=7, bonds=HONEYCOMB)
    m._nchains, m._lib, m._h = nchains, Recorder(), 1
    return m


def ssh(nchains=1):
    m = host_case("hc3_Lt2")
    m._nchains, m._lib, m._h = nchains, Recorder(), 1
    return m


def folders(tmp_path, n):
    out = [str(tmp_path / ("chain%d" % k)) for k in range(n)]
    for f in out:
        os.mkdir(f)
    return out


def single(mod, names, model, info, tmp_path):
    """The lifecycle of a single-configuration module; names: its constructor, folders, accumulate, fetch, process, write, reset."""
    new, mkdirs, accumulate, fetch, process, write, reset = (getattr(mod, n) for n in names)
    c = new(model, info, folders(tmp_path, 1)[0])
    mkdirs(c)
    with pytest.raises(RuntimeError) as e:
        fetch(c, model)
    Gr = FakeEstimator(model, NV)
    accumulate(c, model, Gr)
    accumulate(c, model, Gr)
    fetch(c, model)
    process(c, 3, model)
    write(c, model, 1)
    reset(c, model)
    return model._lib.calls, str(e.value)


def chains(mod, names, model, info, tmp_path, X=False, mu=False):
    """The lifecycle of a chain module on two chains; X, mu: what its accumulate takes."""
    new, mkdirs, accumulate, fetch, process, write, reset = (getattr(mod, n) for n in names)
    c = new(model, info, folders(tmp_path, NCH))
    mkdirs(c)
    with pytest.raises(RuntimeError) as e:
        fetch(c, model)
    Gr = FakeEstimator(model, NV * NCH)
    x = [np.zeros((NCH, model.Ndof))] if X else []
    accumulate(c, model, Gr, *x)
    if mu:
        accumulate(c, model, Gr, *x, mu=np.ones((NCH, model.Nsites)))
    else:
        accumulate(c, model, Gr, *x)
    accumulate(c, model, FakeEstimator(model, NV * NCH), *x)                # a new estimator has dropped the device side
    fetch(c, model)
    process(c, 3, model)
    write(c, model, 1)
    reset(c, model)
    return model._lib.calls, str(e.value)


MS = ("initialize_measurements_container", "initialize_measurement_folders_", "accumulate_", "fetch_", "process_measurements_",
      "write_measurements_", "reset_measurements_")
SM = ("initialize_ssh_measurements_container",) + MS[1:]
CMS = ("initialize_chain_measurements_container",) + MS[1:]
SCM = ("initialize_ssh_chain_measurements_container",) + MS[1:]
BM = ("initialize_bond_container", "initialize_bond_folders_", "accumulate_bonds_", "fetch_bonds_", "process_bond_measurements_",
      "write_bond_measurements_", "reset_bond_measurements_")
CBM = ("initialize_chain_bond_container",) + BM[1:]
SB = ("initialize_ssh_bond_container", "initialize_ssh_bond_folders_", "accumulate_ssh_bonds_", "fetch_ssh_bonds_",
      "process_ssh_bond_measurements_", "write_ssh_bond_measurements_", "reset_ssh_bond_measurements_")
SCB = ("initialize_ssh_chain_bond_container",) + SB[1:]
CUR = ("initialize_current_container", "initialize_current_folders_", "accumulate_current_", "fetch_current_",
       "process_current_measurements_", "write_current_measurements_", "reset_current_measurements_")

NOTHING = "nothing has been measured on this model yet"


def test_measurements_trace(tmp_path):
    from elphdynamics_amd import measurements as ms
    calls, early = single(ms, MS, holstein(), ONSITE, tmp_path)
    assert early == NOTHING
    assert calls == [("elph_meas_create", (1, 0.1, 18, 3), "sppppssspppppp"),
                     ("elph_meas_accumulate", (1,), "sp"),
                     ("elph_meas_accumulate", (1,), "sp"),
                     ("elph_meas_fetch", (1,), "sppp0p0"),                  # fetch_, then process_measurements_' own
                     ("elph_meas_fetch", (1,), "sppp0p0"),
                     ("elph_meas_reset", (1,), "s")]


def test_ssh_measurements_trace(tmp_path):
    from elphdynamics_amd import ssh_measurements as sm
    calls, early = single(sm, SM, ssh(), SSH_ONSITE, tmp_path)
    assert early == NOTHING
    assert calls == [("elph_ssh_meas_create", (1, 0.05, 27, 3, 27, 3), "spsssppppssppppppp"),
                     ("elph_ssh_meas_accumulate", (1,), "sp"),
                     ("elph_ssh_meas_accumulate", (1,), "sp"),
                     ("elph_ssh_meas_fetch", (1,), "sppp0pp"),
                     ("elph_ssh_meas_fetch", (1,), "sppp0pp"),
                     ("elph_ssh_meas_reset", (1,), "s")]


def test_bond_measurements_trace(tmp_path):
    from elphdynamics_amd import bond_measurements as bm
    calls, early = single(bm, BM, holstein(), BONDS, tmp_path)
    assert early == "no bond correlation has been measured on this model yet"
    assert calls == [("elph_bond_create", (1, 3), "ssppppppp"),
                     ("elph_bond_accumulate", (1,), "s"),
                     ("elph_bond_accumulate", (1,), "s"),
                     ("elph_bond_fetch", (1,), "spp"),
                     ("elph_bond_fetch", (1,), "spp"),
                     ("elph_bond_reset", (1,), "s")]


def test_ssh_bond_measurements_trace(tmp_path):
    from elphdynamics_amd import ssh_bond_measurements as sb
    calls, early = single(sb, SB, ssh(), SSH_BONDS, tmp_path)
    assert early == "no SSH bond correlation has been measured on this model yet"
    assert calls == [("elph_ssh_bond_create", (1, 3, 27, 27), "sspppspppspppppp"),
                     ("elph_ssh_bond_accumulate", (1,), "sp"),
                     ("elph_ssh_bond_accumulate", (1,), "sp"),
                     ("elph_ssh_bond_fetch", (1,), "sppp"),
                     ("elph_ssh_bond_fetch", (1,), "sppp"),
                     ("elph_ssh_bond_reset", (1,), "s")]


def test_chain_measurements_trace(tmp_path):
    from elphdynamics_amd import chain_measurements as cms
    calls, early = chains(cms, CMS, holstein(NCH), ONSITE, tmp_path, X=True, mu=True)
    assert early == NOTHING
    assert calls == [("elph_meas_chains_create", (1, 2, 0.1, 18, 3), "ssppppssspppppp"),
                     ("elph_meas_chains_accumulate", (1,), "sp"),
                     ("elph_meas_chains_set_mu", (1,), "sp"),
                     ("elph_meas_chains_accumulate", (1,), "sp"),
                     ("elph_meas_chains_create", (1, 2, 0.1, 18, 3), "ssppppssspppppp"),       # the fresh estimator
                     ("elph_meas_chains_accumulate", (1,), "sp"),
                     ("elph_meas_chains_fetch", (1, 0), "ssppp0p0"),
                     ("elph_meas_chains_fetch", (1, 1), "ssppp0p0"),
                     ("elph_meas_chains_fetch", (1, 0), "ssppp0p0"),
                     ("elph_meas_chains_fetch", (1, 1), "ssppp0p0"),
                     ("elph_meas_chains_reset", (1,), "s")]


def test_ssh_chain_measurements_trace(tmp_path):
    from elphdynamics_amd import ssh_chain_measurements as scm
    calls, early = chains(scm, SCM, ssh(NCH), SSH_ONSITE, tmp_path, X=True, mu=True)
    assert early == NOTHING
    assert calls == [("elph_ssh_meas_chains_create", (1, 2, 0.05, 27, 3, 27, 3), "sspsssppppssppppppp"),
                     ("elph_ssh_meas_chains_accumulate", (1,), "sp"),
                     ("elph_ssh_meas_chains_set_mu", (1,), "sp"),
                     ("elph_ssh_meas_chains_accumulate", (1,), "sp"),
                     ("elph_ssh_meas_chains_create", (1, 2, 0.05, 27, 3, 27, 3), "sspsssppppssppppppp"),
                     ("elph_ssh_meas_chains_accumulate", (1,), "sp"),
                     ("elph_ssh_meas_chains_fetch", (1, 0), "ssppp0pp"),
                     ("elph_ssh_meas_chains_fetch", (1, 1), "ssppp0pp"),
                     ("elph_ssh_meas_chains_fetch", (1, 0), "ssppp0pp"),
                     ("elph_ssh_meas_chains_fetch", (1, 1), "ssppp0pp"),
                     ("elph_ssh_meas_chains_reset", (1,), "s")]


def test_chain_bond_measurements_trace(tmp_path):
    from elphdynamics_amd import chain_bond_measurements as cbm
    calls, early = chains(cbm, CBM, holstein(NCH), BONDS, tmp_path)
    assert early == "no bond correlation has been measured on this model yet"
    assert calls == [("elph_bond_chains_create", (1, 2, 3), "sssppppppp"),
                     ("elph_bond_chains_accumulate", (1,), "s"),
                     ("elph_bond_chains_accumulate", (1,), "s"),
                     ("elph_bond_chains_create", (1, 2, 3), "sssppppppp"),
                     ("elph_bond_chains_accumulate", (1,), "s"),
                     ("elph_bond_chains_fetch", (1, 0), "sspp"),
                     ("elph_bond_chains_fetch", (1, 1), "sspp"),
                     ("elph_bond_chains_fetch", (1, 0), "sspp"),
                     ("elph_bond_chains_fetch", (1, 1), "sspp"),
                     ("elph_bond_chains_reset", (1,), "s")]


def test_ssh_chain_bond_measurements_trace(tmp_path):
    from elphdynamics_amd import ssh_chain_bond_measurements as scb
    calls, early = chains(scb, SCB, ssh(NCH), SSH_BONDS, tmp_path, X=True)
    assert early == "no SSH bond correlation has been measured on this model yet"
    assert calls == [("elph_ssh_bond_chains_create", (1, 2, 3, 27, 27), "ssspppspppspppppp"),
                     ("elph_ssh_bond_chains_accumulate", (1,), "sp"),
                     ("elph_ssh_bond_chains_accumulate", (1,), "sp"),
                     ("elph_ssh_bond_chains_create", (1, 2, 3, 27, 27), "ssspppspppspppppp"),
                     ("elph_ssh_bond_chains_accumulate", (1,), "sp"),
                     ("elph_ssh_bond_chains_fetch", (1, 0), "ssppp"),
                     ("elph_ssh_bond_chains_fetch", (1, 1), "ssppp"),
                     ("elph_ssh_bond_chains_fetch", (1, 0), "ssppp"),
                     ("elph_ssh_bond_chains_fetch", (1, 1), "ssppp"),
                     ("elph_ssh_bond_chains_reset", (1,), "s")]


def test_current_measurements_trace(tmp_path):
    """One configuration (a single folder name, one chain) and two resident chains."""
    from elphdynamics_amd import current_measurements as cur
    os.mkdir(tmp_path / "one")
    calls, early = single(cur, CUR, holstein(), CURRENT, tmp_path / "one")
    assert early == "no CurrentCurrent has been measured on this model yet"
    assert calls == [("elph_current_create", (1, 1, 3, 18, 1, 1, 9), "ssspppspsssp"),
                     ("elph_current_accumulate", (1,), "s"),
                     ("elph_current_accumulate", (1,), "s"),
                     ("elph_current_fetch", (1, 0), "ssp"),
                     ("elph_current_fetch", (1, 0), "ssp"),
                     ("elph_current_reset", (1,), "s")]
    calls, early = chains(cur, CUR, holstein(NCH), CURRENT, tmp_path)
    assert early == "no CurrentCurrent has been measured on this model yet"
    assert calls == [("elph_current_create", (1, 2, 3, 18, 1, 1, 9), "ssspppspsssp"),
                     ("elph_current_accumulate", (1,), "s"),
                     ("elph_current_accumulate", (1,), "s"),
                     ("elph_current_create", (1, 2, 3, 18, 1, 1, 9), "ssspppspsssp"),
                     ("elph_current_accumulate", (1,), "s"),
                     ("elph_current_fetch", (1, 0), "ssp"),
                     ("elph_current_fetch", (1, 1), "ssp"),
                     ("elph_current_fetch", (1, 0), "ssp"),
                     ("elph_current_fetch", (1, 1), "ssp"),
                     ("elph_current_reset", (1,), "s")]


def chain_families():
    """(module, its names, model maker, request, whether accumulate takes X, whether it takes mu) of the five chain containers."""
    from elphdynamics_amd import (chain_bond_measurements as cbm, chain_measurements as cms, current_measurements as cur,
                                  ssh_chain_bond_measurements as scb, ssh_chain_measurements as scm)
    return [(cms, CMS, holstein, ONSITE, True, True), (scm, SCM, ssh, SSH_ONSITE, True, True), (cbm, CBM, holstein, BONDS, False, False),
            (scb, SCB, ssh, SSH_BONDS, True, False), (cur, CUR, holstein, CURRENT, False, False)]


def message(exc, call, *args, **kw):
    with pytest.raises(exc) as e:
        call(*args, **kw)
    return str(e.value)


def test_the_shared_checks_have_one_text_each_and_come_before_the_library():
    for mod, names, make, info, takes_X, takes_mu in chain_families():
        new, accumulate = getattr(mod, names[0]), getattr(mod, names[2])
        m = make(3)
        assert message(ValueError, new, m, info, ["", ""]) == "2 data folders for the 3 chains resident in the model", mod.__name__
        assert message(ValueError, new, m, info, [""] * 4) == "4 data folders for the 3 chains resident in the model", mod.__name__
        c = new(m, info, ["", "", ""])
        x = [np.zeros((3, m.Ndof))] if takes_X else []
        assert (message(ValueError, accumulate, c, m, FakeEstimator(m, 5), *x)
                == "the estimator holds 5 vectors, the container normalises for num_random_vectors = 2 for each of 3 chains"), mod.__name__
        est = FakeEstimator(m, 6)
        if takes_X:
            assert (message(ValueError, accumulate, c, m, est, np.zeros((2, m.Ndof)))
                    == "X has shape (2, %d), not (nchains, Ndof) = (3, %d)" % (m.Ndof, m.Ndof)), mod.__name__
            assert (message(ValueError, accumulate, c, m, est, np.zeros(3 * m.Ndof))
                    == "X has shape (%d,), not (nchains, Ndof) = (3, %d)" % (3 * m.Ndof, m.Ndof)), mod.__name__
        if takes_mu:
            assert (message(ValueError, accumulate, c, m, est, *x, mu=np.zeros((3, m.Nsites + 1)))
                    == "mu has shape (3, %d), not (nchains, Nsites) = (3, %d)" % (m.Nsites + 1, m.Nsites)), mod.__name__
        m._nchains = 2
        assert (message(ValueError, accumulate, c, m, est, *x)
                == "the container was made for 3 chains, 2 are resident in the model"), mod.__name__
        assert m._lib.calls == [], mod.__name__


def scalar_lines(path, keys):
    """The header lines of a scalar file and the lines of `keys`, as bytes."""
    with open(path, "rb") as f:
        return [line for line in f if line.split()[0].decode() in keys + ("measurement",)]


def test_scalar_files_of_the_two_single_containers_agree_where_their_keys_do(tmp_path):
    """Hand-filled sums (what a fetch would have stored), the same in both containers: two orbitals and three bond definitions each."""
    from elphdynamics_amd import measurements as ms, ssh_measurements as sm
    dirs = folders(tmp_path, 2)
    h, s = holstein(), ssh()
    ch = ms.initialize_measurements_container(h, {}, dirs[0])
    cs = sm.initialize_ssh_measurements_container(s, {}, dirs[1])
    ms.initialize_measurement_folders_(ch)
    sm.initialize_measurement_folders_(cs)
    rng = np.random.default_rng(5)
    shared = []
    for group in ("onsite_meas", "intersite_meas"):
        both = tuple(k for k in getattr(ch, group) if k in getattr(cs, group))
        shared.append(both)
        for c in (ch, cs):
            for k, v in getattr(c, group).items():
                v[:] = rng.standard_normal(v.shape) * 1e3 + 1j
        for k in both:
            getattr(cs, group)[k][:] = getattr(ch, group)[k]
    assert shared == [("density", "double_occ", "mu"), ("el_ke",)]
    for k in ch.global_meas:
        ch.global_meas[k] = cs.global_meas[k] = complex(rng.standard_normal() * 1e3, 2.0)
    ms.write_measurements_(ch, h, 7)
    sm.write_measurements_(cs, s, 7)
    name = os.path.join("global_measurements_f", "global_measurements_00007.out")
    glob = open(os.path.join(dirs[0], name), "rb").read()
    assert glob == open(os.path.join(dirs[1], name), "rb").read() and glob.count(b"\n") == 3
    for kind, keys, n in (("onsite", shared[0], 2), ("intersite", shared[1], 3)):
        name = os.path.join(kind + "_measurements_f", kind + "_measurements_00007.out")
        a, b = scalar_lines(os.path.join(dirs[0], name), keys), scalar_lines(os.path.join(dirs[1], name), keys)
        assert a == b and len(a) == 1 + n * len(keys), kind
