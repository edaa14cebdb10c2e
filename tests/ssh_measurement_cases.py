"""The models of the SSH measurement tests (tests/test_ssh_measurements_host.py, tests/test_gpu_ssh_measurements.py), built as
tests/ssh_cases.py builds its cases: bond definitions of ssh_cases.SHAPES, t and alpha drawn by initialize_model_ from the disorder widths,
alpha2 (both signs), omega (per phonon) and mu (per site) written over afterwards, and a rough synthetic field with both signs."""
import numpy as np

import ssh_cases as sc

ALL_TD = {k: {"measure": True, "time_dependent": True} for k in ("Greens", "DenDen", "SpinSpin", "PairGreens", "PhononGreens")}
CUBIC3 = [(1, 1, (1, 0, 0), True, "x", 1.0), (1, 1, (1, 1, 0), True, "d", 1.0), (1, 1, (1, 0, 1), True, "e", 1.0)]      # no bond removed as a duplicate
HC3_TABLE = {"Greens": {"measure": True, "time_dependent": True, "pairs": [[2, 2], [1, 2]]},
             "DenDen": {"measure": True, "time_dependent": False, "pairs": [[2, 1], [1, 1]]},                          # the equal-time request
             "SpinSpin": {"measure": True, "time_dependent": True, "pairs": [[1, 2]]},
             "PairGreens": {"measure": True, "time_dependent": True, "pairs": [[2, 1], [2, 2]]},
             "PhononGreens": {"measure": True, "time_dependent": True, "pairs": [[3, 1], [1, 2], [2, 2]]}}


def _shape(name):
    norb, dims, defs, L = sc.SHAPES[name]
    return norb, dims, defs, L


# name -> (orbitals, cells, bond definitions, Ltau, [measurements] table, mean alpha, median |x| or None)
CASES = {
    "hc3": _shape("hc3") + (HC3_TABLE, sc.ALPHA_MEAN, None),
    "psq6": _shape("psq6") + (ALL_TD, sc.ALPHA_MEAN, None),
    "tri4_Lt7": _shape("tri4_Lt7") + (ALL_TD, sc.ALPHA_MEAN, None),
    "hc3_Lt2": _shape("hc3_Lt2") + (ALL_TD, sc.ALPHA_MEAN, None),
    "cubic3x2x2": (1, (3, 2, 2), CUBIC3, 5, ALL_TD, sc.ALPHA_MEAN, None),
    # alpha raised to the size of t and the field scaled to a median |x| of one: t' changes sign on some bonds and slices, not on all
    "sq12x6": _shape("sq12x6") + (ALL_TD, 1.0, 1.0),
}


def build_model(norb, dims, defs, L, seed, alpha_mean=sc.ALPHA_MEAN, x_median=None, device=True, tol=1e-13):
    from elphdynamics_amd import lattice as lat, models, synth
    m = models.SSHModel(lat.Lattice(norb, *dims), L * sc.DTAU, sc.DTAU, tol=tol, maxiter=20000)
    assert m.Ltau == L
    for (o1, o2, d, has_phonon, nm, tmean) in defs:
        m.assign_hopping_(tmean, alpha_mean, 0.0, sc.OMEGA_MEAN, o1, o2, d, has_phonon=has_phonon, name=nm, t_std=sc.T_STD, alpha_std=sc.ALPHA_STD)
    if not device:
        m._create = lambda *a, **k: None
    rng = np.random.default_rng(seed)
    m.initialize_model_(rng=rng)
    m.alpha2[:] = 0.03 * rng.standard_normal(m.Nph)
    m.omega = sc.OMEGA_MEAN + 0.05 * rng.standard_normal(m.Nph)
    m.mu[:] = 0.1 * rng.standard_normal(m.Nsites)
    x = synth.phonon_field(m.Nph, L, m.beta, m.dtau, omega=sc.OMEGA_MEAN, lam=0.0, seed=seed)
    x = x - x.mean()
    if x_median is not None:
        x = x * (x_median / np.median(np.abs(x)))
    else:                                                                   # the regime of ssh_cases: the coupling term at most half the smallest |t|
        X = x.reshape(m.Nph, L)
        worst = np.max(np.abs(m.alpha)[:, None] * np.abs(X) + np.abs(m.alpha2)[:, None] * X ** 2)
        x = x * min(1.0, 0.5 * np.min(np.abs(m.t)) / worst)
    m.x[:] = x
    assert m.x.min() < 0.0 < m.x.max()
    if device:
        models.update_model_(m)
    return m


def build_case(name, device=True, tol=1e-13):
    norb, dims, defs, L, table, alpha_mean, x_median = CASES[name]
    return build_model(norb, dims, defs, L, 9000 + list(CASES).index(name), alpha_mean, x_median, device, tol), table


def ref_par(m):
    """The reference's parameters of a model; the bonds come from the lattice per definition (not from the model's sorted table), the
    phonons from a running count over the definitions that carry one."""
    la = m.lattice
    bonds, nb, nph = [], 0, 0
    for d in m.bond_definitions:
        tab = la.calc_neighbor_table(d["o1"], d["o2"], d["v"])
        n = tab.shape[0]
        phn = None
        if d["has_phonon"]:
            phn = np.arange(nph, nph + n)
            nph += n
        bonds.append((tab[:, 0], tab[:, 1], m.t[nb:nb + n], phn))
        nb += n
    assert nb == m.Nbonds and nph == m.Nph
    return dict(L=m.Ltau, ns=la.norbits, dims=(la.L1, la.L2, la.L3), dtau=m.dtau, mu=m.mu, nph=m.nph, omega=m.omega, alpha=m.alpha,
                alpha2=m.alpha2, bonds=bonds)


def request_of(c):
    return {k: (v.position.shape[0], v.pairs) for k, v in list(c.onsite_corr.items()) + list(c.intersite_corr.items())}
