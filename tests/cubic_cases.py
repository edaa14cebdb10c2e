"""Simple-cubic Holstein cases shared by tests/test_cubic_shape.py (host) and tests/test_gpu_cubic.py (device): the lattices the patch layout
pgrid::Cu takes (L x L x L with L = 6, 8, 10, 12 on 1, 1, 2, 4 wavefronts per time slice), a model builder with the decks' parameters
(t = omega = lambda = 1, mu = 0, dtau = 0.1; `varied`: lambda and mu per site — the site tables do not depend on the layout), and the
layout's site map restated in numpy."""
import numpy as np

CUBIC_BONDS = [(1, 1, (1, 0, 0)), (1, 1, (0, 1, 0)), (1, 1, (0, 0, 1))]
DTAU = 0.1
NW = {6: 1, 8: 1, 10: 2, 12: 4}          # wavefronts per slice: ceil((L / 2)^3 / 64)
SIDES = tuple(NW)


def tables(dims, kind="holstein", t_stddev=0.0):
    """(nsites, table, cosht, sinht) of the L1 x L2 x L3 box as HolsteinModel / SSHModel.initialize_model_ build them."""
    from elphdynamics_amd import lattice as lat
    la = lat.Lattice(1, *dims)
    defs = [la.calc_neighbor_table(o1, o2, d) for (o1, o2, d) in CUBIC_BONDS]
    raw = np.concatenate(defs, axis=0)
    if kind == "ssh":
        return la.nsites, lat.initialize_checkerboard(raw)["table"], None, None
    rng = np.random.default_rng(991)
    t = np.concatenate([np.full(d.shape[0], 1.0) + (t_stddev * rng.standard_normal(d.shape[0]) if t_stddev else 0.0) for d in defs])
    cb = lat.initialize_checkerboard(raw, t, DTAU)
    return la.nsites, cb["table"], cb["cosht"], cb["sinht"]


def cubic_model(L, ltau, tol=1e-5, seed=4343, varied=False, maxiter=20000):
    """The Holstein model on the L x L x L box with ltau time slices, its field drawn with `seed`."""
    from elphdynamics_amd import lattice as lat, models, synth
    beta = ltau * DTAU
    m = models.HolsteinModel(lat.Lattice(1, L, L, L), beta, DTAU, tol=tol, maxiter=maxiter)
    for (o1, o2, d) in CUBIC_BONDS:
        m.assign_t_(1.0, o1, o2, d)
    m.assign_omega_(1.0)
    if varied:
        rng = np.random.default_rng(seed + 1)
        m.assign_lambda_(1.0, stddev=0.2, rng=rng)
        m.assign_mu_(0.0, stddev=0.3, rng=rng)
    else:
        m.assign_lambda_(1.0)
        m.assign_mu_(0.0)
    m.initialize_model_()
    assert m.Ltau == ltau and m.Nsites == L ** 3
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, beta, DTAU, omega=1.0, lam=1.0, seed=seed)
    models.update_model_(m)
    return m


def site_of(L):
    """pgrid::Cu::site_of over all patches and registers, (G^3, 8): lane l = (X, Y, Z) = (l % G, (l / G) % G, l / G^2), G = L / 2, register
    q = cx + 2 cy + 4 cz is the site (2 X + cx) + L ((2 Y + cy) + L (2 Z + cz))."""
    G = L // 2
    l, q = np.meshgrid(np.arange(G ** 3), np.arange(8), indexing="ij")
    X, Y, Z = l % G, (l // G) % G, l // (G * G)
    return (2 * X + (q & 1)) + L * ((2 * Y + ((q >> 1) & 1)) + L * (2 * Z + (q >> 2)))
