"""Site-dependent Holstein parameters for the tests of tests/test_site_disorder_host.py and tests/test_gpu_site_disorder.py: what
assign_omega!, assign_lambda!, assign_mu! and the rest give when they are called per orbital and with a standard deviation
(HolsteinModels.jl:323-420), drawn from synth.randn so that every machine sees the same arrays.

disorder_(m) overwrites omega, omega4, lam, lam2 and mu of a Holstein model in place; the field stays the one the model carries.
The dynamics objects (FourierAccelerator, HybridMonteCarlo, the Langevin dynamics) read these arrays when they are constructed:
call disorder_ before any of them exists.
"""
import numpy as np

from elphdynamics_amd import models, synth

SEED = 77

# The seed of a configuration.  tests/test_site_disorder_host.py holds every tag of the dynamics lists to its preconditions: on
# two-orbital lattices the orbitals' means of ω, λ, μ are more than 3 within-orbital standard deviations apart; an index error moves
# every asserted quantity by 1000 bounds; the proposed swap changes S_b by 1e-3 |S_b|.  Where the draw of seed 77 misses one of them
# the tag takes the next seed that meets them all; the conditions stay:
#   b  77: swap ΔS_b / S_b = 5.5e-4                                        -> 78 (2.6e-2)
#   t  77: swap ΔS_b / S_b = 4.8e-4                                        -> 78 (2.8e-3)
#   d  77: μ means 2.72 deviations apart; 78: 1.95                         -> 79 (ω 4.09, λ 3.87, μ 5.59)
#   z  77: H1 moves by 642 bounds under a roll by one site; 78, 79: ω, μ means below 3 deviations apart   -> 80 (3.34, 3.76, 3.31)
SEEDS = {"b": 78, "t": 78, "d": 79, "z": 80}


def seed_of(tag):
    return SEEDS.get(tag, SEED)


def prepare(tag):
    """The hook the checkers of the uniform tests take (prepare=): disorder_ with the seed of `tag`."""
    return lambda m: disorder_(m, seed_of(tag))

# per-orbital means (a lattice with one orbital takes the first entries)
OMEGA = (1.0, 0.7)
LAMBDA = (1.0, 0.6)
MU = (-0.1, 0.2)


def orbitals(m):
    """The orbital of every site: sites are numbered orbital-fastest (lattice.py; _assign's slice(orbit - 1, None, norbits))."""
    return np.arange(m.Nsites) % m.lattice.norbits


def disorder_(m, seed=SEED):
    """Overwrite the model's parameter arrays in place; push them to the device when the model has a handle.  Returns m."""
    assert m.kind == models.HOLSTEIN
    N, orb = m.Nsites, orbitals(m)
    m.omega[:] = np.array(OMEGA)[orb] * (1.0 + 0.1 * synth.randn(seed + 1, N))
    m.omega4[:] = 0.05 * np.abs(synth.randn(seed + 2, N))
    m.lam[:] = np.array(LAMBDA)[orb] * (1.0 + 0.1 * synth.randn(seed + 3, N))
    m.lam2[:] = 0.03 * synth.randn(seed + 4, N)
    m.mu[:] = np.array(MU)[orb] + 0.1 * synth.randn(seed + 5, N)
    if getattr(m, "_h", None):
        models.update_model_(m)
    return m


def chain_mu(m, nchains, seed=SEED):
    """(nchains, Nsites): a chemical potential per chain and site, the rows all different."""
    return np.stack([m.mu + 0.05 * (c + 1) + 0.05 * synth.randn(seed + 10 + c, m.Nsites) for c in range(nchains)])


def rolled(m):
    """The five parameter arrays shifted by one site: what a kernel reading par[s + 1] for par[s] would use."""
    return {k: np.roll(getattr(m, k), 1) for k in ("omega", "omega4", "lam", "lam2", "mu")}


def orbitals_exchanged(m):
    """The five parameter arrays with the values of the two orbitals of every cell exchanged (two-orbital lattices)."""
    assert m.lattice.norbits == 2
    return {k: getattr(m, k).reshape(-1, 2)[:, ::-1].reshape(-1).copy() for k in ("omega", "omega4", "lam", "lam2", "mu")}


def bosonic_action(m, x=None):
    """S_b = Δτ Σ_{i,τ} [ (x_{i,τ+1} − x_{i,τ})² / (2Δτ²) + ω_i² x² / 2 + ω₄,i x⁴ ]  (HMC.jl: calc_Sb, Holstein)."""
    X = np.asarray(m.x if x is None else x).reshape(m.Nsites, m.Ltau)
    kin = (np.roll(X, -1, axis=1) - X) ** 2 / (2.0 * m.dtau ** 2)
    return float(m.dtau * np.sum(kin + 0.5 * m.omega[:, None] ** 2 * X ** 2 + m.omega4[:, None] * X ** 4))


def swap_delta_Sb(m, i, j, x=None):
    """ΔS_b of exchanging the world lines of columns i and j: the kinetic term moves with the line, the site's ω and ω₄ stay:
    Δτ Σ_τ [ (ω_i² − ω_j²)(x_j² − x_i²)/2 + (ω₄,i − ω₄,j)(x_j⁴ − x_i⁴) ]."""
    X = np.asarray(m.x if x is None else x).reshape(m.Nsites, m.Ltau)
    xi, xj = X[i], X[j]
    return float(m.dtau * np.sum(0.5 * (m.omega[i] ** 2 - m.omega[j] ** 2) * (xj ** 2 - xi ** 2)
                                 + (m.omega4[i] - m.omega4[j]) * (xj ** 4 - xi ** 4)))


def swap_columns(m):
    """The two columns the swap tests exchange: 0 and 1 (one cell, two orbitals) on a two-orbital lattice, else the two sites whose
    ω differ most."""
    if m.lattice.norbits == 2:
        return 0, 1
    return int(np.argmin(m.omega)), int(np.argmax(m.omega))
