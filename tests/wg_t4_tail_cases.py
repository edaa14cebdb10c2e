"""Inputs shared by tests/test_gpu_wg_t4_tail.py and tools/record_wg_t4_tail_bits.py: the 4-slice shape of the workgroup-resident CG kernel
(csrc/cg_wg.hip, ELPH_WG_T=4) on the 16 x 16 Holstein lattice of config C at three short time axes, which the fused tail of the iteration
treats differently and config C (teams of five) does not reach:

  * 32 slices: (T, W, G) = (4, 8, 1) — a team of one workgroup: no poll window and no boundary granules;
  * 64 slices: (4, 8, 2) — both neighbours of a workgroup are the same workgroup;
  * 96 slices: (4, 8, 3) — distinct neighbours on a ring of three.
The runs and the digest are those of wg_t4_chain_cases.py; tests/golden/wg_t4_tail_bits.json holds what they gave at the recorded commit."""
import numpy as np

from wg_t4_chain_cases import ITERS, NRHS, digest, fixed_iterations_from_guess, fixed_iterations_from_zero, guess, resident_plan, wg_fallbacks, wg_shape  # noqa: F401

SHAPES = {32: (1, 4, 8, 1), 64: (1, 4, 8, 2), 96: (1, 4, 8, 3)}          # Ltau -> (uses the resident kernel, T, W, G)
DTAU = 0.1


def model(ltau):
    """The 16 x 16 lattice of config C on `ltau` time slices, made the way configs.make_model makes a configuration."""
    from elphdynamics_amd import lattice as lat, models, synth
    beta = ltau * DTAU
    m = models.HolsteinModel(lat.Lattice(1, 16, 16, 1), beta, DTAU, tol=1e-5, maxiter=10000)
    rng = np.random.default_rng(synth.SEED_FIELDS + 991)
    for (o1, o2, d) in lat.SQUARE_BONDS:
        m.assign_t_(1.0, o1, o2, d, stddev=0.0, rng=rng)
    m.assign_omega_(1.0)
    m.assign_lambda_(1.0)
    m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, beta, DTAU, omega=1.0, lam=1.0, rough=True, seed=synth.SEED_FIELDS)
    models.update_model_(m)
    assert m.Ltau == ltau, (m.Ltau, ltau)
    return m


def fixed_iteration_digests(m, B, X0):
    """What the fixture records of one shape: the digest of x after ITERS iterations from x0 = 0 and from the guess X0."""
    rec = {"x0_zero": digest(fixed_iterations_from_zero(m, B)), "x0_guess": digest(fixed_iterations_from_guess(m, B, X0))}
    assert wg_fallbacks(m) == (0, 0), "a resident launch gave up: these are not the resident kernel's bits"
    return rec
