"""GPU (-m gpu): hopping disorder that depends on the bond's direction (assign_t! with a standard deviation, HolsteinModels.jl:427-447;
one generator across the bond definitions: tests/test_hopping_disorder_inputs.py) on every Holstein kernel form with a second
instantiation for it — per-site (cosh, sinh) registers, tables in LDS, UNI = false.

All models: Holstein, t_stddev = 0.1, from configs.make_model; "hc12s" is the honeycomb lattice of 12 x 12 cells at beta = 2.4 (N = 288:
five sites per lane, 24 time slices), built directly.  The assertion bodies and their bounds are those of tests/test_gpu_parity.py
(mat-vecs 1e-13 and adjointness; equal iteration counts up to the knife edge, eps history 1e-10, tight solve 1e-10; KPM apply 1e-11),
of tests/test_gpu_hmc.py and of tests/test_gpu_muldmdx.py, taken as helpers — nothing is restated here.

  B1  mat-vec family + plain CG vs the oracle: the lane programs with 1 ... 5 sites per lane on four colours (s, q, Q, r, R; d, y, w, z,
      W, hc12s), the six-colour lane program (u, t6, t12) and the ragged generic kernels (t).
  B2  KPM apply + preconditioned CG on the oracle's bounds: the recursion of the squares and honeycombs leaves the register forms under
      disorder (elph_reg_cheb_form: REG_NONE) for k_kpm_cheb_ri; the p/x-fused batch around it on q and y; never fused on u.
  B3  every Holstein UNI = false lane-program instantiation of the resident kernel k_cg_wg (cg_wg.hip: launch_npl) once.
  B4  the fermion force inside an HMC update, and muldMdx.
"""
import numpy as np
import pytest

from kpm_bounds_reference import host_model
from test_gpu_hmc import check_hmc_update_vs_oracle
from test_gpu_muldmdx import check_muldMdx_holstein_vs_oracle
from test_gpu_parity import (_oracle_model, _px_fused, _wg_info, _wg_resident_vs_streaming, _wg_status, check_cg_vs_oracle,
                             check_kpm_with_injected_bounds_vs_oracle, check_matvec_vs_oracle, rel)

pytestmark = pytest.mark.gpu

STD = 0.1


def disordered(tag, tol=1e-5):
    from elphdynamics_amd import configs, lattice as lat, models, synth
    if tag != "hc12s":
        return configs.make_model(tag, tol=tol, t_stddev=STD)
    beta, dtau = 2.4, 0.1
    m = models.HolsteinModel(lat.Lattice(2, 12, 12, 1), beta, dtau, tol=tol, maxiter=10000)
    rng = np.random.default_rng(synth.SEED_FIELDS + 991)
    for (o1, o2, d) in lat.HONEYCOMB_BONDS:
        m.assign_t_(1.0, o1, o2, d, stddev=STD, rng=rng)
    m.assign_omega_(1.0); m.assign_lambda_(1.0); m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, beta, dtau, omega=1.0, lam=1.0, seed=synth.SEED_FIELDS)
    models.update_model_(m)
    assert m.Nsites == 288 and m.Ltau == 24
    return m


def test_make_model_draws_what_the_host_restatement_draws():
    """The CPU power check runs on kpm_bounds_reference.host_model: the device models must carry the same hoppings, direction by direction."""
    for tag in ("d", "u", "s"):
        m, hm = disordered(tag), host_model(tag, STD)
        assert np.array_equal(m.t, hm.t) and np.array_equal(m.cosht, hm.cosht) and np.array_equal(m.neighbor_table, hm.neighbor_table)
        n = len(m.t) // len(m.bond_definitions)
        assert not np.array_equal(m.t[:n], m.t[n:2 * n])
        m.close()


# ------------------------------------------------------------------------------------------ B1: mat-vecs and plain CG

B1_TAGS = ["s", "q", "Q", "r", "R", "d", "y", "w", "z", "W", "hc12s", "u", "t6", "t12", "t"]


@pytest.mark.parametrize("tag", B1_TAGS)
def test_matvec_with_hopping_disorder_vs_oracle(oracle, tag):
    m = disordered(tag)
    check_matvec_vs_oracle(oracle, m)
    m.close()


@pytest.mark.parametrize("tag", B1_TAGS)
def test_cg_with_hopping_disorder_vs_oracle(oracle, tag):
    m = disordered(tag)
    check_cg_vs_oracle(oracle, m)
    m.close()


# ------------------------------------------------------------------------------------------ B2: KPM apply and preconditioned CG

@pytest.mark.parametrize("tag", ["q", "r", "y", "W", "u", "t12", "t", "hc12s"])
def test_kpm_with_hopping_disorder_vs_oracle_small_lattices(oracle, tag):
    m = disordered(tag)
    check_kpm_with_injected_bounds_vs_oracle(oracle, m)
    m.close()


def _chains_batch(m, nchains, per, seed):
    from elphdynamics_amd import models, preconditioners as pc, synth
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=seed + c) for c in range(nchains)])
    models.update_model_chains_(m, X)
    P = pc.SymmetricKPMPreconditioner(m, 20, 0.05, 1.0, 1.0)
    pc.setup_chains_(P, rng=np.random.default_rng(16))
    B = np.stack([synth.randn(seed + 100 + r, m.Ndim) for r in range(nchains * per)])
    return X, P, B


@pytest.mark.parametrize("tag", ["q", "y"])
def test_px_fused_batch_with_hopping_disorder(oracle, tag, monkeypatch):
    """8 chains x 2 right-hand sides on a disordered 10 x 10 square / 6 x 6-cell honeycomb lattice: the p/x-fused iteration around the
    Re / Im recursion through the LDS slab (k_kpm_cheb_ri) against the unfused form (ELPH_LDS_CHEB_PX=0) with the bounds of
    test_px_fused_iteration_generic_family — iteration counts within one, two tol = 1e-8 solves to 1e-9, the fused form asserted taken —
    and two right-hand sides (chains 0 and 3) against the oracle's tight solve to 1e-6.  The library's own rules keep so small a batch
    on the unfused iteration (elph_choose_T_px: fewer than 1024 waves; elph_plan_dft: fewer than 448 column-tile waves): the chunk
    length and the matrix-core transforms are pinned, as test_px_fused_preconditioned_iteration_equals_the_unfused_one pins its small batches."""
    from elphdynamics_amd import models
    nchains, per = 8, 2
    monkeypatch.setenv("ELPH_CHUNK_T", "4")         # (read when the handle is created)
    monkeypatch.setenv("ELPH_DFT_MFMA", "1")
    m = disordered(tag, tol=1e-8)
    X, P, B = _chains_batch(m, nchains, per, 9300)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ELPH_LDS_CHEB_PX", mode)
        Xs = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
        assert not fl.any()
        out[mode] = (Xs, it, _px_fused(m))
    assert out["0"][2] is False and out["1"][2] is True, (out["0"][2], out["1"][2])
    assert np.abs(out["0"][1] - out["1"][1]).max() <= 1
    assert rel(out["1"][0], out["0"][0]) < 1e-9
    for r in (0, nchains + 3):                      # right-hand side r runs on the field of chain r % nchains
        m.x[:] = X[r % nchains]
        om = _oracle_model(oracle, m)
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(B[r]), solver_tol=1e-12, solver_maxiter=20000)
        assert flo == 0 and rel(out["1"][0][r], xo) < 1e-6, r
    m.close()


def test_px_fused_form_declines_hopping_disorder_on_six_colours(oracle, monkeypatch):
    """The six-colour lane programs take the patch-form pair for their fused iteration, which needs one (cosh, sinh) for every bond
    (elph_plan_cg: hop_uniform): a disordered u runs the unfused iteration — and solves the right systems — where the uniform u, same
    batch and same switches, runs the fused one (so the disorder is what declines)."""
    from elphdynamics_amd import configs, models
    nchains, per = 8, 2
    monkeypatch.setenv("ELPH_DFT_MFMA", "1")
    m = configs.make_model("u", tol=1e-8)
    X, P, B = _chains_batch(m, nchains, per, 9500)
    Xs = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
    assert not fl.any() and _px_fused(m) is True
    m.close()
    m = disordered("u", tol=1e-8)
    X, P, B = _chains_batch(m, nchains, per, 9500)
    Xs = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(Xs, m, B, P=P)
    assert not fl.any() and _px_fused(m) is False
    for r in (0, nchains + 3):
        m.x[:] = X[r % nchains]
        om = _oracle_model(oracle, m)
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(B[r]), solver_tol=1e-12, solver_maxiter=20000)
        assert flo == 0 and rel(Xs[r], xo) < 1e-6, r
    m.close()


# ------------------------------------------------------------------------------------------ B3: the resident kernel's lane-program forms

# (tag, slices per wave): k_cg_wg<sites per lane, T, false, UNI = false, FORM 0>
WG_CASES = [("s", 1), ("s", 2), ("s", 4), ("s", 5), ("B", 8),      # 1 site per lane
            ("y", 1), ("y", 2), ("r", 1),                          # 2
            ("W", 1), ("W", 2),                                    # 3
            ("Q", 1), ("z", 1),                                    # 4
            ("hc12s", 1)]                                          # 5
SITES_PER_LANE = {"s": 1, "B": 1, "y": 2, "r": 2, "W": 3, "Q": 4, "z": 4, "hc12s": 5}


@pytest.mark.parametrize("tag,T", WG_CASES)
def test_wg_resident_cg_lane_program_forms_with_hopping_disorder(oracle, tag, T, monkeypatch):
    """One disordered instantiation of the resident kernel per case, asserted usable with the pinned slices per wave before the solve
    and not timed out after it: against the streaming iteration (the bounds of _wg_resident_vs_streaming) and, solved to 1e-13, against
    the oracle's solve to 1e-10."""
    from elphdynamics_amd import configs, models
    monkeypatch.setenv("ELPH_WG_ALWAYS", "1")
    monkeypatch.setenv("ELPH_WG_T", str(T))
    m = disordered(tag)
    assert -(-m.Nsites // 64) == SITES_PER_LANE[tag]
    R, B = configs.rhs(m, 3)
    usable, Tw, W, G = _wg_info(m, 3)
    assert usable == 1 and Tw == T, (tag, usable, Tw, W, G)
    _wg_resident_vs_streaming(m, B, [{"ELPH_WG_T": str(T)}], monkeypatch, tag)
    assert _wg_status(m) == (0, 0)
    # (the helper leaves ELPH_WG_T at T and the solver tolerance at 1e-13)
    usable, Tw, W, G = _wg_info(m, 3)
    assert usable == 1 and Tw == T and m.solver.tol == 1e-13
    X = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(X, m, B)
    assert not fl.any() and _wg_status(m) == (0, 0)
    om = _oracle_model(oracle, m)
    for i in range(3):
        xo, ito, reso, flo = oracle.ldiv(om, np.ascontiguousarray(B[i]), solver_tol=1e-13, solver_maxiter=10000)
        assert flo == 0 and rel(X[i], xo) < 1e-10, (tag, T, i, rel(X[i], xo))
    m.close()


@pytest.mark.parametrize("tag", ["B", "Q", "y", "hc12s"])
def test_wg_resident_cg_register_exchange_forms_decline_hopping_disorder(tag, monkeypatch):
    """The 8 x 8, GRID, HGRID and honeycomb DPP forms carry one (cosh, sinh) for the lattice (s8_form, gr_form, hg_form, hc_form: m.uniform):
    on a disordered model the lane-program form runs whether they are switched off (ELPH_WG_NO_DPP=1) or not — the same bits."""
    from elphdynamics_amd import configs, models
    monkeypatch.setenv("ELPH_WG_ALWAYS", "1")
    m = disordered(tag)
    R, B = configs.rhs(m, 3)
    out = []
    for no_dpp in ("0", "1"):
        monkeypatch.setenv("ELPH_WG_NO_DPP", no_dpp)
        info = _wg_info(m, 3)
        assert info[0] == 1, (tag, no_dpp, info)
        X = np.zeros_like(B)
        it, res, fl = models.ldiv_batched_(X, m, B)
        assert not fl.any() and _wg_status(m) == (0, 0)
        out.append((X, it, info))
    assert out[0][2] == out[1][2]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0])
    m.close()


def test_wg_resident_cg_shapes_refused_under_hopping_disorder(monkeypatch):
    """Four sites per lane with per-site hopping: never 2 slices per wave (pick_shape); six colours: no resident form at all (tg_form)."""
    monkeypatch.setenv("ELPH_WG_ALWAYS", "1")
    monkeypatch.setenv("ELPH_WG_T", "2")
    m = disordered("Q")
    usable, T, W, G = _wg_info(m, 3)
    assert not (usable == 1 and T == 2), (usable, T, W, G)
    m.close()
    monkeypatch.delenv("ELPH_WG_T")
    m = disordered("u")
    assert _wg_info(m, 1)[0] == 0 and _wg_info(m, 3)[0] == 0
    m.close()


def test_wg_resident_cg_chains_with_hopping_disorder(monkeypatch):
    """4 fields x 2 right-hand sides on the disordered 8 x 8 lattice in one resident launch (right-hand side r on the field of chain
    r % 4): every solution equals the single-configuration solve of that field bit for bit."""
    from elphdynamics_amd import models, synth
    monkeypatch.setenv("ELPH_WG_ALWAYS", "1")
    nchains, per = 4, 2
    nrhs = nchains * per
    m = disordered("B")
    X = np.stack([synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=5300 + c) for c in range(nchains)])
    B = np.stack([synth.randn(7300 + r, m.Ndim) for r in range(nrhs)])
    models.update_model_chains_(m, X)
    info = _wg_info(m, nrhs)
    assert info[0] == 1
    monkeypatch.setenv("ELPH_WG_T", str(info[1]))      # (the same slices per wave for the batch and the single solves: the same summation trees)
    Xs = np.zeros_like(B)
    it, res, fl = models.ldiv_batched_(Xs, m, B)
    assert not fl.any() and _wg_status(m) == (0, 0)
    for r in range(nrhs):
        m1 = disordered("B")
        m1.x[:] = X[r % nchains]
        models.update_model_(m1)
        assert _wg_info(m1, 1)[:2] == (1, info[1])
        x1 = np.zeros(m.Ndim)
        it1, res1, fl1 = models.ldiv_(x1, m1, np.ascontiguousarray(B[r]))
        assert fl1 == 0 and it1 == it[r] and np.array_equal(x1, Xs[r]), (r, it1, int(it[r]), rel(x1, Xs[r]))
        assert _wg_status(m1) == (0, 0)
        m1.close()
    m.close()


# ------------------------------------------------------------------------------------------ B4: force and HMC

@pytest.mark.parametrize("tag,nb,nt", [("b", 1, 4), ("d", 1, 4)])
def test_hmc_update_with_hopping_disorder_vs_oracle(oracle, tag, nb, nt):
    check_hmc_update_vs_oracle(oracle, tag, nb, nt, t_stddev=STD)


def test_muldMdx_with_hopping_disorder_vs_oracle(oracle):
    check_muldMdx_holstein_vs_oracle(oracle, "b", t_stddev=STD)
