"""GPU parity of the Green's-function estimator (greens.hip) on the shapes tests/test_gpu_greens.py never uses: rectangular
and three-dimensional lattices, one to four orbitals, odd time axes, every form of the time-axis transforms setup! can reach, and
dynamic LDS beyond 64 KB up to the 160 KB refusal of elph_greens_create.

The estimator gets fixed random vectors through elph_greens_set_vectors (no solve, no solver tolerance to inherit) and is compared with
the FFT restatement oracle/greens.py — itself pinned to a direct sum on such shapes by tests/test_oracle_greens.py — at 1e-12 of the
largest element.  The imaginary parts must be exact zeros, the second half of the doubled time axis exactly -/+ the first, and the
device arrays (elph_greens_dev_arrays) the host copies bit for bit.  The estimator reads no bonds: bond-free handles suffice there.

setup! runs four time-axis transforms: forward twisted of 2 vectors and forward plain of 6 vectors over N columns, inverse twisted of
1 vector and inverse plain of 3 vectors over ns*N columns.  On the 3 x 2 honeycomb cells of the time-axis cases (N = 12, ns*N = 24)
the switches select the forms of TIME_AXES below (elph_plan_dft, dft_mfma.hip), which the test asserts of the handle's own plan and of the
device-free probe before it compares numbers: an odd L has no even/odd split; there are no direct matrix-core tables beyond 256 slices; the
split at L = 320 stages a 100 KB W panel; 480, 1000 and 1280 slices split as 20 x 24, 25 x 40 and 32 x 40; 409 is a prime and 422 = 2 x 211
has no divisor >= 4 (scalar tables beyond 400 slices); 1031 is a prime beyond 1024.
No switch reaches the scalar kernels with the twisted pair at L <= 256: ELPH_DFT_MFMA=0 leaves the one-tile form, which the planner
chooses without reading a switch.  ELPH_DFT_R2=1 alone at L = 320 keeps the scalar kernels on a lattice this small (the split starts at
100 column-tile waves), hence ELPH_DFT_MFMA=1 with it.

End to end (update_ on the device's own solve to 1e-13, with and without the KPM preconditioner): rectangular honeycomb, a chain and two
cubic lattices, M^-1 R against the oracle's solve within the README's 1e-10, the tables within 1e-12 on the device's vectors; the cubic
handles — the first three-dimensional ones in the suite — also through the mat-vecs.  4 x 4 x 4 has 3N bonds in 6 colours, the counts of
an 8 x 8 triangular lattice (tests/test_lattice_shape.py: recognised as no special lattice)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _oracle_model, rel

pytestmark = pytest.mark.gpu

NAMES = ["GD0", "GD0_GD0", "GDD_G00", "GD0_G0D"]
SWITCHES = ("ELPH_DFT_MFMA", "ELPH_DFT_R2", "ELPH_DFT_BIG_BLOCKED")
CUBIC_BONDS = [(1, 1, (1, 0, 0)), (1, 1, (0, 1, 0)), (1, 1, (0, 0, 1))]
CHAIN_BONDS = [(1, 1, (1, 0, 0))]


def lds_bytes(ns, L1, L2, L3):
    """Dynamic LDS of k_gr_spatial: three buffers of N complex numbers and two of one per cell."""
    nc = L1 * L2 * L3
    return (3 * ns * nc + 2 * nc) * 16


def bondfree_model(ns, L1, L2, L3, L):
    from elphdynamics_amd import lattice as lat, models
    m = models.HolsteinModel(lat.Lattice(ns, L1, L2, L3), L * 0.1, 0.1)
    assert m.Ltau == L
    m.initialize_model_()
    return m


def check_tables(est, orc, n1, n2):
    """setup! of the pair (n1, n2) on the device against the oracle, plus the exact properties of the device's tables."""
    from elphdynamics_amd import _lib, greens
    greens.setup_(est, n1, n2)
    orc.setup(n1, n2)
    L = est.L
    for nm in NAMES:
        got, ref = getattr(est, nm), getattr(orc, nm)
        assert not got.imag.any(), nm
        assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max(), (nm, n1, n2)
    assert np.array_equal(est.GD0[L:], -est.GD0[:L])
    for nm in NAMES[1:]:
        assert np.array_equal(getattr(est, nm)[L:], getattr(est, nm)[:L]), nm
    m = est.model
    arrs, cnt = (C.c_void_p * 4)(), C.c_int64()
    _lib.check(m._lib.elph_greens_dev_arrays(m._h, arrs, C.byref(cnt)))
    assert cnt.value == est.GD0.size
    hip = C.CDLL("libamdhip64.so")
    for k, nm in enumerate(NAMES):
        out = np.empty(2 * cnt.value)
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(arrs[k]), C.c_size_t(16 * cnt.value), 2) == 0
        assert np.array_equal(out, getattr(est, nm).reshape(-1, order="F").view(np.float64)), nm


def parity_on_fixed_vectors(ns, L1, L2, L3, L, seed, forms=None):
    from elphdynamics_amd import _lib, greens
    from oracle.greens import EstimateGreensFunction as OracleEst
    m = bondfree_model(ns, L1, L2, L3, L)
    try:
        if forms:      # setup!'s four transforms: (kind, direction, columns, vectors) and the form each is planned in
            N = m.Nsites
            for (which, inv, ncol, nvec), form in zip(((0, 0, N, 2), (1, 0, N, 6), (0, 1, ns * N, 1), (1, 1, ns * N, 3)), forms):
                plan = _lib.dft_plan(L, which, inv, ncol, nvec, handle=m._h)
                assert plan == _lib.dft_plan(L, which, inv, ncol, nvec), (which, inv)
                assert plan["form"] == _lib.DFT_FORMS[form] and not plan["short_slots"], (which, inv, plan)
        est = greens.EstimateGreensFunction(m, nv=3)
        assert est.GD0.shape == (2 * L, ns, ns, L1, L2, L3)
        rng = np.random.default_rng(seed)
        R, X = rng.standard_normal((3, m.Ndim)), rng.standard_normal((3, m.Ndim))
        greens.set_vectors_(est, R, X)
        orc = OracleEst(L, ns, L1, L2, L3, nv=3)
        orc.R[:], orc.MinvR[:] = R, X
        for (n1, n2) in [(1, 2), (3, 1)]:
            check_tables(est, orc, n1, n2)
    finally:
        m.close()


# (norbits, L1, L2, L3, L)
CELL_SHAPES = {
    "sq12x6": (1, 12, 6, 1, 8),
    "hc6x4": (2, 6, 4, 1, 7),
    "cubic4x4x2": (1, 4, 4, 2, 6),
    "cubic3x2x2": (1, 3, 2, 2, 5),
    "chain16": (1, 16, 1, 1, 9),
    "orb3_2x3": (3, 2, 3, 1, 5),
    "orb4_1cell": (4, 1, 1, 1, 10),
    "sq30x30": (1, 30, 30, 1, 4),         # 72,000 B of LDS: past the 64 KB default
    "hc24x24": (2, 24, 24, 1, 3),         # 73,728 B
    "sq45x45": (1, 45, 45, 1, 4),         # 162,000 B: the largest accepted one-orbital lattice
}


@pytest.mark.parametrize("case", list(CELL_SHAPES))
def test_setup_matches_oracle_across_cell_shapes(case):
    """Cell axes of different lengths (a stride or twiddle offset of the wrong axis shows), a third cell axis, a single axis, one cell
    (no spatial transform at all), up to four orbitals interleaved in the output index, and LDS beyond 64 KB."""
    ns, L1, L2, L3, L = CELL_SHAPES[case]
    if case in ("sq30x30", "hc24x24", "sq45x45"):
        assert 64 * 1024 < lds_bytes(ns, L1, L2, L3) <= 160 * 1024
    parity_on_fixed_vectors(ns, L1, L2, L3, L, seed=sum(CELL_SHAPES[case]))


# (L, switches, (form of the twisted pair, form of the plain pair)): _lib.DFT_FORMS
TIME_AXES = [
    (7, {"ELPH_DFT_MFMA": "0"}, ("ONE_TILE", "SCALAR")), (7, {"ELPH_DFT_MFMA": "1"}, ("DIRECT", "DIRECT")),
    (45, {"ELPH_DFT_MFMA": "0"}, ("ONE_TILE", "SCALAR")), (45, {"ELPH_DFT_MFMA": "1"}, ("DIRECT", "DIRECT")),
    (160, {"ELPH_DFT_MFMA": "0"}, ("ONE_TILE", "SCALAR")), (160, {"ELPH_DFT_MFMA": "1"}, ("SPLIT_LDS", "DIRECT")),
    (160, {"ELPH_DFT_MFMA": "1", "ELPH_DFT_R2": "0"}, ("DIRECT", "DIRECT")),
    (320, {"ELPH_DFT_R2": "0"}, ("SCALAR", "SCALAR")), (320, {"ELPH_DFT_R2": "1", "ELPH_DFT_MFMA": "1"}, ("SPLIT_LDS", "SCALAR")),
    (480, {"ELPH_DFT_BIG_BLOCKED": "0"}, ("BIG_ROW", "BIG_ROW")), (480, {"ELPH_DFT_BIG_BLOCKED": "1"}, ("BIG_BLOCKED", "BIG_BLOCKED")),
    (1000, {"ELPH_DFT_BIG_BLOCKED": "0"}, ("BIG_ROW", "BIG_ROW")), (1000, {"ELPH_DFT_BIG_BLOCKED": "1"}, ("BIG_BLOCKED", "BIG_BLOCKED")),
    (409, {}, ("SCALAR", "SCALAR")), (422, {}, ("SCALAR", "SCALAR")), (1031, {}, ("BIG_DIRECT", "BIG_DIRECT")),
    (1280, {"ELPH_DFT_BIG_BLOCKED": "0"}, ("BIG_ROW", "BIG_ROW")), (1280, {"ELPH_DFT_BIG_BLOCKED": "1"}, ("BIG_BLOCKED", "BIG_BLOCKED")),
]


# every form but the register-resident split, which no time axis reaches (tests/test_dft_plan.py)
_FORMS_REACHABLE = ("SCALAR", "ONE_TILE", "DIRECT", "SPLIT_LDS", "BIG_ROW", "BIG_BLOCKED", "BIG_DIRECT")


def _time_id(case):
    L, env, _ = case
    return "L%d" % L + "".join("-%s%s" % (k[len("ELPH_DFT_"):], v) for k, v in sorted(env.items()))


@pytest.mark.parametrize("L,env,forms", TIME_AXES, ids=[_time_id(c) for c in TIME_AXES])
def test_setup_matches_oracle_across_time_axes(L, env, forms, monkeypatch):
    """Odd and even time axes through every transform form the planner can choose for setup!'s four calls (module docstring), on 3 x 2
    honeycomb cells (rectangular, two orbitals: 24 columns for the inverse transforms): the handle plans the listed form, as the
    device-free probe does, and the tables match the oracle."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    twisted, plain = forms
    assert {f for _, _, fs in TIME_AXES for f in fs} == set(_FORMS_REACHABLE)
    parity_on_fixed_vectors(2, 3, 2, 1, L, seed=L, forms=(twisted, plain, twisted, plain))


@pytest.mark.parametrize("ns,L1,L2,nbytes", [(1, 46, 46, 169280), (2, 36, 36, 165888)])
def test_lds_refusal_leaves_the_handle_usable(oracle, ns, L1, L2, nbytes):
    """A frequency slice beyond 160 KB of LDS: elph_greens_create refuses with ELPH_E_UNSUPPORTED and a message, keeps no estimator,
    and the handle still computes its mat-vecs."""
    from elphdynamics_amd import _lib, greens, models, synth
    assert lds_bytes(ns, L1, L2, 1) == nbytes > 160 * 1024
    m = bondfree_model(ns, L1, L2, 1, 4)
    try:
        lib = m._lib
        assert lib.elph_greens_create(m._h, ns, L1, L2, 1, 2) == _lib.ELPH_E_UNSUPPORTED
        msg = lib.elph_last_error().decode()
        assert "160 KB" in msg and str(m.Nsites) in msg, msg
        assert lib.elph_greens_setup(m._h, 1, 2, None, None, None, None) == _lib.ELPH_E_STATE
        with pytest.raises(_lib.ElphError):
            greens.EstimateGreensFunction(m, 2)
        m.lam[:], m.mu[:] = 1.0, 0.1
        m.x[:] = synth.phonon_field(m.Nph, m.Ltau, m.beta, m.dtau, seed=46)
        models.update_model_(m)
        om = _oracle_model(oracle, m)
        v = synth.randn(5, m.Ndim)
        y = np.zeros(m.Ndim)
        models.mulM_(y, m, v)
        assert rel(y, oracle.mulM(om, v)) < 1e-13
    finally:
        m.close()


# (norbits, L1, L2, L3, bonds, beta); the rectangular honeycomb is configuration w
E2E = {
    "w": None,
    "chain12": (1, 12, 1, 1, CHAIN_BONDS, 1.1),
    "cubic4x4x2": (1, 4, 4, 2, CUBIC_BONDS, 0.9),
    "cubic4x4x4": (1, 4, 4, 4, CUBIC_BONDS, 1.0),
}


def e2e_model(tag):
    from elphdynamics_amd import configs, lattice as lat, models, synth
    if E2E[tag] is None:
        return configs.make_model(tag, tol=1e-13, maxiter=20000)
    ns, L1, L2, L3, bonds, beta = E2E[tag]
    dtau = 0.1
    m = models.HolsteinModel(lat.Lattice(ns, L1, L2, L3), beta, dtau, tol=1e-13, maxiter=20000)
    for (o1, o2, d) in bonds:
        m.assign_t_(1.0, o1, o2, d)
    m.assign_omega_(1.0); m.assign_lambda_(1.0); m.assign_mu_(0.0)
    m.initialize_model_()
    m.x[:] = synth.phonon_field(m.Nph, m.Ltau, beta, dtau, seed=4343)
    models.update_model_(m)
    return m


@pytest.mark.parametrize("kpm", [False, True], ids=["plain", "kpm"])
@pytest.mark.parametrize("tag", list(E2E))
def test_update_and_setup_end_to_end(oracle, tag, kpm):
    """update_ (batched solve of n_v = 3 vectors to 1e-13) then setup! on new geometries: M^-1 R against the oracle's solve, the tables
    against oracle/greens.py on the device's own vectors."""
    from elphdynamics_amd import greens, models, preconditioners as pc, synth
    from oracle.greens import EstimateGreensFunction as OracleEst
    m = e2e_model(tag)
    try:
        la = m.lattice
        if tag == "cubic4x4x4":
            assert m.Nbonds == 3 * m.Nsites and int(m.colours.max()) == 6
        om = _oracle_model(oracle, m)
        if tag.startswith("cubic") and not kpm:
            v = synth.randn(77, m.Ndim)
            y = np.empty(m.Ndim)
            for fn, ofn in ((models.mulM_, oracle.mulM), (models.mulMt_, oracle.mulMT), (models.mulMtM_, oracle.mulMTM)):
                fn(y, m, v)
                assert rel(y, ofn(om, v)) < 1e-13
        est = greens.EstimateGreensFunction(m, nv=3)
        R = np.stack([synth.randn(3100 + i, m.Ndim) for i in range(3)])
        P = pc.SymmetricKPMPreconditioner(m, n=min(20, m.Nsites), buf=0.05, c1=1.0, c2=1.0) if kpm else None
        it, res, fl = greens.update_(est, m, P, rng=np.random.default_rng(2), R=R)
        assert not fl.any()
        if kpm:
            assert P.active
        for i in range(3):
            xo, ito, reso, flo = oracle.ldiv(om, oracle.mulMT(om, np.ascontiguousarray(R[i])), solver_tol=1e-13, solver_maxiter=20000)
            assert flo == 0
            assert np.abs(est.MinvR[i] - xo).max() < 1e-10 * np.abs(xo).max(), i
        orc = OracleEst(m.Ltau, la.norbits, la.L1, la.L2, la.L3, nv=3)
        orc.R[:], orc.MinvR[:] = est.R, est.MinvR
        for (n1, n2) in [(1, 2), (3, 1)]:
            check_tables(est, orc, n1, n2)
    finally:
        m.close()
