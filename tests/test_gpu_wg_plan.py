"""The resident CG launch plan on the device (csrc/cg_wg.hip: plan_wg, the launch table wg_kernels): a real handle plans what the device-free
probe elph_bench_wg_plan says for its bond table (tests/test_wg_plan.py holds the probe to the recorded rule), and the kernel the table
launches for that plan solves — one model per form at the smallest shape that selects it, at 1 and 9 right-hand sides, with the slices per
wave left to the rule and pinned (ELPH_WG_T) to every value the plan is usable with.  ELPH_WG_ALWAYS=1 keeps the cost rule from handing a
usable plan to the streaming iteration, so every variant runs the resident kernel; the solutions are held against the streaming iteration
at the bounds of test_gpu_parity.py::test_wg_resident_cg_equals_the_two_kernel_iteration."""
import pytest

from test_gpu_parity import _wg_info, _wg_resident_vs_streaming, _wg_status

pytestmark = pytest.mark.gpu

NRHS = (1, 9)
PINS = (None, 1, 2, 3, 4, 5, 8)
# model: (form, a configuration tag | (kind, orbitals, L, bonds, beta, dtau))
MODELS = {
    "e": ("LANE", "e"),                                            # SSH 4 x 4
    "b": ("GRID", "b"),                                            # 4 x 4
    "sq8_L20": ("S8", ("holstein", 1, 8, "sq", 2.0, 0.1)),         # config B's lattice
    "d": ("HGRID", "d"),                                           # 3 x 3 cells: one cell per lane
    "u": ("TGRID", "u"),                                           # triangular 4 x 4
    "sq16_L32": ("SQ16", ("holstein", 1, 16, "sq", 3.2, 0.1)),     # (the time axis of test_gpu_wg_sweep_order.py: T = 1, 2, 4 divide it)
    "ssh16_L32": ("SQ16", ("ssh", 1, 16, "sq", 1.6, 0.05)),
    "hc12_L12": ("HC12", ("holstein", 2, 12, "hc", 1.2, 0.1)),     # (T = 1, 2, 3 all divide it)
}


def _model(spec):
    """configs.make_model's model of a tag, or the same parameters on another lattice and time axis"""
    from elphdynamics_amd import configs, models, synth
    from elphdynamics_amd import lattice as lat
    if isinstance(spec, str):
        return configs.make_model(spec, tol=1e-5)
    kind, norb, L, bonds, beta, dtau = spec
    bonds = {"sq": lat.SQUARE_BONDS, "hc": lat.HONEYCOMB_BONDS}[bonds]
    if kind == "holstein":
        m = models.HolsteinModel(lat.Lattice(norb, L, L, 1), beta, dtau, tol=1e-5, maxiter=10000)
        for (o1, o2, d) in bonds:
            m.assign_t_(1.0, o1, o2, d)
        m.assign_omega_(1.0); m.assign_lambda_(1.0); m.assign_mu_(0.0)
        m.initialize_model_()
        m.x[:] = synth.phonon_field(m.Nph, m.Ltau, beta, dtau, omega=1.0, lam=1.0, seed=21)
    else:
        m = models.SSHModel(lat.Lattice(norb, L, L, 1), beta, dtau, tol=1e-5, maxiter=10000)
        for (o1, o2, d) in bonds:
            m.assign_hopping_(1.0, 0.1, 0.0, 0.1, o1, o2, d, name="xyz"[d.index(1)])
        m.initialize_model_()
        m.x[:] = 0.25 * synth.phonon_field(m.Nph, m.Ltau, beta, dtau, omega=0.1, lam=0.0, seed=21)      # (|alpha x| < t, as configs.make_model)
    models.update_model_(m)
    return m


def _probe(m, nrhs):
    from elphdynamics_amd import _lib
    hol = m.kind == 0
    return _lib.wg_plan(m.kind, m.Nsites, m.Ltau, m.neighbor_table, m.cosht if hol else None, m.sinht if hol else None, nrhs=nrhs)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_handle_plans_what_the_probe_says_and_the_planned_kernel_solves(name, monkeypatch):
    from elphdynamics_amd import _lib, configs
    form, spec = MODELS[name]
    m = _model(spec)
    try:
        for nrhs in NRHS:
            variants = []
            for pin in PINS:
                env = {"ELPH_WG_ALWAYS": "1", **({"ELPH_WG_T": str(pin)} if pin else {})}
                for k in ("ELPH_NO_WG", "ELPH_WG_T", "ELPH_WG_NO_DPP", "ELPH_WG_W"):
                    monkeypatch.delenv(k, raising=False)
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                plan = _probe(m, nrhs)
                info = _wg_info(m, nrhs)
                print(f"{name} nrhs={nrhs} ELPH_WG_T={pin}: probe {plan}, handle {info}")
                assert info == ((1, plan["T"], plan["W"], plan["G"]) if plan["usable"] else (0, 0, 0, 0)), (name, nrhs, pin)
                if plan["usable"]:
                    assert plan["form"] == _lib.WG_FORMS[form] and plan["has_kernel"] == 1 and plan["resident"] == 1, (name, nrhs, pin, plan)
                    variants.append(env)
            assert variants and "ELPH_WG_T" not in variants[0], (name, nrhs)      # the rule's own choice is among them
            _, B = configs.rhs(m, nrhs)
            before = _wg_status(m)
            _wg_resident_vs_streaming(m, B, variants, monkeypatch, name)
            assert _wg_status(m) == (0, before[1]), (name, nrhs)                  # no launch was given up, the handle is not cooling down
    finally:
        m.close()


def test_models_cover_every_form():
    from elphdynamics_amd import _lib
    assert {form for form, _ in MODELS.values()} == set(_lib.WG_FORMS)
