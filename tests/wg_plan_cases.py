"""The cases of the resident CG launch plan (csrc/cg_wg.hip: WgPlan) that tests/test_wg_plan.py checks through the device-free probe
elph_bench_wg_plan, and how one of them is probed.  A case is a bond table, a time axis and — for one rank of a sharded solve — the number
of ranks; every case is crossed with the batch sizes NRHS and the settings KNOBS of the ELPH_*WG* switches."""
import conftest  # noqa: F401  (the repository root on sys.path)
from elphdynamics_amd import _lib, configs
from elphdynamics_amd import lattice as lat
from test_lattice_shape import bonds_key, tables

SWITCHES = ("ELPH_NO_WG", "ELPH_WG_NO_DPP", "ELPH_WG_ALWAYS", "ELPH_WG_T", "ELPH_WG_W")
NRHS = (1, 2, 8, 9, 24, 25, 48, 49, 64, 65, 72, 73, 256, 288)
KNOBS = {
    "none": {},
    **{f"T{t}": {"ELPH_WG_T": str(t)} for t in (1, 2, 3, 4, 5, 8)},
    "no_dpp": {"ELPH_WG_NO_DPP": "1"},
    "no_dpp_T2": {"ELPH_WG_NO_DPP": "1", "ELPH_WG_T": "2"},
    "no_wg": {"ELPH_NO_WG": "1"},
    "always": {"ELPH_WG_ALWAYS": "1"},
    "W2": {"ELPH_WG_W": "2"},
}
# the slots of a recorded row: _lib.WG_PLAN_SLOTS without has_kernel (which the rule the table was recorded from did not have)
ROW_SLOTS = _lib.WG_PLAN_SLOTS[:-1]

# case: (kind, orbitals, Lspatial, bonds, dtau, t_stddev, Ltau, world)
CASES = {tag: (k, norb, Ls, bonds_key(b), dtau, 0.0, lat.ltau_from_beta(beta, dtau), 0)
         for tag, (k, norb, Ls, b, beta, dtau) in configs.CONFIGS.items()}
for ltau in (12, 20, 30, 32, 40, 50):
    CASES[f"sq16_L{ltau}"] = ("holstein", 1, 16, "sq", 0.1, 0.0, ltau, 0)
    CASES[f"ssh16_L{ltau}"] = ("ssh", 1, 16, "sq", 0.05, 0.0, ltau, 0)
    CASES[f"hc12_L{ltau}"] = ("holstein", 2, 12, "hc", 0.1, 0.0, ltau, 0)
for tag in ("b", "s", "C", "D"):      # hopping disorder: per-bond tables instead of one (cosh, sinh)
    CASES[f"disorder_{tag}"] = CASES[tag][:5] + (0.1,) + CASES[tag][6:]
# periodic rectangles of the shapes a sharded solve's ring-closed slabs take, as one rank of 2, 4 or 8 (time axis of configs q, Q, z)
RINGS = [("sq", 1, ab) for ab in ((16, 4), (16, 6), (16, 8), (16, 10), (32, 4))] + [("hc", 2, ab) for ab in ((12, 2), (12, 4), (12, 6), (16, 4))]
for bk, norb, (a, b) in RINGS:
    for world in (2, 4, 8):
        CASES[f"ring_{bk}{a}x{b}_w{world}"] = ("holstein", norb, (a, b), bk, 0.1, 0.0, 40, world)


def probe(case, nrhs):
    """The plan of `case` for nrhs right-hand sides under the switches now in the environment, as {slot: value} (_lib.WG_PLAN_SLOTS)."""
    kind, norb, Ls, bkey, dtau, t_stddev, ltau, world = CASES[case]
    n, tab, c, s = tables(kind, norb, Ls, bkey, dtau, t_stddev)
    return _lib.wg_plan(0 if kind == "holstein" else 1, n, ltau, tab, c, s, nrhs=nrhs, world=world)
