"""CPU test of the tau-axis transform plan (csrc/dft_mfma.hip: dft_shape, dft_switches, elph_plan_dft, elph_dft_pair) through the
device-free probe elph_bench_dft_plan.  tests/golden/dft_plan.json holds, for every case of dft_plan_cases.py, the plan of the rule this
planner replaced: the seven predicates (elph_dft_big, elph_dft_mfma_usable, elph_dft_mfma1_usable, the three *_usable of the fused
iteration, blocked_form), the cascades of the five entry points of dft.hip and the second layer in elph_dft_mfma_fwd / _inv, walked on a
host-only handle filled by the arithmetic of the two table builders — recorded before they were folded into the planner.

The even/odd split with its data in registers (SPLIT_REG) is in no row: the largest split table has 50 reduction tiles, a W panel of
5 * 50 * 64 * 8 = 128,000 bytes, under the 144 KB from which the recorded rule leaves the streaming form.  The table therefore reaches
seven of the eight forms and one side of that limit; test_the_panel_limit_is_never_reached holds exactly that."""
import json
import os

import pytest

from conftest import ROOT
from elphdynamics_amd import _lib
import dft_plan_cases as dc

with open(os.path.join(ROOT, "tests", "golden", "dft_plan.json")) as _f:
    TABLE = json.load(_f)
F = _lib.DFT_FORMS
LDS_LIMIT = 160 * 1024
PANEL_LIMIT = 144 * 1024


def recorded(L=None, knob=None):
    """(L, knob, which, inverse, nrz, N, nvec, {slot: value}) of every recorded plan (of one time axis / setting)."""
    for l in ([L] if L else dc.LTAU):
        for kn in ([knob] if knob else dc.KNOBS):
            for (w, d, z, n), line in zip(dc.cases(l, kn), TABLE["plans"][str(l)][kn]):
                for nv, i in zip(dc.NVEC, TABLE["lines"][line]):
                    yield l, kn, w, d, z, n, nv, dict(zip(TABLE["slots"], TABLE["rows"][i]))


def test_table_is_the_table_of_these_cases():
    assert tuple(TABLE["slots"]) == _lib.DFT_PLAN_SLOTS
    assert (tuple(TABLE["ltau"]), tuple(TABLE["ncol"]), tuple(TABLE["nvec"]), tuple(TABLE["nrz"])) == (dc.LTAU, dc.NCOL, dc.NVEC, dc.NRZ)
    assert sorted(TABLE["plans"]) == sorted(str(l) for l in dc.LTAU)
    for l in dc.LTAU:
        assert sorted(TABLE["plans"][str(l)]) == sorted(dc.KNOBS)
        assert all(len(ids) == len(dc.cases(l, kn)) for kn, ids in TABLE["plans"][str(l)].items())
    assert all(len(line) == len(dc.NVEC) for line in TABLE["lines"])
    assert set(dc.SWITCHES) == {k for kn in dc.KNOBS.values() for k in kn}


def test_cases_reach_the_forms_both_values_of_every_capability_and_the_error_rows():
    rows = [v for *_, v in recorded()]
    assert {v["form"] for v in rows} == set(F.values()) - {F["SPLIT_REG"]}
    assert {v["pair_form"] for v in rows} == set(F.values()) - {F["SPLIT_REG"]}
    for cap in ("xr", "px", "fold"):
        assert {v[cap] for v in rows} == {0, 1}, cap
    assert {v["form"] for v in rows if v["short_slots"]} == {F["DIRECT"], F["SPLIT_LDS"]}      # (long axes: test_long_axis_slot_rules)
    # a plain pair whose two directions disagree falls to the scalar tables as a pair
    assert any(v["form"] == F["DIRECT"] and v["pair_form"] == F["SCALAR"] for v in rows)


def test_long_axis_slot_rules(monkeypatch):
    """The slot counts of the table (0, L, L ceil(N/64)) never offer a long axis fewer than L: the rule as dft_big.hip stated it — fewer
    than L slots is an error in either form, from L to below L ceil(N/64) the blocked pair falls to one row per wave."""
    for name in dc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("ELPH_DFT_BIG_BLOCKED", "1")
    for L, row in ((1000, "BIG_ROW"), (1031, "BIG_DIRECT")):
        nst = (256 + 63) // 64
        for nrz, form, slots, short in ((L - 1, row, L, 1), (L, row, L, 0), (L * nst - 1, row, L, 0),
                                        (L * nst, row if L == 1031 else "BIG_BLOCKED", L if L == 1031 else L * nst, 0)):
            got = _lib.dft_plan(L, 0, 1, 256, 16, nrz)
            assert (got["form"], got["slots"], got["short_slots"]) == (F[form], slots, short), (L, nrz, got)


def test_the_panel_limit_is_never_reached():
    panels = {v["lds"] for *_, v in recorded() if v["form"] == F["SPLIT_LDS"]}
    assert max(panels) == 5 * 50 * 64 * 8 <= PANEL_LIMIT and min(panels) > 0


def _sides(thr, cases):
    """cases: (count, taken).  The rule `taken iff count >= thr` holds on every case, and the cases lie on both sides of thr."""
    cases = list(cases)
    below, above = [c for c, t in cases if not t], [c for c, t in cases if t]
    assert below and above and max(below) < thr <= min(above), (thr, max(below, default=None), min(above, default=None))


def test_cases_reach_both_sides_of_each_threshold():
    none = [c for c in recorded(knob="none") if c[4] == "0"]
    nct = lambda n: (n + 15) // 16      # noqa: E731
    # the split form against the scalar tables (no one-tile form beyond 256 slices): 100 column-tile waves
    _sides(100, ((nct(n) * nv, v["form"] == F["SPLIT_LDS"]) for l, _, w, d, _, n, nv, v in none if w == 0 and l in (258, 320, 400)))
    # ... against the one-tile form: 448
    _sides(448, ((nct(n) * nv, v["form"] == F["SPLIT_LDS"]) for l, _, w, d, _, n, nv, v in none if w == 0 and l % 2 == 0 and 8 <= l <= 256))
    assert {v["form"] for l, _, w, d, _, n, nv, v in none if w == 0 and l % 2 == 0 and 8 <= l <= 256} == {F["SPLIT_LDS"], F["ONE_TILE"]}

    # the direct form (plain transforms up to 256 slices): 512 waves = column tiles x row groups x vectors
    def groups(l, d):
        rows = l if d else 2 * (l // 2 + 1)
        return ((rows + 15) // 16 + 4) // 5
    has_table = lambda l, d: ((2 * (l // 2 + 1) if d else l) + 3) // 4 <= 64      # noqa: E731  (the plain inverse at 256 slices has none)
    _sides(512, ((nct(n) * groups(l, d) * nv, v["form"] == F["DIRECT"]) for l, _, w, d, _, n, nv, v in none if w == 1 and l <= 256 and has_table(l, d)))
    # the blocked long-axis pair: 16384 one-row waves
    _sides(16384, ((nv * ((n + 63) // 64) * l, v["form"] == F["BIG_BLOCKED"]) for l, _, w, d, _, n, nv, v in none if l in (480, 1000, 1024, 1280)))


@pytest.mark.parametrize("L", dc.LTAU)
def test_dft_plan(L, monkeypatch):
    """The plan equals the recorded one for every case and setting; every plan's kernel is instantiated and fits the LDS."""
    for knob, env in dc.KNOBS.items():
        for name in dc.SWITCHES:
            if name in env:
                monkeypatch.setenv(name, env[name])
            else:
                monkeypatch.delenv(name, raising=False)
        for _, _, w, d, z, n, nv, want in recorded(L, knob):
            got = dc.probe(L, w, d, n, nv, z)
            assert got == want, (L, knob, w, d, z, n, nv)
            assert got["nt"] in dc.NT_SIZES[got["form"]], (L, knob, w, d, z, n, nv, got)
            if got["form"] != F["SCALAR"]:      # (the forward split stages the chain's fold table of L/2 pairs behind its W panel)
                assert got["lds"] + 8 * L <= LDS_LIMIT, (L, knob, w, d, z, n, nv, got)
