"""CPU test of the resident CG launch plan (csrc/cg_wg.hip: plan_wg, plan_shard, the launch table), through the device-free probe
elph_bench_wg_plan.  tests/golden/wg_plan.json holds, for every case of wg_plan_cases.py, batch size and setting of the switches, the plan
of the rule this record replaced — elph_wg_usable's refusals, pick_shape, the form predicates, the cost comparison of elph_wg_cg and the
arithmetic of shard_rank_setup, recorded through the same probe before they were folded into it."""
import json
import os

import pytest

from conftest import ROOT
from elphdynamics_amd import _lib, configs
import wg_plan_cases as wc

with open(os.path.join(ROOT, "tests", "golden", "wg_plan.json")) as _f:
    TABLE = json.load(_f)
LDS_LIMIT = 160 * 1024


def recorded(case=None):
    """(case, setting, nrhs, {slot: value}) of every recorded plan (of one case)."""
    for c in ([case] if case else sorted(TABLE["plans"])):
        for kname, ids in TABLE["plans"][c].items():
            for nrhs, i in zip(TABLE["nrhs"], ids):
                yield c, kname, nrhs, dict(zip(TABLE["slots"], TABLE["rows"][i]))


def test_table_is_the_table_of_these_cases():
    assert tuple(TABLE["slots"]) == wc.ROW_SLOTS and tuple(TABLE["nrhs"]) == wc.NRHS
    assert sorted(TABLE["plans"]) == sorted(wc.CASES)
    assert all(sorted(p) == sorted(wc.KNOBS) for p in TABLE["plans"].values())
    assert set(configs.CONFIGS) <= set(wc.CASES)


def test_cases_reach_every_form():
    """... and both the Holstein and the SSH variant of the 16 x 16 DPP form."""
    seen = {(v["form"], wc.CASES[c][0]) for c, _, _, v in recorded() if v["usable"]}
    assert {f for f, _ in seen} == set(_lib.WG_FORMS.values())
    assert {(_lib.WG_FORMS["SQ16"], "holstein"), (_lib.WG_FORMS["SQ16"], "ssh")} <= seen


def test_cases_reach_every_team_shape_and_both_sides_of_the_cost_rule():
    usable = [v for _, _, _, v in recorded() if v["usable"]]
    assert {v["T"] for v in usable} == {1, 2, 3, 4, 5, 8}
    assert {v["resident"] for v in usable} == {0, 1}


@pytest.mark.parametrize("case", sorted(wc.CASES))
def test_wg_plan(case, monkeypatch):
    """The plan equals the recorded one for every batch size and setting; every usable plan has its kernel in the launch table and
    fits the LDS."""
    setting_now = None
    for c, kname, nrhs, want in recorded(case):
        if kname != setting_now:
            for name in wc.SWITCHES:
                if name in wc.KNOBS[kname]:
                    monkeypatch.setenv(name, wc.KNOBS[kname][name])
                else:
                    monkeypatch.delenv(name, raising=False)
            setting_now = kname
        got = wc.probe(c, nrhs)
        assert {k: got[k] for k in wc.ROW_SLOTS} == want, (c, kname, nrhs)
        assert got["shm"] <= LDS_LIMIT, (c, kname, nrhs, got["shm"])
        if got["usable"]:
            assert got["has_kernel"] == 1, (c, kname, nrhs, got)
