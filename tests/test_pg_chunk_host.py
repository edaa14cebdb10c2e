"""CPU tests of the time-axis chunking of the patch mat-vec kernels (pgrid.hip: elph_pg_chunks) and of the case table of tests/test_gpu_pg_chunks.py:
the rule against a numpy restatement of the two loops the launchers carried before it, the pin ELPH_PG_T, the pg_dispatch aliases covered, and — for
every case of tests/pg_chunk_cases.py — the chunking it was designed for (through the device-free probe elph_bench_pg_chunks, on the launch shape the
library recognises in the case's bond table) and the oracle's margin at the stop test of its solves.  An entry that does not deliver fails here."""
import pytest

import conftest  # noqa: F401  (the repository root on sys.path)
import pg_chunk_cases as pc
from elphdynamics_amd import _lib

ENV = ("ELPH_PG_T", "ELPH_NO_FAST", "ELPH_PG_MW", "ELPH_PG_2X2_FROM")


@pytest.fixture
def env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)

    def use(d):
        for k, v in d.items():
            monkeypatch.setenv(k, v)
    return use


@pytest.fixture(scope="module")
def orc():
    from oracle.oracle import Oracle
    return Oracle()


# ------------------------------------------------------------------------------------------ the rule and the pin

@pytest.mark.parametrize("slots", sorted(pc.SLOT_SHAPES))
def test_rule_equals_the_launchers_loops(slots, env):
    """Every slots class, 1 ... 300 vectors, Ltau = 1 ... 200 and 1280, the three kernels: T, chunks and last chunk of the two loops (the fall-through to
    20 and the clamp to Ltau among them: asserted reached)."""
    seen = set()
    for shape in pc.SLOT_SHAPES[slots]:
        assert pc.slots_of(*shape) == slots
        first = shape == pc.SLOT_SHAPES[slots][0]
        for kernel in pc.KERNELS:
            # the whole grid for k_mul_pg and k_cg_ap_pg on the first shape of the class; every fifth time axis and seventh batch for the fused kernel
            # (the same branch of the rule) and for the other shapes of the class
            full = first and kernel != "cg_ap_px"
            # (k_mul_pg's 2048 workgroups leave no clamp below 300 vectors: batches of 700, 2049 and 5000 on one to three slices for it)
            grid = [(L, nvec) for L in list(range(1, 201, 1 if full else 5)) + [1280] for nvec in range(1, 301, 1 if full else 7)]
            for L, nvec in grid + [(L, nvec) for L in (1, 2, 3) for nvec in (700, 2049, 5000)]:
                want = pc.parent_rule(kernel, *shape, nvec, L)
                got = _lib.pg_chunks(kernel, *shape, nvec, L)
                assert got == want, (kernel, shape, nvec, L, got, want)
                c, fell = pc.parent_choice(kernel, *shape, nvec, L)
                if fell:
                    seen.add((kernel, "fall"))
                    assert want[0] == min(20, L)
                if c > L:
                    seen.add((kernel, "clamp"))
                    assert want == (L, 1, L)
    assert {(k, w) for k in pc.KERNELS for w in ("fall", "clamp")} <= seen


def test_rule_reads_the_whole_launch_shape(env):
    """Honeycomb shapes hold one wave per SIMD whatever their patch; 8 registers per vector hold two; nw divides."""
    assert _lib.pg_chunks("cg_ap", 2, 2, 1, False, 100, 40) != _lib.pg_chunks("cg_ap", 2, 2, 1, True, 100, 40)
    assert _lib.pg_chunks("cg_ap", 2, 4, 1, False, 100, 40) != _lib.pg_chunks("cg_ap", 2, 6, 1, False, 100, 40)
    assert _lib.pg_chunks("cg_ap", 2, 2, 2, False, 100, 40) != _lib.pg_chunks("cg_ap", 2, 2, 4, False, 100, 40)
    assert _lib.pg_chunks("cg_ap", 2, 2, 4, False, 64, 40) == (5, 8, 5)          # the production batch of 12^3: five slices per workgroup
    assert _lib.pg_chunks("mul", 2, 2, 4, False, 48, 40) == (1, 40, 1)           # 1920 workgroups: the largest batched mat-vec the suite had


@pytest.mark.parametrize("kernel", pc.KERNELS)
def test_pin(kernel, env):
    """ELPH_PG_T=n: T = n clamped to [1, Ltau] for every kernel, whatever the batch; n < 1, n > Ltau; not a whole number: the rule."""
    shape = (2, 2, 4, False)
    for L, nvec in ((7, 2), (11, 3), (1, 1), (40, 64), (200, 300)):
        rule = pc.parent_rule(kernel, *shape, nvec, L)
        for n in (1, 2, 3, 4, 6, 7, 10, 40, 199):
            env({"ELPH_PG_T": str(n)})
            assert _lib.pg_chunks(kernel, *shape, nvec, L) == pc.pinned(n, L)
        for n in ("0", "-3", "-2147483649"):
            env({"ELPH_PG_T": n})
            assert _lib.pg_chunks(kernel, *shape, nvec, L) == (1, L, 1)
        for n in ("1000000", "99999999999999999999"):
            env({"ELPH_PG_T": n})
            assert _lib.pg_chunks(kernel, *shape, nvec, L) == (L, 1, L)
        for n in ("", "abc", "4x", "2.5", " "):
            env({"ELPH_PG_T": n})
            assert _lib.pg_chunks(kernel, *shape, nvec, L) == rule, n
    for T, nch, last in (_lib.pg_chunks(kernel, *shape, 2, L) for L in range(1, 60)):
        assert T >= 1 and nch >= 1 and 1 <= last <= T          # (the last value pinned above is not a number: the rule)


def test_probe_refuses_bad_arguments(env):
    lib = _lib.load()
    out = (_lib.c_int * 3)()
    for args in ((3, 2, 2, 1, 0, 1, 7), (-1, 2, 2, 1, 0, 1, 7), (0, 0, 2, 1, 0, 1, 7), (0, 2, 2, 0, 0, 1, 7), (0, 2, 2, 1, 0, 0, 7), (0, 2, 2, 1, 0, 1, 0)):
        assert lib.elph_bench_pg_chunks(*args, out) == _lib.ELPH_E_ARG
    assert lib.elph_bench_pg_chunks(0, 2, 2, 1, 0, 1, 7, None) == _lib.ELPH_E_ARG


# ------------------------------------------------------------------------------------------ the case table

def test_every_alias_is_covered_or_listed():
    """pg_dispatch's aliases = the aliases PIN runs k_mul_pg and the un-fused k_cg_ap_pg in + the aliases listed as unreached: a new rung cannot
    arrive untested."""
    names = pc.dispatch_aliases()
    covered = {v[4] for v in pc.PIN.values()}
    assert len(names) == len(set(names)) == 36
    assert not covered & set(pc.UNREACHED)
    assert len(covered) + len(pc.UNREACHED) == len(names) and covered | set(pc.UNREACHED) == set(names)
    assert {v[3] for v in pc.FUSED.values()} <= set(names) and "M22_4" in {v[3] for v in pc.FUSED.values()}


@pytest.mark.parametrize("name", sorted(pc.PIN))
def test_pin_case(name, env, orc):
    """The lattice is recognised in the shape of its alias; under every pin both kernels take the designed chunking; the oracle's solves from the
    case's guesses stop with a margin."""
    fam, side, e, sd, alias, nvec = pc.PIN[name]
    env(e)
    fs, rs = pc.seeds(name)
    m = pc.make_model(fam, side, pc.PIN_LTAU, sd, fs, host=True)
    kind, px, py, nw, tables = pc.shape_of(m)
    assert kind == pc.family(fam)[3] and pc.alias_of(kind, px, py, nw, tables) == alias
    for kernel in ("mul", "cg_ap"):
        for T in pc.PIN_T:
            env({"ELPH_PG_T": str(T)})
            assert _lib.pg_chunks(kernel, px, py, nw, kind == 2, 1 if kernel == "mul" else nvec, pc.PIN_LTAU) == pc.pinned(T, pc.PIN_LTAU)
    om = pc.oracle_model(orc, m)
    B, X0 = pc.inputs(orc, om, m.Ndim, nvec, rs)
    pc.oracle_solves(orc, om, B, X0)
    if name in pc.LONG:
        m = pc.make_model(fam, side, pc.LONG_LTAU, sd, fs, host=True)
        om = pc.oracle_model(orc, m)
        B, X0 = pc.inputs(orc, om, m.Ndim, 2, rs)
        pc.oracle_solves(orc, om, B, X0)
        for T in pc.LONG_T:
            env({"ELPH_PG_T": str(T)})
            assert _lib.pg_chunks("cg_ap", px, py, nw, kind == 2, 2, pc.LONG_LTAU) == pc.pinned(T, pc.LONG_LTAU)


def test_designed_reach(env):
    """What the table must hold.  k_cg_ap_pg: T = 2, 4, 5, one of 8 and 10, T = Ltau, last chunks of one slice and of T - 1 >= 2 slices; k_mul_pg:
    T = 2 and a T >= 4, both ragged.  PIN and LONG deliver it on EVERY lattice they name (test_pin_case asserts each through the probe); RULE
    delivers T = 2 and T = 4 without the pin."""
    cg = {pc.pinned(T, pc.PIN_LTAU) for T in pc.PIN_T} | {pc.pinned(T, pc.LONG_LTAU) for T in pc.LONG_T}
    Ts = {c[0] for c in cg}
    assert {2, 4, 5} <= Ts and Ts & {8, 10} and pc.PIN_LTAU in Ts
    assert any(last == 1 and T > 1 for T, _, last in cg) and any(last == T - 1 >= 2 for T, _, last in cg)
    assert pc.pinned(40, pc.PIN_LTAU) == (pc.PIN_LTAU, 1, pc.PIN_LTAU)          # the clamp
    mul = {pc.pinned(T, pc.PIN_LTAU) for T in pc.PIN_T}
    assert any(T == 2 and last < T for T, _, last in mul) and any(T >= 4 and last < T for T, _, last in mul)
    assert {v[4][0] for v in pc.RULE.values()} == {2, 4} and {v[5][0] for v in pc.RULE.values()} == {1, 2}
    assert all(v[4][2] < v[4][0] for v in pc.RULE.values())                      # every rule case ends in a short chunk
    assert set(pc.LONG) <= set(pc.PIN)


@pytest.mark.parametrize("name", sorted(pc.RULE))
def test_rule_case(name, env, orc):
    """Part (a): without the pin, the batch reaches the designed chunking in both kernels; the un-preconditioned solves from the guesses and the
    preconditioned solves from zero stop with a margin on the oracle."""
    fam, side, ltau, nrhs, cg, mul = pc.RULE[name]
    fs, rs = pc.seeds("rule-" + name)
    m = pc.make_model(fam, side, ltau, 0.0, fs, host=True, dtau=pc.RULE_DTAU)
    kind, px, py, nw, tables = pc.shape_of(m)
    assert not tables and pc.alias_of(kind, px, py, nw, tables) is not None
    assert _lib.pg_chunks("cg_ap", px, py, nw, kind == 2, nrhs, ltau) == cg
    assert _lib.pg_chunks("mul", px, py, nw, kind == 2, nrhs, ltau) == mul
    assert _lib.pg_chunks("mul", px, py, nw, kind == 2, 1, ltau) == (1, ltau, 1)
    N = m.Nsites
    assert not (_lib.dft_plan(ltau, 0, False, N, nrhs)["xr"] and _lib.dft_plan(ltau, 0, True, N, nrhs)["px"])      # an odd time axis never fuses
    om = pc.oracle_model(orc, m)
    B, X0 = pc.inputs(orc, om, m.Ndim, nrhs, rs)
    pc.oracle_solves(orc, om, B, X0)
    oP, _, _ = pc.oracle_kpm(orc, om, N)
    pc.oracle_solves(orc, om, B, None, oP)


@pytest.mark.parametrize("name", sorted(pc.FUSED))
def test_fused_case(name, env, orc):
    """The transform plan fuses at the case's shape and not on the next shorter even time axis or, where the batch can shrink, with one right-hand side
    fewer than the smallest batch that fuses there (the cubic rows: test_gpu_cubic.FUSED); the launch shape of the fused kernel is the alias's; the
    pin gives a ragged walk."""
    lattice, ltau, nrhs, alias = pc.FUSED[name]
    fam, side, e, sd, _, _ = pc.PIN[lattice]
    env(e)
    m = pc.make_model(fam, side, ltau, sd, host=True)          # (the shape does not depend on the field)
    kind, px, py, nw, tables = pc.shape_of(m)
    N = m.Nsites

    def fuses(lt, n):
        return bool(_lib.dft_plan(lt, 0, False, N, n)["xr"] and _lib.dft_plan(lt, 0, True, N, n)["px"])
    assert fuses(ltau, nrhs)
    if nrhs < 48:
        assert not fuses(ltau - 2, nrhs)
        assert pc.alias_of(kind, px, py, nw, tables) == alias
    else:
        # pg_launch_shape: 4 x 4 patches on one wavefront run a fused batch from 48 right-hand sides as 2 x 2 patches
        assert (px, py, nw) == (4, 4, 1) and pc.alias_of(kind, 2, 2, ((side // 2) ** 2 + 63) // 64, tables) == alias
    T = pc.ragged_T(ltau)
    env({"ELPH_PG_T": str(T)})
    got = _lib.pg_chunks("cg_ap_px", px, py, nw, kind == 2, nrhs, ltau)
    assert got == pc.pinned(T, ltau) and got[2] < T
    fs, rs = pc.seeds("fused-" + name)
    m = pc.make_model(fam, side, ltau, sd, fs, host=True)
    om = pc.oracle_model(orc, m)
    B, _ = pc.inputs(orc, om, m.Ndim, nrhs, rs)
    pc.oracle_solves(orc, om, B, None, pc.oracle_kpm(orc, om, N)[0])
