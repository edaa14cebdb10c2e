"""CPU-side tests (no GPU): host set-up logic of the product against the golden integer tables, the
C-ABI library loads and exports every symbol include/elph_gpu.h declares, and the product refuses to
compute without a device (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from elphdynamics_amd import lattice as lat
from elphdynamics_amd import synth

CASES = [("sq2", 1, 2, 2, lat.SQUARE_BONDS), ("sq4", 1, 4, 4, lat.SQUARE_BONDS), ("sq8", 1, 8, 8, lat.SQUARE_BONDS),
         ("sq16", 1, 16, 16, lat.SQUARE_BONDS), ("hc3", 2, 3, 3, lat.HONEYCOMB_BONDS),
         ("hc12", 2, 12, 12, lat.HONEYCOMB_BONDS), ("tri3", 1, 3, 3, lat.TRIANGULAR_BONDS),
         ("chain6", 1, 6, 1, [(1, 1, (1, 0, 0))])]


@pytest.mark.parametrize("tag,norb,L1,L2,bonds", CASES)
def test_product_tables_bit_exact(tag, norb, L1, L2, bonds):
    """elphdynamics_amd.lattice reproduces the golden neighbour table / colouring / permutation bit-for-bit."""
    g = golden("tables.npz")
    la = lat.Lattice(norb, L1, L2, 1)
    raw = np.concatenate([la.calc_neighbor_table(o1, o2, d) for (o1, o2, d) in bonds], axis=0)
    assert np.array_equal(raw, g[tag + "_raw"])
    cb = lat.initialize_checkerboard(raw, np.ones(raw.shape[0]), 0.1)
    assert np.array_equal(cb["table"], g[tag + "_table"])
    assert np.array_equal(cb["colours"], g[tag + "_colour"])
    assert np.array_equal(cb["cb_perm"], g[tag + "_cbperm"])
    assert np.array_equal(cb["inv_cb_perm"][cb["cb_perm"] - 1], np.arange(1, raw.shape[0] + 1))


def test_product_tables_match_oracle(oracle):
    la = lat.Lattice(2, 4, 4, 1)
    raw = np.concatenate([la.calc_neighbor_table(o1, o2, d) for (o1, o2, d) in lat.HONEYCOMB_BONDS], axis=0)
    assert np.array_equal(raw, oracle.neighbor_table(2, 4, 4, 1, lat.HONEYCOMB_BONDS))
    t = 1.0 + 0.1 * synth.randn(3, raw.shape[0])
    cb = lat.initialize_checkerboard(raw, t, 0.1)
    tab, c, s, perm, grp, ng = oracle.holstein_initialize(raw, t, 0.1)
    assert np.array_equal(cb["table"], tab) and np.array_equal(cb["cb_perm"], perm)
    assert np.allclose(cb["cosht"], c, rtol=4e-16, atol=0) and np.allclose(cb["sinht"], s, rtol=4e-16, atol=0)   # libm vs numpy: <= 1 ulp
    assert cb["ncolours"] == ng


def test_ltau_and_site_numbering():
    assert lat.ltau_from_beta(16.0, 0.1) == 160 and lat.ltau_from_beta(2.5, 1.0) == 2 and lat.ltau_from_beta(3.5, 1.0) == 4
    la = lat.Lattice(2, 3, 4, 1)
    assert la.nsites == 24
    assert la.loc_to_site(1, 0, 0) == 1 and la.loc_to_site(2, 0, 0) == 2 and la.loc_to_site(1, 1, 0) == 3
    assert la.loc_to_site(1, -1, 0) == la.loc_to_site(1, 2, 0)
    assert la.site_to_site(1, (0, -1, 0), 2) == la.loc_to_site(2, 0, 3)


def test_synth_is_deterministic_and_sane():
    a, b = synth.randn(5, 1001), synth.randn(5, 1001)
    assert np.array_equal(a, b) and len(a) == 1001
    g = synth.randn(1, 200000)
    assert abs(g.mean()) < 0.01 and abs(g.std() - 1) < 0.01
    x = synth.phonon_field(8, 10, 1.0, 0.1, rough=False)
    assert np.all(x.reshape(8, 10) == x.reshape(8, 10)[:, :1])          # cold start: tau-constant per site


def test_abi_library_exports_every_declared_symbol():
    """Every function declared in include/elph_gpu.h is exported by the built library and bound in _lib.SIGNATURES."""
    from elphdynamics_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "elph_gpu.h")).read()
    declared = set(re.findall(r"\b(elph_[a-z_0-9A-Z]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    # the private measurement hooks (csrc/elph_bench.h) stay out of the public header and are bound separately
    priv = open(os.path.join(ROOT, "elphdynamics_amd", "csrc", "elph_bench.h")).read()
    hooks = set(re.findall(r"\b(elph_[a-z_0-9A-Z]+)\s*\(", priv))
    assert hooks == set(_lib.BENCH_SIGNATURES) and not (hooks & declared), hooks ^ set(_lib.BENCH_SIGNATURES)
    assert not [n for n in declared if n.startswith(("elph_bench_", "elph_cgstep_"))]
    lib = _lib.load()
    for name in declared | hooks:
        assert hasattr(lib, name)
    assert lib.elph_abi_version() == _lib.ABI_VERSION == 2
    assert isinstance(lib.elph_last_error(), bytes)


def test_no_cpu_fallback_without_device():
    """Without a HIP device the product must fail loudly, never compute on the host."""
    from elphdynamics_amd import _lib
    lib = _lib.load()
    if lib.elph_device_count() > 0:
        pytest.skip("a GPU is visible here")
    h = _lib.Handle()
    rc = lib.elph_create(C.byref(h), 0, 4, 4, 0, None, None, None, 0)
    assert rc == -4 and b"no HIP device" in lib.elph_last_error()
    from elphdynamics_amd import configs
    with pytest.raises(_lib.ElphError):
        configs.make_model("b")


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under elphdynamics_amd/ may reference it."""
    pkg = os.path.join(ROOT, "elphdynamics_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "elph_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, f


def test_every_environment_switch_is_in_the_design_table():
    """DESIGN.md §9 promises ONE table with every ELPH_* switch the library or the Python host reads: a switch added to the sources without a
    row there fails here."""
    import glob
    import re
    names = set()
    for f in glob.glob(os.path.join(ROOT, "elphdynamics_amd", "csrc", "*")):
        if os.path.isfile(f):
            names |= set(re.findall(r'getenv\("(ELPH_[A-Z0-9_]+)"\)', open(f, errors="replace").read()))
    for f in glob.glob(os.path.join(ROOT, "elphdynamics_amd", "*.py")) + [os.path.join(ROOT, "bench.py")]:
        names |= set(re.findall(r'environ(?:\.get)?[\(\[]\s*"(ELPH_[A-Z0-9_]+)"', open(f).read()))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = design[design.index("## 9. Environment switches"):]
    missing = sorted(n for n in names if n not in table)
    assert len(names) > 30 and not missing, missing
    # ... and the other way: every switch named in the first column of the table is still read somewhere (a retired switch leaves no row)
    listed = set()
    for line in table.splitlines():
        cells = line.split("|")
        if line.startswith("| `ELPH_") and len(cells) > 2:
            listed |= set(re.findall(r"ELPH_[A-Z0-9_]+", cells[1]))
    csrc, py = [], []
    for f in glob.glob(os.path.join(ROOT, "elphdynamics_amd", "csrc", "*")):
        if os.path.isfile(f):
            csrc.append(open(f, errors="replace").read())
    for pattern in ("elphdynamics_amd/*.py", "bench.py", "tests/**/*.py", "tools/**/*.py"):
        for f in glob.glob(os.path.join(ROOT, pattern), recursive=True):
            py.append(open(f, errors="replace").read())
    csrc, py = "\n".join(csrc), "\n".join(py)

    def read(n):   # getenv or a preprocessor condition in csrc; os.environ[...] / os.environ.get(...) in Python
        return (re.search(r'getenv\("' + n + r'"\)', csrc) or re.search(r'^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b[^\n]*\b' + n + r'\b', csrc, re.M)
                or re.search(r'environ(?:\.get|\.pop|\.setdefault)?[\(\[]\s*["\']' + n + r'["\']', py))
    stale = sorted(n for n in listed if not read(n))
    assert len(listed) > 30 and not stale, stale


def test_tools_compile_and_are_indexed():
    """Every helper under tools/ is valid Python (byte-compiles: they only run on the GPU box, where a syntax error costs a gpurun call) and has a
    row in tools/README.md."""
    import glob
    import py_compile
    import tempfile
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    missing = []
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(glob.glob(os.path.join(ROOT, "tools", "*.py"))):
            py_compile.compile(f, cfile=os.path.join(tmp, os.path.basename(f) + "c"), doraise=True)
            if "`" + os.path.basename(f) + "`" not in readme:
                missing.append(os.path.basename(f))
    for f in sorted(glob.glob(os.path.join(ROOT, "tools", "*.sh"))):
        if "`" + os.path.basename(f) + "`" not in readme:
            missing.append(os.path.basename(f))
    assert not missing, missing


def test_every_abi_entry_point_is_driven_by_a_test_or_the_host_mirror():
    """include/elph_gpu.h declares the drop-in boundary; an entry point nobody calls — no host-mirror function, no test, not abi_smoke.c — is
    unverified surface.  (The signature table of _lib.py does not count.)"""
    import glob
    import re
    hdr = open(os.path.join(ROOT, "include", "elph_gpu.h")).read()
    names = sorted(set(re.findall(r"^\s*(?:int|const char \*|void)\s+\*?(elph_[a-z0-9_]+)\s*\(", hdr, re.M)))
    assert len(names) >= 70, len(names)
    text = ""
    for f in glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "elphdynamics_amd", "*.py")) + \
            [os.path.join(ROOT, "tests", "abi_c", "abi_smoke.c"), os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]:
        if os.path.basename(f) in ("_lib.py", "test_host_cpu.py"):
            continue
        text += open(f).read()
    exempt = {"elph_langevin_create_ssh"}      # Langevin dynamics of the bond-phonon model: SURVEY §2 out of scope (its Holstein twin is tested)
    missing = [n for n in names if n not in exempt and not re.search(r"\b" + n + r"\b", text)]
    assert not missing, missing
