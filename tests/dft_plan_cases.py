"""The cases of the tau-axis transform plan (csrc/dft_mfma.hip: elph_plan_dft) that tests/test_dft_plan.py checks through the device-free
probe elph_bench_dft_plan.  A case is a time axis, a kind (twisted / plain), a direction, a number of columns, a number of vectors, the
r.z partial slots the caller offers and a setting of the five switches; tests/golden/dft_plan.json holds all of their products."""
import conftest  # noqa: F401  (the repository root on sys.path)
from elphdynamics_amd import _lib

SWITCHES = ("ELPH_DFT_MFMA", "ELPH_DFT_R2", "ELPH_FUSE_XR", "ELPH_FUSE_PX", "ELPH_DFT_BIG_BLOCKED")
LTAU = (4, 6, 7, 8, 20, 40, 45, 80, 100, 160, 200, 256, 258, 320, 400, 402, 409, 422, 480, 1000, 1024, 1031, 1280)
NCOL = (12, 24, 64, 256, 324, 1024)
NVEC = (1, 2, 3, 6, 8, 10, 24, 28, 32, 48, 64, 144, 288)
KINDS = (0, 1)             # twisted, plain
DIRECTIONS = (0, 1)        # forward, inverse
NRZ = ("0", "L", "L*ceil(N/64)")
KNOBS = {
    "none": {},
    "mfma0": {"ELPH_DFT_MFMA": "0"},
    "mfma1": {"ELPH_DFT_MFMA": "1"},
    "mfma1_r2_0": {"ELPH_DFT_MFMA": "1", "ELPH_DFT_R2": "0"},
    "r2_0": {"ELPH_DFT_R2": "0"},
    "fuse_xr0": {"ELPH_FUSE_XR": "0"},
    "fuse_px0": {"ELPH_FUSE_PX": "0"},
    "big_blocked0": {"ELPH_DFT_BIG_BLOCKED": "0"},
    "big_blocked1": {"ELPH_DFT_BIG_BLOCKED": "1"},
}
# the reduction-tile counts the kernels are instantiated for (dft_mfma.hip: the switch of each launch function), by form
F = _lib.DFT_FORMS
NT_SIZES = {
    F["SCALAR"]: {0}, F["BIG_ROW"]: {0}, F["BIG_BLOCKED"]: {0}, F["BIG_DIRECT"]: {0},
    F["ONE_TILE"]: {12, 20, 32, 40, 44, 64}, F["DIRECT"]: {12, 20, 32, 40, 44, 64},
    F["SPLIT_REG"]: {5, 10, 15, 20, 25, 32}, F["SPLIT_LDS"]: {5, 10, 15, 20, 25, 32, 40, 50},
}


def nrz_slots(which, L, N):
    return (0, L, L * ((N + 63) // 64))[NRZ.index(which)]


def cases(L, knob):
    """The cases of one time axis and setting in the table's order: (which, inverse, nrz, N), each a line of len(NVEC) plans."""
    return [(w, d, z, n) for w in KINDS for d in DIRECTIONS for z in NRZ for n in NCOL]


def probe(L, which, inverse, N, nvec, nrz):
    """The plan under the switches now in the environment, as {slot: value} (_lib.DFT_PLAN_SLOTS)."""
    return _lib.dft_plan(L, which, inverse, N, nvec, nrz_slots(nrz, L, N))
