"""ctypes binding of libelphgpu.so — the C ABI declared in include/elph_gpu.h.

The library is hand-written HIP for gfx950; there is no CPU path.  Loading fails loudly if the
shared object has not been built (`python -c "import __graft_entry__ as g; g.build()"`), and every
compute entry point returns ELPH_E_NOGPU / ELPH_E_HIP without a usable MI355X.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

c_i64, c_dbl, c_int = C.c_int64, C.c_double, C.c_int
P_i64, P_dbl, P_int = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int)
Handle = C.c_void_p

ELPH_OK = 0
ABI_VERSION = 2          # include/elph_gpu.h: ELPH_ABI_VERSION this binding was written against (checked exactly at load)
ELPH_E_ARG, ELPH_E_HIP, ELPH_E_STATE, ELPH_E_NOGPU, ELPH_E_UNSUPPORTED = -1, -2, -3, -4, -5
ERRORS = {-1: "ELPH_E_ARG", -2: "ELPH_E_HIP", -3: "ELPH_E_STATE", -4: "ELPH_E_NOGPU", -5: "ELPH_E_UNSUPPORTED"}

# every symbol include/elph_gpu.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "elph_last_error": (C.c_char_p, []),
    "elph_abi_version": (c_int, []),
    "elph_build_info": (C.c_char_p, []),
    "elph_device_count": (c_int, []),
    "elph_create": (c_int, [C.POINTER(Handle), c_int, c_i64, c_i64, c_i64, P_i64, P_dbl, P_dbl, c_int]),
    "elph_destroy": (c_int, [Handle]),
    "elph_set_stream": (c_int, [Handle, C.c_void_p]),
    "elph_synchronize": (c_int, [Handle]),
    "elph_update_model_holstein": (c_int, [Handle, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl]),
    "elph_update_model_holstein_chains": (c_int, [Handle, c_int, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl]),
    "elph_set_expV": (c_int, [Handle, P_dbl]),
    "elph_update_model_ssh": (c_int, [Handle, P_dbl, P_dbl, P_dbl]),
    "elph_update_model_ssh_fields": (c_int, [Handle, P_dbl, c_i64, P_i64, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl]),
    "elph_update_model_ssh_fields_chains": (c_int, [Handle, c_int, P_dbl, c_i64, P_i64, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl]),
    "elph_get_cosh_sinh": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_mulM": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_mulMT": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_mulMTM": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_mulMMT": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_mulM_dev": (c_int, [Handle, C.c_void_p, C.c_void_p]),
    "elph_mulMT_dev": (c_int, [Handle, C.c_void_p, C.c_void_p]),
    "elph_mulMTM_dev": (c_int, [Handle, C.c_void_p, C.c_void_p]),
    "elph_solver_set": (c_int, [Handle, c_dbl, c_i64, c_dbl]),
    "elph_solver_set_kind": (c_int, [Handle, c_int, c_int]),
    "elph_cg_solve": (c_int, [Handle, P_dbl, P_dbl, c_dbl, c_i64, c_dbl, c_int, P_i64, P_dbl]),
    "elph_ldiv": (c_int, [Handle, P_dbl, P_dbl, c_int, c_i64, P_i64, P_dbl, P_int]),
    "elph_ldiv_batched": (c_int, [Handle, c_int, P_dbl, P_dbl, c_int, c_i64, P_i64, P_dbl, P_int]),
    "elph_ldiv_dev": (c_int, [Handle, C.c_void_p, C.c_void_p, c_int, c_i64, P_i64, P_dbl, P_int]),
    "elph_ldiv_batched_dev": (c_int, [Handle, c_int, C.c_void_p, C.c_void_p, c_int, c_i64, P_i64, P_dbl, P_int]),
    "elph_fermion_force_holstein": (c_int, [Handle, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_dbl, P_dbl, c_int, c_dbl, P_dbl, P_dbl, P_dbl,
                                            P_i64, P_int]),
    "elph_fermion_force_ssh": (c_int, [Handle, P_dbl, P_dbl, c_int, c_dbl, P_dbl, P_dbl, P_dbl, P_i64, P_int]),
    "elph_fermion_force_ssh_fields": (c_int, [Handle, P_dbl, P_dbl, c_int, c_dbl, P_dbl, P_dbl, P_dbl, P_i64, P_int]),
    "elph_muldMdx_holstein": (c_int, [Handle, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl]),
    "elph_muldMdx_holstein_dev": (c_int, [Handle, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P_dbl, P_dbl, c_dbl]),
    "elph_muldMdx_ssh": (c_int, [Handle, P_dbl, P_dbl, P_dbl]),
    "elph_muldMdx_ssh_fields": (c_int, [Handle, P_dbl, P_dbl, P_dbl]),
    "elph_muldMdx_ssh_fields_dev": (c_int, [Handle, C.c_void_p, C.c_void_p, C.c_void_p]),
    "elph_hmc_create": (c_int, [Handle, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_dbl]),
    "elph_hmc_set_state": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_hmc_get_state": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_hmc_update": (c_int, [Handle, c_dbl, c_i64, c_int, c_dbl, c_int, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_int, P_dbl, P_dbl,
                                P_int]),
    "elph_hmc_set_mu": (c_int, [Handle, P_dbl]),
    "elph_hmc_set_mu_chains": (c_int, [Handle, P_dbl]),
    "elph_hmc_set_shared_fields": (c_int, [Handle, P_i64]),
    "elph_hmc_set_rng": (c_int, [Handle, C.c_uint64]),
    "elph_hmc_rng_batches": (c_int, [Handle, C.POINTER(C.c_uint64)]),
    "elph_hmc_special_move_chains": (c_int, [Handle, c_int, P_i64, P_i64, P_dbl, P_dbl, c_int, P_dbl, P_dbl, P_int, P_dbl, P_dbl, P_i64, P_int]),
    "elph_hmc_special_move": (c_int, [Handle, c_int, c_i64, c_i64, P_dbl, P_dbl, c_int, P_dbl, c_dbl, P_int, P_dbl, P_dbl, P_i64, P_int]),
    "elph_hmc_special_update_chains": (c_int, [Handle, c_int, c_i64, c_int, P_int, P_i64, P_i64, P_dbl, P_dbl, P_i64, P_int]),
    "elph_langevin_create": (c_int, [Handle, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_dbl]),
    "elph_langevin_create_ssh": (c_int, [Handle, c_i64, P_dbl, P_dbl, P_i64, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_dbl]),
    "elph_langevin_create_chains": (c_int, [Handle, c_int, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_dbl]),
    "elph_langevin_evolve": (c_int, [Handle, c_int, c_dbl, c_int, P_dbl, P_dbl, P_dbl, P_dbl, P_i64, P_int]),
    "elph_greens_create": (c_int, [Handle, c_int, c_int, c_int, c_int, c_int]),
    "elph_greens_nv": (c_int, [Handle, P_int]),
    "elph_greens_update": (c_int, [Handle, P_dbl, c_int, P_i64, P_dbl, P_int]),
    "elph_greens_set_rng": (c_int, [Handle, C.c_uint64]),
    "elph_greens_rng_batches": (c_int, [Handle, C.POINTER(C.c_uint64)]),
    "elph_greens_update_rng": (c_int, [Handle, c_int, P_i64, P_dbl, P_int]),
    "elph_greens_set_vectors": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_greens_get_vectors": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_greens_setup": (c_int, [Handle, c_int, c_int, P_dbl, P_dbl, P_dbl, P_dbl]),
    "elph_greens_dev_arrays": (c_int, [Handle, C.POINTER(C.c_void_p), P_i64]),
    "elph_meas_create": (c_int, [Handle, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, c_i64, c_int, P_i64, P_dbl, P_int, P_int, P_int, P_int]),
    "elph_meas_accumulate": (c_int, [Handle, P_dbl]),
    "elph_meas_fetch": (c_int, [Handle, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl]),
    "elph_meas_reset": (c_int, [Handle]),
    "elph_meas_chains_create": (c_int, [Handle, c_int, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, c_i64, c_int, P_i64, P_dbl, P_int, P_int, P_int, P_int]),
    "elph_meas_chains_set_mu": (c_int, [Handle, P_dbl]),
    "elph_meas_chains_accumulate": (c_int, [Handle, P_dbl]),
    "elph_meas_chains_fetch": (c_int, [Handle, c_int, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl]),
    "elph_meas_chains_reset": (c_int, [Handle]),
    "elph_density_moments": (c_int, [Handle, c_int, P_dbl, P_dbl]),
    "elph_snapshots": (c_int, [Handle, c_int, P_dbl, P_dbl]),
    "elph_bond_create": (c_int, [Handle, c_int, P_int, P_int, P_int, P_int, P_int, P_int, P_int]),
    "elph_bond_accumulate": (c_int, [Handle]),
    "elph_bond_fetch": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_bond_reset": (c_int, [Handle]),
    "elph_bond_chains_create": (c_int, [Handle, c_int, c_int, P_int, P_int, P_int, P_int, P_int, P_int, P_int]),
    "elph_bond_chains_accumulate": (c_int, [Handle]),
    "elph_bond_chains_fetch": (c_int, [Handle, c_int, P_dbl, P_dbl]),
    "elph_bond_chains_reset": (c_int, [Handle]),
    "elph_ssh_meas_create": (c_int, [Handle, P_dbl, c_dbl, c_i64, c_int, P_i64, P_dbl, P_i64, P_i64, c_i64, c_int, P_dbl, P_dbl, P_dbl, P_int, P_int,
                                     P_int, P_int]),
    "elph_ssh_meas_accumulate": (c_int, [Handle, P_dbl]),
    "elph_ssh_meas_fetch": (c_int, [Handle, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl]),
    "elph_ssh_meas_reset": (c_int, [Handle]),
    "elph_ssh_meas_free": (c_int, [Handle]),
    "elph_ssh_meas_chains_create": (c_int, [Handle, c_int, P_dbl, c_dbl, c_i64, c_int, P_i64, P_dbl, P_i64, P_i64, c_i64, c_int, P_dbl, P_dbl, P_dbl, P_int,
                                            P_int, P_int, P_int]),
    "elph_ssh_meas_chains_set_mu": (c_int, [Handle, P_dbl]),
    "elph_ssh_meas_chains_accumulate": (c_int, [Handle, P_dbl]),
    "elph_ssh_meas_chains_fetch": (c_int, [Handle, c_int, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl]),
    "elph_ssh_meas_chains_reset": (c_int, [Handle]),
    "elph_ssh_bond_create": (c_int, [Handle, c_int, P_int, P_int, P_int, c_i64, P_dbl, P_i64, P_i64, c_i64, P_dbl, P_dbl, P_int, P_int, P_int, P_int]),
    "elph_ssh_bond_accumulate": (c_int, [Handle, P_dbl]),
    "elph_ssh_bond_fetch": (c_int, [Handle, P_dbl, P_dbl, P_dbl]),
    "elph_ssh_bond_reset": (c_int, [Handle]),
    "elph_ssh_bond_chains_create": (c_int, [Handle, c_int, c_int, P_int, P_int, P_int, c_i64, P_dbl, P_i64, P_i64, c_i64, P_dbl, P_dbl, P_int, P_int, P_int,
                                            P_int]),
    "elph_ssh_bond_chains_accumulate": (c_int, [Handle, P_dbl]),
    "elph_ssh_bond_chains_fetch": (c_int, [Handle, c_int, P_dbl, P_dbl, P_dbl]),
    "elph_ssh_bond_chains_reset": (c_int, [Handle]),
    "elph_current_create": (c_int, [Handle, c_int, c_int, P_int, P_int, P_int, c_i64, P_dbl, c_int, c_int, c_int, P_int]),
    "elph_current_accumulate": (c_int, [Handle]),
    "elph_current_fetch": (c_int, [Handle, c_int, P_dbl]),
    "elph_current_reset": (c_int, [Handle]),
    "elph_hmc_create_ssh": (c_int, [Handle, c_i64, P_dbl, P_dbl, P_i64, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_dbl]),
    "elph_hmc_create_ssh_chains": (c_int, [Handle, c_int, c_i64, P_dbl, P_dbl, P_i64, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_dbl]),
    "elph_hmc_create_chains": (c_int, [Handle, c_int, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_dbl]),
    "elph_hmc_update_chains": (c_int, [Handle, c_dbl, c_i64, c_int, c_dbl, c_int, P_dbl, P_dbl, P_dbl, P_dbl, P_dbl, P_int, P_dbl, P_dbl,
                                       P_int]),
    "elph_kpm_create": (c_int, [Handle, c_int, c_dbl, c_dbl, c_dbl]),
    "elph_kpm_setup": (c_int, [Handle, P_dbl, P_dbl, c_dbl, c_dbl, P_int, P_dbl, P_dbl]),
    "elph_kpm_setup_chains": (c_int, [Handle, P_dbl, P_dbl, P_dbl, P_dbl, P_int, P_dbl, P_dbl]),
    "elph_kpm_orders": (c_int, [Handle, P_i64, P_i64]),
    "elph_kpm_apply": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_kpm_apply_dev": (c_int, [Handle, C.c_void_p, C.c_void_p]),
    "elph_kpm_apply_side": (c_int, [Handle, c_int, P_dbl, P_dbl, c_int]),
    "elph_msolve": (c_int, [Handle, c_int, c_int, c_int, P_dbl, P_dbl, c_int, c_dbl, c_i64, c_i64, c_int, P_i64]),
    "elph_mldiv": (c_int, [Handle, c_int, c_int, c_int, P_dbl, P_dbl, c_int, c_i64, c_int, P_i64, P_dbl, P_int]),
    "elph_fourier_accelerate": (c_int, [Handle, P_dbl, P_dbl, P_dbl, c_dbl, c_i64]),
    "elph_tau_to_omega": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_omega_to_tau": (c_int, [Handle, P_dbl, P_dbl]),
    "elph_wg_status": (c_int, [Handle, P_int, P_i64]),
    "elph_shard_shape": (c_int, [c_i64, c_int, P_int, P_int, P_int, P_int]),
    "elph_shard_create": (c_int, [Handle, c_int, c_int, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, P_i64, C.c_void_p]),
    "elph_shard_connect": (c_int, [Handle, C.c_void_p]),
    "elph_shard_prepare": (c_int, [Handle]),
    "elph_shard_selftest": (c_int, [Handle, c_int, P_dbl, P_dbl]),
    "elph_peer_access": (c_int, [c_int, c_int, P_int]),
    "elph_shard_solve": (c_int, [Handle, P_dbl, P_dbl, c_dbl, c_i64, c_dbl, P_i64, P_int, P_dbl]),
    "elph_shard_solve_kpm": (c_int, [Handle, Handle, P_dbl, P_dbl, c_dbl, c_i64, c_dbl, P_i64, P_int, P_dbl]),
    "elph_shard_destroy": (c_int, [Handle]),
    "elph_shard_set_collectives": (c_int, [Handle, C.c_void_p, C.c_void_p, C.c_void_p]),
    "elph_shard_hmc_set_columns": (c_int, [Handle, P_i64, c_i64, P_dbl]),
    "elph_shard_set_full_lattice": (c_int, [Handle, Handle]),
    "elph_shard_set_bonds": (c_int, [Handle, P_i64, c_i64, P_dbl]),
    "elph_shard_ghost_stats": (c_int, [Handle, P_i64, P_i64]),
    "elph_shard_ldiv": (c_int, [Handle, Handle, P_dbl, P_dbl, c_int, c_i64, P_i64, P_dbl, P_int]),
    "elph_shard_fermion_force_holstein": (c_int, [Handle, Handle, P_dbl, P_dbl, P_dbl, P_dbl, c_dbl, P_dbl, P_dbl, c_int, c_dbl, P_dbl, P_dbl,
                                                  P_dbl, P_i64, P_int]),
    "elph_shard_fermion_force_ssh": (c_int, [Handle, Handle, P_dbl, P_dbl, c_int, c_dbl, P_dbl, P_dbl, P_dbl, P_i64, P_int]),
}

# private measurement hooks (csrc/elph_bench.h: exported by the library, not part of the drop-in ABI; bench.py and tools/ use them)
BENCH_SIGNATURES = {
    "elph_shard_iterate": (c_int, [Handle, P_dbl, c_i64, P_dbl]),
    "elph_bench_prepare": (c_int, [Handle, c_int, c_int, P_dbl]),
    "elph_bench_run": (c_int, [Handle, c_int, c_int, c_int, c_int, P_dbl]),
    "elph_bench_get_x": (c_int, [Handle, c_int, P_dbl]),
    "elph_bench_msolve_pair": (c_int, [Handle, c_int, c_int, c_int, c_int, P_dbl, P_i64]),
    "elph_bench_info": (c_int, [Handle, c_int, P_int]),
    "elph_bench_wg_info": (c_int, [Handle, c_int, P_int, P_int, P_int, P_int]),
    "elph_bench_px_info": (c_int, [Handle, P_int]),
    "elph_bench_pg_info": (c_int, [Handle, P_int, P_int, P_int, P_int, P_int]),
    "elph_bench_pg_chunks": (c_int, [c_int, c_int, c_int, c_int, c_int, c_i64, c_i64, P_int]),
    "elph_bench_pg_chunk_info": (c_int, [Handle, c_int, c_int, P_int]),
    "elph_bench_slabs_info": (c_int, [Handle, c_int, P_int, P_int, P_int, P_int]),
    "elph_bench_lattice_shape": (c_int, [c_int, c_i64, c_i64, P_i64, P_dbl, P_dbl, P_int]),
    "elph_bench_wg_plan": (c_int, [c_int, c_i64, c_i64, c_i64, P_i64, P_dbl, P_dbl, c_int, c_int, P_int]),
    "elph_bench_dft_plan": (c_int, [c_i64, c_int, c_int, c_int, c_int, c_int, P_int]),
    "elph_bench_dft_info": (c_int, [Handle, c_int, c_int, c_int, c_int, c_int, P_int]),
    "elph_bench_kpm_plan": (c_int, [c_i64, c_dbl, c_dbl, c_dbl, c_int, c_int, P_dbl, P_int, P_int, P_dbl, P_int, P_int, P_int, P_dbl,
                                    P_dbl, P_dbl, c_i64, P_i64]),
    "elph_bench_hess_max_real": (c_int, [Handle, c_int, c_int, c_int, P_dbl, P_dbl]),
    "elph_bench_kpm_bounds": (c_int, [Handle, c_int, P_dbl, P_dbl, P_dbl, P_int]),
    "elph_bench_greens_noise": (c_int, [Handle, c_int, c_i64, C.c_uint64, c_int, P_dbl, c_i64, c_i64, P_dbl]),
    "elph_bench_kpm_side_info": (c_int, [Handle, P_int]),
}

# the slots of elph_bench_lattice_shape's vector, in order (elph_bench.h)
LATTICE_SHAPE_SLOTS = ("sq_LX", "sq_LY", "sq_dpp", "hc_LX", "hc_LY", "hc12", "patch_kind", "patch_L", "patch_PX", "patch_PY", "patch_NW",
                       "grid_GX", "grid_GY", "hgrid_regs", "hop_uniform", "bond_map")


def lattice_shape(kind, nsites, table, cosht=None, sinht=None):
    """What the library recognises in a checkerboard-ordered bond table (1-based, (nbonds, 2)), as {slot: value}.  Needs no device."""
    lib = load()
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 2)
    c = None if cosht is None else np.ascontiguousarray(cosht, dtype=np.float64)
    s = None if sinht is None else np.ascontiguousarray(sinht, dtype=np.float64)
    out = (c_int * len(LATTICE_SHAPE_SLOTS))()
    check(lib.elph_bench_lattice_shape(int(kind), int(nsites), table.shape[0], iptr(table) if table.size else None,
                                       None if c is None else dptr(c), None if s is None else dptr(s), out))
    return dict(zip(LATTICE_SHAPE_SLOTS, list(out)))


# the kernels of elph_bench_pg_chunks / elph_bench_pg_chunk_info (elph_bench.h)
PG_KERNELS = {"mul": 0, "cg_ap": 1, "cg_ap_px": 2}


def pg_chunks(kernel, px, py, nw, honeycomb, nvec, ltau):
    """(T, chunks per vector, slices of the last chunk) of one launch of a patch mat-vec kernel ("mul", "cg_ap", "cg_ap_px") of nvec vectors in the
    launch shape (px, py, nw, honeycomb or not) on ltau time slices, under ELPH_PG_T of the environment.  Needs no device."""
    out = (c_int * 3)()
    check(load().elph_bench_pg_chunks(PG_KERNELS[kernel], int(px), int(py), int(nw), int(bool(honeycomb)), int(nvec), int(ltau), out))
    return tuple(out)


def pg_chunk_info(handle, kernel, nvec):
    """{px, py, nw, T, chunks, last, taken}: the launch shape and the chunking this handle would take now for nvec vectors through `kernel`, and
    whether its mat-vecs and streaming CG iteration run the patch kernels at all."""
    out = (c_int * 7)()
    check(load().elph_bench_pg_chunk_info(handle, PG_KERNELS[kernel], int(nvec), out))
    return dict(zip(("px", "py", "nw", "T", "chunks", "last", "taken"), list(out)))


# the slots of elph_bench_wg_plan's vector, in order (elph_bench.h); WG_FORMS: the numbers of its "form" slot (cg_wg.hip: wg::Form)
WG_PLAN_SLOTS = ("usable", "form", "npl", "T", "W", "G", "shm", "resident", "has_kernel")
WG_FORMS = {"LANE": 0, "SQ16": 1, "HC12": 2, "S8": 4, "GRID": 5, "HGRID": 6, "TGRID": 7}


def wg_plan(kind, nsites, ltau, table, cosht=None, sinht=None, nrhs=1, world=0):
    """The resident CG launch a handle made from this bond table plans for nrhs right-hand sides (world > 0: as one rank of a sharded solve
    over that many), as {slot: value}.  Reads the ELPH_*WG* switches of the environment as a solve does.  Needs no device."""
    lib = load()
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 2)
    c = None if cosht is None else np.ascontiguousarray(cosht, dtype=np.float64)
    s = None if sinht is None else np.ascontiguousarray(sinht, dtype=np.float64)
    out = (c_int * len(WG_PLAN_SLOTS))()
    check(lib.elph_bench_wg_plan(int(kind), int(nsites), int(ltau), table.shape[0], iptr(table) if table.size else None,
                                 None if c is None else dptr(c), None if s is None else dptr(s), int(nrhs), int(world), out))
    return dict(zip(WG_PLAN_SLOTS, list(out)))


# the slots of elph_bench_dft_plan's vector, in order (elph_bench.h); DFT_FORMS: the numbers of its "form" slots (elph_internal.h: DftForm)
DFT_PLAN_SLOTS = ("form", "nt", "groups", "lds", "slots", "xr", "px", "fold", "short_slots", "pair_form")
DFT_FORMS = {"SCALAR": 0, "ONE_TILE": 1, "DIRECT": 2, "SPLIT_REG": 3, "SPLIT_LDS": 4, "BIG_ROW": 5, "BIG_BLOCKED": 6, "BIG_DIRECT": 7}


def dft_plan(ltau, which, inverse, N, nvec, nrz_slots=0, handle=None):
    """The plan of one tau-axis transform (which: 0 twisted, 1 plain) of nvec vectors of N columns under the ELPH_DFT_* / ELPH_FUSE_* switches of
    the environment, as {slot: value}: on a time axis of ltau slices without a device, or (handle given) from that handle's own record."""
    lib = load()
    out = (c_int * len(DFT_PLAN_SLOTS))()
    args = (int(which), int(bool(inverse)), int(N), int(nvec), int(nrz_slots), out)
    check(lib.elph_bench_dft_plan(int(ltau), *args) if handle is None else lib.elph_bench_dft_info(handle, *args))
    return dict(zip(DFT_PLAN_SLOTS, list(out)))


KPM_SIDE_SLOTS = ("cbs", "npl", "lds_tables", "refused", "ms_block")


def kpm_side_info(handle):
    """The launch shape of the one-sided KPM apply and of the BiCGStab / GMRES vector kernels on a handle (elph_bench_kpm_side_info), as
    {slot: value}."""
    out = (c_int * len(KPM_SIDE_SLOTS))()
    check(load().elph_bench_kpm_side_info(handle, out))
    return dict(zip(KPM_SIDE_SLOTS, list(out)))


def kpm_plan(ltau, bounds, buf=0.05, c1=1.0, c2=1.0):
    """What setup!(P) plans at Ltau = ltau for successive steps of per-chain eigenvalue bounds, bounds[step][chain] = (e_min, e_max).  Needs no
    device.  Returns {"uploaded": [steps], and after the last step "active": [nch], "lam_lo", "lam_hi", "lam_avg", "lam_mag": [nch], "order",
    "wsched": [nch, Lo2], "coff": [nch, Lo2 + 1], "c0": [nch, Lo2] complex (schedule order), "fold": [nch, Lo2, 2], "coeff": complex}."""
    lib = load()
    eb = np.ascontiguousarray(bounds, dtype=np.float64)
    nsteps, nch = eb.shape[0], eb.shape[1]
    Lo2 = (int(ltau) + 1) // 2
    up, act = np.zeros(nsteps, dtype=np.int32), np.zeros(nch, dtype=np.int32)
    lam, order, wsched = np.zeros((nch, 4)), np.zeros((nch, Lo2), dtype=np.int32), np.zeros((nch, Lo2), dtype=np.int32)
    coff, c0, fold = np.zeros((nch, Lo2 + 1), dtype=np.int32), np.zeros((nch, Lo2, 2)), np.zeros((nch, Lo2, 2))
    n = C.c_int64()
    ip32 = lambda a: a.ctypes.data_as(P_int)  # noqa: E731
    args = [int(ltau), float(buf), float(c1), float(c2), nch, nsteps, dptr(eb), ip32(up), ip32(act), dptr(lam), ip32(order), ip32(coff),
            ip32(wsched), dptr(c0), dptr(fold)]
    check(lib.elph_bench_kpm_plan(*args, None, 0, C.byref(n)))
    coeff = np.zeros(n.value)
    check(lib.elph_bench_kpm_plan(*args, dptr(coeff), n.value, C.byref(n)))
    return dict(uploaded=up.astype(bool).tolist(), active=act.astype(bool).tolist(), lam_lo=lam[:, 0], lam_hi=lam[:, 1], lam_avg=lam[:, 2],
                lam_mag=lam[:, 3], order=order, wsched=wsched, coff=coff, c0=c0[..., 0] + 1j * c0[..., 1], fold=fold,
                coeff=coeff[0::2] + 1j * coeff[1::2])


def hess_max_real(mats, where=0, handle=None):
    """The largest real part of the eigenvalues of each upper-Hessenberg matrix of `mats` (all n x n) by the library's QR iteration: the host's
    (where = 0, needs no device) or the device's (where = 1, needs a handle); +inf where it did not converge."""
    lib = load()
    mats = [np.asarray(a, dtype=np.float64) for a in mats]
    n = mats[0].shape[0]
    assert all(a.shape == (n, n) for a in mats)
    A = np.ascontiguousarray(np.stack([a.T for a in mats]))          # column-major
    out = np.zeros(len(mats))
    check(lib.elph_bench_hess_max_real(handle, int(where), len(mats), n, dptr(A), dptr(out)))
    return out


def kpm_bounds(handle, nchains, b_max, b_min, where):
    """The raw Arnoldi bounds of the resident chains (elph_bench_kpm_bounds): ((nchains, 2) array of (e_min, e_max), ran_on_device).
    where: 0 host, 1 device (host where the kernel refuses), 2 as setup!(P) chooses."""
    lib = load()
    b_max, b_min = np.ascontiguousarray(b_max, dtype=np.float64), np.ascontiguousarray(b_min, dtype=np.float64)
    assert b_max.shape[0] == nchains and b_max.shape == b_min.shape
    e = np.zeros((nchains, 2))
    ran = c_int(-1)
    check(lib.elph_bench_kpm_bounds(handle, int(where), dptr(b_max), dptr(b_min), dptr(e), C.byref(ran)))
    return e, ran.value


class ElphError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"{ERRORS.get(code, code)}: {text}")
        self.code = code


_lib = None


def library_path():
    return _build.LIB


def load():
    """Load libelphgpu.so (once). Raises if it has not been built — there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with hipcc first (python -c 'import __graft_entry__ as g; g.build()'); "
                          "elphdynamics_amd has no CPU fallback")
    lib = C.CDLL(path)
    for name, (res, args) in list(SIGNATURES.items()) + list(BENCH_SIGNATURES.items()):
        fn = getattr(lib, name)   # AttributeError here == ABI mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.elph_abi_version() != ABI_VERSION:
        raise ImportError(f"{path} speaks ABI {lib.elph_abi_version()}, this binding was written for {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def check(code):
    if code != ELPH_OK:
        raise ElphError(code, load().elph_last_error().decode())


def dptr(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], "float64 C-contiguous array required"
    return a.ctypes.data_as(P_dbl)


def iptr(a):
    assert a.dtype == np.int64 and a.flags["C_CONTIGUOUS"], "int64 C-contiguous array required"
    return a.ctypes.data_as(P_i64)
