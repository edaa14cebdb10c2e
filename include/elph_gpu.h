/*
 * elph_gpu.h — C ABI of libelphgpu.so, the MI355X (gfx950) fermion-force solver for ElPhDynamics.
 *
 * This is the drop-in boundary for the reference's operator API.  The reference has
 * no FFI: its callers reach the path through Julia multiple dispatch on the model type
 * (Models.jl / IterativeSolvers.jl / KPMPreconditioners.jl / FourierAcceleration.jl).  Each entry
 * point below names the reference method it replaces (file:line under the reference's src/); the
 * Julia-side binding (`ccall`) a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no exceptions across the boundary.
 *   - Every function returns an int status: ELPH_OK (0) or a negative ELPH_E_* code.
 *     Solver outcomes (iterations, residual, flag 0/1/2) are out-parameters, exactly the tuple
 *     the reference's ldiv! returns (Models.jl:74,139) — non-convergence is NOT an error.
 *   - Host entry points take host pointers in the REFERENCE layout: flat double[Nsites*Ltau],
 *     tau fastest, idx = site*Ltau + tau (Utilities.jl:12-15); neighbour table int64[2*Nbonds],
 *     column-major 2 x Nbonds, 1-based, already in checkerboard order (HolsteinModels.jl:484-517).
 *     No host pointer is retained after return.
 *   - `_dev` twins take device pointers in the same reference layout and run on the handle's stream.
 *   - One handle = one model on one GPU; a handle is not reentrant (the reference's model is not
 *     either: shared scratch v', v'', v''', Models.jl:218,94).
 */
#ifndef ELPH_GPU_H
#define ELPH_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ELPH_OK 0
#define ELPH_E_ARG (-1)      /* bad argument / shape mismatch */
#define ELPH_E_HIP (-2)      /* HIP runtime error (elph_last_error() has the text) */
#define ELPH_E_STATE (-3)    /* call out of order (e.g. KPM apply before setup) */
#define ELPH_E_NOGPU (-4)    /* no usable gfx950 device */
#define ELPH_E_UNSUPPORTED (-5)

#define ELPH_MODEL_HOLSTEIN 0
#define ELPH_MODEL_SSH 1

typedef struct elph_handle_s *elph_handle;

/* Text of the last error on this thread (never NULL). */
const char *elph_last_error(void);

/* ABI version this header describes.  Bumped whenever an entry point is removed or changes meaning (2: round 4 removed the
 * elph_cgstep_*, elph_dev_buffer, elph_buffer_* exports and round 5 added elph_muldMdx_*); loaders check for EXACTLY the version they
 * were written against (julia/ElPhGPU.jl, elphdynamics_amd/_lib.py). */
#define ELPH_ABI_VERSION 2
/* ABI version of the loaded library. */
int elph_abi_version(void);
/* How this library was built: "libelphgpu abi=<ELPH_ABI_VERSION> src=<sha256 of csrc/ + include/, 16 hex digits> arch=gfx950 variant=... built=<UTC>
 * flags=... compiler=[hipcc --version]" — static storage.  elphdynamics_amd/build.py compares `src` with the sources at hand: a stale
 * shipped library is rebuilt, a current one reused; smoke() and bench.py print it so that a run's log names the code that ran. */
const char *elph_build_info(void);

/* Number of visible HIP devices (0 if none); does not create a context. */
int elph_device_count(void);

/* ---------------------------------------------------------------- model life cycle */

/* Replaces HolsteinModel / SSHModel construction + initialize_model!
 * (HolsteinModels.jl:192-314,484-517; SSHModels.jl:348-505) for the fields the path uses.
 *   kind            ELPH_MODEL_HOLSTEIN | ELPH_MODEL_SSH
 *   nsites, ltau    Nsites, Ltau (Ndim = nsites*ltau)
 *   nbonds          number of bonds (0 allowed: single-site deck, HolsteinModels.jl:486)
 *   neighbor_table  int64[2*nbonds], 1-based, checkerboard order (model.neighbor_table)
 *   cosht, sinht    Holstein: double[nbonds] (model.cosht/.sinht); may be NULL for SSH
 *                   (SSH matrix elements arrive through elph_update_model_ssh)
 *   device          HIP device ordinal
 * The colour boundaries are recomputed from the table (maximal runs of site-disjoint bonds),
 * which reproduces the reference's groups for any table produced by checkerboard_order!. */
int elph_create(elph_handle *out, int kind, int64_t nsites, int64_t ltau, int64_t nbonds,
                const int64_t *neighbor_table, const double *cosht, const double *sinht, int device);

/* Frees all device memory of the handle. */
int elph_destroy(elph_handle h);

/* Use an existing HIP stream (hipStream_t passed as void*; NULL = the handle's own stream). */
int elph_set_stream(elph_handle h, void *hip_stream);

/* Block until all work queued on the handle's stream has finished. */
int elph_synchronize(elph_handle h);

/* ---------------------------------------------------------------- update_model! */

/* update_model!(holstein) — HolsteinModels.jl:526-549:
 * expnDtauV[i,tau] = exp(-dtau*(lambda_i x + lambda2_i x^2 - mu_i)), computed on the device.
 * x: double[nsites*ltau] (reference layout); lambda, lambda2, mu: double[nsites]. */
int elph_update_model_holstein(elph_handle h, const double *x, const double *lambda,
                               const double *lambda2, const double *mu, double dtau);

/* Several independent phonon configurations (Markov chains; the reference runs them as separate processes with
 * run-IDs, ElPhDynamics.jl:90-95) resident in ONE handle: X is double[nchains*nsites*ltau], chain-major.  In a
 * subsequent batched solve / mat-vec right-hand side r uses the fermion matrix of chain r % nchains, so e.g.
 * nrhs = 2*nchains advances both pseudofermion solves of nchains HMC force evaluations together.  The KPM
 * preconditioner and the force call are per-configuration and require nchains == 1. */
int elph_update_model_holstein_chains(elph_handle h, int nchains, const double *X, const double *lambda,
                                      const double *lambda2, const double *mu, double dtau);

/* Same, but hands over an already exponentiated model.expnDtauV (double[nsites*ltau]). */
int elph_set_expV(elph_handle h, const double *expnDtauV);

/* update_model!(ssh) matrix elements — SSHModels.jl:510-535 (computed by the caller):
 * cosht, sinht: double[ltau*nbonds], Julia (Ltau x Nbonds) column-major (tau fastest),
 * already in checkerboard column order; expDtauMu: double[nsites]. */
int elph_update_model_ssh(elph_handle h, const double *cosht, const double *sinht,
                          const double *expDtauMu);

/* Several independent phonon configurations (chains) of one SSH deck in one handle (the reference runs chains as separate
 * processes, ElPhDynamics.jl:90-95): X[nchains][nph*ltau]; the other arguments as elph_update_model_ssh_fields.  In a batched
 * call right-hand side r then uses the hopping tables of chain r % nchains. */
int elph_update_model_ssh_fields_chains(elph_handle h, int nchains, const double *X, int64_t nph, const int64_t *cb_index,
                                        const double *t_ph, const double *alpha, const double *alpha2, const double *t_bare_cb,
                                        const double *mu, double dtau);

/* update_model!(ssh) computed on the device from the phonon fields — SSHModels.jl:510-562: expΔτμ = exp(Δτ μ); per field
 * t′ = t − (α x + sign(x) α₂ x²), cosht[τ, index] = cosh(Δτ t′), sinht likewise (no host cosh/sinh, no tables over PCIe).
 *   x         double[nph * ltau]  ssh.x (field = (phonon−1)·Lτ + τ)
 *   cb_index  int64[nph]          1-based checkerboard position of each phonon's bond: checkerboard_perm[phonon_to_bond[p]]
 *   t_ph, alpha, alpha2  double[nph]   ssh.t[bond of p], ssh.α, ssh.α₂
 *   t_bare_cb double[nbonds]      bare hopping of every bond in checkerboard order (bonds without a phonon keep cosh/sinh(Δτ t))
 *   mu        double[nsites]
 * elph_get_cosh_sinh: model.cosht / model.sinht as the reference stores them ((Lτ × Nbonds) column-major), for callers that
 * read those fields after a device-side update (Holstein handles: Nbonds values each). */
int elph_update_model_ssh_fields(elph_handle h, const double *x, int64_t nph, const int64_t *cb_index, const double *t_ph,
                                 const double *alpha, const double *alpha2, const double *t_bare_cb, const double *mu, double dtau);
int elph_get_cosh_sinh(elph_handle h, double *cosht, double *sinht);

/* ---------------------------------------------------------------- mul! family */

/* mulM!(y, model, v) — HolsteinModels.jl:569-626 / SSHModels.jl:581-640 */
int elph_mulM(elph_handle h, double *y, const double *v);
/* mulMᵀ!(y, model, v) — HolsteinModels.jl:631-684 / SSHModels.jl:646-701 */
int elph_mulMT(elph_handle h, double *y, const double *v);
/* mulMᵀM!(y, model, v) — Models.jl:215-224 (one fused kernel; no v' round trip) */
int elph_mulMTM(elph_handle h, double *y, const double *v);
/* mulMMᵀ!(y, model, v) — Models.jl:229-238 (the `transposed` branch of mul!, :192-209; only the non-CG solvers use it) */
int elph_mulMMT(elph_handle h, double *y, const double *v);
/* device-pointer twins (reference layout, handle's stream, asynchronous) */
int elph_mulM_dev(elph_handle h, double *y_dev, const double *v_dev);
int elph_mulMT_dev(elph_handle h, double *y_dev, const double *v_dev);
int elph_mulMTM_dev(elph_handle h, double *y_dev, const double *v_dev);

/* ---------------------------------------------------------------- solver */

/* ConjugateGradient fields — IterativeSolvers.jl:36-57 (model.solver.tol/.maxiter/.kmax). */
int elph_solver_set(elph_handle h, double tol, int64_t maxiter, double kappa_max);

/* solve!(x, model, b, cg[, P]; maxiter, tol, κmax) -> iters
 * IterativeSolvers.jl:239-314 (use_precond=0) / :153-234 (use_precond=1, KPM must be set up).
 * x is both the initial guess and the result (callers zero it: HMC.jl:854).
 * tol/maxiter/kappa_max of 0 select the handle's solver defaults (as iszero() does there).
 * eps_hist (optional, may be NULL): receives eps_0..eps_iters (needs maxiter+1 doubles). */
int elph_cg_solve(elph_handle h, double *x, const double *b, double tol, int64_t maxiter,
                  double kappa_max, int use_precond, int64_t *iters, double *eps_hist);

/* ldiv!(x, model, b, P; maxiter=0) -> (iters, residual_error, flag) — Models.jl:74-137 (use_precond=1)
 * and Models.jl:139-186 (use_precond=0): solve, true residual ‖Ax−b‖/‖b‖, flag 0/1/2 with x zeroed
 * when flag>0, and the un-preconditioned retry with 10*maxiter. */
int elph_ldiv(elph_handle h, double *x, const double *b, int use_precond, int64_t maxiter,
              int64_t *iters, double *residual_error, int *flag);

/* Batched ldiv!: nrhs independent right-hand sides of the same matrix advanced together
 * (φ₊/φ₋ of calc_O⁻¹Λϕ!, HMC.jl:851-886; the nᵥ vectors of GreensFunctions.update!, :201-234).
 * X, B: double[nrhs*ndim], RHS-major; iters/residual_error/flag: arrays of nrhs.
 * Each RHS follows exactly the single-RHS recurrences and stop rule. */
int elph_ldiv_batched(elph_handle h, int nrhs, double *X, const double *B, int use_precond,
                      int64_t maxiter, int64_t *iters, double *residual_error, int *flag);

/* device-pointer twins (reference layout) */
int elph_ldiv_dev(elph_handle h, double *x_dev, const double *b_dev, int use_precond,
                  int64_t maxiter, int64_t *iters, double *residual_error, int *flag);
int elph_ldiv_batched_dev(elph_handle h, int nrhs, double *X_dev, const double *B_dev,
                          int use_precond, int64_t maxiter, int64_t *iters,
                          double *residual_error, int *flag);

/* ---------------------------------------------------------------- fermion force */

/* One fermion-force evaluation of the Holstein model with the phonon field, both pseudofermion fields and both
 * solutions resident on the device between the steps:
 *   update_model!(model)                                   HolsteinModels.jl:526-549
 *   calc_O⁻¹Λϕ!(hmc, model, P, power)                      HMC.jl:820-915  (Λ: :921-968; two solves as one batch,
 *                                                          tolerance tol^power, iters = cld(total,2), flag)
 *   calc_dSfdx!(hmc, model)                                HMC.jl:790-814  (mulM!, muldMdx! HolsteinModels.jl:691-755,
 *                                                          muldΛdx! HMC.jl:1005-1025)
 * dSfdx is ACCUMULATED into (the reference adds the fermionic force to hmc.dSdx).  Xp_out / Xm_out (optional)
 * receive O⁻¹Λϕ₊ / O⁻¹Λϕ₋.  use_precond needs elph_kpm_setup on the *updated* field, so preconditioned callers
 * call elph_update_model_holstein + elph_kpm_setup first (setup! runs inside calc_O⁻¹Λϕ!, HMC.jl:834). */
int elph_fermion_force_holstein(elph_handle h, const double *x, const double *lambda, const double *lambda2,
                                const double *mu, double dtau, const double *phi_plus, const double *phi_minus,
                                int use_precond, double tol_power, double *dSfdx, double *Xp_out, double *Xm_out,
                                int64_t *iters, int *flag);

/* The same for the SSH model (bond phonons): the two solves of calc_O⁻¹Λϕ! on the given right-hand sides (Λ is the
 * identity for SSH, HMC.jl:943-946,970-973, so the caller passes hmc.Λϕ₊/Λϕ₋ = MᵀR±) and the bond-local part of
 * muldMdx! (SSHModels.jl:707-829) fused with mulM! (HMC.jl:797-806):
 *   q_out[n*Ltau + tau] = sum_± ( c_j b_i + c_i b_j ) for checkerboard bond n (tau fastest), so that
 *   dMdx[field(phonon(n), tau)] = sg(tau) * dtau * (alpha + 2 alpha2 x) * q_out[...],   sg(1) = -1, else +1,
 * which the caller scatters to the phonon fields (primary_field bookkeeping stays on the host) and SUBTRACTS from
 * dSdx (HMC.jl:803,808).  elph_update_model_ssh must have been called for the current field. */
int elph_fermion_force_ssh(elph_handle h, const double *rhs_plus, const double *rhs_minus, int use_precond,
                           double tol_power, double *q_out, double *Xp_out, double *Xm_out, int64_t *iters, int *flag);

/* As elph_fermion_force_ssh, with the scatter onto the phonon fields done on the device as well:
 *   dSdx[(p−1)·Lτ + τ] −= sg(τ)·Δτ·(α_p + 2 α₂_p x)·q[τ][bond(p)]      (SSHModels.jl:797-823, HMC.jl:803,808)
 * for the fields x, couplings and checkerboard positions of the last elph_update_model_ssh_fields call (one field per
 * bond and τ; the reference's primary_field aliasing of equivalent fields stays with the caller).  dSdx: double[nph·Lτ],
 * accumulated into. */
int elph_fermion_force_ssh_fields(elph_handle h, const double *rhs_plus, const double *rhs_minus, int use_precond,
                                  double tol_power, double *dSdx, double *Xp_out, double *Xm_out, int64_t *iters, int *flag);

/* muldMdx!(dMdx, u, model, v): dMdx[field] = uᵀ·(∂M/∂x_field)·v for caller-given u and v — the L3 operator that calc_dSfdx! applies
 * to (u, v) = (M·O⁻¹Λϕ±, O⁻¹Λϕ±) (HMC.jl:799,804) and LangevinDynamics.calc_dSfdx! to (g, M⁻¹g) (:378).  The matrix is the handle's
 * current one (the last update_model).
 *   Holstein (HolsteinModels.jl:691-755): dMdx[i,τ] = [CBᵀu](i,τ) · sg(τ) Δτ (λ_i + 2 λ₂_i x(i,τ)) e^{-ΔτV}(i,τ) · v(i,τ−1), sg(1) = −1 with
 *   v(i,0) = v(i,Lτ); x, u, v, dMdx: double[Ndim], reference layout; lambda, lambda2: double[nsites] (host arrays in both forms). */
int elph_muldMdx_holstein(elph_handle h, double *dMdx, const double *u, const double *v, const double *x,
                          const double *lambda, const double *lambda2, double dtau);
int elph_muldMdx_holstein_dev(elph_handle h, double *dMdx_dev, const double *u_dev, const double *v_dev, const double *x_dev,
                              const double *lambda, const double *lambda2, double dtau);
/*   SSH (SSHModels.jl:707-829), bond-local part: q_out[n·Lτ + τ] = c_j b_i + c_i b_j for checkerboard bond n (τ fastest) with
 *   b = the partial forward product of e^{Δτμ}v(τ−1), c = the partial inverse product of CBᵀu, both after bond n (:775-806), so that
 *   dMdx[primary_field[field(phonon(n), τ)]] += sg(τ) Δτ (α + 2 α₂ x) q_out[...]  (:797-823) is the caller's scatter — as for
 *   elph_fermion_force_ssh.  Works after either elph_update_model_ssh or elph_update_model_ssh_fields. */
int elph_muldMdx_ssh(elph_handle h, double *q_out, const double *u, const double *v);
/*   SSH with the scatter on the device, for the fields, couplings and bond positions of the last elph_update_model_ssh_fields:
 *   dMdx[(p−1)·Lτ + τ] = sg(τ) Δτ (α_p + 2 α₂_p x) q[τ][bond(p)], double[nph·Lτ]; the primary_field sum over equivalent fields
 *   (:820-826) stays with the caller. */
int elph_muldMdx_ssh_fields(elph_handle h, double *dMdx, const double *u, const double *v);
int elph_muldMdx_ssh_fields_dev(elph_handle h, double *dMdx_dev, const double *u_dev, const double *v_dev);

/* ---------------------------------------------------------------- HMC trajectory */

/* One HMC update of the Holstein model, update!(model, hmc, fa, P) — HMC.jl:313-337 — i.e. standard_update!
 * (:343-463, nb == 1) or multitimestep_update! (:469-638, nb > 1), with refresh_v!/refresh_ϕ! (:648-692), calc_H
 * (:697-784), calc_Sb/calc_dSbdx! (PhononAction.jl:11-66,114-187), calc_O⁻¹Λϕ! and calc_dSfdx! inside.  The phonon
 * field x, the velocity v, ϕ±, O⁻¹Λϕ± and dS/dx stay on the device for the whole trajectory and between updates.
 *
 * elph_hmc_create: per-site omega, omega4, lambda, lambda2, mu (double[nsites]), dtau, and FourierAccelerator.M
 *   (fa_mass: double[nsites*ltau], frequency index fastest — FourierAcceleration.jl:222-240).  Dispersive phonon modes
 *   are not supported (the reference's calc_Sb reads an undefined variable for them, PhononAction.jl:49).
 * elph_hmc_set_state / get_state: model.x and hmc.v (double[nsites*ltau], tau fastest; NULL = leave / skip).
 * elph_hmc_update: dt = hmc.Δt, nt = hmc.Nt, nb = hmc.Nb, alpha = partial momentum refresh.  The random numbers the
 *   reference draws from model.rng are inputs: R[Ndof] (refresh_v!), Rp, Rm [Ndim] (refresh_ϕ!), kpm_randn[(nt+2)*2*nsites]
 *   (the Arnoldi start vector pairs of the up to nt+2 setup!(P) calls, in call order; NULL without preconditioner) and
 *   u_accept (the uniform of the Metropolis test, :441).  Solver settings are elph_solver_set's (tol^2 for the two
 *   action evaluations, tol for the forces, :373,:398,:428).
 *   Outputs: accepted (0/1); iters_per_solve = cld(iters, nt+2) as the reference returns; energies[5] = H0, H1,
 *   S and K of the last calc_H, acceptance probability; flag = last linear-solve flag (> 0: trajectory killed, rejected).
 *   On rejection x is restored, v = -v0 and exp(-dtau V) is rebuilt (:447-456). */
int elph_hmc_create(elph_handle h, const double *omega, const double *omega4, const double *lambda, const double *lambda2,
                    const double *mu, double dtau, const double *fa_mass);
int elph_hmc_set_state(elph_handle h, const double *x, const double *v);
int elph_hmc_get_state(elph_handle h, double *x, double *v);
int elph_hmc_update(elph_handle h, double dt, int64_t nt, int nb, double alpha, int use_precond, const double *R,
                    const double *Rp, const double *Rm, const double *kpm_randn, double u_accept, int *accepted,
                    double *iters_per_solve, double *energies, int *flag);

/* The same trajectory for an SSH model (bond phonons; SURVEY config E): the fields are the Nph·Lτ bond-phonon displacements,
 * update_model! is the device-side cosh/sinh of t′ = t − (αx + sign(x)α₂x²) (SSHModels.jl:510-562), Λ ≡ 1
 * (HMC.jl:943-946), the force is −dMdx(M X±, X±) scattered from the bond brackets (SSHModels.jl:707-829), calc_Sb /
 * calc_dSbdx! are PhononAction.jl:68-112,189-234 with every field its own primary field.  elph_hmc_create_ssh replaces
 * elph_hmc_create (omega, omega4: double[nph]; fa_mass: double[nph·Lτ]; the other arguments as in
 * elph_update_model_ssh_fields); elph_hmc_set_state / _get_state / elph_hmc_update then work on double[nph·Lτ] fields
 * (R: [nph·Lτ]; Rp, Rm: [Ndim]). */
int elph_hmc_create_ssh(elph_handle h, int64_t nph, const double *omega, const double *omega4, const int64_t *cb_index,
                        const double *t_ph, const double *alpha, const double *alpha2, const double *t_bare_cb, const double *mu,
                        double dtau, const double *fa_mass);
/* The same for nchains independent chains of one SSH deck in lockstep (x, v, R chain-major as for elph_hmc_create_chains;
 * elph_hmc_update_chains / elph_langevin_evolve then act on all of them; special moves stay single-chain). */
int elph_hmc_create_ssh_chains(elph_handle h, int nchains, int64_t nph, const double *omega, const double *omega4,
                               const int64_t *cb_index, const double *t_ph, const double *alpha, const double *alpha2,
                               const double *t_bare_cb, const double *mu, double dtau, const double *fa_mass);

/* Several Markov chains (same deck, independent phonon fields — the reference runs them as separate processes,
 * ElPhDynamics.jl:90-95) advanced in LOCKSTEP by one handle: the leapfrog schedule is common, every chain has its own
 * x, v, ϕ±, energies, Metropolis test and failure flag, and all 2·nchains pseudofermion solves of a force / action
 * evaluation run as ONE batched CG (with use_precond: one KPM expansion per chain, elph_kpm_setup_chains).
 * elph_hmc_create_chains replaces elph_hmc_create; elph_hmc_set_state / _get_state then move double[nchains * ndim]
 * (chain-major).  elph_hmc_update_chains: R [nchains*Ndof], Rp, Rm [nchains*Ndim] chain-major;
 * kpm_randn [(nt+2)][2 (b_max, b_min)][nchains][nsites]; u_accept, accepted, iters_per_solve, flag [nchains];
 * energies [nchains][5].  A chain whose linear solve fails is rejected (flag > 0) without stopping the others. */
int elph_hmc_create_chains(elph_handle h, int nchains, const double *omega, const double *omega4, const double *lambda,
                           const double *lambda2, const double *mu, double dtau, const double *fa_mass);
int elph_hmc_update_chains(elph_handle h, double dt, int64_t nt, int nb, double alpha, int use_precond, const double *R,
                           const double *Rp, const double *Rm, const double *kpm_randn, const double *u_accept, int *accepted,
                           double *iters_per_solve, double *energies, int *flag);

/* model.μ changed while the field lives on the device (the chemical-potential tuner, MuFinder.jl:68-107 adds Δμ to every site):
 * new μ[nsites] for the HMC / Langevin state, followed by update_model!. */
int elph_hmc_set_mu(elph_handle h, const double *mu);
/* chains in lockstep, each with its own tuner: mu[nchains][nsites] (elph_hmc_set_mu / a new elph_hmc_create* return to one μ) */
int elph_hmc_set_mu_chains(elph_handle h, const double *mu);

/* SSH phonon types of the same name (the default "" included) share their fields: primary_field of initialize_model!
 * (SSHModels.jl:480-502).  primary_column[Nph]: 0-based column of the primary phonon of every phonon (itself for a primary; the
 * sharing is the same on every time slice).  Call after elph_hmc_create_ssh / elph_langevin_create_ssh.  Then, as in the
 * reference: the fermion force of a class is summed over its members and given to each (muldMdx!, :820-826), calc_Sb and
 * calc_K count primary fields only (PhononAction.jl:83, HMC.jl:720-738), elph_hmc_set_state refuses fields that differ
 * from their primary (update_model!, :549-559), generated random field vectors are copied from their primaries (randn!,
 * :568-575; host-supplied R / eta must already be v[primary_field]); elph_hmc_special_move returns ELPH_E_UNSUPPORTED. */
int elph_hmc_set_shared_fields(elph_handle h, const int64_t *primary_column);

/* Optional on-device generator for the random inputs of elph_hmc_update[_chains], elph_hmc_special_move and
 * elph_langevin_evolve (the reference draws them from model.rng on the CPU: randn! HMC.jl:655,675-676, LangevinDynamics.jl:97,360,
 * KPMPreconditioners.jl:860,903; with 64 chains the host generator and the PCIe transfer of 3 x nchains vectors per update cost
 * a quarter of the update).  After elph_hmc_set_rng(h, seed) any of R, Rp, Rm, eta, g1, g2, kpm_randn, u_accept may be NULL
 * (u_accept < 0 where it is passed by value): each missing input is one batch of the build's counter-based generator
 * (SplitMix64 -> uniform(0,1) -> Box-Muller, elphdynamics_amd/synth.py), batch b (1-based, counted per handle since
 * elph_hmc_set_rng) seeded with output b of SplitMix64(seed), numbered in the layout the host array would have had — so a run
 * is reproducible from (seed, batch count) and equals the run that is handed synth.randn(batch seed, n) explicitly.  Field and
 * site vectors are generated on the device; Arnoldi start vectors and Metropolis uniforms (small) on the host.  Order of the
 * batches within a call: HMC update R, Rp, Rm, kpm_randn, u_accept; special move Rp, Rm, kpm_randn, u_accept; every move of
 * elph_hmc_special_update_chains draw, Rp, Rm, kpm_randn, u_accept; Langevin step eta, kpm_randn, g1, g2. */
int elph_hmc_set_rng(elph_handle h, uint64_t seed);
int elph_hmc_rng_batches(elph_handle h, uint64_t *batches);

/* One proposed move of special_update! (SpecialUpdates.jl:103-136 ReflectionUpdate, :205-275 SwapUpdate) on the device-resident
 * field of the (single-chain) HMC state:  S₀ = refresh_ϕ!(…, sample_R = true) with the fresh R± = Rp, Rm (HMC.jl:665-692);
 * kind 0: x_col(τ) → −x_col(τ) on phonon column col_i; kind 1: columns col_i, col_j exchange their world lines (0-based; sites
 * for Holstein, bond phonons for SSH); update_model!, calc_O⁻¹Λϕ!(…, 2.0), S₁ = calc_S; accepted iff u_accept <
 * min(1, e^{−(S₁−S₀)}) and flag == 0, else the move is undone.  kpm_randn: [2][nsites] or NULL.  Which sites / bonds are tried
 * (sample!(model.rng, …)) is the caller's bookkeeping. */
int elph_hmc_special_move(elph_handle h, int kind, int64_t col_i, int64_t col_j, const double *Rp, const double *Rm, int use_precond,
                          const double *kpm_randn, double u_accept, int *accepted, double *S0, double *S1, int64_t *iters, int *flag);
/* The same for chains in lockstep: every chain proposes its own move (col_i[c], col_j[c]) on its own field, one batched action
 * evaluation serves all of them, acceptance is per chain (all arrays [nchains]; Rp, Rm chain-major like elph_hmc_update_chains;
 * kpm_randn [2][nchains][nsites]). */
int elph_hmc_special_move_chains(elph_handle h, int kind, const int64_t *col_i, const int64_t *col_j, const double *Rp,
                                 const double *Rm, int use_precond, const double *kpm_randn, const double *u_accept,
                                 int *accepted, double *S0, double *S1, int64_t *iters, int *flag);
/* special_update! itself for every chain of the HMC state (SpecialUpdates.jl:97-366; the draws it replaces: :113 the site of a
 * reflection, :248-258 the bond of a Holstein swap, :324-328 the phonon pair of an SSH swap): nmoves moves in one call, the columns
 * drawn on the device by the generator of elph_hmc_set_rng (required: ELPH_E_STATE without it), the Metropolis test decided there.
 * kind 0 reflection, 1 swap.  Batches per move: draw, Rp, Rm, [kpm_randn], u_accept; the last four as the move entry above lays
 * them out.  The draw batch: chain c takes u0 = uniform 2c and u1 = uniform 2c + 1; with pick(u, n) = min(floor(u n), n - 1):
 *   reflection      column pick(u0, Nph);
 *   Holstein swap   the two sites of bond pick(u0, nbonds) of the handle's neighbor table;
 *   SSH swap        i = pick(u0, Nph); D = the columns, in increasing order, whose world line is not isapprox that of i
 *                   (|x_i - x_q| <= sqrt(eps) max(|x_i|, |x_q|) in the 2-norm); j = D[pick(u1, |D|)], and j = i when D is empty:
 *                   the move is then the identity and is evaluated like any other (the reference's while loop would not end).
 * Outputs are [nmoves][nchains]: accepted; col_i, col_j the 0-based columns drawn (col_j = col_i for a reflection); S0, S1; iters,
 * flag of the move's two solves — all but accepted may be NULL.  Per move the number of launches and of copies does not depend on
 * the number of chains and no field vector leaves the device.  Shared fields, sharded lattices and slab handles:
 * ELPH_E_UNSUPPORTED. */
int elph_hmc_special_update_chains(elph_handle h, int kind, int64_t nmoves, int use_precond, int *accepted, int64_t *col_i,
                                   int64_t *col_j, double *S0, double *S1, int64_t *iters, int *flag);

/* ---------------------------------------------------------------- Langevin dynamics (caller of the path) */

/* LangevinDynamics.jl on a Holstein handle.  elph_langevin_create: the arguments of elph_hmc_create with
 * fa_Q = FourierAccelerator.Q (evolve! calls fourier_accelerate! without use_mass); the field moves through
 * elph_hmc_set_state / elph_hmc_get_state (v = NULL).
 * elph_langevin_evolve = evolve!(model, dyn, fa, P): scheme 0 EulerDynamics (:81-130), 1 RungeKuttaDynamics (:162-232),
 * 2 HeunsDynamics (:272-328), with calc_dSdx! (:334-384: one solve MᵀM x = Mᵀg, dSf/dx = −2 gᵀ(∂M/∂x)M⁻¹g via muldMdx!
 * HolsteinModels.jl:691-755, plus the shifted calc_dSbdx!) on the device.  The random numbers are inputs: eta [Ndof], g1, g2
 * [Ndim] (g2 unused by Euler), kpm_randn [2][2][nsites] (b_max, b_min per setup!(P)).  iters: what evolve! returns; flag:
 * the last ldiv! flag (the reference ignores it). */
int elph_langevin_create(elph_handle h, const double *omega, const double *omega4, const double *lambda, const double *lambda2,
                         const double *mu, double dtau, const double *fa_Q);
/* SSH handles (examples/ssh_langevin_square.toml): the arguments of elph_hmc_create_ssh with fa_Q per phonon; eta has
 * nph·Lτ entries, calc_dSfdx! uses muldMdx! of SSHModels.jl:707-829 with u = g, and the shifted flag changes nothing. */
int elph_langevin_create_ssh(elph_handle h, int64_t nph, const double *omega, const double *omega4, const int64_t *cb_index,
                             const double *t_ph, const double *alpha, const double *alpha2, const double *t_bare_cb, const double *mu,
                             double dtau, const double *fa_Q);
/* nchains independent Langevin trajectories of one (Holstein) deck in lockstep: every step is one batched solve of nchains
 * right-hand sides with one KPM expansion per chain.  State and random vectors are chain-major (x, eta: [nchains·Ndof];
 * g1, g2: [nchains·Ndim]; kpm_randn: [2 set-ups][b_max | b_min][nchains][nsites]); elph_langevin_evolve then returns
 * iters and flag per chain ([nchains]). */
int elph_langevin_create_chains(elph_handle h, int nchains, const double *omega, const double *omega4, const double *lambda,
                                const double *lambda2, const double *mu, double dtau, const double *fa_Q);
int elph_langevin_evolve(elph_handle h, int scheme, double dt, int use_precond, const double *eta, const double *g1, const double *g2,
                         const double *kpm_randn, int64_t *iters, int *flag);

/* ---------------------------------------------------------------- Green's-function estimator */

/* EstimateGreensFunction(model, n_v) — GreensFunctions.jl:155-195.  norbits*L1*L2*L3 must equal nsites
 * (site = norbits*cell + orbit, cell = l1 + L1*(l2 + L2*l3), Lattices.jl:56-107).  n_v = max(2, nv) (:167). */
int elph_greens_create(elph_handle h, int norbits, int L1, int L2, int L3, int nv);
int elph_greens_nv(elph_handle h, int *nv);

/* update!(estimator, model, P) — GreensFunctions.jl:201-234: for every noise vector r (R: double[n_v * ndim], the
 * vectors the reference draws with randn!(model.rng, r₁), :212) solve MᵀM x = Mᵀ r from x = 0 with ldiv!'s semantics
 * (Models.jl:74-186; flags, zero-fill, un-preconditioned retry) — the n_v solves run as ONE batched CG.  R and M⁻¹R
 * stay on the device.  iters / residual_error / flag: per vector, each may be NULL.  With use_precond the caller has
 * run elph_kpm_setup on the current field (setup!(preconditioner), :206).  With several chains resident (elph_update_model_*_chains /
 * elph_hmc_create_*chains) row r of R belongs to chain r % nchains: create the estimator with n_v * nchains vectors and find
 * vector v of chain c at row v * nchains + c (elph_greens_setup then takes those 1-based indices). */
int elph_greens_update(elph_handle h, const double *R, int use_precond, int64_t *iters, double *residual_error, int *flag);

/* The estimator's own on-device generator, so that update! draws its randn!(R) (:212) where the solve runs: with 64 chains and n_v = 10
 * the host route draws 26 million normals and moves 210 MB in each direction per update.  elph_greens_set_rng gives the estimator a
 * generator of its own (ELPH_E_STATE before elph_greens_create; a new elph_greens_create returns it to having none): batch b (1-based,
 * counted since this call, independently of the HMC state's generator and its batch count) is seeded with output b of SplitMix64(seed),
 * as for elph_hmc_set_rng.  The HMC generator and the estimator's MUST get different seeds: with the same seed they produce the same
 * batches.  elph_greens_rng_batches: the batches drawn so far.
 * elph_greens_update_rng is elph_greens_update with R drawn on the device: ONE batch of n_v * ndim normals, numbered in the layout the
 * host array would have had ([n_v][ndim], tau fastest) — R equals synth.randn(batch seed, n_v * ndim).reshape(n_v, ndim) handed to
 * elph_greens_update — written straight into the estimator's R; no vector is copied to or from the host, and the call synchronises once.
 * Same chain-count rule (ELPH_E_ARG) and same outputs as elph_greens_update; ELPH_E_STATE without elph_greens_set_rng.  A refused call
 * draws no batch.  The KPM set-up stays the caller's call before it, with the caller's Arnoldi start vectors. */
int elph_greens_set_rng(elph_handle h, uint64_t seed);
int elph_greens_rng_batches(elph_handle h, uint64_t *batches);
int elph_greens_update_rng(elph_handle h, int use_precond, int64_t *iters, double *residual_error, int *flag);

/* estimator.R / estimator.M⁻¹R (double[n_v * ndim], vector-major, tau fastest); NULL = skip.  set: replay of vectors
 * produced elsewhere (both must have been given before elph_greens_setup). */
int elph_greens_set_vectors(elph_handle h, const double *R, const double *MinvR);
int elph_greens_get_vectors(elph_handle h, double *R, double *MinvR);

/* setup!(estimator, n₁, n₂) — GreensFunctions.jl:239-288 with convolve! (:351-400), antiperiodic_copy! (:406-418),
 * periodic_product! (:424-440); n₁, n₂ 1-based.  Outputs (NULL = not copied to the host), each
 * Complex{Float64}[2L, n_s, n_s, L1, L2, L3] as interleaved (re, im) doubles, first index fastest:
 *   GD0      G[Δ,0]            measure_GΔ0      (:293-298)  = array[mod1(τ+1,2L), o₂, o₁, l₁+1, l₂+1, l₃+1]
 *   GD0_GD0  G[Δ,0]·G[Δ,0]     measure_GΔ0_GΔ0  (:303-308)
 *   GDD_G00  G[Δ,Δ]·G[0,0]     measure_GΔΔ_G00  (:313-318)
 *   GD0_G0D  G[Δ,0]·G[0,Δ]     measure_GΔ0_G0Δ  (:324-329)
 * Imaginary parts are exact zeros (the reference's are FFT round-off, ~1e-17). */
int elph_greens_setup(elph_handle h, int n1, int n2, double *GD0, double *GD0_GD0, double *GDD_G00, double *GD0_G0D);

/* Device-resident results of the last elph_greens_setup: arrays[0..3] in the order above, `count` complex numbers each
 * (valid until the next elph_greens_setup / elph_greens_create / elph_destroy).  elph_meas_accumulate runs setup! for every pair of
 * vectors: after it these arrays hold the tables of the LAST pair (n_v - 1, n_v), not those of the caller's last elph_greens_setup. */
int elph_greens_dev_arrays(elph_handle h, void **arrays, int64_t *count);

/* ---------------------------------------------------------------- measurements (Holstein model; Measurements.jl) */

/* The device side of a measurements container (initialize_measurements_container, Measurements.jl:27-178, for what make_measurements!
 * adds up): accumulators for the global (density, Nsqr, mu; :845-861, :1283-1312), on-site (:916-976) and inter-site (el_ke, :1029-1070)
 * measurements and for the requested on-site correlations (:1469-1650), all doubles on the device.  Needs elph_greens_create first (n_s,
 * L1..L3 and n_v are the estimator's); a new elph_greens_create drops the container.
 *   omega, omega4, lambda, mu   double[nsites]: model.ω, .ω₄, .λ, .μ;  dtau: model.Δτ
 *   nbonds, ndef                nbonds = ndef * ncells bonds of ndef bond definitions, in the reference's bond order
 *                               bond = (definition - 1) * ncells + cell (:1048)
 *   bond_sites                  int64[2 * nbonds], column-major 2 x nbonds, 1-based: neighbor_table[:, checkerboard_perm[bond]] (:1050-1052)
 *   bond_t                      double[nbonds]: model.t[bond] (:1054)
 *   measure, time_dependent, npairs   int[5] for Greens, DenDen, SpinSpin, PairGreens, PhononGreens in this order: measured or not;
 *                               L_tau + 1 slices (tau = beta included) or the equal-time slice alone; number of orbital pairs
 *   pairs                       int[2 * sum of npairs over the measured ones]: their (o1, o2) lists one after the other, 1-based, in the
 *                               order the container keeps them (:776-782)
 * ELPH_E_ARG (an orbital outside 1..n_s, a bond site outside the lattice, a bond count that is not ndef * ncells) and
 * ELPH_E_UNSUPPORTED (SSH model, several chains resident, a sharded or slab handle) leave the handle without a container and usable. */
int elph_meas_create(elph_handle h, const double *omega, const double *omega4, const double *lambda, const double *mu, double dtau,
                     int64_t nbonds, int ndef, const int64_t *bond_sites, const double *bond_t, const int *measure,
                     const int *time_dependent, const int *npairs, const int *pairs);

/* make_measurements! (Measurements.jl:545-566) without its update!: the estimator holds vectors already (elph_greens_update or
 * elph_greens_set_vectors; ELPH_E_STATE otherwise).  x: model.x, double[ndim], reference layout.  For every pair i < j of the n_v vectors
 * the device part of setup! and the folds into the accumulators run on the handle's stream with no copy to the host and no
 * synchronisation in between; the call synchronises once before it returns.  Sums are taken in one fixed order without atomics: the
 * same inputs give the same bits. */
int elph_meas_accumulate(elph_handle h, const double *x);

/* The un-normalised sums since the last reset; one device-to-host copy, one synchronisation.  Each pointer may be NULL.
 *   scalars    double[3 + 9 n_s + ndef]: density, Nsqr, mu; then n_s values each of density, double_occ, x, x2, x4, phonon_pe,
 *              phonon_ke, elph_energy, mu; then el_ke per bond definition
 *   Greens … PhononGreens   Complex{Float64}[L0, L1, L2, L3, n_p] as interleaved (re, im) doubles, first index fastest, L0 = L_tau + 1 or 1:
 *              the container's `position` arrays (:786-790); imaginary parts are exact zeros.  Unmeasured ones are left untouched. */
int elph_meas_fetch(elph_handle h, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                    double *PhononGreens);

/* reset_measurements! (Measurements.jl:698-758): every accumulator to zero (stream-ordered). */
int elph_meas_reset(elph_handle h);

/* ---------------------------------------------------------------- measurements of resident chains (Holstein model; Measurements.jl) */

/* elph_meas_create for every chain resident in the handle (elph_update_model_holstein_chains, elph_hmc_create_chains): one container per
 * chain (initialize_measurements_container, Measurements.jl:27-178) in one device allocation [chain][scalars | Greens | DenDen | SpinSpin
 * | PairGreens | PhononGreens], beside (not inside) the container of elph_meas_create, and the scratch in which the estimator's setup!
 * (GreensFunctions.jl:239-288) runs for one pair of vectors of all chains at once.  The estimator serves the chains with
 * n_v * nchains vectors, vector v of chain c at index v * nchains + c (0-based).  Arguments as elph_meas_create, except
 *   nchains   >= 1 and equal to the number of chains resident in the handle (ELPH_E_ARG otherwise, naming both)
 *   mu        double[nchains * nsites], a row per chain: a tuner per chain moves it (elph_hmc_set_mu_chains); the global mu (:858) and
 *             the on-site mu (:970) of chain c come from row c
 * ELPH_E_ARG and ELPH_E_UNSUPPORTED (SSH model, a sharded or slab handle) as elph_meas_create: a refused request allocates nothing and
 * leaves the handle without this container and usable. */
int elph_meas_chains_create(elph_handle h, int nchains, const double *omega, const double *omega4, const double *lambda, const double *mu,
                            double dtau, int64_t nbonds, int ndef, const int64_t *bond_sites, const double *bond_t, const int *measure,
                            const int *time_dependent, const int *npairs, const int *pairs);

/* The chemical-potential tuners moved the chains' mu (MuFinder.jl:68-107: model.μ .= μ′ between two updates; elph_hmc_set_mu_chains for
 * the dynamics): mu, double[nchains * nsites], replaces the rows elph_meas_chains_create took, for the global mu (Measurements.jl:858) and
 * the on-site mu (:970) of the accumulates that follow.  The sums so far are kept. */
int elph_meas_chains_set_mu(elph_handle h, const double *mu);

/* make_measurements! (Measurements.jl:545-566) without its update!, for every chain: X is double[nchains * ndim], chain c's model.x in
 * the reference layout at X + c * ndim.  For every pair v1 < v2 of a chain's n_v vectors the device part of setup! and the folds run
 * once for all chains (the chain is a grid axis: the number of launches does not depend on nchains), stream-ordered, with one
 * synchronisation before the call returns.  Sums as elph_meas_accumulate: one fixed order, no atomics; chain c's numbers depend on chain
 * c's inputs alone.  ELPH_E_STATE: the handle no longer holds the number of chains the container was created for (after
 * elph_update_model_holstein, say), the estimator's vectors are not a multiple of it (the message names both counts), or it holds no
 * vectors yet. */
int elph_meas_chains_accumulate(elph_handle h, const double *X);

/* One chain's un-normalised sums since the last reset (process_measurements!, Measurements.jl:574-676, reads them): the outputs of
 * elph_meas_fetch for chain `chain` (0-based; ELPH_E_ARG outside 0..nchains-1).  One device-to-host copy, one synchronisation. */
int elph_meas_chains_fetch(elph_handle h, int chain, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                           double *PhononGreens);

/* reset_measurements! (Measurements.jl:698-758) of every chain: one memset (stream-ordered). */
int elph_meas_chains_reset(elph_handle h);

/* ---------------------------------------------------------------- density moments for the chemical-potential tuner (MuFinder.jl) */

/* <N> and <N^2> of every resident chain from the estimator's vectors, as update_mu! measures them for its tuner (MuFinder.jl:77-97;
 * measure_density and measure_N2, Measurements.jl:1283-1312), averaged over the binomial(n_v, 2) pairs of a chain's n_v vectors.  No setup!:
 * with C_pq(tau) = sum_site (M^-1 r_p)[site, tau] r_q[site, tau] the pair's T_p = (1/L) sum_tau C_pp(tau), N_p = 2 (N - T_p) and
 * N^2_pq = N_p N_q + T_p + T_q - (2/L) sum_tau C_pq(tau) C_qp(tau), the table's sum over every displacement at equal time, slice by slice.
 * One pass over R and M^-1 R on the handle's stream (two launches, stream-ordered), one device-to-host copy of 2 nchains doubles, one
 * synchronisation.  Holstein and SSH handles alike: only the vectors, nsites and L_tau enter.  Vector v of chain c is row v * nchains + c
 * (0-based) of the estimator.  Fixed summation order, no atomics: the same inputs give the same bits, and chain c's numbers depend on chain
 * c's rows alone.  The scratch (nchains L_tau n_v^2 doubles) is made on first use, regrown when the shape grows, dropped by
 * elph_greens_create and freed by elph_destroy.
 *   nchains   the number of chains resident in the handle (1 for one configuration); ELPH_E_ARG otherwise, naming both counts
 *   N, Nsqr   double[nchains] each
 *   ELPH_E_STATE         elph_greens_create has not been called; the estimator holds no vectors yet; its vector count is not a multiple
 *                        of nchains, or leaves a chain fewer than two vectors
 *   ELPH_E_UNSUPPORTED   a sharded or slab handle
 * A refused call leaves the handle usable. */
int elph_density_moments(elph_handle h, int nchains, double *N, double *Nsqr);

/* ---------------------------------------------------------------- snapshots (make_snapshot_measurements!, Measurements.jl) */

/* The density and double-occupancy snapshots of every resident chain from the estimator's vectors: the per-site profiles
 * take_density_snapshot! and take_double_occupancy_snapshot! write to one file per measurement (Measurements.jl:1351-1435).  With R and
 * M^-1 R viewed as (L_tau, nsites, n_v) and d_n(tau, i) = 1 - M^-1R[tau, i, n] R[tau, i, n]:
 *   density[i]          = sum_tau sum_{n = 1..n_v} 2 d_n                          / (n_v L_tau)
 *   double_occupancy[i] = sum_tau sum_{n = 1..n_v - 1} sum_{m = 2..n_v} d_n d_m   / (binomial(n_v, 2) L_tau)
 * The ranges of n and m are the reference's (:1416-1417): for n_v > 2 they hold n = m terms and both orders of some pairs, and so does
 * this call, through the double sum's product form (S - d_{n_v}) (S - d_1), S = sum_n d_n, per (tau, i).  One pass over R and M^-1 R on
 * the handle's stream (two launches, stream-ordered: partial sums over segments of the tau axis, then the segments in order), one
 * device-to-host copy per requested output, one synchronisation.  Holstein and SSH handles alike: only the vectors, nsites and L_tau
 * enter.  A chain's n_v is the estimator's vector count / nchains; vector v of chain c is row v * nchains + c (0-based).  Fixed summation
 * order, no atomics: the same inputs give the same bits; the segments depend on L_tau alone, so chain c's profiles depend on chain c's
 * rows alone and equal those of a single-configuration handle holding these rows.  The scratch (about nchains nsites L_tau / 2 doubles)
 * is made on first use, regrown when the shape grows, dropped by elph_greens_create and freed by elph_destroy.
 *   nchains      the number of chains resident in the handle (1 for one configuration); ELPH_E_ARG otherwise, naming both counts
 *   density      double[nchains * nsites], chain-major, sites in the handle's order, normalised; NULL: not wanted
 *   double_occ   the same for the double occupancy; NULL: not wanted.  Both NULL: ELPH_E_ARG
 *   ELPH_E_STATE         elph_greens_create has not been called; the estimator holds no vectors yet; its vector count is not a multiple
 *                        of nchains, or leaves a chain fewer than two vectors (binomial(1, 2) = 0: the reference would divide by zero)
 *   ELPH_E_UNSUPPORTED   a sharded or slab handle
 * A refused call leaves the handle usable.  (The phonon_position snapshot is the tau-mean of the field the caller holds: host arithmetic.) */
int elph_snapshots(elph_handle h, int nchains, double *density, double *double_occ);

/* ---------------------------------------------------------------- bond correlations (Holstein model; Measurements.jl) */

/* The device side of the inter-site correlation group of a measurements container (init_corr_container!, Measurements.jl:156-175,
 * :767-796): accumulators for BondBond (measure_BondBond!, :1663-1785) and BondPairGreens (measure_BondPairGreens!, :2390-2483), all
 * doubles on the device, beside (not inside) the container of elph_meas_create.  Needs elph_greens_create first (n_s, L1..L3 and n_v are
 * the estimator's); a new elph_greens_create drops it.
 *   n_def, o1, o2, v            model.bond_definitions: int[n_def] starting orbital Bond.o1, int[n_def] ending orbital Bond.o2 (1-based),
 *                               int[3 * n_def] displacement Bond.v in unit cells, definition-major
 *   measure, time_dependent, npairs   int[2] for BondBond, BondPairGreens in this order: measured or not; L_tau + 1 slices (tau = beta
 *                               included) or the equal-time slice alone; number of pairs of bond definitions
 *   pairs                       int[2 * sum of npairs over the measured ones]: their (pairs[1,p], pairs[2,p]) lists one after the other,
 *                               1-based indices of bond definitions, in the order the container keeps them (:776-782)
 * ELPH_E_ARG (an orbital outside 1..n_s, a bond index outside 1..n_def; the message names the correlation or definition and the
 * offending index) and ELPH_E_UNSUPPORTED (SSH model, several chains resident, a sharded or slab handle, a lattice whose frequency
 * slice does not fit the LDS) leave the handle without bond accumulators and usable. */
int elph_bond_create(elph_handle h, int n_def, const int *o1, const int *o2, const int *v, const int *measure, const int *time_dependent,
                     const int *npairs, const int *pairs);

/* The calls to measure_BondBond! / measure_BondPairGreens! of make_intersite_measurements! for every pair i < j of the estimator's n_v
 * vectors (elph_greens_update or elph_greens_set_vectors first; ELPH_E_STATE otherwise): per pair the device part of setup! (for G[D,0]
 * of the delta terms), the fields of shifted vectors, their transforms, one inverse transform per listed pair and correlation, and the
 * fold into the accumulators, on the handle's stream with no copy and no synchronisation in between; the call synchronises once before
 * it returns.  No atomics: the same inputs give the same bits.  Afterwards elph_greens_dev_arrays holds the tables of the LAST pair. */
int elph_bond_accumulate(elph_handle h);

/* The un-normalised sums since the last reset; one device-to-host copy, one synchronisation.  Each pointer may be NULL.
 *   BondBond, BondPairGreens   Complex{Float64}[L0, L1, L2, L3, n_p] as interleaved (re, im) doubles, first index fastest, L0 = L_tau + 1
 *              or 1: the container's `position` arrays (:786-790); imaginary parts are exact zeros.  Unmeasured ones are left untouched. */
int elph_bond_fetch(elph_handle h, double *BondBond, double *BondPairGreens);

/* reset_measurements! (Measurements.jl:698-758) for the two bond correlations: every accumulator to zero (stream-ordered). */
int elph_bond_reset(elph_handle h);

/* ---------------------------------------------------------------- bond correlations of resident chains (Holstein model; Measurements.jl) */

/* elph_bond_create for every chain resident in the handle (elph_update_model_holstein_chains, elph_hmc_create_chains): the accumulators of
 * BondBond (measure_BondBond!, Measurements.jl:1663-1785) and BondPairGreens (measure_BondPairGreens!, :2390-2483) of every chain in one
 * device allocation [chain][BondBond | BondPairGreens], the buffers of one pair of vectors of all chains, and the scratch in which the
 * estimator's setup! (GreensFunctions.jl:239-288) runs for one pair of vectors of all chains at once.  It stands beside the containers of
 * elph_bond_create and elph_meas_chains_create in a slot of its own.  Needs elph_greens_create first; a new elph_greens_create drops it.
 * The estimator serves the chains with n_v * nchains vectors, vector v of chain c at index v * nchains + c (0-based).  Arguments as
 * elph_bond_create, and
 *   nchains   >= 1 and equal to the number of chains resident in the handle
 * Checked in this order, before anything is allocated; a refused request leaves the handle without this container and usable:
 *   ELPH_E_UNSUPPORTED   the SSH model; a sharded or slab handle
 *   ELPH_E_ARG           nchains < 1 or not the resident number (the message names both)
 *   ELPH_E_STATE         elph_greens_create has not been called
 *   ELPH_E_ARG           n_def < 1 or a null array; an orbital outside 1..n_s (naming the definition); a measured correlation without
 *                        pairs, or a bond index outside 1..n_def (naming the correlation, the pair and the index)
 *   ELPH_E_UNSUPPORTED   a lattice whose frequency slice does not fit the LDS; a request whose grids would exceed 65535 in y or z:
 *                        (fields transformed: 4 for BondBond + 2 for BondPairGreens) * n_def * nchains slices, or (listed pairs of both
 *                        correlations) * nchains transforms (the message says which product)
 *   ELPH_E_HIP           an allocation failed */
int elph_bond_chains_create(elph_handle h, int nchains, int n_def, const int *o1, const int *o2, const int *v, const int *measure,
                            const int *time_dependent, const int *npairs, const int *pairs);

/* measure_BondBond! / measure_BondPairGreens! (Measurements.jl:1663-1785, :2390-2483) for every pair v1 < v2 of a chain's n_v vectors, of
 * every chain: per pair the device part of setup! (for G[D,0] of the delta terms), the fields, their transforms, one inverse transform per
 * listed pair and the fold run once for all chains (the chain is a grid axis: the number of launches does not depend on nchains),
 * stream-ordered, with one synchronisation before the call returns.  The correlations read the vectors and neither the field nor mu: no
 * X.  Sums as elph_bond_accumulate: every element one thread's sum in index order, no atomics; chain c's numbers depend on chain c's
 * vectors alone.  The estimator's own tables (elph_greens_dev_arrays) are not touched.  With no pair requested nothing is launched.
 *   ELPH_E_STATE   elph_bond_chains_create has not been called; the handle no longer holds the number of chains the container was created
 *                  for (after elph_update_model_holstein, say); the estimator's vectors are not a multiple of it (the message names both
 *                  counts); the estimator holds no vectors yet */
int elph_bond_chains_accumulate(elph_handle h);

/* One chain's un-normalised sums since the last reset: the outputs of elph_bond_fetch for chain `chain` (0-based).  One device-to-host
 * copy, one synchronisation.  ELPH_E_STATE: not created; ELPH_E_ARG: a chain outside 0..nchains-1. */
int elph_bond_chains_fetch(elph_handle h, int chain, double *BondBond, double *BondPairGreens);

/* reset_measurements! (Measurements.jl:698-758) for the bond correlations of every chain: one memset (stream-ordered).  ELPH_E_STATE: not
 * created. */
int elph_bond_chains_reset(elph_handle h);

/* ---------------------------------------------------------------- CurrentCurrent of the Holstein model (Measurements.jl) */

/* The device side of a Holstein container's CurrentCurrent (measure_CurrentCurrent!(..., model::HolsteinModel, ...),
 * Measurements.jl:1790-2098), for one configuration or for every chain resident in the handle: the accumulators of every chain in one
 * device allocation [chain][CurrentCurrent] and the buffers of one pair of vectors of all chains, in a slot of its own beside the
 * containers of elph_bond_create, elph_bond_chains_create and elph_meas_create.  The reference is mirrored as it executes: the eight
 * translation averages, the four delta terms and the tau = beta slice of the SSH method (:2100-2384, elph_ssh_bond_create), every factor
 * weighted by the static hopping t = reshaped(model.t, (L1, L2, L3, n_def)) (:1835) inside `for tau in L_tau` (:1868-1871), which visits
 * the last time slice alone: the weight of bond cell + ncells * (definition - 1) is 1 on slices 1 .. L_tau - 1 and t on slice L_tau.
 * The b == c delta term's displacement r'' is reduced mod L (unreduced the reference's index throws).  Needs elph_greens_create first;
 * a new elph_greens_create drops it.  The estimator serves the chains with n_v * nchains vectors, vector v of chain c at index
 * v * nchains + c (0-based).
 *   nchains          >= 1 and equal to the number of chains resident in the handle (1: one configuration)
 *   n_def, o1, o2, v model.bond_definitions, as elph_bond_create
 *   Nbonds, t        model.Nbonds, double[Nbonds] model.t in definition order (assign_t! appends, initialize_model! never permutes it)
 *   measure, time_dependent, npairs, pairs   the request for CurrentCurrent: measured or not; L_tau + 1 slices or the equal-time slice
 *                    alone; int[2 * npairs] 1-based (pairs[1,p], pairs[2,p]) indices of bond definitions
 * Checked before anything is allocated; a refused request leaves the handle without this container and usable:
 *   ELPH_E_UNSUPPORTED   the SSH model (elph_ssh_bond_create measures its CurrentCurrent); a sharded or slab handle
 *   ELPH_E_ARG           nchains < 1 or not the resident number (the message names both)
 *   ELPH_E_STATE         elph_greens_create has not been called
 *   ELPH_E_ARG           n_def < 1 or a null array; an orbital outside 1..n_s (naming the definition); measured without pairs, or a bond
 *                        index outside 1..n_def (naming the pair and the index); Nbonds not the handle's, or t null
 *   ELPH_E_UNSUPPORTED   Nbonds != n_def * ncells, where the reference's reshape of t fails (the message names both counts); a lattice
 *                        whose frequency slice does not fit the LDS; a request whose grids would exceed 65535 in y or z:
 *                        8 * n_def * nchains slices, or npairs * nchains transforms (the message says which product)
 *   ELPH_E_HIP           an allocation failed */
int elph_current_create(elph_handle h, int nchains, int n_def, const int *o1, const int *o2, const int *v, int64_t Nbonds, const double *t,
                        int measure, int time_dependent, int npairs, const int *pairs);

/* measure_CurrentCurrent! (Measurements.jl:1790-2098) for every pair v1 < v2 of a chain's n_v vectors, of every chain: the fields, their
 * transforms, one inverse transform per listed pair, the delta terms and the fold run once for all chains (the chain is a grid axis: the
 * number of launches does not depend on nchains), stream-ordered, with no copy and no synchronisation in between and one
 * synchronisation before the call returns.  The method reads R and M^-1 R and nothing setup! makes: the estimator's pipeline does not
 * run and its tables (elph_greens_dev_arrays) are not touched.  Every element is one thread's sum in index order, the delta means in
 * the reduction order of elph_meas_accumulate, no atomics: the same inputs give the same bits, and chain c's bits depend on chain c's
 * vectors alone and equal those of a single-configuration handle holding them.  With no pair requested nothing is launched.
 *   ELPH_E_STATE   elph_current_create has not been called; the handle no longer holds the number of chains the container was created
 *                  for (the message names both counts); the estimator's vectors are not a multiple of it; the estimator holds no
 *                  vectors yet */
int elph_current_accumulate(elph_handle h);

/* One chain's un-normalised sums since the last reset (chain 0-based; 0 for one configuration): Complex{Float64}[L0, L1, L2, L3, n_p]
 * as interleaved (re, im) doubles, first index fastest, L0 = L_tau + 1 or 1, laid out as elph_ssh_bond_fetch's CurrentCurrent; imaginary
 * parts are exact zeros.  NULL or unmeasured: left untouched.  One device-to-host copy, one synchronisation.  ELPH_E_STATE: not
 * created; ELPH_E_ARG: a chain outside 0..nchains-1. */
int elph_current_fetch(elph_handle h, int chain, double *CurrentCurrent);

/* reset_measurements! (Measurements.jl:698-758) for CurrentCurrent of every chain: one memset (stream-ordered).  ELPH_E_STATE: not
 * created. */
int elph_current_reset(elph_handle h);

/* ---------------------------------------------------------------- measurements of the bond-phonon (SSH) model (Measurements.jl) */

/* The device side of initialize_measurements_container(ssh, ...) (Measurements.jl:180-338): accumulators, all doubles on the device, for the
 * global scalars, the on-site scalars density, double_occ, mu per orbital (:978-1024), the inter-site scalars x, x2, x4, phonon_pe,
 * phonon_ke, elph_energy, el_ke, sign_switch per bond definition (:1072-1155), the on-site correlations Greens, DenDen, SpinSpin,
 * PairGreens and the inter-site PhononGreens over phonon types (:2488-2541).  It stands beside elph_meas_create (Holstein handles only)
 * in a slot of its own.  Needs elph_greens_create first; a new elph_greens_create drops it.
 *   mu                          double[N] model.mu
 *   nbonds, ndef                model.Nbonds, model.nbonds; the normalisation of the inter-site scalars is (nbonds / ndef) * L_tau
 *   bond_sites, bond_t          int64[2 * nbonds] 1-based (s1, s2) = neighbor_table[:, checkerboard_perm[bond]] and double[nbonds] model.t,
 *                               both in the reference's bond order (the order of model.t)
 *   bond_to_definition          int64[nbonds] 1-based definition of every bond
 *   bond_to_phonon              int64[nbonds] 1-based phonon of every bond, 0 on a bare bond
 *   Nph, nph                    phonons, phonon types; omega, alpha, alpha2: double[Nph] (NULL allowed when Nph = 0)
 *   measure, time_dependent, npairs   int[5] in the order Greens, DenDen, SpinSpin, PairGreens, PhononGreens
 *   pairs                       as elph_meas_create; a PhononGreens pair names phonon types 1..nph
 * ELPH_E_ARG (an orbital outside 1..n_s, a phonon type outside 1..nph, a site, definition or phonon outside its range, a bond count
 * that is not the handle's) and ELPH_E_UNSUPPORTED (Holstein model, several chains resident, a sharded or slab handle, PhononGreens
 * requested with Nph != nph * ncells, where the reference's reshape of the field fails) leave the handle without a container and usable. */
int elph_ssh_meas_create(elph_handle h, const double *mu, double dtau, int64_t nbonds, int ndef, const int64_t *bond_sites,
                         const double *bond_t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph, int nph,
                         const double *omega, const double *alpha, const double *alpha2, const int *measure, const int *time_dependent,
                         const int *npairs, const int *pairs);

/* make_measurements! without its update! for the SSH model: x is model.x (L_tau * Nph doubles, host, phonon slowest), from which the
 * modulated hopping t' = t - (alpha x + sign(x) alpha2 x^2) is recomputed.  Stream-ordered like elph_meas_accumulate; one
 * synchronisation before it returns; one fixed summation order without atomics: the same inputs give the same bits.  Afterwards
 * elph_greens_dev_arrays holds the tables of the LAST pair. */
int elph_ssh_meas_accumulate(elph_handle h, const double *x);

/* The un-normalised sums since the last reset; one device-to-host copy, one synchronisation.  Each pointer may be NULL.
 *   scalars    double[3 + 3 n_s + 8 ndef]: density, Nsqr, mu; then n_s values each of density, double_occ, mu; then ndef values each of
 *              x, x2, x4, phonon_pe, phonon_ke, elph_energy, el_ke, sign_switch
 *   Greens … PhononGreens   as elph_meas_fetch */
int elph_ssh_meas_fetch(elph_handle h, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                        double *PhononGreens);

/* reset_measurements! (Measurements.jl:698-758): every accumulator to zero (stream-ordered). */
int elph_ssh_meas_reset(elph_handle h);

/* Drops the container (elph_greens_create and elph_destroy do so as well). */
int elph_ssh_meas_free(elph_handle h);

/* ---------------------------------------------------------------- measurements of resident chains (bond-phonon (SSH) model) */

/* elph_ssh_meas_create for every chain resident in the handle (elph_update_model_ssh_fields_chains, elph_hmc_create_ssh_chains): one
 * container per chain in one device allocation [chain][scalars | Greens | DenDen | SpinSpin | PairGreens | PhononGreens], in a slot of
 * its own beside the container of elph_ssh_meas_create, with the buffers of the fields of all chains and the scratch in which the
 * estimator's setup! (GreensFunctions.jl:239-288) runs for one pair of vectors of all chains at once.  Needs elph_greens_create first; a
 * new elph_greens_create drops it.  The estimator serves the chains with n_v * nchains vectors, vector v of chain c at index
 * v * nchains + c (0-based).  Arguments as elph_ssh_meas_create, except
 *   nchains   >= 1 and equal to the number of chains resident in the handle
 *   mu        double[nchains * nsites], a row per chain: a tuner per chain moves it (elph_hmc_set_mu_chains); the global mu (:858) and
 *             the on-site mu (:1018) of chain c come from row c
 * The bonds, the phonon parameters and the requests are the model's and serve every chain.  Checked in this order, before anything is
 * allocated; a refused request leaves the handle without this container and usable:
 *   ELPH_E_UNSUPPORTED   the Holstein model ("SSH only"); a sharded or slab handle
 *   ELPH_E_ARG           nchains < 1 or not the resident number (the message names both)
 *   ELPH_E_STATE         elph_greens_create has not been called
 *   ELPH_E_ARG           as elph_ssh_meas_create: a null array, a site, definition, phonon, orbital or phonon type outside its range
 *   ELPH_E_UNSUPPORTED   PhononGreens requested with Nph != nph * ncells, or on a lattice whose frequency slice does not fit the LDS */
int elph_ssh_meas_chains_create(elph_handle h, int nchains, const double *mu, double dtau, int64_t nbonds, int ndef, const int64_t *bond_sites,
                                const double *bond_t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph, int nph,
                                const double *omega, const double *alpha, const double *alpha2, const int *measure, const int *time_dependent,
                                const int *npairs, const int *pairs);

/* The chemical-potential tuners moved the chains' mu: mu, double[nchains * nsites], replaces the rows elph_ssh_meas_chains_create took,
 * for the global and the on-site mu of the accumulates that follow.  The sums so far are kept.  ELPH_E_STATE: not created. */
int elph_ssh_meas_chains_set_mu(elph_handle h, const double *mu);

/* make_measurements! (Measurements.jl:545-566) without its update!, for every chain: X is double[nchains * Nph * L_tau], chain c's
 * model.x (phonon slowest) at X + c * Nph * L_tau.  The field-only terms, PhononGreens and, for every pair v1 < v2 of a chain's n_v
 * vectors, the device part of setup! and the folds run once for all chains (the chain is a grid axis: the number of launches does not
 * depend on nchains), stream-ordered, with one synchronisation before the call returns.  Sums as elph_ssh_meas_accumulate: one fixed
 * order, no atomics; chain c's numbers depend on chain c's inputs alone.  The estimator's own tables (elph_greens_dev_arrays) are not
 * touched.
 *   ELPH_E_STATE   elph_ssh_meas_chains_create has not been called; the handle no longer holds the number of chains the container was
 *                  created for (after elph_update_model_ssh_fields, say; the message names both counts); the estimator's vectors are
 *                  not a multiple of it; the estimator holds no vectors yet */
int elph_ssh_meas_chains_accumulate(elph_handle h, const double *X);

/* One chain's un-normalised sums since the last reset: the outputs of elph_ssh_meas_fetch for chain `chain` (0-based).  One
 * device-to-host copy, one synchronisation.  ELPH_E_STATE: not created; ELPH_E_ARG: a chain outside 0..nchains-1. */
int elph_ssh_meas_chains_fetch(elph_handle h, int chain, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                               double *PhononGreens);

/* reset_measurements! (Measurements.jl:698-758) of every chain: one memset (stream-ordered).  ELPH_E_STATE: not created. */
int elph_ssh_meas_chains_reset(elph_handle h);

/* ---------------------------------------------------------------- inter-site correlations of the bond-phonon (SSH) model */

/* The device side of the SSH container's BondBond, CurrentCurrent and BondPairGreens (init_corr_container! over ssh.nbonds bond
 * definitions, Measurements.jl:295-302): accumulators, all doubles on the device, in a slot of their own beside elph_ssh_meas_create.
 * BondBond (measure_BondBond!, :1663-1785) and BondPairGreens (measure_BondPairGreens!, :2390-2483) are the AbstractModel methods
 * elph_bond_create measures on a Holstein handle; CurrentCurrent is measure_CurrentCurrent!(..., model::SSHModel, ...) (:2100-2384).
 * Needs elph_greens_create first; a new elph_greens_create drops it.
 *   n_def, o1, o2, v            model.bond_definitions, as elph_bond_create
 *   Nbonds, t                   model.Nbonds, double[Nbonds] model.t in the reference's bond order (CurrentCurrent only; bond
 *                               cell + ncells * (definition - 1) is the reference's reshape of t' to (L_tau, L1, L2, L3, n_def))
 *   bond_to_definition, bond_to_phonon   int64[Nbonds] 1-based, 0 = a bare bond, as elph_ssh_meas_create (CurrentCurrent only)
 *   Nph, alpha, alpha2          phonons; double[Nph] (CurrentCurrent only; NULL allowed when Nph = 0)
 *   measure, time_dependent, npairs   int[3] in the order BondBond, CurrentCurrent, BondPairGreens
 *   pairs                       as elph_bond_create: the measured ones' lists one after the other in that order
 * ELPH_E_ARG (an orbital outside 1..n_s, a bond index outside 1..n_def, a definition or phonon outside its range, a bond count that is
 * not the handle's) and ELPH_E_UNSUPPORTED (Holstein model, several chains resident: elph_ssh_bond_chains_create measures those, a sharded
 * or slab handle, a lattice whose frequency slice does not fit the LDS, CurrentCurrent requested with Nbonds != n_def * ncells, where the
 * reference's reshape of t' fails; BondBond and BondPairGreens stay available there) leave the handle without these accumulators and
 * usable. */
int elph_ssh_bond_create(elph_handle h, int n_def, const int *o1, const int *o2, const int *v, int64_t Nbonds, const double *t,
                         const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph, const double *alpha,
                         const double *alpha2, const int *measure, const int *time_dependent, const int *npairs, const int *pairs);

/* The calls to measure_BondBond! / measure_CurrentCurrent! / measure_BondPairGreens! of make_intersite_measurements! for every pair
 * i < j of the estimator's n_v vectors (ELPH_E_STATE without vectors).  x is model.x (L_tau * Nph doubles, host, phonon slowest), from
 * which CurrentCurrent recomputes t' = t - (alpha x + sign(x) alpha2 x^2); it may be NULL when CurrentCurrent is not requested.
 * Stream-ordered like elph_bond_accumulate; one synchronisation before it returns; no atomics and one fixed summation order: the same
 * inputs give the same bits.  Afterwards elph_greens_dev_arrays holds the tables of the LAST pair. */
int elph_ssh_bond_accumulate(elph_handle h, const double *x);

/* The un-normalised sums since the last reset, as elph_bond_fetch.  Each pointer may be NULL; unmeasured ones are left untouched. */
int elph_ssh_bond_fetch(elph_handle h, double *BondBond, double *CurrentCurrent, double *BondPairGreens);

/* reset_measurements! (Measurements.jl:698-758) for the three correlations: every accumulator to zero (stream-ordered). */
int elph_ssh_bond_reset(elph_handle h);

/* ---------------------------------------------------------------- inter-site correlations of resident chains (bond-phonon (SSH) model) */

/* elph_ssh_bond_create for every chain resident in the handle (elph_update_model_ssh_fields_chains, elph_hmc_create_ssh_chains): the
 * accumulators of BondBond, CurrentCurrent and BondPairGreens of every chain, [chain][BondBond | BondPairGreens] in one device allocation
 * and [chain][CurrentCurrent] in another, the buffers of one pair of vectors of all chains, the fields of all chains, and the scratch in
 * which the estimator's setup! (GreensFunctions.jl:239-288) runs for one pair of vectors of all chains at once.  It stands beside the
 * containers of elph_ssh_bond_create and elph_ssh_meas_chains_create in a slot of its own.  Needs elph_greens_create first; a new
 * elph_greens_create drops it.  The estimator serves the chains with n_v * nchains vectors, vector v of chain c at index v * nchains + c
 * (0-based).  Arguments as elph_ssh_bond_create (request order BondBond, CurrentCurrent, BondPairGreens), and
 *   nchains   >= 1 and equal to the number of chains resident in the handle
 * The bonds, the phonon parameters and the requests are the model's and serve every chain.  Checked in this order, before anything is
 * allocated; a refused request leaves the handle without this container and usable:
 *   ELPH_E_UNSUPPORTED   the Holstein model ("SSH only"); a sharded or slab handle
 *   ELPH_E_ARG           nchains < 1 or not the resident number (the message names both)
 *   ELPH_E_STATE         elph_greens_create has not been called
 *   ELPH_E_ARG / ELPH_E_UNSUPPORTED   as elph_ssh_bond_create: n_def < 1 or a null array, an orbital outside 1..n_s, a lattice whose
 *                        frequency slice does not fit the LDS, a measured correlation without pairs, a bond index outside 1..n_def; for
 *                        CurrentCurrent a bond count that is not the handle's, Nbonds != n_def * ncells (ELPH_E_UNSUPPORTED; BondBond and
 *                        BondPairGreens alone stay available there), a definition or phonon outside its range
 *   ELPH_E_UNSUPPORTED   a request whose grids would exceed 65535 in y or z: (fields transformed: 8 for CurrentCurrent, 4 for BondBond +
 *                        2 for BondPairGreens, the larger of the two) * n_def * nchains slices, or (listed pairs of CurrentCurrent, or of
 *                        the other two together, the larger) * nchains transforms (the message says which product)
 *   ELPH_E_HIP           an allocation failed */
int elph_ssh_bond_chains_create(elph_handle h, int nchains, int n_def, const int *o1, const int *o2, const int *v, int64_t Nbonds,
                                const double *t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph,
                                const double *alpha, const double *alpha2, const int *measure, const int *time_dependent, const int *npairs,
                                const int *pairs);

/* measure_BondBond! / measure_CurrentCurrent! / measure_BondPairGreens! for every pair v1 < v2 of a chain's n_v vectors, of every chain.
 * X is double[nchains * Nph * L_tau] (host), chain c's model.x (phonon slowest) at X + c * Nph * L_tau, from which CurrentCurrent
 * recomputes chain c's t'; it may be NULL when CurrentCurrent is not requested or Nph = 0.  One asynchronous copy of X, then per pair of
 * vectors the device part of setup! and the kernels of the three correlations run once for all chains (the chain is a grid axis: the
 * number of launches does not depend on nchains), stream-ordered, with one synchronisation before the call returns (X is not retained).
 * Sums as elph_ssh_bond_accumulate: one fixed order, no atomics, the same inputs give the same bits; chain c's numbers depend on chain
 * c's vectors and field alone.  The estimator's own tables (elph_greens_dev_arrays) are not touched.
 *   ELPH_E_STATE   elph_ssh_bond_chains_create has not been called; the handle no longer holds the number of chains the container was
 *                  created for (the message names both counts); the estimator's vectors are not a multiple of it; the estimator holds
 *                  no vectors yet
 *   ELPH_E_ARG     X is NULL although CurrentCurrent is requested and Nph > 0 */
int elph_ssh_bond_chains_accumulate(elph_handle h, const double *X);

/* One chain's un-normalised sums since the last reset: the outputs of elph_ssh_bond_fetch for chain `chain` (0-based).  One
 * device-to-host copy and one synchronisation per accumulator allocation.  ELPH_E_STATE: not created; ELPH_E_ARG: a chain outside
 * 0..nchains-1. */
int elph_ssh_bond_chains_fetch(elph_handle h, int chain, double *BondBond, double *CurrentCurrent, double *BondPairGreens);

/* reset_measurements! (Measurements.jl:698-758) for the three correlations of every chain: one memset per accumulator allocation
 * (stream-ordered).  ELPH_E_STATE: not created. */
int elph_ssh_bond_chains_reset(elph_handle h);

/* ---------------------------------------------------------------- KPM preconditioner */

/* SymmetricKPMPreconditioner(model, n, buf, c1, c2) — KPMPreconditioners.jl:219-235, ctor :101-146 */
int elph_kpm_create(elph_handle h, int n, double buf, double c1, double c2);

/* KPMPreconditioners.setup!(P) — :259-321.  Averages expnDtauV over tau on the device
 * (update_A!, :332-381), estimates the spectrum of A by Arnoldi (:845-942) and rebuilds the
 * Chebyshev coefficients when the bounds moved by more than buf (:293-309).
 *   b_max, b_min  the two random Arnoldi start vectors (double[nsites]); the reference draws
 *                 them from model.rng (:859-861,902-904) — the caller supplies them.
 *   e_min, e_max  if both finite, skip Arnoldi and use these eigenvalue bounds (parity runs);
 *                 pass NaN to run Arnoldi.
 * Out: active flag (P.expansion.active), and the bounds used. */
int elph_kpm_setup(elph_handle h, const double *b_max, const double *b_min, double e_min,
                   double e_max, int *active, double *lam_lo, double *lam_hi);

/* The same for every phonon configuration resident after elph_update_model_holstein_chains (nchains of them): one
 * expansion per chain — its own Ē, eigenvalue bounds, orders and coefficients; in a batched solve right-hand side r is
 * preconditioned with the expansion of chain r % nchains.  b_max, b_min: double[nchains * nsites] (chain-major);
 * e_min, e_max: double[nchains] or NULL (NULL or non-finite entries: run Arnoldi for that chain); active, lam_lo,
 * lam_hi: per chain, each may be NULL.  A chain whose bounds fail the test of :280 is preconditioned with the identity. */
int elph_kpm_setup_chains(elph_handle h, const double *b_max, const double *b_min, const double *e_min,
                          const double *e_max, int *active, double *lam_lo, double *lam_hi);

/* Inspect the expansion (of chain 0): orders[cld(ltau,2)], total = sum(orders) (either pointer may be NULL). */
int elph_kpm_orders(elph_handle h, int64_t *orders, int64_t *total);

/* ldiv!(z, P, r) — KPMPreconditioners.jl:426-481 (identity copy when inactive, :475-478) */
int elph_kpm_apply(elph_handle h, double *z, const double *r);
int elph_kpm_apply_dev(elph_handle h, double *z_dev, const double *r_dev);

/* ---- BiCGStab and GMRES on M x = b or Mᵀ x = b (csrc/msolve.hip): the solvers of `mul_by_M = true` models, HolsteinModels.jl:286-298 ----
 *
 * One side of the expansion of the last setup!, on nvec vectors in the reference layout (vector r: the expansion of chain r % nchains) —
 * mul!(v′, P, v) per frequency block between the twisted transforms: transposed = 0 the LeftKPMPreconditioner ~ M⁻¹ (KPMPreconditioners.jl:514-554), transposed = 1 the
 * RightKPMPreconditioner ~ M⁻ᵀ with the conjugated coefficients (:560-600); Left after Right is the symmetric apply above.  An inactive
 * expansion copies (:475-478). */
int elph_kpm_apply_side(elph_handle h, int nvec, double *vout, const double *vin, int transposed);

#define ELPH_SOLVER_CG 0
#define ELPH_SOLVER_BICGSTAB 1
#define ELPH_SOLVER_GMRES 2

/* The solver of the handle's model (model.solver's type; the default is CG on MᵀM): what the callers of the solve run — the Green's-function
 * estimator (elph_greens_update[_rng]), the HMC force and action (elph_hmc_update[_chains], elph_fermion_force_*), the Langevin force and
 * the special updates.  solver: ELPH_SOLVER_CG / _BICGSTAB / _GMRES; restart: GMRES only, < 0: min(20, ndim).
 * With BiCGStab or GMRES these callers follow the reference's mul_by_M branches: calc_O⁻¹Λϕ! is two solves per pseudofermion field, Mᵀ y = Λϕ
 * then M x = y (HMC.jl:851-903); the estimator and the Langevin force solve M x = r directly (GreensFunctions.jl:216-226,
 * LangevinDynamics.jl:366-375).  use_precond = 1 then means LeftRightKPMPreconditioner: the Right side of the handle's expansion for an Mᵀ
 * solve, the Left side for an M solve.  Such a caller returns ELPH_E_STATE on a sharded or slab handle and with a restricted inner-product
 * range.  A handle whose kind is CG behaves exactly as before this entry point existed. */
int elph_solver_set_kind(elph_handle h, int solver, int restart);

/* solve!(x, A, b, solver[, P]; maxiter, tol) -> iters for nrhs right-hand sides at once (IterativeSolvers.jl:354-417 BiCGStab, :464-570
 * GMRES with update! :552-570 and the rotations :572-584), A = M (transposed = 0) or Mᵀ (1).  X: initial guesses in, solutions out; X, B:
 * double[nrhs*ndim], RHS-major; right-hand side r uses chain r % nchains; each follows exactly the single-vector recurrences and stop rule,
 * every inner product is summed in a fixed order.  use_precond: the side of the expansion that LeftRightKPMPreconditioner takes for
 * model.transposed (:494-508) — Left for transposed = 0, Right for 1.  tol = 0: the handle's; solver_maxiter is the solver's own maxiter field
 * (0: the handle's), maxiter the call's keyword (0: solver_maxiter); restart < 0: min(20, ndim) (:448-450; ignored by BiCGStab).
 * As the reference executes: BiCGStab returns maxiter on breakdown (ρ = 0, ω = 0); GMRES runs whole cycles — iter < maxiter is tested between
 * cycles only, inside a cycle only the tolerance and iter == solver_maxiter end it, so iters may exceed a maxiter below solver_maxiter.
 * ONE deliberate difference: a cycle cut at iter == solver_maxiter after i < restart steps updates x with the i columns it built; the
 * reference back-substitutes over all `restart` columns there (:538), through columns this cycle never wrote (0/0 in the first cycle).
 * Whenever solver_maxiter is a multiple of restart the two coincide.
 * GMRES keeps its Krylov basis on the device from the first GMRES solve until the handle is destroyed: (restart + 1) ndim doubles per
 * right-hand side (6.9 MB at 16 x 16 sites, 160 slices, restart 20).
 * ELPH_E_STATE on a sharded handle or one with a restricted inner-product range. */
int elph_msolve(elph_handle h, int solver, int transposed, int nrhs, double *X, const double *B, int use_precond, double tol,
                int64_t maxiter, int64_t solver_maxiter, int restart, int64_t *iters);

/* ldiv!(x, model, b[, P]; maxiter) of a mul_by_M model for nrhs right-hand sides (Models.jl:74-186) with the handle's tol and maxiter
 * (the solver-set entry point above): the solve, the true residual |A x - b| / |b|, flag 0 / 1 (out of iterations: iters == maxiter with a
 * preconditioner, :103; == solver.maxiter without, :160) / 2, x zeroed where the flag is positive; a flagged preconditioned right-hand side
 * is solved again without the expansion from x = 0 with 10 maxiter (:129-133) and reports that solve. */
int elph_mldiv(elph_handle h, int solver, int transposed, int nrhs, double *X, const double *B, int use_precond, int64_t maxiter,
               int restart, int64_t *iters, double *residual_error, int *flag);

/* ---------------------------------------------------------------- Fourier acceleration */

/* fourier_accelerate!(v', fa, v, power; use_mass) — FourierAcceleration.jl:91-143, real in/out.
 * diag: the accelerator's M (use_mass=true) or Q (false) vector, double[nph*ltau],
 * frequency index fastest (update_M!/update_Q!, :149-167,176-266); nph = number of phonon
 * columns (nsites for Holstein, Nph for SSH). */
int elph_fourier_accelerate(elph_handle h, double *vout, const double *vin, const double *diag,
                            double power, int64_t nph);

/* τ_to_ω! / ω_to_τ! — TimeFreqFFTs.jl:55-73,112-130 (twisted FFT; complex interleaved re,im) */
int elph_tau_to_omega(elph_handle h, double *nu_complex, const double *v);
int elph_omega_to_tau(elph_handle h, double *v, const double *nu_complex);

/* ---------------------------------------------------------------- one solve over several GPUs
 *
 * Slabs of rows of cells along the slowest spatial index, one process per GPU, no reference equivalent (the reference is
 * single-process): solve!(x, A, b, cg) of IterativeSolvers.jl:239-314 with x0 = 0 for ONE fermion matrix whose lattice is
 * spread over `world` ranks.  The handle lives on the rank's SLAB lattice — [ghost rows from below | own rows | ghost rows
 * from above], site-contiguous, created with the bonds / exp(-dtau V) / (SSH) per-(tau, bond) tables of that slab; the ghost
 * rows are the dependency closure of the fused MtM on the own rows (elphdynamics_amd/sharded.py computes it from the bond
 * table).  Per CG iteration the ranks exchange the two partial inner products and ONE set of checkerboard boundary rows of
 * the residual, by device-initiated stores into each other's mailbox (hipIpc-mapped device memory: xGMI peer stores between
 * GPUs) from inside the resident CG kernel — no collective, no host.  Sequence on every rank:
 *   elph_shard_create   geometry (0-based local site ranges) -> a 64-byte IPC handle of this rank's mailbox
 *   (caller: all-gather the handles — torch.distributed / MPI)
 *   elph_shard_connect  map the other ranks' mailboxes
 *   per solve: elph_shard_prepare (zero the own mailbox) ; caller's BARRIER ; elph_shard_solve
 * own_lo / own_n: own sites [own_lo, own_lo + own_n) of the slab; n_to_prev / n_to_next: how many own sites (counted from
 * the bottom / from the top) the previous / next rank of the periodic ring holds as ghosts; cap_ghost: capacity in sites of
 * a ghost region of the mailbox, the SAME number on all ranks (>= every rank's ghost and send counts).
 * x_slab / b_slab: host vectors on the slab lattice, reference layout (site-major), b with its ghost entries filled from
 * the global right-hand side; x_slab's own rows are this rank's part of the solution.
 * iters / done / eps: identical on all ranks (done: 1 eps < tol, 2 kappa bound, 3 maxiter).
 * n_global / own_global_start / global_sites (0-based global site of every slab site; n_global = 0 and NULL when only
 * un-preconditioned solves are wanted): the geometry the preconditioned solve needs.
 * elph_shard_solve_kpm — solve!(x, A, b, cg, P) (IterativeSolvers.jl:153-234) with the KPM preconditioner under sharding:
 * hfull is a second handle on the WHOLE lattice (same bonds, exp(-dtau V) of all sites, elph_kpm_create + elph_kpm_setup done
 * with the same inputs on every rank).  Per iteration the ranks trade three partial inner products and all-gather the tau-spectrum
 * of the residual (peer stores into the mailboxes); every rank runs the per-frequency Chebyshev recursion on the whole lattice and
 * transforms back its own and ghost rows — no omega-sharded all-to-all: the recursion's critical path is its longest frequency
 * block either way (KPMPreconditioners.jl:426-481).
 * Ranks that live in ONE process (a host thread or task per GPU) use the same calls: a handle in the all-gathered list that this
 * process created itself is mapped by its device pointer (peer access enabled between devices) instead of through hipIpc.
 * elph_shard_shape — host arithmetic, no device: the team shape (waves per workgroup, workgroups per rank) the sharded kernel
 * takes for a time axis and the number of records world ranks put into a meeting against the capacity; ELPH_E_UNSUPPORTED
 * when they do not fit (every BASELINE config fits at 1, 2, 4 and 8 ranks: 8 x 20 = 160 of 256 at Ltau = 160). */
#define ELPH_SHARD_IPC_BYTES 64
int elph_shard_shape(int64_t ltau, int world, int *waves, int *groups, int *records, int *max_records);
int elph_shard_create(elph_handle h, int rank, int world, int64_t own_lo, int64_t own_n, int64_t n_to_prev,
                      int64_t n_to_next, int64_t cap_ghost, int64_t n_global, int64_t own_global_start,
                      const int64_t *global_sites, void *ipc_handle_out);
int elph_shard_connect(elph_handle h, const void *all_ipc_handles /* world * ELPH_SHARD_IPC_BYTES, rank order */);
int elph_shard_prepare(elph_handle h);
/* Preflight of the mailbox protocol, a collective like a solve (elph_shard_prepare on every rank, the caller's barrier, then this on
 * every rank): `rounds` lock-step exchanges of one tagged granule between ALL pairs of ranks through the mapped mailboxes — the stores
 * and polls a solve uses (xGMI peer stores between GPUs).  us_per_round[world] (may be NULL): mean time from this rank's store to the
 * sight of rank q's granule; *slowest_us: their maximum.  A rank that does not answer within ELPH_SHARD_SELFTEST_MS (10 s) gives
 * ELPH_E_HIP with the silent ranks named — at set-up instead of a time-out inside the first solve. */
int elph_shard_selftest(elph_handle h, int rounds, double *us_per_round, double *slowest_us);
/* *can = 1 when device dev_a can map memory of dev_b (hipDeviceCanAccessPeer; 1 on the diagonal): what a solve sharded over the
 * GPUs of a node needs between ring neighbours (boundary rows) and all pairs (rank records). */
int elph_peer_access(int dev_a, int dev_b, int *can);
int elph_shard_solve(elph_handle h, double *x_slab, const double *b_slab, double tol, int64_t maxiter, double kappa_max,
                     int64_t *iters, int *done, double *eps);
int elph_shard_solve_kpm(elph_handle h, elph_handle hfull, double *x_slab, const double *b_slab, double tol, int64_t maxiter,
                         double kappa_max, int64_t *iters, int *done, double *eps);
int elph_shard_destroy(elph_handle h);

/* The CALLERS of the solve on a sharded lattice (BASELINE configs "HMC ... spatial-sharded across 8 GPUs"): ldiv!'s wrapper, the fermion
 * force and — elph_hmc_update on a sharded handle — one HMC update.  Everything but the solve is pointwise in the site index or stays
 * inside the MᵀM closure the slab already holds; what crosses ranks besides the solve are a few scalars (true residual, energies) and,
 * once per force evaluation, the ghost rows of one vector (device to device through the mailboxes, see elph_shard_ghost_stats).  The
 * scalars and the barriers go through two host collectives the caller registers once per handle
 * (MPI.Barrier / MPI.Allreduce!(SUM), torch.distributed, a thread barrier for ranks that share a process); the CG iteration itself
 * keeps its device-initiated mailbox stores.  The library arms the mailbox itself (elph_shard_prepare + the barrier) before every solve
 * of these calls.  All vectors are SLAB vectors (own + ghost rows, reference layout, ghost entries filled from the global arrays);
 * results are valid on the OWN rows; scalars (iters, residual_error, flag, energies, accepted) come out identical on every rank.
 *   barrier(ctx) -> 0 on success;  allreduce_sum(ctx, buf, n): in-place sum over the ranks of n doubles, the SAME result on every rank. */
typedef int (*elph_shard_barrier_fn)(void *ctx);
typedef int (*elph_shard_allreduce_fn)(void *ctx, double *buf, int n);
int elph_shard_set_collectives(elph_handle h, elph_shard_barrier_fn barrier, elph_shard_allreduce_fn allreduce_sum, void *ctx);
/* ldiv!(x, model, b[, P]; maxiter) -> (iters, residual_error, flag) — Models.jl:74-137,139-186 — on a sharded lattice: the solve, the true
 * residual |MᵀM x − b| / |b| over all ranks' own rows, flag 1 / 2 with zero-fill, and with use_precond (hfull: the full-lattice handle
 * with elph_kpm_setup done, as for elph_shard_solve_kpm) the un-preconditioned retry with 10·maxiter.  Solver settings: elph_solver_set
 * on h. */
int elph_shard_ldiv(elph_handle h, elph_handle hfull, double *x_slab, const double *b_slab, int use_precond, int64_t maxiter,
                    int64_t *iters, double *residual_error, int *flag);
/* elph_fermion_force_holstein on a sharded lattice: update_model!, Λϕ±, the two solves (one after the other: the sharded kernel carries
 * one right-hand side; a failed first solve suppresses the second, iters = cld(total, 2): HMC.jl:851-909) and calc_dSfdx! on the slab;
 * dSfdx is accumulated into on the OWN rows only. */
int elph_shard_fermion_force_holstein(elph_handle h, elph_handle hfull, const double *x, const double *lambda, const double *lambda2,
                                      const double *mu, double dtau, const double *phi_plus, const double *phi_minus, int use_precond,
                                      double tol_power, double *dSfdx, double *Xp_out, double *Xm_out, int64_t *iters, int *flag);
/* elph_fermion_force_ssh on a sharded lattice: q_out[n·Ltau + tau] for the slab's bonds in their local checkerboard order; a bracket is
 * exact on the rank that owns the bond — the caller keeps those and scatters them onto the phonon fields. */
int elph_shard_fermion_force_ssh(elph_handle h, elph_handle hfull, const double *rhs_plus, const double *rhs_minus, int use_precond,
                                 double tol_power, double *q_out, double *Xp_out, double *Xm_out, int64_t *iters, int *flag);

/* elph_hmc_update on a SHARDED handle (elph_hmc_create / elph_hmc_create_ssh + elph_hmc_set_state on the slab handle, collectives set): one HMC
 * update of the whole lattice over the ranks — one chain; R, Rp, Rm and every per-site / per-phonon array are the slab's
 * part of the global ones (ghost entries included), u_accept the same number on every rank.  Bond phonons additionally need the slab's phonon
 * columns in the numbering of the whole lattice and their owners (the phonons of the slab's bonds; owner = the rank whose own rows hold the
 * bond's first site): global_column[nph_slab], own_weight[nph_slab] in {0, 1}; the state vectors of elph_hmc_set_state / _get_state are then
 * double[nph_slab * Ltau] in that column order. */
int elph_shard_hmc_set_columns(elph_handle h, const int64_t *global_column, int64_t n_global_columns, const double *own_weight);
/* A KPM-preconditioned update on a sharded Holstein handle (use_precond = 1): hfull = a handle on the WHOLE lattice with elph_kpm_create done
 * (it needs no field: every setup!(P) inside the update injects the τ-averaged exp(−ΔτV) of the whole lattice, summed over the ranks' own
 * rows); kpm_randn of elph_hmc_update then holds the (nt + 2) pairs of Arnoldi start vectors of the WHOLE lattice, the same on every rank. */
int elph_shard_set_full_lattice(elph_handle h, elph_handle hfull);
/* ... and on a sharded BOND-PHONON handle: hfull = a bond-phonon handle on the whole lattice with one elph_update_model_ssh (for exp(Δτμ), which does
 * not move) and elph_kpm_create done; every setup!(P) inside the update injects the τ-means of cosh / sinh of every bond of the lattice
 * (update_A!, KPMPreconditioners.jl:355-381), taken by each rank from its slab's tables for the bonds it owns and summed over the ranks.  For that
 * the slab's bonds in the numbering of the whole lattice: global_bond[nbonds_slab] = checkerboard position on the whole lattice (0-based),
 * own_weight[nbonds_slab] in {0, 1} — owner = the rank whose own rows hold the bond's first site, as for elph_shard_hmc_set_columns. */
int elph_shard_set_bonds(elph_handle h, const int64_t *global_bond, int64_t n_global_bonds, const double *own_weight);
/* The ghost rows of ϕ± (once per update) and of the fermion force (once per force evaluation) travel from their owners' devices into the
 * holders' mailboxes by peer stores — the spectrum area of the mailbox is the exchange area between solves; two of the caller's barriers per
 * exchange, no host copy of a vector.  ELPH_SHARD_GHOST_HOST=1 (A/B), or a vector that does not fit the area, stages through the caller's
 * all-reduce instead.  Counts of both since elph_shard_create: */
int elph_shard_ghost_stats(elph_handle h, int64_t *through_mailboxes, int64_t *through_host);

/* ---------------------------------------------------------------- health of the resident kernels */

/* The whole-solve-in-one-launch kernels (cg_wg.hip) wait for their team members with a wall-clock bound (ELPH_WG_TIMEOUT_MS, 2 s); a
 * launch that gives up — the GPU's CUs were held by other work — is solved again by the streaming iteration (same result to the
 * solver tolerance; ldiv!'s flags unchanged) and the handle stays on the streaming iteration for ELPH_WG_COOLDOWN solves (16) before
 * it tries again.  *cooling_down: solves left in that state (0 = the resident kernel is in use); *fallbacks: launches given up so far. */
int elph_wg_status(elph_handle h, int *cooling_down, int64_t *fallbacks);

#ifdef __cplusplus
}
#endif
#endif
