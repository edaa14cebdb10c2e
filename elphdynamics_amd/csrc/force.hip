// force.hip — the fermion forces of both models and the muldMdx! family.  Host orchestration only; the kernels are kernels.hip's.

#include "elph_internal.h"

// ------------------------------------------------------------------------------------------
// fermion force: update_model! + calc_O⁻¹Λϕ! + calc_dSfdx! with x, phi± , X± resident
// ------------------------------------------------------------------------------------------

// Room for nrhs vectors and for the bond brackets q[chain][tau][bond] of nch chains (SSH force).  The brackets go to work.p (two vectors per
// right-hand side) and their scatter onto the phonon fields to work.tmp (one), so a lattice with more than two bonds per site (triangular,
// cubic) needs more than the two right-hand sides of the solves: ceil(nb/N) vectors per chain hold both.
int elph_i_ssh_bracket_capacity(elph_handle_s *h, int nrhs, int nch) {
    const int per_site = (int)((h->nb + h->N - 1) / h->N);
    return elph_work_reserve(h, std::max(nrhs, nch * per_site));
}

int elph_i_force_holstein(elph_handle_s *h, const double *x, const double *lambda, const double *lambda2, const double *mu, double dtau,
                          const double *phi_plus, const double *phi_minus, double *dSfdx, double *Xp_out, double *Xm_out, int64_t *iters,
                          int *flag, int own_lo, int own_hi, const ElphPairSolve &solve_pair) {
    RC(elph_work_reserve(h, 2));
    const SolveWork &W = h->work;
    const size_t nd = (size_t)h->ndim, L = (size_t)h->L;
    // update_model! (HolsteinModels.jl:526-549) and x in layout S
    RC(elph_i_holstein_upload_params(h, lambda, lambda2, mu));
    HIPCHK(hipMemcpyAsync(W.stage_in, x, nd * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_expV(h, W.stage_in, dtau));
    RC(elph_launch_r2s(h, W.xfield, W.stage_in, 1));
    h->have_E = true;
    // phi± -> layout S; b± = Λ phi± (HMC.jl:840-842)
    RC(elph_stage_in(h, W.phi, phi_plus, 1));
    RC(elph_stage_in(h, W.phi + nd, phi_minus, 1));
    RC(elph_launch_lambda_rhs(h, W.b, W.phi, W.xfield, dtau));
    RC(solve_pair(iters, flag));
    // dSf/dx (HMC.jl:790-814)
    RC(elph_launch_force_holstein(h, W.tmp, W.x, W.phi, W.xfield, dtau));
    std::vector<double> F(nd);
    RC(elph_stage_out(h, F.data(), W.tmp, 1));
    if (Xp_out) RC(elph_stage_out(h, Xp_out, W.x, 1));
    if (Xm_out) RC(elph_stage_out(h, Xm_out, W.x + nd, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = (size_t)own_lo * L; i < (size_t)own_hi * L; ++i) dSfdx[i] += F[i];      // "@. dSfdx += ..." accumulates (:803-811)
    return ELPH_OK;
}

// the two solves of calc_O⁻¹Λϕ! as one batch from x = 0 (fill!(O⁻¹Λϕ, 0), HMC.jl:854,883) at tol^power
static ElphPairSolve batch_pair(elph_handle_s *h, int use_precond, double tol_power) {
    return [=](int64_t *iters, int *flag) -> int {
        const size_t nd = (size_t)h->ndim;
        if (h->solver_kind != ELPH_SOLVER_CG) {      // the mul_by_M branch (HMC.jl:859-873, :888-902): Mᵀ y = Λϕ±, then M x = y, y in work.z
            int64_t it4[4] = {0, 0, 0, 0};
            int fl4[4] = {0, 0, 0, 0}, zero_minus = 0;
            {
                TolPower scope(h, tol_power);
                RC(elph_i_msolve_pair(h, 2, use_precond ? 1 : 0, h->work.x, h->work.z, h->work.b, it4, fl4));
            }
            elph_fold_pair_stages(1, it4, fl4, iters, flag, &zero_minus);
            if (zero_minus) RC(elph_launch_zero(h, h->work.x + nd, (int64_t)nd));
            return ELPH_OK;
        }
        HIPCHK(hipMemsetAsync(h->work.x, 0, 2 * nd * sizeof(double), h->stream));
        h->x_zero = true;
        int64_t it2[2] = {0, 0};
        double res2[2];
        int fl2[2] = {0, 0};
        {
            TolPower scope(h, tol_power);
            RC(elph_i_ldiv_core(h, 2, use_precond, 0, it2, res2, fl2));
        }
        elph_fold_pair(1, it2, fl2, iters, flag);
        if (fl2[0]) RC(elph_launch_zero(h, h->work.x + nd, (int64_t)nd));
        return ELPH_OK;
    };
}

extern "C" int elph_fermion_force_holstein(elph_handle h, const double *x, const double *lambda, const double *lambda2,
                                           const double *mu, double dtau, const double *phi_plus, const double *phi_minus,
                                           int use_precond, double tol_power, double *dSfdx, double *Xp_out, double *Xm_out,
                                           int64_t *iters, int *flag) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    if (!x || !lambda || !lambda2 || !mu || !phi_plus || !phi_minus || !dSfdx || !iters || !flag) { elph_set_error("null argument"); return ELPH_E_ARG; }
    set_nchains(h, 1);   // expansions were per chain
    return elph_i_force_holstein(h, x, lambda, lambda2, mu, dtau, phi_plus, phi_minus, dSfdx, Xp_out, Xm_out, iters, flag, 0, (int)h->N,
                                 batch_pair(h, use_precond, tol_power));
}

// the two solves of calc_O⁻¹Λϕ! for an SSH handle (Λ = identity) + the bond brackets q[tau][n] left in h->work.p
static int ssh_force_core(elph_handle_s *h, const double *rhs_plus, const double *rhs_minus, int64_t *iters, int *flag,
                          const ElphPairSolve &solve_pair) {
    RC(elph_i_ssh_bracket_capacity(h, 2, 1));
    RC(elph_stage_in(h, h->work.b, rhs_plus, 1));
    RC(elph_stage_in(h, h->work.b + h->ndim, rhs_minus, 1));
    RC(solve_pair(iters, flag));
    return elph_launch_force_ssh(h, h->work.p, h->work.x);     // work.p: scratch, free once the solves are done
}

static int ssh_solutions_out(elph_handle_s *h, double *Xp_out, double *Xm_out) {
    if (Xp_out) RC(elph_stage_out(h, Xp_out, h->work.x, 1));
    if (Xm_out) RC(elph_stage_out(h, Xm_out, h->work.x + h->ndim, 1));
    return ELPH_OK;
}

// Bond brackets out: q[tau][n] of work.p (tau-major) -> q_out[n*L + tau] (tau fastest, like the reference's (Ltau x Nbonds) arrays), with
// the solutions of the force's two solves where the caller asks for them; drains the stream
static int ssh_brackets_out(elph_handle_s *h, double *q_out, double *Xp_out = nullptr, double *Xm_out = nullptr) {
    const size_t L = (size_t)h->L, nb = (size_t)h->nb, nq = L * nb;
    std::vector<double> qt(nq);
    if (nq) HIPCHK(hipMemcpyAsync(qt.data(), h->work.p, nq * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RC(ssh_solutions_out(h, Xp_out, Xm_out));
    HIPCHK(hipStreamSynchronize(h->stream));
    elph_tb_to_bt(q_out, qt.data(), L, nb);
    return ELPH_OK;
}

static int ssh_fields_current(elph_handle_s *h) {
    if (!h->cs_host_stale || h->ssh_nph < 0) { elph_set_error("elph_update_model_ssh_fields has not been called for the current field"); return ELPH_E_STATE; }
    return ELPH_OK;
}

// Bracket scatter onto those phonon fields: work.p -> *dF (work.tmp: cap*ndim doubles), *nf fields
static int ssh_scatter_fields(elph_handle_s *h, double **dF, size_t *nf) {
    RC(ssh_fields_current(h));
    *nf = (size_t)h->ssh_nph * (size_t)h->L;
    *dF = h->work.tmp;
    if (*nf > (size_t)h->work.cap_rhs * (size_t)h->ndim) { elph_set_error("more phonon fields than scratch"); return ELPH_E_UNSUPPORTED; }
    return elph_launch_ssh_scatter(h, *dF, h->work.p, h->d_ssh_x, h->d_ssh_par, h->d_ssh_cb, h->ssh_nph, h->ssh_dtau);
}

int elph_i_force_ssh(elph_handle_s *h, const double *rhs_plus, const double *rhs_minus, double *q_out, double *Xp_out, double *Xm_out,
                     int64_t *iters, int *flag, const ElphPairSolve &solve_pair) {
    RC(ssh_force_core(h, rhs_plus, rhs_minus, iters, flag, solve_pair));
    return ssh_brackets_out(h, q_out, Xp_out, Xm_out);
}

extern "C" int elph_fermion_force_ssh(elph_handle h, const double *rhs_plus, const double *rhs_minus, int use_precond,
                                      double tol_power, double *q_out, double *Xp_out, double *Xm_out, int64_t *iters,
                                      int *flag) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    RC(need_model(h));
    if (!rhs_plus || !rhs_minus || !q_out || !iters || !flag) { elph_set_error("null argument"); return ELPH_E_ARG; }
    return elph_i_force_ssh(h, rhs_plus, rhs_minus, q_out, Xp_out, Xm_out, iters, flag, batch_pair(h, use_precond, tol_power));
}

// The same with the scatter onto the phonon fields done on the device (SSHModels.jl:797-823 with one field per bond):
//   dSdx[(p-1) Ltau + tau] -= sg(tau) dtau (alpha_p + 2 alpha2_p x) q[tau][bond(p)],   sg(1) = -1   (HMC.jl:803,808)
// for the fields, couplings and checkerboard positions given to the last elph_update_model_ssh_fields call.
extern "C" int elph_fermion_force_ssh_fields(elph_handle h, const double *rhs_plus, const double *rhs_minus, int use_precond,
                                             double tol_power, double *dSdx, double *Xp_out, double *Xm_out, int64_t *iters,
                                             int *flag) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    RC(need_model(h));
    if (!rhs_plus || !rhs_minus || !dSdx || !iters || !flag) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(ssh_fields_current(h));                                   // (before the solves, not only at the scatter)
    RC(ssh_force_core(h, rhs_plus, rhs_minus, iters, flag, batch_pair(h, use_precond, tol_power)));
    double *dF = nullptr; size_t nf = 0;
    RC(ssh_scatter_fields(h, &dF, &nf));
    std::vector<double> F(nf);
    if (nf) HIPCHK(hipMemcpyAsync(F.data(), dF, nf * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RC(ssh_solutions_out(h, Xp_out, Xm_out));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < nf; ++i) dSdx[i] -= F[i];         // the reference accumulates into hmc.dSdx (HMC.jl:808)
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// muldMdx!(dMdx, u, model, v): ⟨∂M/∂x⟩ = uᵀ(∂M/∂x)v per field, for caller-given u and v — the operator calc_dSfdx! (HMC.jl:799,804)
// and LangevinDynamics.calc_dSfdx! (:378) call; HolsteinModels.jl:691-755, SSHModels.jl:707-829
// ------------------------------------------------------------------------------------------

// u, v, x, dMdx: device pointers, reference layout; lambda, lambda2: host double[nsites]
extern "C" int elph_muldMdx_holstein_dev(elph_handle h, double *dMdx_dev, const double *u_dev, const double *v_dev, const double *x_dev,
                                         const double *lambda, const double *lambda2, double dtau) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    RC(need_model(h));
    if (!dMdx_dev || !u_dev || !v_dev || !x_dev || !lambda || !lambda2) { elph_set_error("null argument"); return ELPH_E_ARG; }
    if (h->nchains != 1) { elph_set_error("muldMdx! acts on one phonon configuration; the handle holds %d chains", h->nchains); return ELPH_E_STATE; }
    RC(elph_work_reserve(h, 2));
    const size_t nd = (size_t)h->ndim;
    RC(elph_i_holstein_upload_params(h, lambda, lambda2, nullptr));
    RC(elph_launch_r2s(h, h->work.xfield, x_dev, 1));
    RC(elph_launch_r2s(h, h->work.b, u_dev, 1));
    RC(elph_launch_r2s(h, h->work.b + nd, v_dev, 1));
    RC(elph_launch_dmdx_holstein(h, h->work.tmp, h->work.b, h->work.b + nd, h->work.xfield, dtau, 1.0));
    RC(elph_launch_s2r(h, dMdx_dev, h->work.tmp, 1));
    HIPCHK(hipStreamSynchronize(h->stream));           // lambda / lambda2 are the caller's host arrays
    return ELPH_OK;
}

extern "C" int elph_muldMdx_holstein(elph_handle h, double *dMdx, const double *u, const double *v, const double *x,
                                     const double *lambda, const double *lambda2, double dtau) {
    CHECK_H(h);
    if (!dMdx || !u || !v || !x) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_work_reserve(h, 3));                         // stage_in: u, v, x
    const size_t nd = (size_t)h->ndim, bytes = nd * sizeof(double);
    HIPCHK(hipMemcpyAsync(h->work.stage_in, u, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->work.stage_in + nd, v, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->work.stage_in + 2 * nd, x, bytes, hipMemcpyHostToDevice, h->stream));
    RC(elph_muldMdx_holstein_dev(h, h->work.stage_out, h->work.stage_in, h->work.stage_in + nd, h->work.stage_in + 2 * nd, lambda, lambda2, dtau));
    HIPCHK(hipMemcpyAsync(dMdx, h->work.stage_out, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// the bond brackets q[tau][n] of muldMdx!(·, u, ssh, v) left in h->work.p (u, v: device, reference layout)
static int ssh_dmdx_core(elph_handle_s *h, const double *u_dev, const double *v_dev) {
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    RC(need_model(h));
    if (!u_dev || !v_dev) { elph_set_error("null argument"); return ELPH_E_ARG; }
    if (h->nchains != 1) { elph_set_error("muldMdx! acts on one phonon configuration; the handle holds %d chains", h->nchains); return ELPH_E_STATE; }
    RC(elph_i_ssh_bracket_capacity(h, 2, 1));          // no-op when u_dev, v_dev are the handle's own staging (ssh_dmdx_stage)
    const size_t nd = (size_t)h->ndim;
    RC(elph_launch_r2s(h, h->work.b, u_dev, 1));
    RC(elph_launch_r2s(h, h->work.b + nd, v_dev, 1));
    return elph_launch_force_ssh(h, h->work.p, h->work.b + nd, h->work.b, 1);      // b0 = e^{Δτμ} v(τ−1), c0 = CBᵀ u
}

static int ssh_dmdx_stage(elph_handle_s *h, const double *u, const double *v) {
    if (!u || !v) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_i_ssh_bracket_capacity(h, 2, 1));
    const size_t nd = (size_t)h->ndim, bytes = nd * sizeof(double);
    HIPCHK(hipMemcpyAsync(h->work.stage_in, u, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->work.stage_in + nd, v, bytes, hipMemcpyHostToDevice, h->stream));
    return ssh_dmdx_core(h, h->work.stage_in, h->work.stage_in + nd);
}

extern "C" int elph_muldMdx_ssh(elph_handle h, double *q_out, const double *u, const double *v) {
    CHECK_H(h);
    if (!q_out) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(ssh_dmdx_stage(h, u, v));
    return ssh_brackets_out(h, q_out);
}

extern "C" int elph_muldMdx_ssh_fields(elph_handle h, double *dMdx, const double *u, const double *v) {
    CHECK_H(h);
    if (!dMdx) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(ssh_dmdx_stage(h, u, v));
    double *dF = nullptr; size_t nf = 0;
    RC(ssh_scatter_fields(h, &dF, &nf));
    if (nf) HIPCHK(hipMemcpyAsync(dMdx, dF, nf * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_muldMdx_ssh_fields_dev(elph_handle h, double *dMdx_dev, const double *u_dev, const double *v_dev) {
    CHECK_H(h);
    if (!dMdx_dev) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(ssh_dmdx_core(h, u_dev, v_dev));
    double *dF = nullptr; size_t nf = 0;
    RC(ssh_scatter_fields(h, &dF, &nf));
    if (nf) HIPCHK(hipMemcpyAsync(dMdx_dev, dF, nf * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return ELPH_OK;
}
