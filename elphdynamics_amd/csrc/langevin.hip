// langevin.hip — Langevin dynamics (LangevinDynamics.jl) on the device.  Shares the HMC state (x, scratch vectors, ω, ω₄, the
// accelerator table, here FourierAccelerator.Q) and its helpers (hmc_dev.h).
//   calc_dSdx! = calc_dSfdx! (:350-384: one solve MᵀM x = Mᵀg — M x = g on a BiCGStab / GMRES handle —, dSf/dx = -2 gᵀ(∂M/∂x)M⁻¹g, the flag is ignored) + shifted
//                calc_dSbdx! (:334-344)
//   evolve!    = EulerDynamics (:81-130), RungeKuttaDynamics (:162-232), HeunsDynamics (:272-328)

#include "hmc_dev.h"

using namespace hmc;

namespace {

__global__ void __launch_bounds__(TPB) k_lv_axpby(double *__restrict__ out, double a, const double *__restrict__ x, double b,
                                                  const double *__restrict__ y, double c, const double *__restrict__ z, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) out[i] = a * x[i] + b * y[i] + (z ? c * z[i] : 0.0);
}

int axpby(elph_handle_s *h, double *out, double a, const double *x, double b, const double *y, double c, const double *z, long long n) {
    hipLaunchKernelGGL(k_lv_axpby, dim3(nblk(n)), dim3(TPB), 0, h->stream, out, a, x, b, y, c, z, n);
    return chk("k_lv_axpby");
}

// dS (layout S) = calc_dSdx!(x; g) for every chain (g: [nch][Ndim] on the host, NULL: the next batch); per-chain iteration counts and flags
int langevin_force(elph_handle_s *h, HmcState *st, double *dS, const double *g_host, int use_precond, const double *bmax,
                   const double *bmin, int64_t *iters, int *flag) {
    const size_t nd = (size_t)h->ndim;
    const int nch = st->nch;
    RC(randn_vectors(h, st, st->R2, g_host, nch));                              // g in layout S
    if (use_precond) RC(elph_kpm_setup_chains(h, bmax, bmin, nullptr, nullptr, nullptr, nullptr, nullptr));   // setup!(P), :366
    HIPCHK(hipMemsetAsync(h->work.x, 0, (size_t)nch * nd * sizeof(double), h->stream));   // fill!(M⁻¹g, 0), :367
    h->x_zero = true;
    std::vector<double> res((size_t)nch);
    if (h->solver_kind != ELPH_SOLVER_CG) {      // the mul_by_M branch: M x = g itself, with the Left side (:369-372)
        RC(elph_i_mldiv_core(h, 0, nch, use_precond ? 1 : 0, 0, h->work.x, st->R2, iters, res.data(), flag));
    } else {
        RC(elph_launch_mul(h, 1, h->work.b, st->R2, nch));                         // Mᵀg (model.v″, :378)
        RC(elph_i_ldiv_core(h, nch, use_precond ? 1 : 0, 0, iters, res.data(), flag));
    }
    if (st->ssh) {      // muldMdx!(dSfdx, g, ssh, M⁻¹g) (SSHModels.jl:707-829) with u = g given; no shifted term for bond phonons
        RC(elph_launch_force_ssh(h, h->work.p, h->work.x, st->R2, nch));
        RC(elph_launch_ssh_scatter(h, dS, h->work.p, st->x, h->d_ssh_par, h->d_ssh_cb, st->nf, st->dtau, 1, -2.0, nch));
        RC(alias_sum(h, st, dS));
        return add_dsb(h, st, dS, 1);
    }
    RC(elph_launch_dmdx_holstein(h, dS, st->R2, h->work.x, st->x, st->dtau, -2.0, nch));   // -2 gᵀ(∂M/∂x)M⁻¹g, :381-384
    return add_dsb(h, st, dS, 1, h->d_lam);                                                // calc_dSbdx!(dSdx, model, true), :341
}

}  // namespace

// LangevinDynamics on a Holstein handle: same arguments as elph_hmc_create, with fa_Q = FourierAccelerator.Q (evolve! calls
// fourier_accelerate! without use_mass).  elph_hmc_set_state / elph_hmc_get_state move the field x.
extern "C" int elph_langevin_create(elph_handle h, const double *omega, const double *omega4, const double *lambda,
                                    const double *lambda2, const double *mu, double dtau, const double *fa_Q) {
    return elph_hmc_create_chains(h, 1, omega, omega4, lambda, lambda2, mu, dtau, fa_Q);
}

// nchains independent Langevin trajectories of one deck in lockstep (every step one batched solve of nchains right-hand sides,
// one KPM expansion per chain); state and random vectors are chain-major: x, eta [nchains*Ndof], g1, g2 [nchains*Ndim],
// kpm_randn [2 set-ups][b_max|b_min][nchains][nsites]; iters, flag [nchains].
extern "C" int elph_langevin_create_chains(elph_handle h, int nchains, const double *omega, const double *omega4, const double *lambda,
                                           const double *lambda2, const double *mu, double dtau, const double *fa_Q) {
    return elph_hmc_create_chains(h, nchains, omega, omega4, lambda, lambda2, mu, dtau, fa_Q);
}

// The same for an SSH handle: the arguments of elph_hmc_create_ssh with fa_Q (per phonon) in place of the mass table.
extern "C" int elph_langevin_create_ssh(elph_handle h, int64_t nph, const double *omega, const double *omega4, const int64_t *cb_index,
                                        const double *t_ph, const double *alpha, const double *alpha2, const double *t_bare_cb,
                                        const double *mu, double dtau, const double *fa_Q) {
    return elph_hmc_create_ssh(h, nph, omega, omega4, cb_index, t_ph, alpha, alpha2, t_bare_cb, mu, dtau, fa_Q);
}

// evolve!(model, dyn, fa, P): scheme 0 Euler, 1 Runge-Kutta, 2 Heun.  The random numbers the reference draws are inputs:
// eta [Ndof] (randn!(η, model)), g1, g2 [Ndim] (the noise vectors of the first / second force estimate; g2 unused by Euler),
// kpm_randn [2][2][nsites] (b_max, b_min of the first and second setup!(P); NULL without preconditioner).
// iters: the count evolve! returns (Euler: the solve; RK: the second solve; Heun: div(it1 + it2, 2)); flag: last ldiv! flag
// (the reference ignores it: a failed solve contributes M⁻¹g = 0).
extern "C" int elph_langevin_evolve(elph_handle h, int scheme, double dt, int use_precond, const double *eta, const double *g1,
                                    const double *g2, const double *kpm_randn, int64_t *iters, int *flag) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st, true));
    if (scheme < 0 || scheme > 2 || !(dt > 0.0)) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(need_randoms(st, eta && g1 && (scheme == 0 || g2) && (!use_precond || kpm_randn), "eta, g1 (g2 beyond Euler, kpm_randn with a preconditioner)"));
    if (use_precond && !h->kpm.created) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    const int nch = st->nch;
    RC(elph_work_reserve(h, std::max(2, 2 * nch)));
    RC(elph_i_reserve_chains(h, nch));
    const size_t N = (size_t)h->N;
    const long long n = (long long)st->nf * h->L * nch;      // field vectors of all chains (Holstein: nch * ndim)
    const double s2 = sqrt(2.0 * dt);
    std::vector<double> kpm_own;
    RC(update_model(h, st));
    RC(randn_vectors(h, st, st->v, eta, nch, st->nf));
    if (use_precond) RC(given_or_drawn(st, &kpm_randn, kpm_own, 4 * (size_t)nch * N, true));
    // start vectors of the two set-ups: [set-up][b_max | b_min][chain][N]
    const double *bm1 = kpm_randn, *bn1 = kpm_randn ? kpm_randn + (size_t)nch * N : nullptr;
    const double *bm2 = kpm_randn ? kpm_randn + 2 * (size_t)nch * N : nullptr, *bn2 = kpm_randn ? kpm_randn + 3 * (size_t)nch * N : nullptr;
    double *F1 = st->dS, *F2 = st->y, *xi = st->v, *dx = st->v0;      // the momentum buffers are free: Langevin has none
    std::vector<int64_t> it1((size_t)nch, 0), it2((size_t)nch, 0);
    std::vector<int> fl((size_t)nch, 0);
    if (scheme == 0) {
        RC(langevin_force(h, st, F1, g1, use_precond, bm1, bn1, it1.data(), fl.data()));
        RC(fa(h, st, F1, F1, 1.0));
        RC(fa(h, st, xi, xi, 0.5));
        RC(axpby(h, st->x, 1.0, st->x, s2, xi, -dt, F1, n));                       // x += √(2Δt) Q^½η − Δt Q dS/dx
    } else if (scheme == 1) {
        RC(langevin_force(h, st, F1, g1, use_precond, bm1, bn1, it1.data(), fl.data()));
        RC(axpby(h, dx, s2, xi, -dt, F1, 0.0, nullptr, n));                        // Δx = √(2Δt) η − Δt dS/dx   (no acceleration)
        RC(axpby(h, st->x, 1.0, st->x, 1.0, dx, 0.0, nullptr, n));
        RC(update_model(h, st));
        RC(langevin_force(h, st, F2, g2, use_precond, bm2, bn2, it2.data(), fl.data()));
        RC(axpby(h, st->x, 1.0, st->x, -1.0, dx, 0.0, nullptr, n));                // x = x′ − Δx
        RC(axpby(h, F1, 0.5, F2, 0.5, F1, 0.0, nullptr, n));                       // (dSdx′ + dSdx)/2
        RC(fa(h, st, F1, F1, 1.0));
        RC(fa(h, st, xi, xi, 0.5));
        RC(axpby(h, st->x, 1.0, st->x, s2, xi, -dt, F1, n));
        it1 = it2;
    } else {
        RC(fa(h, st, xi, xi, 0.5));                                                // ξ = Q^½η
        RC(langevin_force(h, st, F1, g1, use_precond, bm1, bn1, it1.data(), fl.data()));
        RC(fa(h, st, F1, F1, 1.0));                                                // dΓ/dx
        RC(axpby(h, dx, s2, xi, -dt, F1, 0.0, nullptr, n));
        RC(axpby(h, st->x, 1.0, st->x, 1.0, dx, 0.0, nullptr, n));
        RC(update_model(h, st));
        RC(langevin_force(h, st, F2, g2, use_precond, bm2, bn2, it2.data(), fl.data()));
        RC(fa(h, st, F2, F2, 1.0));
        RC(axpby(h, st->x, 1.0, st->x, -1.0, dx, 0.0, nullptr, n));                // x = x′ − Δx
        RC(axpby(h, F1, 0.5, F1, 0.5, F2, 0.0, nullptr, n));                       // (dΓ + dΓ′)/2
        RC(axpby(h, st->x, 1.0, st->x, s2, xi, -dt, F1, n));
        for (int c = 0; c < nch; ++c) it1[(size_t)c] = (it1[(size_t)c] + it2[(size_t)c]) / 2;
    }
    RC(update_model(h, st));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < nch; ++c) {
        if (iters) iters[c] = it1[(size_t)c];
        if (flag) flag[c] = fl[(size_t)c];
    }
    return ELPH_OK;
}
