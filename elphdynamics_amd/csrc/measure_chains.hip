// measure_chains.hip — the Holstein measurements of measure.hip for EVERY chain resident in the handle at once (DESIGN.md "Measurements
// of resident chains"): the chain is a grid axis of every kernel, so the launches of one accumulate depend on the vectors per chain and
// on the request, not on the number of chains.
//   make_measurements!            Measurements.jl:545-566   per chain, without its update!
//     make_global_measurements!   :845-861, :1283-1312      make_onsite_measurements! :916-976      make_intersite_measurements! :1029-1070
//     measure_Greens! / _DenDen! / _SpinSpin! / _PairGreens! / _PhononGreens!   :1469-1650
//   reset_measurements!           :698-758
// What a workgroup computes is measure.hip's (meas_holstein_dev.h), and so is the rule of the reductions: one fixed order, partials per
// slice added in slice order, no floating-point atomics.  A workgroup reads one chain's field, parameters, vectors and tables only, so
// chain c's numbers depend on nothing of another chain.
//
// Layouts.  Vector v (0-based) of chain c is row v nchains + c of the estimator (greens.chain_vector), so the v-th vectors of all chains
// are one block [chain][ndim].  The accumulator is ONE allocation [chain][scalars | Greens | DenDen | SpinSpin | PairGreens |
// PhononGreens], a chain's block exactly what elph_meas_fetch returns: reset is one memset, fetch one copy.  mu is [chain][N] (a tuner per
// chain moves it, elph_hmc_set_mu_chains); omega, omega4, lambda and the bonds are the model's.  The estimator's pipeline for one pair of
// vectors of all chains runs in scratch this state owns (elph_i_greens_setup_chains_dev): its four real tables come out
// [table][chain][L][n_s N], which meas_fold reads with a table stride.

#include <vector>

#include "corr_req.h"
#include "elph_internal.h"
#include "meas_holstein_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int NWAVE = MEAS_NWAVE;
constexpr int NCORR = MS_NCORR;
const char *const CORR_NAMES[NCORR] = {"Greens", "DenDen", "SpinSpin", "PairGreens", "PhononGreens"};
const CorrWords WORDS = {"chain measurements", "orbital", "with no orbital pair"};

struct MeasChainsState {
    int nchains = 1, ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0, nsc = 0;
    int64_t nbonds = 0;
    double dtau = 0.0;
    double *par = nullptr;          // [3][N] omega, omega4, lambda
    double *mu = nullptr;           // [nchains][N], then [nchains] the rows' means
    int *bs = nullptr;              // [2][nbonds] 0-based sites of every bond, the reference's bond order
    double *bt = nullptr;           // [nbonds]
    CorrPlan<NCORR> cr;             // ONE chain's plan: cr.total doubles per chain; cr.acc: [nchains][cr.total], cr.req bound to chain 0
    double *xr = nullptr;           // [nchains][ndim] staging of the fields as they arrive (reference layout): the handle's solver
                                    // workspace is not grown for a measurement
    double *x = nullptr;            // [nchains][ndim] the fields, layout S
    double *ph = nullptr;           // [nchains][L][ns*N] the fields' translation averages (PhononGreens requested)
    double *xs = nullptr;           // [nchains][MS_NXONLY][ns] the field-only on-site terms of this accumulate, normalised
    double *part = nullptr;         // [nchains][L][nqmax] one partial per workgroup
    int nqmax = 0;
    ElphGreensChainScratch gs{};    // the estimator's pipeline for all chains
};

MeasChainsState *mc_of(elph_handle_s *h) { return (MeasChainsState *)h->meas_chains; }

// ---- the kernels of measure.hip with the chain as the last grid axis
__global__ void __launch_bounds__(TPB) k_mc_x(double *__restrict__ part, const double *__restrict__ x, const double *__restrict__ par,
                                              const double *__restrict__ mu, int N, int L, int ns, int nc, int nqmax, double dtau) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.y;
    ms_x_slice(part + ch * L * nqmax, x + ch * L * N, par, par + N, mu + ch * N, N, L, ns, nc, dtau, blockIdx.x, red);
}

__global__ void __launch_bounds__(TPB) k_mc_x_finish(double *__restrict__ xs, const double *__restrict__ part, int L, int ns, int nqmax, double norm) {
    const size_t ch = blockIdx.x;
    ms_x_finish(xs + ch * MS_NXONLY * ns, part + ch * L * nqmax, L, ns, norm);
}

__global__ void __launch_bounds__(TPB) k_mc_pair(double *__restrict__ part, ElphGreensPair v, const double *__restrict__ x,
                                                 const double *__restrict__ lam, const int *__restrict__ bs, const double *__restrict__ bt, int N,
                                                 int L, int ns, int nc, int ndef, long long nbonds, int nqmax) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.y, o = ch * L * N;
    ms_pair_slice(part + ch * L * nqmax, v.X1 + o, v.X2 + o, v.R1 + o, v.R2 + o, x + o, lam, bs, bt, N, ns, nc, ndef, nbonds, blockIdx.x, red);
}

// C3: table 3 (G[D,0] G[0,D]) of chain 0; mu_mean: [nchains]; block: doubles of a chain's accumulators
__global__ void __launch_bounds__(TPB) k_mc_finish(double *__restrict__ acc, const double *__restrict__ part, const double *__restrict__ xs,
                                                   const double *__restrict__ C3, const double *__restrict__ mu_mean, int N, int L, int ns, int nc,
                                                   int ndef, int nqmax, size_t block) {
    extern __shared__ double tot[];                    // [nq] + red[NWAVE]
    const size_t ch = blockIdx.x;
    ms_finish(acc + ch * block, part + ch * L * nqmax, xs + ch * MS_NXONLY * ns, C3 + ch * L * ns * N, N, L, ns, nc, ndef, mu_mean[ch], tot);
}

// One thread per (tau, cell, listed pair) of correlation blockIdx.y of chain blockIdx.z.  C: [table][chain][L][ns N]
__global__ void __launch_bounds__(TPB) k_mc_fold(CorrReq<NCORR> rq, const double *__restrict__ C, const double *__restrict__ ph, int N, int L, int ns,
                                                 int L1, int L2, int L3, int nchains, size_t block) {
    const size_t ch = blockIdx.z, tab = (size_t)L * ns * N;
    ms_fold(rq, blockIdx.y, (long long)blockIdx.x * TPB + threadIdx.x, C + ch * tab, ph, N, L, ns, L1, L2, L3, (size_t)nchains * tab, ch * block,
            ch * tab);
}

// mu[nchains][N] and, behind it, mean(model.mu) of every chain's row (:858)
int upload_mu(MeasChainsState *m, const double *mu, int N) {
    const size_t nch = (size_t)m->nchains;
    std::vector<double> mum(nch);
    for (size_t c = 0; c < nch; ++c) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += mu[c * N + i];
        mum[c] = s / N;
    }
    RC(corr_up(m->mu, mu, nch * N * sizeof(double)));
    return corr_up(m->mu + nch * N, mum.data(), nch * sizeof(double));
}

int need_state(elph_handle_s *h) { return corr_need(h->meas_chains, "elph_meas_chains_create"); }

}  // namespace

void elph_meas_chains_free(elph_handle_s *h) {
    MeasChainsState *m = mc_of(h);
    if (!m) return;
    corr_free({m->par, m->mu, m->bs, m->bt, m->cr.pairs, m->cr.acc, m->xr, m->x, m->ph, m->xs, m->part});
    elph_i_greens_chain_scratch_free(&m->gs);
    delete m;
    h->meas_chains = nullptr;
}

extern "C" int elph_meas_chains_create(elph_handle h, int nchains, const double *omega, const double *omega4, const double *lambda, const double *mu,
                                       double dtau, int64_t nbonds, int ndef, const int64_t *bond_sites, const double *bond_t, const int *measure,
                                       const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_meas_chains_free(h);
    RC(corr_refuse_model(h, WORDS.prefix));
    if (nchains < 1 || nchains != h->nchains) {
        elph_set_error("chain measurements: created for %d chains, %d are resident in this handle", nchains, h->nchains);
        return ELPH_E_ARG;
    }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    const int N = (int)h->N, L = (int)h->L, ns = g.ns, nc = g.nc;
    std::vector<int> bs;
    RC(corr_check_onsite_params(h, WORDS.prefix, nc, omega, omega4, lambda, mu, dtau, nbonds, ndef, bond_sites, bond_t, measure, time_dependent, npairs, bs));
    const int nsc = 3 + MS_NONSITE * ns + ndef;
    CorrPlan<NCORR> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, WORDS, CORR_NAMES, measure, time_dependent, npairs, pairs, ns, L, nc, (size_t)nsc));
    MeasChainsState *m = new MeasChainsState;
    h->meas_chains = m;
    m->cr = plan;
    m->nchains = nchains; m->ns = ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = ndef; m->nbonds = nbonds; m->dtau = dtau; m->nsc = nsc;
    m->nqmax = std::max(3 * ns + 2 + ndef, MS_NXONLY * ns);
    const size_t nch = (size_t)nchains, nd = (size_t)h->ndim, ncol = (size_t)ns * N;
    const bool phonon = m->cr.req.np[MS_PHONONGREENS] != 0;
    CorrFirstError ok;
    const bool allocated = ok(corr_alloc(&m->par, 3 * (size_t)N)) && ok(corr_alloc(&m->mu, nch * N + nch)) && ok(corr_alloc(&m->bs, 2 * (size_t)nbonds)) &&
        ok(corr_alloc(&m->bt, (size_t)nbonds)) && ok(corr_alloc(&m->cr.pairs, m->cr.prs.size())) && ok(corr_alloc(&m->cr.acc, nch * m->cr.total)) &&
        ok(corr_alloc(&m->xr, nch * nd)) && ok(corr_alloc(&m->x, nch * nd)) && ok(corr_alloc(&m->xs, nch * MS_NXONLY * ns)) && ok(corr_alloc(&m->part, nch * L * m->nqmax)) &&
        (!phonon || ok(corr_alloc(&m->ph, nch * L * ncol))) && ok(elph_i_greens_chain_scratch_alloc(h, nchains, &m->gs));
    if (!allocated) { elph_meas_chains_free(h); return ok.rc; }
    const double *pp[3] = {omega, omega4, lambda};
    for (int k = 0; k < 3; ++k) ok(corr_up(m->par + (size_t)k * N, pp[k], (size_t)N * sizeof(double)));
    ok(upload_mu(m, mu, N));
    ok(corr_up(m->bs, bs.data(), bs.size() * sizeof(int)));
    ok(corr_up(m->bt, bond_t, (size_t)nbonds * sizeof(double)));
    if (ok.rc == ELPH_OK) ok(corr_upload(m->cr, WORDS.prefix));       // the pairs; zeroes chain 0's block and binds req to it
    if (ok.rc == ELPH_OK && hipMemset(m->cr.acc, 0, nch * m->cr.total * sizeof(double)) != hipSuccess) {
        elph_set_error("chain measurements: hipMemset failed");
        ok(ELPH_E_HIP);
    }
    if (ok.rc != ELPH_OK) elph_meas_chains_free(h);
    return ok.rc;
}

extern "C" int elph_meas_chains_set_mu(elph_handle h, const double *mu) {
    CHECK_H(h);
    RC(need_state(h));
    if (!mu) { elph_set_error("chain measurements: mu is null"); return ELPH_E_ARG; }
    HIPCHK(hipStreamSynchronize(h->stream));
    return upload_mu(mc_of(h), mu, (int)h->N);
}

// Everything one accumulate queues on the handle's stream, the copy of the host's X first; the caller synchronises, whatever this returns.
static int accumulate_launches(elph_handle_s *h, MeasChainsState *m, const ElphGreensView &g, const double *X) {
    const int nch = m->nchains, N = (int)h->N, L = (int)h->L, ns = m->ns, nc = m->nc, nvc = g.nv / nch, nqmax = m->nqmax;
    // the tau-DFT launchers read their tables and the buffers they are handed, whatever the batch: nothing of the handle's workspace is used
    HIPCHK(hipMemcpyAsync(m->xr, X, (size_t)nch * (size_t)h->ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_r2s(h, m->x, m->xr, nch));
    const double *mu = m->mu, *mu_mean = m->mu + (size_t)nch * N;
    const double norm = (double)nc * (double)L;
    // what depends on the fields alone: once per call, added once per pair below
    hipLaunchKernelGGL(k_mc_x, dim3((unsigned)L, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, m->x, m->par, mu, N, L, ns, nc, nqmax, m->dtau);
    RC(elph_launch_check("k_mc_x"));
    hipLaunchKernelGGL(k_mc_x_finish, dim3((unsigned)nch), dim3(TPB), 0, h->stream, m->xs, m->part, L, ns, nqmax, norm);
    RC(elph_launch_check("k_mc_x_finish"));
    if (m->cr.req.np[MS_PHONONGREENS]) RC(elph_i_greens_autocorr_chains_dev(h, m->gs, m->ph, m->x));
    const int nq = 3 * ns + 2 + m->ndef;
    const size_t shm = ((size_t)nq + NWAVE) * sizeof(double);
    const size_t tab = (size_t)L * ns * N, block = m->cr.total;
    for (int i = 1; i < nvc; ++i)
        for (int j = i + 1; j <= nvc; ++j) {           // pairs of a chain's vectors; every launch serves all chains
            ElphGreensPair v;
            RC(elph_i_greens_setup_chains_dev(h, m->gs, i, j, &v));
            hipLaunchKernelGGL(k_mc_pair, dim3((unsigned)L, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, v, m->x, m->par + 2 * (size_t)N, m->bs, m->bt,
                               N, L, ns, nc, m->ndef, (long long)m->nbonds, nqmax);
            RC(elph_launch_check("k_mc_pair"));
            hipLaunchKernelGGL(k_mc_finish, dim3((unsigned)nch), dim3(TPB), shm, h->stream, m->cr.acc, m->part, m->xs, m->gs.C + 3 * (size_t)nch * tab,
                               mu_mean, N, L, ns, nc, m->ndef, nqmax, block);
            RC(elph_launch_check("k_mc_finish"));
            if (m->cr.fold_max) {
                hipLaunchKernelGGL(k_mc_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), NCORR, (unsigned)nch), dim3(TPB), 0, h->stream, m->cr.req,
                                   m->gs.C, m->ph, N, L, ns, m->L1, m->L2, m->L3, nch, block);
                RC(elph_launch_check("k_mc_fold"));
            }
        }
    return ELPH_OK;
}

extern "C" int elph_meas_chains_accumulate(elph_handle h, const double *X) {
    CHECK_H(h);
    RC(need_state(h));
    if (!X) { elph_set_error("X is null"); return ELPH_E_ARG; }
    MeasChainsState *m = mc_of(h);
    const int nch = m->nchains;
    if (h->nchains != nch) {
        elph_set_error("chain measurements: created for %d chains, %d are resident in this handle now", nch, h->nchains);
        return ELPH_E_STATE;
    }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (g.nv % nch) {
        elph_set_error("chain measurements: the estimator's %d vectors are not a multiple of the %d resident chains", g.nv, nch);
        return ELPH_E_STATE;
    }
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    const int rc = accumulate_launches(h, m, g, X);
    const hipError_t e = hipStreamSynchronize(h->stream);      // on every path: X (a host pointer) is not retained after return
    if (rc == ELPH_OK && e != hipSuccess) { elph_set_error("chain measurements: hipStreamSynchronize -> %s", hipGetErrorString(e)); return ELPH_E_HIP; }
    return rc;
}
 extern "C" int elph_meas_chains_fetch(elph_handle h, int chain, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                                      double *PhononGreens) {
    CHECK_H(h);
    RC(need_state(h));
    MeasChainsState *m = mc_of(h);
    if (chain < 0 || chain >= m->nchains) { elph_set_error("chain measurements: chain %d outside 0..%d", chain, m->nchains - 1); return ELPH_E_ARG; }
    CorrPlan<NCORR> one = m->cr;                       // the chain's block, laid out as the plan says
    one.acc = m->cr.acc + (size_t)chain * m->cr.total;
    std::vector<double> host;
    double *outs[NCORR] = {Greens, DenDen, SpinSpin, PairGreens, PhononGreens};
    RC(corr_fetch(h, one, host, outs));
    if (scalars)
        for (int i = 0; i < m->nsc; ++i) scalars[i] = host[(size_t)i];
    return ELPH_OK;
}

extern "C" int elph_meas_chains_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_state(h));
    const MeasChainsState *m = mc_of(h);
    HIPCHK(hipMemsetAsync(m->cr.acc, 0, (size_t)m->nchains * m->cr.total * sizeof(double), h->stream));
    return ELPH_OK;
}
