// ssh_measure_chains.hip — the bond-phonon (SSH) measurements of ssh_measure.hip for EVERY chain resident in the handle at once
// (DESIGN.md "Measurements of resident chains"): the chain is the last grid axis of every kernel, so the launches of one accumulate
// depend on the vectors per chain and on the request, not on the number of chains.
//   make_measurements!             Measurements.jl:545-566   per chain, without its update!
//     make_global_measurements!    :845-861, :1283-1312      make_onsite_measurements! :978-1024      make_intersite_measurements! :1072-1155
//     measure_Greens! / _DenDen! / _SpinSpin! / _PairGreens!  :1469-1596      measure_PhononGreens! :2488-2541
//   reset_measurements!            :698-758
// What a workgroup computes is ssh_measure.hip's (meas_ssh_dev.h), and so is the rule of the reductions: one fixed order, partials per
// slice added in slice order, no floating-point atomics.  A workgroup reads one chain's field, mu, vectors and tables only, so chain c's
// numbers depend on nothing of another chain.  One accumulate adds its pairs of vectors up from zero in a buffer of its own (cur) and adds
// that to the accumulators once at the end: two accumulations of the same inputs are twice one, to the bit.
//
// Layouts.  Vector v (0-based) of chain c is row v nchains + c of the estimator (greens.chain_vector), so the v-th vectors of all chains
// are one block [chain][ndim].  The fields arrive as X[chain][Nph][L] (the reference's layout per chain) and become [chain][L][Nph]; their
// half spectra are [chain][Lh][Nph], the per-frequency correlations of the listed phonon-type pairs [chain][nP][Lh][nc] and their
// translation averages [chain][nP][L][nc], each one batched tau-transform.  The accumulator is ONE allocation [chain][scalars | Greens |
// DenDen | SpinSpin | PairGreens | PhononGreens], a chain's block exactly what elph_ssh_meas_fetch returns: reset is one memset, fetch one
// copy; cur has the same shape.  Of mu the kernels need its means alone: [chain][n_s] over the sites of an orbital, then [chain] over all
// sites, made on the host at create and at set_mu (a tuner per chain moves mu, elph_hmc_set_mu_chains).  The bonds, the phonon parameters
// and the definition lists are the model's.  The estimator's pipeline for one pair of vectors of all chains runs in scratch this state
// owns (elph_i_greens_setup_chains_dev): its four real tables come out [table][chain][L][n_s N], which meas_fold reads with a table
// stride.  Nothing of the handle's solver workspace is grown or used.

#include <vector>

#include "corr_req.h"
#include "elph_internal.h"
#include "meas_ssh_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int NWAVE = MEAS_NWAVE;
constexpr int NCORR = SM_NCORR;
const char *const CORR_NAMES[NCORR] = {"Greens", "DenDen", "SpinSpin", "PairGreens", "PhononGreens"};
constexpr int PHONONGREENS = SM_PHONONGREENS;
const CorrWords WORDS = {"SSH chain measurements", "orbital", "with no orbital pair", PHONONGREENS, "phonon type", "with no pair of phonon types"};

struct SshMeasChainsState {
    int nchains = 1, ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0, nph = 0, nsc = 0, nqmax = 0;
    int64_t nbonds = 0, Nph = 0;
    double dtau = 0.0, V = 1.0;
    int *bs = nullptr;              // [2][nbonds] 0-based sites of every bond, the reference's bond order
    int *bph = nullptr;             // [nbonds] 0-based phonon of the bond, -1 on a bare bond
    double *bpar = nullptr;         // [SM_NBPAR][nbonds]
    int *doff = nullptr;            // [ndef + 1] offsets into dlist
    int *dlist = nullptr;           // [nbonds] the bonds of every definition, in bond order
    double *mu = nullptr;           // [nchains][ns] mean of a chain's mu over the sites of an orbital, then [nchains] its mean over all sites
    CorrPlan<NCORR> cr;             // ONE chain's plan: cr.total doubles per chain; cr.acc: [nchains][cr.total], cr.req bound to chain 0
    double *cur = nullptr;          // [nchains][cr.total] this accumulate's sums
    CorrReq<NCORR> rq_cur{};        // cr.req with its accumulators in chain 0's block of cur
    double *xr = nullptr;           // [nchains][Nph][L] the fields as the caller holds them
    double *x = nullptr;            // [nchains][L][Nph] the fields, layout S
    double *xs = nullptr;           // [nchains][SM_NXONLY][ndef] the field-only terms of this accumulate, normalised
    double *part = nullptr;         // [nchains][L][nqmax] one partial per workgroup
    double2 *nu = nullptr;          // [nchains][Lh][Nph] the fields' half spectra          (PhononGreens requested)
    double2 *Y = nullptr;           // [nchains][nP][Lh][nc] per-frequency correlations of the listed pairs
    double *B = nullptr;            // [nchains][nP][L][nc] the translation averages of this accumulate
    ElphGreensChainScratch gs{};    // the estimator's pipeline for all chains
};

SshMeasChainsState *smc_of(elph_handle_s *h) { return (SshMeasChainsState *)h->ssh_meas_chains; }

// ---- the kernels of ssh_measure.hip with the chain as the last grid axis
__global__ void __launch_bounds__(TPB) k_smc_x(double *__restrict__ part, const double *__restrict__ x, const double *__restrict__ bpar,
                                               const int *__restrict__ bph, const int *__restrict__ doff, const int *__restrict__ dlist, int Nph,
                                               int L, int ndef, long long nbonds, int nqmax, double dtau) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.y;
    sm_x_slice(part + ch * L * nqmax, x + ch * L * Nph, bpar, bph, doff, dlist, Nph, L, ndef, nbonds, dtau, blockIdx.x, red);
}

__global__ void __launch_bounds__(TPB) k_smc_x_finish(double *__restrict__ xs, const double *__restrict__ part, int L, int ndef, int nqmax, double V) {
    const size_t ch = blockIdx.x;
    sm_x_finish(xs + ch * SM_NXONLY * ndef, part + ch * L * nqmax, L, ndef, V);
}

// v: chain 0's vectors; chain c's lie c L N further
__global__ void __launch_bounds__(TPB) k_smc_pair(double *__restrict__ part, ElphGreensPair v, const double *__restrict__ x,
                                                  const int *__restrict__ bs, const double *__restrict__ bpar, const int *__restrict__ bph,
                                                  const int *__restrict__ doff, const int *__restrict__ dlist, int N, int Nph, int L, int ns, int nc,
                                                  int ndef, long long nbonds, int nqmax) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.y, o = ch * L * N;
    sm_pair_slice(part + ch * L * nqmax, v.X1 + o, v.X2 + o, v.R1 + o, v.R2 + o, x + ch * L * Nph, bs, bpar, bph, doff, dlist, N, Nph, ns, nc, ndef,
                  nbonds, blockIdx.x, red);
}

// C3: table 3 (G[D,0] G[0,D]) of chain 0; muo: [nchains][ns]; mu_mean: [nchains]; block: doubles of a chain's accumulators
__global__ void __launch_bounds__(TPB) k_smc_finish(double *__restrict__ acc, const double *__restrict__ part, const double *__restrict__ xs,
                                                    const double *__restrict__ muo, const double *__restrict__ mu_mean,
                                                    const double *__restrict__ C3, int N, int L, int ns, int nc, int ndef, int nqmax, double V,
                                                    size_t block) {
    extern __shared__ double tot[];                    // [nq] + red[NWAVE]
    const size_t ch = blockIdx.x;
    sm_finish(acc + ch * block, part + ch * L * nqmax, xs + ch * SM_NXONLY * ndef, muo + ch * ns, C3 + ch * L * ns * N, N, L, ns, nc, ndef,
              mu_mean[ch], V, tot);
}

// One workgroup per (frequency, listed pair of phonon types, chain).  LDS: 4 buffers of nc complex.
__global__ void __launch_bounds__(TPB) k_smc_ph(double2 *__restrict__ Y, const double2 *__restrict__ nu, const int *__restrict__ pairs, int Lh,
                                                int Nph, int L1, int L2, int L3, const double2 *__restrict__ tw, double norm) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3, k = blockIdx.x, p = blockIdx.y;
    const size_t ch = blockIdx.z, nP = gridDim.y;
    sm_ph(Y + ((ch * nP + p) * Lh + k) * nc, nu + (ch * Lh + k) * Nph, pairs[2 * p], pairs[2 * p + 1], L1, L2, L3, tw, norm, lds);
}

// One thread per (tau, cell, listed pair) of correlation blockIdx.y of chain blockIdx.z.  C: [table][chain][L][ns N]; B: [chain][nP][L][nc]
__global__ void __launch_bounds__(TPB) k_smc_fold(CorrReq<NCORR> rq, const double *__restrict__ C, const double *__restrict__ B, int N, int L, int ns,
                                                  int L1, int L2, int L3, int nchains, size_t block) {
    const size_t ch = blockIdx.z, tab = (size_t)L * ns * N;
    const size_t bch = (size_t)rq.np[PHONONGREENS] * L * L1 * L2 * L3;
    sm_fold(rq, blockIdx.y, (long long)blockIdx.x * TPB + threadIdx.x, C + ch * tab, B + ch * bch, N, L, ns, L1, L2, L3, (size_t)nchains * tab,
            ch * block);
}

__global__ void __launch_bounds__(TPB) k_smc_add(double *__restrict__ acc, const double *__restrict__ cur, long long n) { sm_add(acc, cur, n); }

// of every chain's row of mu[nchains][N]: its mean over the sites of an orbital (:1018), and behind them mean(model.mu) (:858)
int upload_mu(SshMeasChainsState *m, const double *mu, int N) {
    const size_t nch = (size_t)m->nchains, ns = (size_t)m->ns, nc = (size_t)m->nc;
    std::vector<double> means(nch * ns + nch, 0.0);
    for (size_t c = 0; c < nch; ++c) {
        const double *row = mu + c * N;
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += row[i];
        means[nch * ns + c] = s / N;
        for (size_t o = 0; o < ns; ++o) {
            double so = 0.0;
            for (size_t cell = 0; cell < nc; ++cell) so += row[cell * ns + o];
            means[c * ns + o] = so / nc;
        }
    }
    return corr_up(m->mu, means.data(), means.size() * sizeof(double));
}

int need_state(elph_handle_s *h) { return corr_need(h->ssh_meas_chains, "elph_ssh_meas_chains_create"); }

}  // namespace

void elph_ssh_meas_chains_free(elph_handle_s *h) {
    SshMeasChainsState *m = smc_of(h);
    if (!m) return;
    corr_free({m->bs, m->bph, m->bpar, m->doff, m->dlist, m->mu, m->cr.pairs, m->cr.acc, m->cur, m->xr, m->x, m->xs, m->part, m->nu, m->Y, m->B});
    elph_i_greens_chain_scratch_free(&m->gs);
    delete m;
    h->ssh_meas_chains = nullptr;
}

extern "C" int elph_ssh_meas_chains_create(elph_handle h, int nchains, const double *mu, double dtau, int64_t nbonds, int ndef,
                                           const int64_t *bond_sites, const double *bond_t, const int64_t *bond_to_definition,
                                           const int64_t *bond_to_phonon, int64_t Nph, int nph, const double *omega, const double *alpha,
                                           const double *alpha2, const int *measure, const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_ssh_meas_chains_free(h);
    RC(corr_refuse_model(h, WORDS.prefix, ELPH_MODEL_SSH));
    if (nchains < 1 || nchains != h->nchains) {
        elph_set_error("SSH chain measurements: created for %d chains, %d are resident in this handle", nchains, h->nchains);
        return ELPH_E_ARG;
    }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = g.ns, nc = g.nc;
    CorrSshBonds T;
    RC(corr_check_ssh_params(h, WORDS.prefix, mu, dtau, nbonds, ndef, bond_sites, bond_t, bond_to_definition, bond_to_phonon, Nph, nph, omega, alpha,
                             alpha2, measure, time_dependent, npairs, T));
    const int nsc = 3 + SM_NONSITE * ns + SM_NINTER * ndef;
    CorrPlan<NCORR> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, WORDS, CORR_NAMES, measure, time_dependent, npairs, pairs, ns, L, nc, (size_t)nsc, nph));
    const int nP = plan.req.np[PHONONGREENS];
    if (nP) RC(corr_check_phonongreens(WORDS.prefix, nph, Nph, g.L1, g.L2, g.L3, sm_ph_lds_bytes(nc)));
    SshMeasChainsState *m = new SshMeasChainsState;
    h->ssh_meas_chains = m;
    m->cr = plan;
    m->nchains = nchains; m->ns = ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = ndef; m->nph = nph; m->nbonds = nbonds;
    m->Nph = Nph; m->dtau = dtau; m->nsc = nsc;
    m->V = ndef ? (double)(nbonds / ndef) * (double)L : 1.0;           // div(Nbonds, nbonds) * Ltau, :1094
    m->nqmax = std::max(2 * ns + 2 + 2 * ndef, SM_NXONLY * ndef);
    const size_t nch = (size_t)nchains, nx = (size_t)L * (size_t)Nph, total = m->cr.total;
    CorrFirstError ok;
    const bool allocated = ok(corr_alloc(&m->bs, T.bs.size())) && ok(corr_alloc(&m->bph, T.bph.size())) && ok(corr_alloc(&m->bpar, T.bpar.size())) &&
        ok(corr_alloc(&m->doff, T.doff.size())) && ok(corr_alloc(&m->dlist, T.dlist.size())) && ok(corr_alloc(&m->mu, nch * ns + nch)) &&
        ok(corr_alloc(&m->cr.pairs, m->cr.prs.size())) && ok(corr_alloc(&m->cr.acc, nch * total)) && ok(corr_alloc(&m->cur, nch * total)) &&
        ok(corr_alloc(&m->xr, nch * nx)) && ok(corr_alloc(&m->x, nch * nx)) && ok(corr_alloc(&m->xs, nch * SM_NXONLY * ndef)) &&
        ok(corr_alloc(&m->part, nch * L * m->nqmax)) &&
        (nP == 0 || (ok(corr_alloc(&m->nu, nch * Lh * Nph)) && ok(corr_alloc(&m->Y, nch * nP * Lh * nc)) && ok(corr_alloc(&m->B, nch * nP * L * nc)))) &&
        ok(elph_i_greens_chain_scratch_alloc(h, nchains, &m->gs));
    if (!allocated) { elph_ssh_meas_chains_free(h); return ok.rc; }
    ok(corr_up(m->bs, T.bs.data(), T.bs.size() * sizeof(int)));
    ok(corr_up(m->bph, T.bph.data(), T.bph.size() * sizeof(int)));
    ok(corr_up(m->bpar, T.bpar.data(), T.bpar.size() * sizeof(double)));
    ok(corr_up(m->doff, T.doff.data(), T.doff.size() * sizeof(int)));
    ok(corr_up(m->dlist, T.dlist.data(), T.dlist.size() * sizeof(int)));
    ok(upload_mu(m, mu, N));
    if (ok.rc == ELPH_OK) ok(corr_upload(m->cr, WORDS.prefix));        // the pairs; zeroes chain 0's block and binds req to it
    if (ok.rc == ELPH_OK && hipMemset(m->cr.acc, 0, nch * total * sizeof(double)) != hipSuccess) {
        elph_set_error("SSH chain measurements: hipMemset failed");
        ok(ELPH_E_HIP);
    }
    m->rq_cur = m->cr.req;
    for (int c = 0; c < NCORR; ++c) m->rq_cur.acc[c] = m->cur + m->cr.off[c];
    const int lds = (int)sm_ph_lds_bytes(nc);
    if (ok.rc == ELPH_OK && nP && hipFuncSetAttribute((const void *)k_smc_ph, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
        elph_set_error("SSH chain measurements: %d bytes of LDS were refused", lds);
        ok(ELPH_E_HIP);
    }
    if (ok.rc != ELPH_OK) elph_ssh_meas_chains_free(h);
    return ok.rc;
}

extern "C" int elph_ssh_meas_chains_set_mu(elph_handle h, const double *mu) {
    CHECK_H(h);
    RC(need_state(h));
    if (!mu) { elph_set_error("SSH chain measurements: mu is null"); return ELPH_E_ARG; }
    HIPCHK(hipStreamSynchronize(h->stream));
    return upload_mu(smc_of(h), mu, (int)h->N);
}

// Everything one accumulate queues on the handle's stream, the copy of the host's X first; the caller synchronises, whatever this returns.
static int accumulate_launches(elph_handle_s *h, SshMeasChainsState *m, const ElphGreensView &g, const double *X) {
    const int nch = m->nchains, N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = m->ns, nc = m->nc, nvc = g.nv / nch, ndef = m->ndef;
    const int Nph = (int)m->Nph, nP = m->cr.req.np[PHONONGREENS], nqmax = m->nqmax;
    const size_t block = m->cr.total, all = (size_t)nch * block;
    HIPCHK(hipMemsetAsync(m->cur, 0, all * sizeof(double), h->stream));
    // the tau-DFT launchers read their tables and the buffers they are handed, whatever the batch: nothing of the handle's workspace is used
    if (Nph > 0) {
        HIPCHK(hipMemcpyAsync(m->xr, X, (size_t)nch * L * Nph * sizeof(double), hipMemcpyHostToDevice, h->stream));
        RC(elph_launch_r2s(h, m->x, m->xr, nch, Nph));
    }
    // what depends on the fields alone: once per call, added once per pair below
    if (ndef) {
        hipLaunchKernelGGL(k_smc_x, dim3((unsigned)L, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, m->x, m->bpar, m->bph, m->doff, m->dlist, Nph, L,
                           ndef, (long long)m->nbonds, nqmax, m->dtau);
        RC(elph_launch_check("k_smc_x"));
        hipLaunchKernelGGL(k_smc_x_finish, dim3((unsigned)nch), dim3(TPB), 0, h->stream, m->xs, m->part, L, ndef, nqmax, m->V);
        RC(elph_launch_check("k_smc_x_finish"));
    }
    if (nP) {
        RC(elph_dft_fwd_plain(h, m->nu, m->x, Nph, nch));
        const double norm = 1.0 / ((double)L * (double)nc * (double)nc);       // 1/(L Nc)² in all: the other 1/L is in the inverse τ table
        hipLaunchKernelGGL(k_smc_ph, dim3((unsigned)Lh, (unsigned)nP, (unsigned)nch), dim3(TPB), sm_ph_lds_bytes(nc), h->stream, m->Y, m->nu,
                           m->cr.req.pairs[PHONONGREENS], Lh, Nph, m->L1, m->L2, m->L3, g.tw, norm);
        RC(elph_launch_check("k_smc_ph"));
        RC(elph_dft_inv_plain(h, m->B, m->Y, nc, nP * nch));
    }
    const int nq = 2 * ns + 2 + 2 * ndef;
    const size_t shm = ((size_t)nq + NWAVE) * sizeof(double);
    const size_t tab = (size_t)L * ns * N;
    const double *muo = m->mu, *mu_mean = m->mu + (size_t)nch * ns;
    for (int i = 1; i < nvc; ++i)
        for (int j = i + 1; j <= nvc; ++j) {           // pairs of a chain's vectors; every launch serves all chains
            ElphGreensPair v;
            RC(elph_i_greens_setup_chains_dev(h, m->gs, i, j, &v));
            hipLaunchKernelGGL(k_smc_pair, dim3((unsigned)L, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, v, m->x, m->bs, m->bpar, m->bph, m->doff,
                               m->dlist, N, Nph, L, ns, nc, ndef, (long long)m->nbonds, nqmax);
            RC(elph_launch_check("k_smc_pair"));
            hipLaunchKernelGGL(k_smc_finish, dim3((unsigned)nch), dim3(TPB), shm, h->stream, m->cur, m->part, m->xs, muo, mu_mean,
                               m->gs.C + 3 * (size_t)nch * tab, N, L, ns, nc, ndef, nqmax, m->V, block);
            RC(elph_launch_check("k_smc_finish"));
            if (m->cr.fold_max) {
                hipLaunchKernelGGL(k_smc_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), NCORR, (unsigned)nch), dim3(TPB), 0, h->stream, m->rq_cur,
                                   m->gs.C, m->B, N, L, ns, m->L1, m->L2, m->L3, nch, block);
                RC(elph_launch_check("k_smc_fold"));
            }
        }
    hipLaunchKernelGGL(k_smc_add, dim3((unsigned)((all + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->cr.acc, m->cur, (long long)all);
    return elph_launch_check("k_smc_add");
}

extern "C" int elph_ssh_meas_chains_accumulate(elph_handle h, const double *X) {
    CHECK_H(h);
    RC(need_state(h));
    SshMeasChainsState *m = smc_of(h);
    if (!X && m->Nph > 0) { elph_set_error("X is null"); return ELPH_E_ARG; }
    const int nch = m->nchains;
    if (h->nchains != nch) {
        elph_set_error("SSH chain measurements: created for %d chains, %d are resident in this handle now", nch, h->nchains);
        return ELPH_E_STATE;
    }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (g.nv % nch) {
        elph_set_error("SSH chain measurements: the estimator's %d vectors are not a multiple of the %d resident chains", g.nv, nch);
        return ELPH_E_STATE;
    }
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    const int rc = accumulate_launches(h, m, g, X);
    const hipError_t e = hipStreamSynchronize(h->stream);      // on every path: X (a host pointer) is not retained after return
    if (rc == ELPH_OK && e != hipSuccess) { elph_set_error("SSH chain measurements: hipStreamSynchronize -> %s", hipGetErrorString(e)); return ELPH_E_HIP; }
    return rc;
}

extern "C" int elph_ssh_meas_chains_fetch(elph_handle h, int chain, double *scalars, double *Greens, double *DenDen, double *SpinSpin,
                                          double *PairGreens, double *PhononGreens) {
    CHECK_H(h);
    RC(need_state(h));
    SshMeasChainsState *m = smc_of(h);
    if (chain < 0 || chain >= m->nchains) { elph_set_error("SSH chain measurements: chain %d outside 0..%d", chain, m->nchains - 1); return ELPH_E_ARG; }
    CorrPlan<NCORR> one = m->cr;                       // the chain's block, laid out as the plan says
    one.acc = m->cr.acc + (size_t)chain * m->cr.total;
    std::vector<double> host;
    double *outs[NCORR] = {Greens, DenDen, SpinSpin, PairGreens, PhononGreens};
    RC(corr_fetch(h, one, host, outs));
    if (scalars)
        for (int i = 0; i < m->nsc; ++i) scalars[i] = host[(size_t)i];
    return ELPH_OK;
}

extern "C" int elph_ssh_meas_chains_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_state(h));
    const SshMeasChainsState *m = smc_of(h);
    HIPCHK(hipMemsetAsync(m->cr.acc, 0, (size_t)m->nchains * m->cr.total * sizeof(double), h->stream));
    return ELPH_OK;
}
