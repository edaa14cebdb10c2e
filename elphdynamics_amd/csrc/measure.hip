// measure.hip — the Holstein measurements of Measurements.jl accumulated on the device, for one configuration or for EVERY chain resident
// in the handle at once (DESIGN.md "Measurements on the device"):
//   make_measurements!            Measurements.jl:545-566   per chain, without its update!: the estimator's vectors are there already
//     make_global_measurements!   :845-861, :1283-1312      density, Nsqr, mu
//     make_onsite_measurements!   :916-976                  density, double_occ, x, x2, x4, phonon_pe, phonon_ke, elph_energy, mu per orbital
//     make_intersite_measurements! :1029-1070               el_ke per bond definition
//     measure_Greens! / _DenDen! / _SpinSpin! / _PairGreens! / _PhononGreens!   :1469-1650
//   reset_measurements!           :698-758
// Everything the reference adds up is real, so every accumulator is a double; the complex arrays of the reference appear when a fetch
// copies out.
//
// ONE state, one kernel set and one host path serve both families of entry points.  The chain is the last grid axis of every kernel, so
// the launches of one accumulate depend on the vectors per chain and on the request, not on the number of chains; nchains = 1 is the
// single configuration.  elph_meas_* (the slot meas) hold a state for one chain, refuse a handle with several resident chains and run
// the estimator's pipeline in the estimator's own scratch, so that its tables and their doubled complex copies are left holding the last
// pair of vectors; elph_meas_chains_* (the slot meas_chains) measure every resident chain in scratch the state owns and leave the
// estimator's tables alone, even with one chain resident.  What a workgroup computes is in meas_holstein_dev.h.
//
// Reductions have ONE order, whatever the device does: a thread walks its cells in index order, the 64 lanes of a wave fold by halves
// (shuffles), the waves of a workgroup are added in index order through LDS, each workgroup (= one time slice of one chain) writes one
// partial, and a single workgroup per chain adds the L partials in slice order and updates the accumulator.  No floating-point atomics
// anywhere: the same inputs give the same bits.  A workgroup reads one chain's field, parameters, vectors and tables only, so chain c's
// numbers depend on nothing of another chain.
//
// Layouts: vectors in layout S (element (tau, site) at tau * N + site, orbital = site % n_s, cell = site / n_s); vector v (0-based) of chain
// c is row v nchains + c of the estimator (greens.chain_vector), so the v-th vectors of all chains are one block [chain][ndim].  The
// pipeline's real correlations come out C[c][chain][tau < L][s2 + n_s (s1 + n_s cell)], c = 0 G[D,0], 1 G[D,0] G[D,0], 2 G[D,D] G[0,0],
// 3 G[D,0] G[0,D], so that measure_*(l, o1, o2, tau) (GreensFunctions.jl:293-329) is C[c][chain][tau][(o2 - 1) + n_s ((o1 - 1) + n_s
// cell(l))], which meas_fold reads with a table stride.  A correlation accumulator is [L0][L1][L2][L3][n_p], first index fastest, L0 = L + 1
// (time-dependent) or 1 (equal-time); the accumulator is ONE allocation [chain][scalars | Greens | DenDen | SpinSpin | PairGreens |
// PhononGreens], a chain's block exactly what a fetch returns: reset is one memset, fetch one copy.  mu is [chain][N] (a tuner per chain
// moves it, elph_hmc_set_mu_chains); omega, omega4, lambda and the bonds are the model's.  The field is staged in a buffer of the
// state's: the handle's solver workspace is not grown for a measurement.

#include <vector>

#include "corr_req.h"
#include "elph_internal.h"
#include "meas_holstein_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int NWAVE = MEAS_NWAVE;
constexpr int NCORR = MS_NCORR;
const char *const CORR_NAMES[NCORR] = {"Greens", "DenDen", "SpinSpin", "PairGreens", "PhononGreens"};
const CorrWords WORDS = {"measurements", "orbital", "with no orbital pair"};
const CorrWords WORDS_CHAINS = {"chain measurements", "orbital", "with no orbital pair"};

struct MeasState {
    int nchains = 1, ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0, nsc = 0;
    int64_t nbonds = 0;
    double dtau = 0.0;
    double *par = nullptr;          // [3][N] omega, omega4, lambda
    double *mu = nullptr;           // [nchains][N], then [nchains] the rows' means
    int *bs = nullptr;              // [2][nbonds] 0-based sites of every bond, the reference's bond order
    double *bt = nullptr;           // [nbonds]
    CorrPlan<NCORR> cr;             // ONE chain's plan: cr.total doubles per chain; cr.acc: [nchains][cr.total], cr.req bound to chain 0
    double *xr = nullptr;           // [nchains][ndim] staging of the fields as they arrive (reference layout)
    double *x = nullptr;            // [nchains][ndim] the fields, layout S
    double *ph = nullptr;           // [nchains][L][ns*N] the fields' translation averages (PhononGreens requested)
    double *xs = nullptr;           // [nchains][MS_NXONLY][ns] the field-only on-site terms of this accumulate, normalised
    double *part = nullptr;         // [nchains][L][nqmax] one partial per workgroup
    int nqmax = 0;
    ElphGreensChainScratch gs{};    // the estimator's pipeline for all chains (the _chains entry points; the others borrow the estimator's)
                                    // — those leave gs all null, so that freeing it frees nothing
};

// ---- the kernels: the bodies of meas_holstein_dev.h, the chain the last grid axis
// The field-only on-site terms, one workgroup per (time slice, chain): part[chain][t][o * MS_NXONLY + k].
__global__ void __launch_bounds__(TPB) k_ms_x(double *__restrict__ part, const double *__restrict__ x, const double *__restrict__ par,
                                              const double *__restrict__ mu, int N, int L, int ns, int nc, int nqmax, double dtau) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.y;
    ms_x_slice(part + ch * L * nqmax, x + ch * L * N, par, par + N, mu + ch * N, N, L, ns, nc, dtau, blockIdx.x, red);
}

__global__ void __launch_bounds__(TPB) k_ms_x_finish(double *__restrict__ xs, const double *__restrict__ part, int L, int ns, int nqmax, double norm) {
    const size_t ch = blockIdx.x;
    ms_x_finish(xs + ch * MS_NXONLY * ns, part + ch * L * nqmax, L, ns, norm);
}

// The terms of one pair of vectors that need the estimate, one workgroup per (slice, chain).  v: chain 0's vectors.
__global__ void __launch_bounds__(TPB) k_ms_pair(double *__restrict__ part, ElphGreensPair v, const double *__restrict__ x,
                                                 const double *__restrict__ lam, const int *__restrict__ bs, const double *__restrict__ bt, int N,
                                                 int L, int ns, int nc, int ndef, long long nbonds, int nqmax) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.y, o = ch * L * N;
    ms_pair_slice(part + ch * L * nqmax, v.X1 + o, v.X2 + o, v.R1 + o, v.R2 + o, x + o, lam, bs, bt, N, ns, nc, ndef, nbonds, blockIdx.x, red);
}

// One workgroup per chain: every scalar accumulator of this pair.  C3: table 3 (G[D,0] G[0,D]) of chain 0; mu_mean: [nchains]; block:
// doubles of a chain's accumulators
__global__ void __launch_bounds__(TPB) k_ms_finish(double *__restrict__ acc, const double *__restrict__ part, const double *__restrict__ xs,
                                                   const double *__restrict__ C3, const double *__restrict__ mu_mean, int N, int L, int ns, int nc,
                                                   int ndef, int nqmax, size_t block) {
    extern __shared__ double tot[];                    // [nq] + red[NWAVE]
    const size_t ch = blockIdx.x;
    ms_finish(acc + ch * block, part + ch * L * nqmax, xs + ch * MS_NXONLY * ns, C3 + ch * L * ns * N, N, L, ns, nc, ndef, mu_mean[ch], tot);
}

// One thread per (tau, cell, listed pair) of correlation blockIdx.y of chain blockIdx.z.  C: [table][chain][L][ns N]
__global__ void __launch_bounds__(TPB) k_ms_fold(CorrReq<NCORR> rq, const double *__restrict__ C, const double *__restrict__ ph, int N, int L, int ns,
                                                 int L1, int L2, int L3, int nchains, size_t block) {
    const size_t ch = blockIdx.z, tab = (size_t)L * ns * N;
    ms_fold(rq, blockIdx.y, (long long)blockIdx.x * TPB + threadIdx.x, C + ch * tab, ph, N, L, ns, L1, L2, L3, (size_t)nchains * tab, ch * block,
            ch * tab);
}

// mu[nchains][N] and, behind it, mean(model.mu) of every chain's row (:858)
int upload_mu(MeasState *m, const double *mu, int N) {
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

void ms_free(void *&slot) {
    MeasState *m = (MeasState *)slot;
    if (!m) return;
    corr_free({m->par, m->mu, m->bs, m->bt, m->cr.pairs, m->cr.acc, m->xr, m->x, m->ph, m->xs, m->part});
    elph_i_greens_chain_scratch_free(&m->gs);
    delete m;
    slot = nullptr;
}

// The state of a request for nchains chains into the (freed) slot, after the entry point's refusals; mu: [nchains][N].  own_scratch: the
// state brings the scratch of the estimator's pipeline (the _chains entry points).
int ms_create(elph_handle_s *h, void *&slot, const CorrWords &W, int nchains, bool own_scratch, const double *omega, const double *omega4,
              const double *lambda, const double *mu, double dtau, int64_t nbonds, int ndef, const int64_t *bond_sites, const double *bond_t,
              const int *measure, const int *time_dependent, const int *npairs, const int *pairs) {
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    const int N = (int)h->N, L = (int)h->L, ns = g.ns, nc = g.nc;
    std::vector<int> bs;
    RC(corr_check_onsite_params(h, W.prefix, nc, omega, omega4, lambda, mu, dtau, nbonds, ndef, bond_sites, bond_t, measure, time_dependent, npairs, bs));
    const int nsc = 3 + MS_NONSITE * ns + ndef;
    CorrPlan<NCORR> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, W, CORR_NAMES, measure, time_dependent, npairs, pairs, ns, L, nc, (size_t)nsc));
    MeasState *m = new MeasState;
    slot = m;
    m->cr = plan;
    m->nchains = nchains; m->ns = ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = ndef; m->nbonds = nbonds; m->dtau = dtau; m->nsc = nsc;
    m->nqmax = std::max(3 * ns + 2 + ndef, MS_NXONLY * ns);
    const size_t nch = (size_t)nchains, nd = (size_t)h->ndim, ncol = (size_t)ns * N;
    const bool phonon = m->cr.req.np[MS_PHONONGREENS] != 0;
    CorrFirstError ok;
    const bool allocated = ok(corr_alloc(&m->par, 3 * (size_t)N)) && ok(corr_alloc(&m->mu, nch * N + nch)) && ok(corr_alloc(&m->bs, 2 * (size_t)nbonds)) &&
        ok(corr_alloc(&m->bt, (size_t)nbonds)) && ok(corr_alloc(m->cr, nch)) && ok(corr_alloc(&m->xr, nch * nd)) && ok(corr_alloc(&m->x, nch * nd)) &&
        ok(corr_alloc(&m->xs, nch * MS_NXONLY * ns)) && ok(corr_alloc(&m->part, nch * L * m->nqmax)) && (!phonon || ok(corr_alloc(&m->ph, nch * L * ncol))) &&
        (!own_scratch || ok(elph_i_greens_chain_scratch_alloc(h, nchains, &m->gs)));
    if (!allocated) { ms_free(slot); return ok.rc; }
    const double *pp[3] = {omega, omega4, lambda};
    for (int k = 0; k < 3; ++k) ok(corr_up(m->par + (size_t)k * N, pp[k], (size_t)N * sizeof(double)));
    ok(upload_mu(m, mu, N));
    ok(corr_up(m->bs, bs.data(), bs.size() * sizeof(int)));
    ok(corr_up(m->bt, bond_t, (size_t)nbonds * sizeof(double)));
    if (ok.rc == ELPH_OK) ok(corr_upload(m->cr, W.prefix, nch));
    if (ok.rc != ELPH_OK) ms_free(slot);
    return ok.rc;
}

// Everything one accumulate queues on the handle's stream, the copy of the host's X first; the caller synchronises, whatever this returns.
// S: the scratch the estimator's pipeline runs in.
int ms_launches(elph_handle_s *h, MeasState *m, const ElphGreensView &g, const ElphGreensChainScratch &S, const double *X) {
    const int nch = m->nchains, N = (int)h->N, L = (int)h->L, ns = m->ns, nc = m->nc, nvc = g.nv / nch, nqmax = m->nqmax;
    // the tau-DFT launchers read their tables and the buffers they are handed, whatever the batch: nothing of the handle's workspace is used
    HIPCHK(hipMemcpyAsync(m->xr, X, (size_t)nch * (size_t)h->ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_r2s(h, m->x, m->xr, nch));
    const double *mu = m->mu, *mu_mean = m->mu + (size_t)nch * N;
    const double norm = (double)nc * (double)L;
    // what depends on the fields alone: once per call, added once per pair below (the reference's loop recomputes it per pair)
    hipLaunchKernelGGL(k_ms_x, dim3((unsigned)L, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, m->x, m->par, mu, N, L, ns, nc, nqmax, m->dtau);
    RC(elph_launch_check("k_ms_x"));
    hipLaunchKernelGGL(k_ms_x_finish, dim3((unsigned)nch), dim3(TPB), 0, h->stream, m->xs, m->part, L, ns, nqmax, norm);
    RC(elph_launch_check("k_ms_x_finish"));
    if (m->cr.req.np[MS_PHONONGREENS]) RC(elph_i_greens_autocorr_chains_dev(h, S, m->ph, m->x));
    const int nq = 3 * ns + 2 + m->ndef;
    const size_t shm = ((size_t)nq + NWAVE) * sizeof(double);
    const size_t tab = (size_t)L * ns * N, block = m->cr.total;
    for (int i = 1; i < nvc; ++i)
        for (int j = i + 1; j <= nvc; ++j) {           // pairs of a chain's vectors; every launch serves all chains
            ElphGreensPair v;
            RC(elph_i_greens_setup_chains_dev(h, S, i, j, &v));
            hipLaunchKernelGGL(k_ms_pair, dim3((unsigned)L, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, v, m->x, m->par + 2 * (size_t)N, m->bs, m->bt,
                               N, L, ns, nc, m->ndef, (long long)m->nbonds, nqmax);
            RC(elph_launch_check("k_ms_pair"));
            hipLaunchKernelGGL(k_ms_finish, dim3((unsigned)nch), dim3(TPB), shm, h->stream, m->cr.acc, m->part, m->xs, S.C + 3 * (size_t)nch * tab, mu_mean,
                               N, L, ns, nc, m->ndef, nqmax, block);
            RC(elph_launch_check("k_ms_finish"));
            if (m->cr.fold_max) {
                hipLaunchKernelGGL(k_ms_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), NCORR, (unsigned)nch), dim3(TPB), 0, h->stream, m->cr.req,
                                   S.C, m->ph, N, L, ns, m->L1, m->L2, m->L3, nch, block);
                RC(elph_launch_check("k_ms_fold"));
            }
        }
    return ELPH_OK;
}

// after the entry point's own checks: the estimator's vectors, the launches, one synchronisation
int ms_accumulate(elph_handle_s *h, MeasState *m, const CorrWords &W, const ElphGreensChainScratch *S, const double *X) {
    ElphGreensView g;
    RC(corr_vectors(h, W.prefix, m->nchains, &g));
    return corr_synchronised(h, W.prefix, ms_launches(h, m, g, *S, X));
}

int ms_fetch(elph_handle_s *h, const MeasState *m, int chain, double *scalars, double *const *outs) {
    std::vector<double> host;
    RC(corr_fetch(h, m->cr, host, outs, chain));
    if (scalars)
        for (int i = 0; i < m->nsc; ++i) scalars[i] = host[(size_t)i];
    return ELPH_OK;
}

MeasState *ms_of(void *slot) { return (MeasState *)slot; }
int need_meas(elph_handle_s *h) { return corr_need(h->meas, "elph_meas_create"); }
int need_chains(elph_handle_s *h) { return corr_need(h->meas_chains, "elph_meas_chains_create"); }

}  // namespace

void elph_meas_free(elph_handle_s *h) { ms_free(h->meas); }
void elph_meas_chains_free(elph_handle_s *h) { ms_free(h->meas_chains); }

// ---- one configuration per handle: mu[N]
extern "C" int elph_meas_create(elph_handle h, const double *omega, const double *omega4, const double *lambda, const double *mu, double dtau,
                                int64_t nbonds, int ndef, const int64_t *bond_sites, const double *bond_t, const int *measure,
                                const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_meas_free(h);
    RC(corr_refuse_handle(h, WORDS.prefix));
    return ms_create(h, h->meas, WORDS, 1, false, omega, omega4, lambda, mu, dtau, nbonds, ndef, bond_sites, bond_t, measure, time_dependent, npairs, pairs);
}

extern "C" int elph_meas_accumulate(elph_handle h, const double *x) {
    CHECK_H(h);
    RC(need_meas(h));
    RC(corr_refuse_chains(h, WORDS.prefix));
    if (!x) { elph_set_error("x is null"); return ELPH_E_ARG; }
    return ms_accumulate(h, ms_of(h->meas), WORDS, elph_i_greens_own_scratch(h), x);
}

extern "C" int elph_meas_fetch(elph_handle h, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                               double *PhononGreens) {
    CHECK_H(h);
    RC(need_meas(h));
    double *outs[NCORR] = {Greens, DenDen, SpinSpin, PairGreens, PhononGreens};
    return ms_fetch(h, ms_of(h->meas), 0, scalars, outs);
}

extern "C" int elph_meas_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_meas(h));
    return corr_reset(h, ms_of(h->meas)->cr);
}

// ---- every resident chain at once: mu[nchains][N], X[nchains][ndim]
extern "C" int elph_meas_chains_create(elph_handle h, int nchains, const double *omega, const double *omega4, const double *lambda, const double *mu,
                                       double dtau, int64_t nbonds, int ndef, const int64_t *bond_sites, const double *bond_t, const int *measure,
                                       const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_meas_chains_free(h);
    RC(corr_refuse_model(h, WORDS_CHAINS.prefix));
    RC(corr_check_chain_count(h, WORDS_CHAINS.prefix, nchains));
    return ms_create(h, h->meas_chains, WORDS_CHAINS, nchains, true, omega, omega4, lambda, mu, dtau, nbonds, ndef, bond_sites, bond_t, measure,
                     time_dependent, npairs, pairs);
}

extern "C" int elph_meas_chains_set_mu(elph_handle h, const double *mu) {
    CHECK_H(h);
    RC(need_chains(h));
    if (!mu) { elph_set_error("chain measurements: mu is null"); return ELPH_E_ARG; }
    HIPCHK(hipStreamSynchronize(h->stream));
    return upload_mu(ms_of(h->meas_chains), mu, (int)h->N);
}

extern "C" int elph_meas_chains_accumulate(elph_handle h, const double *X) {
    CHECK_H(h);
    RC(need_chains(h));
    if (!X) { elph_set_error("X is null"); return ELPH_E_ARG; }
    MeasState *m = ms_of(h->meas_chains);
    RC(corr_same_chains(h, WORDS_CHAINS.prefix, m->nchains));
    return ms_accumulate(h, m, WORDS_CHAINS, &m->gs, X);
}

extern "C" int elph_meas_chains_fetch(elph_handle h, int chain, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                                      double *PhononGreens) {
    CHECK_H(h);
    RC(need_chains(h));
    const MeasState *m = ms_of(h->meas_chains);
    RC(corr_check_chain(WORDS_CHAINS.prefix, chain, m->nchains));
    double *outs[NCORR] = {Greens, DenDen, SpinSpin, PairGreens, PhononGreens};
    return ms_fetch(h, m, chain, scalars, outs);
}

extern "C" int elph_meas_chains_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_chains(h));
    const MeasState *m = ms_of(h->meas_chains);
    return corr_reset(h, m->cr, (size_t)m->nchains);
}
