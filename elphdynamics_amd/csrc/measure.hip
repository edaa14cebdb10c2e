// measure.hip — the Holstein measurements of Measurements.jl accumulated on the device (DESIGN.md "Measurements on the device"):
//   make_measurements!            Measurements.jl:545-566   (without its update!: the estimator's vectors are there already)
//     make_global_measurements!   :845-861, :1283-1312      density, Nsqr, mu
//     make_onsite_measurements!   :916-976                  density, double_occ, x, x2, x4, phonon_pe, phonon_ke, elph_energy, mu per orbital
//     make_intersite_measurements! :1029-1070               el_ke per bond definition
//     measure_Greens! / _DenDen! / _SpinSpin! / _PairGreens! / _PhononGreens!   :1469-1650
//   reset_measurements!           :698-758
// Everything the reference adds up is real, so every accumulator is a double; the complex arrays of the reference appear when
// elph_meas_fetch copies out.  One allocation holds [scalars | Greens | DenDen | SpinSpin | PairGreens | PhononGreens]: reset is one
// memset, fetch one copy.
//
// Reductions have ONE order, whatever the device does: a thread walks its cells in index order, the 64 lanes of a wave fold by halves
// (shuffles), the waves of a workgroup are added in index order through LDS, each workgroup (= one time slice) writes one partial, and
// a single workgroup adds the L partials in slice order and updates the accumulator.  No floating-point atomics anywhere: the same
// inputs give the same bits.
//
// Layouts: vectors in layout S (element (tau, site) at tau * N + site, orbital = site % n_s, cell = site / n_s); the estimator's real
// correlations C[c][tau < L][s2 + n_s (s1 + n_s cell)], c = 0 G[D,0], 1 G[D,0] G[D,0], 2 G[D,D] G[0,0], 3 G[D,0] G[0,D], so that
// measure_*(l, o1, o2, tau) (GreensFunctions.jl:293-329) is C[c][tau][(o2 - 1) + n_s ((o1 - 1) + n_s cell(l))]; a correlation accumulator
// is [L0][L1][L2][L3][n_p], first index fastest, L0 = L + 1 (time-dependent) or 1 (equal-time).

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
constexpr int PHONONGREENS = MS_PHONONGREENS, NONSITE = MS_NONSITE, NXONLY = MS_NXONLY;      // the kernels' bodies: meas_holstein_dev.h

struct MeasState {
    int ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0;
    int64_t nbonds = 0;
    double dtau = 0.0, mu_mean = 0.0;
    double *par = nullptr;          // [4][N] omega, omega4, lambda, mu
    int *bs = nullptr;              // [2][nbonds] 0-based sites of every bond, the reference's bond order
    double *bt = nullptr;           // [nbonds]
    CorrPlan<NCORR> cr;             // the requests, pairs (o1, o2); cr.acc: [nsc | the measured correlations]
    int nsc = 0;
    double *x = nullptr;            // [ndim] the field, layout S
    double *ph = nullptr;           // [L][ns*N] the field's translation average (PhononGreens requested)
    double *xs = nullptr;           // [NXONLY][ns] the field-only on-site terms of this accumulate, normalised
    double *part = nullptr;         // [L][max(nq, NXONLY*ns)] one partial per workgroup
};

MeasState *ms_of(elph_handle_s *h) { return (MeasState *)h->meas; }

// The field-only on-site terms, one workgroup per time slice: part[t][o * NXONLY + k].
__global__ void __launch_bounds__(TPB) k_ms_x(double *__restrict__ part, const double *__restrict__ x, const double *__restrict__ par, int N,
                                              int L, int ns, int nc, double dtau) {
    __shared__ double red[NWAVE];
    ms_x_slice(part, x, par, par + N, par + 3 * (size_t)N, N, L, ns, nc, dtau, blockIdx.x, red);
}

__global__ void __launch_bounds__(TPB) k_ms_x_finish(double *__restrict__ xs, const double *__restrict__ part, int L, int ns, double norm) {
    ms_x_finish(xs, part, L, ns, norm);
}

// The terms of one pair of vectors that need the estimate, one workgroup per slice.
__global__ void __launch_bounds__(TPB) k_ms_pair(double *__restrict__ part, const double *__restrict__ X1, const double *__restrict__ X2,
                                                 const double *__restrict__ R1, const double *__restrict__ R2, const double *__restrict__ x,
                                                 const double *__restrict__ lam, const int *__restrict__ bs, const double *__restrict__ bt,
                                                 int N, int ns, int nc, int ndef, long long nbonds) {
    __shared__ double red[NWAVE];
    ms_pair_slice(part, X1, X2, R1, R2, x, lam, bs, bt, N, ns, nc, ndef, nbonds, blockIdx.x, red);
}

// One workgroup: every scalar accumulator of this pair.
__global__ void __launch_bounds__(TPB) k_ms_finish(double *__restrict__ acc, const double *__restrict__ part, const double *__restrict__ xs,
                                                   const double *__restrict__ C3, int N, int L, int ns, int nc, int ndef, double mu_mean) {
    extern __shared__ double tot[];                    // [nq] + red[NWAVE]
    ms_finish(acc, part, xs, C3, N, L, ns, nc, ndef, mu_mean, tot);
}

// One thread per (tau, cell, listed pair) of correlation blockIdx.y.
__global__ void __launch_bounds__(TPB) k_ms_fold(CorrReq<NCORR> rq, const double *__restrict__ C, const double *__restrict__ ph, int N, int L, int ns,
                                                 int L1, int L2, int L3) {
    ms_fold(rq, blockIdx.y, (long long)blockIdx.x * TPB + threadIdx.x, C, ph, N, L, ns, L1, L2, L3);
}

int need_meas(elph_handle_s *h) { return corr_need(h->meas, "elph_meas_create"); }

}  // namespace

void elph_meas_free(elph_handle_s *h) {
    MeasState *m = ms_of(h);
    if (!m) return;
    corr_free({m->par, m->bs, m->bt, m->cr.pairs, m->cr.acc, m->x, m->ph, m->xs, m->part});
    delete m;
    h->meas = nullptr;
}

extern "C" int elph_meas_create(elph_handle h, const double *omega, const double *omega4, const double *lambda, const double *mu, double dtau,
                                int64_t nbonds, int ndef, const int64_t *bond_sites, const double *bond_t, const int *measure,
                                const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_meas_free(h);
    RC(corr_refuse_handle(h, WORDS.prefix));
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    const int N = (int)h->N, L = (int)h->L, ns = g.ns, nc = g.nc;
    std::vector<int> bs;
    RC(corr_check_onsite_params(h, WORDS.prefix, nc, omega, omega4, lambda, mu, dtau, nbonds, ndef, bond_sites, bond_t, measure, time_dependent, npairs, bs));
    const int nsc = 3 + NONSITE * ns + ndef;
    CorrPlan<NCORR> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, WORDS, CORR_NAMES, measure, time_dependent, npairs, pairs, ns, L, nc, (size_t)nsc));
    MeasState *m = new MeasState;
    h->meas = m;
    m->cr = plan;
    m->ns = ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = ndef; m->nbonds = nbonds; m->dtau = dtau; m->nsc = nsc;
    double mus = 0.0;
    for (int i = 0; i < N; ++i) mus += mu[i];
    m->mu_mean = mus / N;                              // mean(model.mu), :858
    const int nq = std::max(3 * ns + 2 + ndef, NXONLY * ns);
    CorrFirstError ok;
    const bool allocated = ok(corr_alloc(&m->par, 4 * (size_t)N)) && ok(corr_alloc(&m->bs, 2 * (size_t)nbonds)) && ok(corr_alloc(&m->bt, (size_t)nbonds)) &&
        ok(corr_alloc(m->cr)) && ok(corr_alloc(&m->x, (size_t)h->ndim)) && ok(corr_alloc(&m->xs, (size_t)NXONLY * ns)) &&
        ok(corr_alloc(&m->part, (size_t)L * nq)) && (m->cr.req.np[PHONONGREENS] == 0 || ok(corr_alloc(&m->ph, (size_t)L * ns * N)));
    if (!allocated) { elph_meas_free(h); return ok.rc; }
    const double *pp[4] = {omega, omega4, lambda, mu};
    for (int k = 0; k < 4; ++k) ok(corr_up(m->par + (size_t)k * N, pp[k], (size_t)N * sizeof(double)));
    ok(corr_up(m->bs, bs.data(), bs.size() * sizeof(int)));
    ok(corr_up(m->bt, bond_t, (size_t)nbonds * sizeof(double)));
    if (ok.rc == ELPH_OK) ok(corr_upload(m->cr, WORDS.prefix));
    if (ok.rc != ELPH_OK) elph_meas_free(h);
    return ok.rc;
}

extern "C" int elph_meas_accumulate(elph_handle h, const double *x) {
    CHECK_H(h);
    RC(need_meas(h));
    RC(corr_refuse_chains(h, WORDS.prefix));
    if (!x) { elph_set_error("x is null"); return ELPH_E_ARG; }
    MeasState *m = ms_of(h);
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    const int N = (int)h->N, L = (int)h->L, ns = m->ns, nc = m->nc, nv = g.nv;
    RC(elph_i_ensure_capacity(h, 1));
    HIPCHK(hipMemcpyAsync(h->d_stage_in, x, (size_t)h->ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_r2s(h, m->x, h->d_stage_in, 1));
    // what depends on the field alone: once per call, added once per pair below (the reference's loop recomputes it per pair)
    hipLaunchKernelGGL(k_ms_x, dim3((unsigned)L), dim3(TPB), 0, h->stream, m->part, m->x, m->par, N, L, ns, nc, m->dtau);
    RC(elph_launch_check("k_ms_x"));
    hipLaunchKernelGGL(k_ms_x_finish, dim3(1), dim3(TPB), 0, h->stream, m->xs, m->part, L, ns, (double)nc * (double)L);
    RC(elph_launch_check("k_ms_x_finish"));
    if (m->cr.req.np[PHONONGREENS]) RC(elph_i_greens_autocorr_dev(h, m->ph, m->x));
    const int nq = 3 * ns + 2 + m->ndef;
    const size_t shm = ((size_t)nq + NWAVE) * sizeof(double);
    const size_t tab = (size_t)L * ns * N;
    for (int i = 1; i < nv; ++i)
        for (int j = i + 1; j <= nv; ++j) {
            ElphGreensPair v;
            RC(elph_i_greens_pair_dev(h, i, j, &v));
            hipLaunchKernelGGL(k_ms_pair, dim3((unsigned)L), dim3(TPB), 0, h->stream, m->part, v.X1, v.X2, v.R1, v.R2, m->x, m->par + 2 * (size_t)N, m->bs,
                               m->bt, N, ns, nc, m->ndef, (long long)m->nbonds);
            RC(elph_launch_check("k_ms_pair"));
            hipLaunchKernelGGL(k_ms_finish, dim3(1), dim3(TPB), shm, h->stream, m->cr.acc, m->part, m->xs, g.C + 3 * tab, N, L, ns, nc, m->ndef,
                               m->mu_mean);
            RC(elph_launch_check("k_ms_finish"));
            if (m->cr.fold_max) {
                hipLaunchKernelGGL(k_ms_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), NCORR), dim3(TPB), 0, h->stream, m->cr.req, g.C, m->ph, N,
                                   L, ns, m->L1, m->L2, m->L3);
                RC(elph_launch_check("k_ms_fold"));
            }
        }
    HIPCHK(hipStreamSynchronize(h->stream));           // x (a host pointer) is not retained after return
    return ELPH_OK;
}

extern "C" int elph_meas_fetch(elph_handle h, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                               double *PhononGreens) {
    CHECK_H(h);
    RC(need_meas(h));
    MeasState *m = ms_of(h);
    std::vector<double> host;
    double *outs[NCORR] = {Greens, DenDen, SpinSpin, PairGreens, PhononGreens};
    RC(corr_fetch(h, m->cr, host, outs));
    if (scalars)
        for (int i = 0; i < m->nsc; ++i) scalars[i] = host[(size_t)i];
    return ELPH_OK;
}

extern "C" int elph_meas_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_meas(h));
    return corr_reset(h, ms_of(h)->cr);
}
