// ssh_measure.hip — the measurements of the bond-phonon (SSH) model accumulated on the device, for one configuration or for EVERY chain
// resident in the handle at once (DESIGN.md "Measurements on the device"):
//   make_measurements!             Measurements.jl:545-566   per chain, without its update!: the estimator's vectors are there already
//     make_global_measurements!    :845-861, :1283-1312      density, Nsqr, mu
//     make_onsite_measurements!    :978-1024                 density, double_occ, mu per orbital
//     make_intersite_measurements! :1072-1155                x, x2, x4, phonon_pe, phonon_ke, elph_energy, el_ke, sign_switch per bond definition
//     measure_Greens! / _DenDen! / _SpinSpin! / _PairGreens!  :1469-1596   the folds of meas_dev.h, shared with measure.hip
//     measure_PhononGreens!        :2488-2541                the field's translation average over phonon types
//   reset_measurements!            :698-758
// Everything the reference adds up is real: all accumulators are doubles (corr_req.h).
//
// ONE state, one kernel set and one host path serve both families of entry points.  The chain is the last grid axis of every kernel, so
// the launches of one accumulate depend on the vectors per chain and on the request, not on the number of chains; nchains = 1 is the
// single configuration.  elph_ssh_meas_* (the slot ssh_meas) hold a state for one chain, refuse a handle with several resident chains
// and run the estimator's pipeline in the estimator's own scratch, so that its tables and their doubled complex copies are left holding
// the last pair of vectors; elph_ssh_meas_chains_* (the slot ssh_meas_chains) measure every resident chain in scratch the state owns and
// leave the estimator's tables alone, even with one chain resident.  What a workgroup computes is in meas_ssh_dev.h.
//
// Bonds come in the reference's order (model.t, bond_to_definition, bond_to_phonon; sites neighbor_table[:, checkerboard_perm[bond]]).
// The bonds of one definition are walked in bond order through a list made at create, so a definition may own any number of bonds; the
// normalisation is the reference's V = (Nbonds / nbonds) Ltau.  The modulated hopping t' = t - (alpha x + sign(x) alpha2 x^2)
// (SSHModels.jl:531-533) is recomputed from the field, t' = t on a bare bond.
//
// Reductions have the ONE order of measure.hip: a thread walks its cells / bonds in index order, the 64 lanes of a wave fold by halves,
// the waves are added in index order through LDS, each workgroup (= one time slice of one chain) writes one partial, a single workgroup
// per chain adds the L partials in slice order.  No floating-point atomics.  A workgroup reads one chain's field, mu, vectors and tables
// only, so chain c's numbers depend on nothing of another chain.  What depends on the field alone (x ... phonon_ke, sign_switch,
// PhononGreens) is computed once per accumulate and added once per pair of vectors.  One accumulate adds its pairs of vectors up from zero
// in a buffer of its own (cur) and adds that to the accumulators once at the end: two accumulations of the same inputs are twice one, to
// the bit.
//
// Layouts.  Vector v (0-based) of chain c is row v nchains + c of the estimator (greens.chain_vector), so the v-th vectors of all chains
// are one block [chain][ndim].  The field is (Ltau, Nph) in the reference, phonon slowest: the fields arrive as X[chain][Nph][L] and
// become layout S with Nph columns, x[chain][tau * Nph + phonon], and for PhononGreens phonon = cell + ncells * type (the reference's
// reshape to (Ltau, L1, L2, L3, nph)).  PhononGreens of the pair (b1, b2) is
//   1/(L Nc) sum_{tau, cell} x_b2[tau + dtau, cell + dcell] x_b1[tau, cell]
// spectrally: plain half spectra along tau of all Nph columns [chain][Lh][Nph], then per (frequency, listed pair, chain) the cell-axis
// DFTs of the two types in LDS (cell_dft_dev.h, unit = 1), their product, the inverse cell-axis DFT into [chain][nP][Lh][nc], and one
// inverse tau-transform of all listed pairs into [chain][nP][L][nc] — in scratch this unit owns (the estimator's is sized for n_s
// orbitals, and nph > n_s is the normal case).  The accumulator is ONE allocation [chain][scalars | Greens | DenDen | SpinSpin |
// PairGreens | PhononGreens], a chain's block exactly what a fetch returns: reset is one memset, fetch one copy; cur has the same shape.
// Of mu the kernels need its means alone: [chain][n_s] over the sites of an orbital, then [chain] over all sites, made on the host at
// create and at set_mu (a tuner per chain moves mu, elph_hmc_set_mu_chains).  The bonds, the phonon parameters and the definition lists
// are the model's.  The pipeline's four real tables come out [table][chain][L][n_s N], which meas_fold reads with a table stride.
// Nothing of the handle's solver workspace is grown or used.

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
const CorrWords WORDS = {"SSH measurements", "orbital", "with no orbital pair", PHONONGREENS, "phonon type", "with no pair of phonon types"};
const CorrWords WORDS_CHAINS = {"SSH chain measurements", "orbital", "with no orbital pair", PHONONGREENS, "phonon type", "with no pair of phonon types"};

struct SshMeasState {
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
    ElphGreensChainScratch gs{};    // the estimator's pipeline for all chains (the _chains entry points; the others borrow the estimator's)
                                    // — those leave gs all null, so that freeing it frees nothing
};

// ---- the kernels: the bodies of meas_ssh_dev.h, the chain the last grid axis
// one workgroup per (time slice, chain)
__global__ void __launch_bounds__(TPB) k_sm_x(double *__restrict__ part, const double *__restrict__ x, const double *__restrict__ bpar,
                                              const int *__restrict__ bph, const int *__restrict__ doff, const int *__restrict__ dlist, int Nph,
                                              int L, int ndef, long long nbonds, int nqmax, double dtau) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.y;
    sm_x_slice(part + ch * L * nqmax, x + ch * L * Nph, bpar, bph, doff, dlist, Nph, L, ndef, nbonds, dtau, blockIdx.x, red);
}

__global__ void __launch_bounds__(TPB) k_sm_x_finish(double *__restrict__ xs, const double *__restrict__ part, int L, int ndef, int nqmax, double V) {
    const size_t ch = blockIdx.x;
    sm_x_finish(xs + ch * SM_NXONLY * ndef, part + ch * L * nqmax, L, ndef, V);
}

// one workgroup per (time slice, chain).  v: chain 0's vectors; chain c's lie c L N further
__global__ void __launch_bounds__(TPB) k_sm_pair(double *__restrict__ part, ElphGreensPair v, const double *__restrict__ x,
                                                 const int *__restrict__ bs, const double *__restrict__ bpar, const int *__restrict__ bph,
                                                 const int *__restrict__ doff, const int *__restrict__ dlist, int N, int Nph, int L, int ns, int nc,
                                                 int ndef, long long nbonds, int nqmax) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.y, o = ch * L * N;
    sm_pair_slice(part + ch * L * nqmax, v.X1 + o, v.X2 + o, v.R1 + o, v.R2 + o, x + ch * L * Nph, bs, bpar, bph, doff, dlist, N, Nph, ns, nc, ndef,
                  nbonds, blockIdx.x, red);
}

// one workgroup per chain.  C3: table 3 (G[D,0] G[0,D]) of chain 0; muo: [nchains][ns]; mu_mean: [nchains]; block: doubles of a chain's
// accumulators
__global__ void __launch_bounds__(TPB) k_sm_finish(double *__restrict__ acc, const double *__restrict__ part, const double *__restrict__ xs,
                                                   const double *__restrict__ muo, const double *__restrict__ mu_mean,
                                                   const double *__restrict__ C3, int N, int L, int ns, int nc, int ndef, int nqmax, double V,
                                                   size_t block) {
    extern __shared__ double tot[];                    // [nq] + red[NWAVE]
    const size_t ch = blockIdx.x;
    sm_finish(acc + ch * block, part + ch * L * nqmax, xs + ch * SM_NXONLY * ndef, muo + ch * ns, C3 + ch * L * ns * N, N, L, ns, nc, ndef,
              mu_mean[ch], V, tot);
}

// One workgroup per (frequency, listed pair of phonon types, chain).  LDS: 4 buffers of nc complex.
__global__ void __launch_bounds__(TPB) k_sm_ph(double2 *__restrict__ Y, const double2 *__restrict__ nu, const int *__restrict__ pairs, int Lh,
                                               int Nph, int L1, int L2, int L3, const double2 *__restrict__ tw, double norm) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3, k = blockIdx.x, p = blockIdx.y;
    const size_t ch = blockIdx.z, nP = gridDim.y;
    sm_ph(Y + ((ch * nP + p) * Lh + k) * nc, nu + (ch * Lh + k) * Nph, pairs[2 * p], pairs[2 * p + 1], L1, L2, L3, tw, norm, lds);
}

// One thread per (tau, cell, listed pair) of correlation blockIdx.y of chain blockIdx.z.  C: [table][chain][L][ns N]; B: [chain][nP][L][nc]
__global__ void __launch_bounds__(TPB) k_sm_fold(CorrReq<NCORR> rq, const double *__restrict__ C, const double *__restrict__ B, int N, int L, int ns,
                                                 int L1, int L2, int L3, int nchains, size_t block) {
    const size_t ch = blockIdx.z, tab = (size_t)L * ns * N;
    const size_t bch = (size_t)rq.np[PHONONGREENS] * L * L1 * L2 * L3;
    sm_fold(rq, blockIdx.y, (long long)blockIdx.x * TPB + threadIdx.x, C + ch * tab, B + ch * bch, N, L, ns, L1, L2, L3, (size_t)nchains * tab,
            ch * block);
}

__global__ void __launch_bounds__(TPB) k_sm_add(double *__restrict__ acc, const double *__restrict__ cur, long long n) { sm_add(acc, cur, n); }

// of every chain's row of mu[nchains][N]: its mean over the sites of an orbital (:1018), and behind them mean(model.mu) (:858)
int upload_mu(SshMeasState *m, const double *mu, int N) {
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

void sm_free(void *&slot) {
    SshMeasState *m = (SshMeasState *)slot;
    if (!m) return;
    corr_free({m->bs, m->bph, m->bpar, m->doff, m->dlist, m->mu, m->cr.pairs, m->cr.acc, m->cur, m->xr, m->x, m->xs, m->part, m->nu, m->Y, m->B});
    elph_i_greens_chain_scratch_free(&m->gs);
    delete m;
    slot = nullptr;
}

// The state of a request for nchains chains into the (freed) slot, after the entry point's refusals; mu: [nchains][N].  own_scratch: the
// state brings the scratch of the estimator's pipeline (the _chains entry points).
int sm_create(elph_handle_s *h, void *&slot, const CorrWords &W, int nchains, bool own_scratch, const double *mu, double dtau, int64_t nbonds,
              int ndef, const int64_t *bond_sites, const double *bond_t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon,
              int64_t Nph, int nph, const double *omega, const double *alpha, const double *alpha2, const int *measure,
              const int *time_dependent, const int *npairs, const int *pairs) {
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = g.ns, nc = g.nc;
    CorrSshBonds T;
    RC(corr_check_ssh_params(h, W.prefix, mu, dtau, nbonds, ndef, bond_sites, bond_t, bond_to_definition, bond_to_phonon, Nph, nph, omega, alpha,
                             alpha2, measure, time_dependent, npairs, T));
    const int nsc = 3 + SM_NONSITE * ns + SM_NINTER * ndef;
    CorrPlan<NCORR> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, W, CORR_NAMES, measure, time_dependent, npairs, pairs, ns, L, nc, (size_t)nsc, nph));
    const int nP = plan.req.np[PHONONGREENS];
    if (nP) RC(corr_check_phonongreens(W.prefix, nph, Nph, g.L1, g.L2, g.L3, sm_ph_lds_bytes(nc)));
    SshMeasState *m = new SshMeasState;
    slot = m;
    m->cr = plan;
    m->nchains = nchains; m->ns = ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = ndef; m->nph = nph; m->nbonds = nbonds;
    m->Nph = Nph; m->dtau = dtau; m->nsc = nsc;
    m->V = ndef ? (double)(nbonds / ndef) * (double)L : 1.0;           // div(Nbonds, nbonds) * Ltau, :1094
    m->nqmax = std::max(2 * ns + 2 + 2 * ndef, SM_NXONLY * ndef);
    const size_t nch = (size_t)nchains, nx = (size_t)L * (size_t)Nph, total = m->cr.total;
    CorrFirstError ok;
    const bool allocated = ok(corr_alloc(&m->bs, T.bs.size())) && ok(corr_alloc(&m->bph, T.bph.size())) && ok(corr_alloc(&m->bpar, T.bpar.size())) &&
        ok(corr_alloc(&m->doff, T.doff.size())) && ok(corr_alloc(&m->dlist, T.dlist.size())) && ok(corr_alloc(&m->mu, nch * ns + nch)) &&
        ok(corr_alloc(m->cr, nch)) && ok(corr_alloc(&m->cur, nch * total)) && ok(corr_alloc(&m->xr, nch * nx)) && ok(corr_alloc(&m->x, nch * nx)) &&
        ok(corr_alloc(&m->xs, nch * SM_NXONLY * ndef)) && ok(corr_alloc(&m->part, nch * L * m->nqmax)) &&
        (nP == 0 || (ok(corr_alloc(&m->nu, nch * Lh * Nph)) && ok(corr_alloc(&m->Y, nch * nP * Lh * nc)) && ok(corr_alloc(&m->B, nch * nP * L * nc)))) &&
        (!own_scratch || ok(elph_i_greens_chain_scratch_alloc(h, nchains, &m->gs)));
    if (!allocated) { sm_free(slot); return ok.rc; }
    ok(corr_up(m->bs, T.bs.data(), T.bs.size() * sizeof(int)));
    ok(corr_up(m->bph, T.bph.data(), T.bph.size() * sizeof(int)));
    ok(corr_up(m->bpar, T.bpar.data(), T.bpar.size() * sizeof(double)));
    ok(corr_up(m->doff, T.doff.data(), T.doff.size() * sizeof(int)));
    ok(corr_up(m->dlist, T.dlist.data(), T.dlist.size() * sizeof(int)));
    ok(upload_mu(m, mu, N));
    if (ok.rc == ELPH_OK) ok(corr_upload(m->cr, W.prefix, nch));
    m->rq_cur = m->cr.req;
    for (int c = 0; c < NCORR; ++c) m->rq_cur.acc[c] = m->cur + m->cr.off[c];
    const int lds = (int)sm_ph_lds_bytes(nc);
    if (ok.rc == ELPH_OK && nP && hipFuncSetAttribute((const void *)k_sm_ph, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
        elph_set_error("%s: %d bytes of LDS were refused", W.prefix, lds);
        ok(ELPH_E_HIP);
    }
    if (ok.rc != ELPH_OK) sm_free(slot);
    return ok.rc;
}

// Everything one accumulate queues on the handle's stream, the copy of the host's X first; the caller synchronises, whatever this returns.
// S: the scratch the estimator's pipeline runs in.
int sm_launches(elph_handle_s *h, SshMeasState *m, const ElphGreensView &g, const ElphGreensChainScratch &S, const double *X) {
    const int nch = m->nchains, N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = m->ns, nc = m->nc, nvc = g.nv / nch, ndef = m->ndef;
    const int Nph = (int)m->Nph, nP = m->cr.req.np[PHONONGREENS], nqmax = m->nqmax;
    const size_t block = m->cr.total, all = (size_t)nch * block;
    HIPCHK(hipMemsetAsync(m->cur, 0, all * sizeof(double), h->stream));
    // the tau-DFT launchers read their tables and the buffers they are handed, whatever the batch: nothing of the handle's workspace is used
    if (Nph > 0) {
        HIPCHK(hipMemcpyAsync(m->xr, X, (size_t)nch * L * Nph * sizeof(double), hipMemcpyHostToDevice, h->stream));
        RC(elph_launch_r2s(h, m->x, m->xr, nch, Nph));
    }
    // what depends on the fields alone: once per call, added once per pair below (the reference's loop recomputes it per pair)
    if (ndef) {
        hipLaunchKernelGGL(k_sm_x, dim3((unsigned)L, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, m->x, m->bpar, m->bph, m->doff, m->dlist, Nph, L,
                           ndef, (long long)m->nbonds, nqmax, m->dtau);
        RC(elph_launch_check("k_sm_x"));
        hipLaunchKernelGGL(k_sm_x_finish, dim3((unsigned)nch), dim3(TPB), 0, h->stream, m->xs, m->part, L, ndef, nqmax, m->V);
        RC(elph_launch_check("k_sm_x_finish"));
    }
    if (nP) {
        RC(elph_dft_fwd_plain(h, m->nu, m->x, Nph, nch));
        const double norm = 1.0 / ((double)L * (double)nc * (double)nc);       // 1/(L Nc)² in all: the other 1/L is in the inverse τ table
        hipLaunchKernelGGL(k_sm_ph, dim3((unsigned)Lh, (unsigned)nP, (unsigned)nch), dim3(TPB), sm_ph_lds_bytes(nc), h->stream, m->Y, m->nu,
                           m->cr.req.pairs[PHONONGREENS], Lh, Nph, m->L1, m->L2, m->L3, g.tw, norm);
        RC(elph_launch_check("k_sm_ph"));
        RC(elph_dft_inv_plain(h, m->B, m->Y, nc, nP * nch));
    }
    const int nq = 2 * ns + 2 + 2 * ndef;
    const size_t shm = ((size_t)nq + NWAVE) * sizeof(double);
    const size_t tab = (size_t)L * ns * N;
    const double *muo = m->mu, *mu_mean = m->mu + (size_t)nch * ns;
    for (int i = 1; i < nvc; ++i)
        for (int j = i + 1; j <= nvc; ++j) {           // pairs of a chain's vectors; every launch serves all chains
            ElphGreensPair v;
            RC(elph_i_greens_setup_chains_dev(h, S, i, j, &v));
            hipLaunchKernelGGL(k_sm_pair, dim3((unsigned)L, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, v, m->x, m->bs, m->bpar, m->bph, m->doff,
                               m->dlist, N, Nph, L, ns, nc, ndef, (long long)m->nbonds, nqmax);
            RC(elph_launch_check("k_sm_pair"));
            hipLaunchKernelGGL(k_sm_finish, dim3((unsigned)nch), dim3(TPB), shm, h->stream, m->cur, m->part, m->xs, muo, mu_mean,
                               S.C + 3 * (size_t)nch * tab, N, L, ns, nc, ndef, nqmax, m->V, block);
            RC(elph_launch_check("k_sm_finish"));
            if (m->cr.fold_max) {
                hipLaunchKernelGGL(k_sm_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), NCORR, (unsigned)nch), dim3(TPB), 0, h->stream, m->rq_cur,
                                   S.C, m->B, N, L, ns, m->L1, m->L2, m->L3, nch, block);
                RC(elph_launch_check("k_sm_fold"));
            }
        }
    hipLaunchKernelGGL(k_sm_add, dim3((unsigned)((all + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->cr.acc, m->cur, (long long)all);
    return elph_launch_check("k_sm_add");
}

// after the entry point's own checks: the estimator's vectors, the launches, one synchronisation
int sm_accumulate(elph_handle_s *h, SshMeasState *m, const CorrWords &W, const ElphGreensChainScratch *S, const double *X) {
    ElphGreensView g;
    RC(corr_vectors(h, W.prefix, m->nchains, &g));
    return corr_synchronised(h, W.prefix, sm_launches(h, m, g, *S, X));
}

int sm_fetch(elph_handle_s *h, const SshMeasState *m, int chain, double *scalars, double *const *outs) {
    std::vector<double> host;
    RC(corr_fetch(h, m->cr, host, outs, chain));
    if (scalars)
        for (int i = 0; i < m->nsc; ++i) scalars[i] = host[(size_t)i];
    return ELPH_OK;
}

SshMeasState *sm_of(void *slot) { return (SshMeasState *)slot; }
int need_ssh_meas(elph_handle_s *h) { return corr_need(h->ssh_meas, "elph_ssh_meas_create"); }
int need_chains(elph_handle_s *h) { return corr_need(h->ssh_meas_chains, "elph_ssh_meas_chains_create"); }

}  // namespace

void elph_i_ssh_meas_free(elph_handle_s *h) { sm_free(h->ssh_meas); }
void elph_ssh_meas_chains_free(elph_handle_s *h) { sm_free(h->ssh_meas_chains); }

// ---- one configuration per handle: mu[N], x[Nph][L]
extern "C" int elph_ssh_meas_free(elph_handle h) {
    CHECK_H(h);
    elph_i_ssh_meas_free(h);
    return ELPH_OK;
}

extern "C" int elph_ssh_meas_create(elph_handle h, const double *mu, double dtau, int64_t nbonds, int ndef, const int64_t *bond_sites,
                                    const double *bond_t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph,
                                    int nph, const double *omega, const double *alpha, const double *alpha2, const int *measure,
                                    const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_i_ssh_meas_free(h);
    RC(corr_refuse_handle(h, WORDS.prefix, ELPH_MODEL_SSH));
    return sm_create(h, h->ssh_meas, WORDS, 1, false, mu, dtau, nbonds, ndef, bond_sites, bond_t, bond_to_definition, bond_to_phonon, Nph, nph, omega,
                     alpha, alpha2, measure, time_dependent, npairs, pairs);
}

extern "C" int elph_ssh_meas_accumulate(elph_handle h, const double *x) {
    CHECK_H(h);
    RC(need_ssh_meas(h));
    RC(corr_refuse_chains(h, WORDS.prefix));
    SshMeasState *m = sm_of(h->ssh_meas);
    if (!x && m->Nph > 0) { elph_set_error("x is null"); return ELPH_E_ARG; }
    return sm_accumulate(h, m, WORDS, elph_i_greens_own_scratch(h), x);
}

extern "C" int elph_ssh_meas_fetch(elph_handle h, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                                   double *PhononGreens) {
    CHECK_H(h);
    RC(need_ssh_meas(h));
    double *outs[NCORR] = {Greens, DenDen, SpinSpin, PairGreens, PhononGreens};
    return sm_fetch(h, sm_of(h->ssh_meas), 0, scalars, outs);
}

extern "C" int elph_ssh_meas_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_ssh_meas(h));
    return corr_reset(h, sm_of(h->ssh_meas)->cr);
}

// ---- every resident chain at once: mu[nchains][N], X[nchains][Nph][L]
extern "C" int elph_ssh_meas_chains_create(elph_handle h, int nchains, const double *mu, double dtau, int64_t nbonds, int ndef,
                                           const int64_t *bond_sites, const double *bond_t, const int64_t *bond_to_definition,
                                           const int64_t *bond_to_phonon, int64_t Nph, int nph, const double *omega, const double *alpha,
                                           const double *alpha2, const int *measure, const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_ssh_meas_chains_free(h);
    RC(corr_refuse_model(h, WORDS_CHAINS.prefix, ELPH_MODEL_SSH));
    RC(corr_check_chain_count(h, WORDS_CHAINS.prefix, nchains));
    return sm_create(h, h->ssh_meas_chains, WORDS_CHAINS, nchains, true, mu, dtau, nbonds, ndef, bond_sites, bond_t, bond_to_definition, bond_to_phonon,
                     Nph, nph, omega, alpha, alpha2, measure, time_dependent, npairs, pairs);
}

extern "C" int elph_ssh_meas_chains_set_mu(elph_handle h, const double *mu) {
    CHECK_H(h);
    RC(need_chains(h));
    if (!mu) { elph_set_error("SSH chain measurements: mu is null"); return ELPH_E_ARG; }
    HIPCHK(hipStreamSynchronize(h->stream));
    return upload_mu(sm_of(h->ssh_meas_chains), mu, (int)h->N);
}

extern "C" int elph_ssh_meas_chains_accumulate(elph_handle h, const double *X) {
    CHECK_H(h);
    RC(need_chains(h));
    SshMeasState *m = sm_of(h->ssh_meas_chains);
    if (!X && m->Nph > 0) { elph_set_error("X is null"); return ELPH_E_ARG; }
    RC(corr_same_chains(h, WORDS_CHAINS.prefix, m->nchains));
    return sm_accumulate(h, m, WORDS_CHAINS, &m->gs, X);
}

extern "C" int elph_ssh_meas_chains_fetch(elph_handle h, int chain, double *scalars, double *Greens, double *DenDen, double *SpinSpin,
                                          double *PairGreens, double *PhononGreens) {
    CHECK_H(h);
    RC(need_chains(h));
    const SshMeasState *m = sm_of(h->ssh_meas_chains);
    RC(corr_check_chain(WORDS_CHAINS.prefix, chain, m->nchains));
    double *outs[NCORR] = {Greens, DenDen, SpinSpin, PairGreens, PhononGreens};
    return sm_fetch(h, m, chain, scalars, outs);
}

extern "C" int elph_ssh_meas_chains_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_chains(h));
    const SshMeasState *m = sm_of(h->ssh_meas_chains);
    return corr_reset(h, m->cr, (size_t)m->nchains);
}
