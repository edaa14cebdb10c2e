// ssh_measure.hip — the measurements of the bond-phonon (SSH) model accumulated on the device (DESIGN.md "Measurements on the device"):
//   make_measurements!             Measurements.jl:545-566   (without its update!: the estimator's vectors are there already)
//     make_global_measurements!    :845-861, :1283-1312      density, Nsqr, mu
//     make_onsite_measurements!    :978-1024                 density, double_occ, mu per orbital
//     make_intersite_measurements! :1072-1155                x, x2, x4, phonon_pe, phonon_ke, elph_energy, el_ke, sign_switch per bond definition
//     measure_Greens! / _DenDen! / _SpinSpin! / _PairGreens!  :1469-1596   the folds of meas_dev.h, shared with measure.hip
//     measure_PhononGreens!        :2488-2541                the field's translation average over phonon types
//   reset_measurements!            :698-758
// One allocation holds [scalars | Greens | DenDen | SpinSpin | PairGreens | PhononGreens], all real doubles (corr_req.h).
//
// Bonds come in the reference's order (model.t, bond_to_definition, bond_to_phonon; sites neighbor_table[:, checkerboard_perm[bond]]).
// The bonds of one definition are walked in bond order through a list made at create, so a definition may own any number of bonds; the
// normalisation is the reference's V = (Nbonds / nbonds) Ltau.  The modulated hopping t' = t - (alpha x + sign(x) alpha2 x^2)
// (SSHModels.jl:531-533) is recomputed from the field, t' = t on a bare bond.
//
// Reductions have the ONE order of measure.hip: a thread walks its cells / bonds in index order, the 64 lanes of a wave fold by halves,
// the waves are added in index order through LDS, each workgroup (= one time slice) writes one partial, a single workgroup adds the L
// partials in slice order.  No floating-point atomics.  What depends on the field alone (x ... phonon_ke, sign_switch, PhononGreens) is
// computed once per accumulate and added once per pair of vectors.  One accumulate adds its pairs of vectors up from zero in a buffer of
// its own (cur) and adds that to the accumulators once at the end: two accumulations of the same inputs are twice one, to the bit.
//
// The field is (Ltau, Nph) in the reference, phonon slowest; here layout S with Nph columns: x[tau * Nph + phonon], and for
// PhononGreens phonon = cell + ncells * type (the reference's reshape to (Ltau, L1, L2, L3, nph)).  PhononGreens of the pair (b1, b2) is
//   1/(L Nc) sum_{tau, cell} x_b2[tau + dtau, cell + dcell] x_b1[tau, cell]
// spectrally: plain half spectra along tau of all Nph columns, then per (frequency, listed pair) the cell-axis DFTs of the two types in
// LDS (cell_dft_dev.h, unit = 1), their product, the inverse cell-axis DFT, and one inverse tau-transform of all listed pairs — in
// scratch this unit owns (the estimator's is sized for n_s orbitals, and nph > n_s is the normal case).
//
// What one workgroup does in each kernel is in meas_ssh_dev.h, shared with ssh_measure_chains.hip (every resident chain of a lockstep run at
// once, the chain a grid axis); this unit holds the kernels of one configuration per handle and keeps refusing resident chains.

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
constexpr int NONSITE = SM_NONSITE, NINTER = SM_NINTER, NXONLY = SM_NXONLY;

struct SshMeasState {
    int ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0, nph = 0;
    int64_t nbonds = 0, Nph = 0;
    double dtau = 0.0, mu_mean = 0.0, V = 1.0;
    int *bs = nullptr;              // [2][nbonds] 0-based sites of every bond, the reference's bond order
    int *bph = nullptr;             // [nbonds] 0-based phonon of the bond, -1 on a bare bond
    double *bpar = nullptr;         // [SM_NBPAR][nbonds]
    int *doff = nullptr;            // [ndef + 1] offsets into dlist
    int *dlist = nullptr;           // [nbonds] the bonds of every definition, in bond order
    double *muo = nullptr;          // [ns] mean of mu over the sites of an orbital
    CorrPlan<NCORR> cr;             // the requests; cr.acc: [nsc | the measured correlations]
    int nsc = 0;
    double *cur = nullptr;          // [cr.total] this accumulate's sums, laid out as cr.acc
    CorrReq<NCORR> rq_cur{};        // cr.req with its accumulators in cur
    double *xr = nullptr;           // [Nph][L] the field as the caller holds it
    double *x = nullptr;            // [L][Nph] the field, layout S
    double *xs = nullptr;           // [NXONLY][ndef] the field-only terms of this accumulate, normalised
    double *part = nullptr;         // [L][max(nq, NXONLY * ndef)] one partial per workgroup
    double2 *nu = nullptr;          // [Lh][Nph] the field's half spectra          (PhononGreens requested)
    double2 *Y = nullptr;           // [nP][Lh][nc] per-frequency correlations of the listed pairs
    double *B = nullptr;            // [nP][L][nc] the translation averages of this accumulate
};

SshMeasState *sm_of(elph_handle_s *h) { return (SshMeasState *)h->ssh_meas; }

// ---- what a workgroup does is in meas_ssh_dev.h; here, where it finds the one configuration of the handle
// one workgroup per time slice
__global__ void __launch_bounds__(TPB) k_sm_x(double *__restrict__ part, const double *__restrict__ x, const double *__restrict__ bpar,
                                              const int *__restrict__ bph, const int *__restrict__ doff, const int *__restrict__ dlist, int Nph,
                                              int L, int ndef, long long nbonds, double dtau) {
    __shared__ double red[NWAVE];
    sm_x_slice(part, x, bpar, bph, doff, dlist, Nph, L, ndef, nbonds, dtau, blockIdx.x, red);
}

__global__ void __launch_bounds__(TPB) k_sm_x_finish(double *__restrict__ xs, const double *__restrict__ part, int L, int ndef, double V) {
    sm_x_finish(xs, part, L, ndef, V);
}

// one workgroup per time slice
__global__ void __launch_bounds__(TPB) k_sm_pair(double *__restrict__ part, const double *__restrict__ X1, const double *__restrict__ X2,
                                                 const double *__restrict__ R1, const double *__restrict__ R2, const double *__restrict__ x,
                                                 const int *__restrict__ bs, const double *__restrict__ bpar, const int *__restrict__ bph,
                                                 const int *__restrict__ doff, const int *__restrict__ dlist, int N, int Nph, int ns, int nc,
                                                 int ndef, long long nbonds) {
    __shared__ double red[NWAVE];
    sm_pair_slice(part, X1, X2, R1, R2, x, bs, bpar, bph, doff, dlist, N, Nph, ns, nc, ndef, nbonds, blockIdx.x, red);
}

// one workgroup
__global__ void __launch_bounds__(TPB) k_sm_finish(double *__restrict__ acc, const double *__restrict__ part, const double *__restrict__ xs,
                                                   const double *__restrict__ muo, const double *__restrict__ C3, int N, int L, int ns, int nc,
                                                   int ndef, double mu_mean, double V) {
    extern __shared__ double tot[];                    // [nq] + red[NWAVE]
    sm_finish(acc, part, xs, muo, C3, N, L, ns, nc, ndef, mu_mean, V, tot);
}

// one workgroup per (frequency, listed pair of phonon types); LDS: 4 buffers of nc complex
__global__ void __launch_bounds__(TPB) k_sm_ph(double2 *__restrict__ Y, const double2 *__restrict__ nu, const int *__restrict__ pairs, int Lh,
                                               int Nph, int L1, int L2, int L3, const double2 *__restrict__ tw, double norm) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3, k = blockIdx.x, p = blockIdx.y;
    sm_ph(Y + ((size_t)p * Lh + k) * nc, nu + (size_t)k * Nph, pairs[2 * p], pairs[2 * p + 1], L1, L2, L3, tw, norm, lds);
}

// one thread per (tau, cell, listed pair) of correlation blockIdx.y
__global__ void __launch_bounds__(TPB) k_sm_fold(CorrReq<NCORR> rq, const double *__restrict__ C, const double *__restrict__ B, int N, int L, int ns,
                                                 int L1, int L2, int L3) {
    sm_fold(rq, blockIdx.y, (long long)blockIdx.x * TPB + threadIdx.x, C, B, N, L, ns, L1, L2, L3);
}

__global__ void __launch_bounds__(TPB) k_sm_add(double *__restrict__ acc, const double *__restrict__ cur, long long n) { sm_add(acc, cur, n); }

int need_ssh_meas(elph_handle_s *h) { return corr_need(h->ssh_meas, "elph_ssh_meas_create"); }

}  // namespace

void elph_i_ssh_meas_free(elph_handle_s *h) {
    SshMeasState *m = sm_of(h);
    if (!m) return;
    corr_free({m->bs, m->bph, m->bpar, m->doff, m->dlist, m->muo, m->cr.pairs, m->cr.acc, m->cur, m->xr, m->x, m->xs, m->part, m->nu, m->Y, m->B});
    delete m;
    h->ssh_meas = nullptr;
}

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
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = g.ns, nc = g.nc;
    CorrSshBonds T;
    RC(corr_check_ssh_params(h, WORDS.prefix, mu, dtau, nbonds, ndef, bond_sites, bond_t, bond_to_definition, bond_to_phonon, Nph, nph, omega, alpha,
                             alpha2, measure, time_dependent, npairs, T));
    const int nsc = 3 + NONSITE * ns + NINTER * ndef;
    CorrPlan<NCORR> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, WORDS, CORR_NAMES, measure, time_dependent, npairs, pairs, ns, L, nc, (size_t)nsc, nph));
    const int nP = plan.req.np[PHONONGREENS];
    if (nP) RC(corr_check_phonongreens(WORDS.prefix, nph, Nph, g.L1, g.L2, g.L3, sm_ph_lds_bytes(nc)));
    SshMeasState *m = new SshMeasState;
    h->ssh_meas = m;
    m->cr = plan;
    m->ns = ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = ndef; m->nph = nph; m->nbonds = nbonds; m->Nph = Nph;
    m->dtau = dtau; m->nsc = nsc;
    m->V = ndef ? (double)(nbonds / ndef) * (double)L : 1.0;           // div(Nbonds, nbonds) * Ltau, :1094
    double mus = 0.0;
    for (int i = 0; i < N; ++i) mus += mu[i];
    m->mu_mean = mus / N;                              // mean(model.mu), :858
    std::vector<double> muo((size_t)ns, 0.0);          // sum over the cells and slices of mu[site] / (Nc L), :1018
    for (int o = 0; o < ns; ++o) {
        for (int c = 0; c < nc; ++c) muo[(size_t)o] += mu[(size_t)c * ns + o];
        muo[(size_t)o] /= nc;
    }
    const int nq = std::max(2 * ns + 2 + 2 * ndef, NXONLY * ndef);
    const size_t nx = (size_t)L * (size_t)Nph;
    CorrFirstError ok;
    const bool allocated = ok(corr_alloc(&m->bs, T.bs.size())) && ok(corr_alloc(&m->bph, T.bph.size())) && ok(corr_alloc(&m->bpar, T.bpar.size())) &&
        ok(corr_alloc(&m->doff, T.doff.size())) && ok(corr_alloc(&m->dlist, T.dlist.size())) && ok(corr_alloc(&m->muo, muo.size())) &&
        ok(corr_alloc(m->cr)) && ok(corr_alloc(&m->cur, m->cr.total)) && ok(corr_alloc(&m->xr, nx)) && ok(corr_alloc(&m->x, nx)) && ok(corr_alloc(&m->xs, (size_t)NXONLY * ndef)) &&
        ok(corr_alloc(&m->part, (size_t)L * nq)) &&
        (nP == 0 || (ok(corr_alloc(&m->nu, (size_t)Lh * Nph)) && ok(corr_alloc(&m->Y, (size_t)nP * Lh * nc)) && ok(corr_alloc(&m->B, (size_t)nP * L * nc))));
    if (!allocated) { elph_i_ssh_meas_free(h); return ok.rc; }
    ok(corr_up(m->bs, T.bs.data(), T.bs.size() * sizeof(int)));
    ok(corr_up(m->bph, T.bph.data(), T.bph.size() * sizeof(int)));
    ok(corr_up(m->bpar, T.bpar.data(), T.bpar.size() * sizeof(double)));
    ok(corr_up(m->doff, T.doff.data(), T.doff.size() * sizeof(int)));
    ok(corr_up(m->dlist, T.dlist.data(), T.dlist.size() * sizeof(int)));
    ok(corr_up(m->muo, muo.data(), muo.size() * sizeof(double)));
    if (ok.rc == ELPH_OK) ok(corr_upload(m->cr, WORDS.prefix));
    m->rq_cur = m->cr.req;
    for (int c = 0; c < NCORR; ++c) m->rq_cur.acc[c] = m->cur + m->cr.off[c];
    const int lds = (int)sm_ph_lds_bytes(nc);
    if (ok.rc == ELPH_OK && nP && hipFuncSetAttribute((const void *)k_sm_ph, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
        elph_set_error("SSH measurements: %d bytes of LDS were refused", lds);
        ok(ELPH_E_HIP);
    }
    if (ok.rc != ELPH_OK) elph_i_ssh_meas_free(h);
    return ok.rc;
}

extern "C" int elph_ssh_meas_accumulate(elph_handle h, const double *x) {
    CHECK_H(h);
    RC(need_ssh_meas(h));
    RC(corr_refuse_chains(h, WORDS.prefix));
    SshMeasState *m = sm_of(h);
    if (!x && m->Nph > 0) { elph_set_error("x is null"); return ELPH_E_ARG; }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = m->ns, nc = m->nc, nv = g.nv, ndef = m->ndef, Nph = (int)m->Nph;
    const int nP = m->cr.req.np[PHONONGREENS];
    const size_t total = std::max<size_t>(m->cr.total, 1);
    HIPCHK(hipMemsetAsync(m->cur, 0, total * sizeof(double), h->stream));
    if (Nph > 0) {
        HIPCHK(hipMemcpyAsync(m->xr, x, (size_t)L * Nph * sizeof(double), hipMemcpyHostToDevice, h->stream));
        RC(elph_launch_r2s(h, m->x, m->xr, 1, Nph));
    }
    // what depends on the field alone: once per call, added once per pair below (the reference's loop recomputes it per pair)
    if (ndef) {
        hipLaunchKernelGGL(k_sm_x, dim3((unsigned)L), dim3(TPB), 0, h->stream, m->part, m->x, m->bpar, m->bph, m->doff, m->dlist, Nph, L, ndef,
                           (long long)m->nbonds, m->dtau);
        RC(elph_launch_check("k_sm_x"));
        hipLaunchKernelGGL(k_sm_x_finish, dim3(1), dim3(TPB), 0, h->stream, m->xs, m->part, L, ndef, m->V);
        RC(elph_launch_check("k_sm_x_finish"));
    }
    if (nP) {
        RC(elph_dft_fwd_plain(h, m->nu, m->x, Nph, 1));
        const double norm = 1.0 / ((double)L * (double)nc * (double)nc);       // 1/(L Nc)² in all: the other 1/L is in the inverse τ table
        hipLaunchKernelGGL(k_sm_ph, dim3((unsigned)Lh, (unsigned)nP), dim3(TPB), sm_ph_lds_bytes(nc), h->stream, m->Y, m->nu,
                           m->cr.req.pairs[PHONONGREENS], Lh, Nph, m->L1, m->L2, m->L3, g.tw, norm);
        RC(elph_launch_check("k_sm_ph"));
        RC(elph_dft_inv_plain(h, m->B, m->Y, nc, nP));
    }
    const int nq = 2 * ns + 2 + 2 * ndef;
    const size_t shm = ((size_t)nq + NWAVE) * sizeof(double);
    const size_t tab = (size_t)L * ns * N;
    for (int i = 1; i < nv; ++i)
        for (int j = i + 1; j <= nv; ++j) {
            ElphGreensPair v;
            RC(elph_i_greens_pair_dev(h, i, j, &v));
            hipLaunchKernelGGL(k_sm_pair, dim3((unsigned)L), dim3(TPB), 0, h->stream, m->part, v.X1, v.X2, v.R1, v.R2, m->x, m->bs, m->bpar, m->bph,
                               m->doff, m->dlist, N, Nph, ns, nc, ndef, (long long)m->nbonds);
            RC(elph_launch_check("k_sm_pair"));
            hipLaunchKernelGGL(k_sm_finish, dim3(1), dim3(TPB), shm, h->stream, m->cur, m->part, m->xs, m->muo, g.C + 3 * tab, N, L, ns, nc, ndef,
                               m->mu_mean, m->V);
            RC(elph_launch_check("k_sm_finish"));
            if (m->cr.fold_max) {
                hipLaunchKernelGGL(k_sm_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), NCORR), dim3(TPB), 0, h->stream, m->rq_cur, g.C, m->B, N, L,
                                   ns, m->L1, m->L2, m->L3);
                RC(elph_launch_check("k_sm_fold"));
            }
        }
    hipLaunchKernelGGL(k_sm_add, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->cr.acc, m->cur, (long long)m->cr.total);
    RC(elph_launch_check("k_sm_add"));
    HIPCHK(hipStreamSynchronize(h->stream));           // x (a host pointer) is not retained after return
    return ELPH_OK;
}

extern "C" int elph_ssh_meas_fetch(elph_handle h, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                                   double *PhononGreens) {
    CHECK_H(h);
    RC(need_ssh_meas(h));
    SshMeasState *m = sm_of(h);
    std::vector<double> host;
    double *outs[NCORR] = {Greens, DenDen, SpinSpin, PairGreens, PhononGreens};
    RC(corr_fetch(h, m->cr, host, outs));
    if (scalars)
        for (int i = 0; i < m->nsc; ++i) scalars[i] = host[(size_t)i];
    return ELPH_OK;
}

extern "C" int elph_ssh_meas_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_ssh_meas(h));
    return corr_reset(h, sm_of(h)->cr);
}
