// ssh_bondcorr_chains.hip — the inter-site correlations of ssh_bondcorr.hip for EVERY chain resident in the handle at once (DESIGN.md
// "SSH bond correlations of resident chains"): the chain is the last grid axis of every kernel, so the launches of one accumulate depend
// on the vectors per chain and on the request, not on the number of chains.
//   measure_BondBond!                Measurements.jl:1663-1785     the chain kernels of bondcorr_dev.h, shared with bondcorr_chains.hip
//   measure_BondPairGreens!          Measurements.jl:2390-2483
//   measure_CurrentCurrent!(ssh)     Measurements.jl:2100-2384     the bodies of currcorr_dev.h, shared with ssh_bondcorr.hip and currcorr.hip
// per chain, for every pair of ITS vectors.  What a thread or workgroup computes is ssh_bondcorr.hip's, and so is the rule of the
// reductions: a thread walks its cells in index order, the lanes of a wave fold by halves, the waves are added in index order through
// LDS, one partial per time slice, the slices added in slice order; everything else is one thread's sum in index order.  No
// floating-point atomics, no reduction split across workgroups.  A workgroup reads one chain's vectors, field and tables only, so chain
// c's numbers depend on nothing of another chain.
//
// Layouts.  Vector v (0-based) of chain c is row v nchains + c of the estimator (greens.chain_vector), so the v-th vectors of all chains
// are one block [chain][ndim].  The fields arrive as X[chain][Nph][L] (the reference's layout per chain) and stay so on the device (xr):
// chain c's t′ reads xr + c Nph L.  Every buffer carries the chain between the definition (or listed pair) and the time axis:
//   f  [NCC][ndef][chain][L][nc]     nu [NCC][ndef][chain][Lh][nc]     Y [pair][chain][Lh][nc]     B [pair][chain][L][nc]
//   part [pair][chain][L][NDELTA]    dl [pair][chain][NDELTA]
// so the forward tau-DFT is one elph_dft_fwd_plain of NCC ndef nchains right-hand sides, the cell-axis DFT k_bc_spatial_fwd as it is over
// as many slices, and the inverse one elph_dft_inv_plain of np nchains.  The CurrentCurrent accumulator is ONE allocation
// [chain][CurrentCurrent], a chain's block laid out as elph_ssh_bond_fetch's; BondBond and BondPairGreens live in a BondState for nchains
// configurations (bondcorr_dev.h) with its own [chain][BondBond | BondPairGreens]: reset is one memset per allocation.  The estimator's
// pipeline for one pair of vectors of all chains runs in scratch this state owns (elph_i_greens_setup_chains_dev); the δ terms of
// CurrentCurrent read vector 1 of the chain's own pair.  LDS per workgroup is ssh_bondcorr.hip's (bc_lds_bytes).

#include <vector>

#include "currcorr_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int NWAVE = MEAS_NWAVE;
const CorrWords WORDS = {"SSH chain bond correlations", "bond", "with no pair of bonds"};
constexpr long long GRID_YZ_MAX = 65535;

struct SshBondChainsState {
    int nchains = 1;
    BondState *bond = nullptr;      // BondBond, BondPairGreens of all chains (null: neither requested)
    ElphGreensChainScratch gs{};    // the estimator's pipeline for all chains
    // CurrentCurrent (allocated when it is requested)
    int ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0;
    int64_t Nph = 0;
    CorrPlan<1> cr;                 // ONE chain's plan; cr.acc: [chain][CurrentCurrent], cr.req bound to chain 0
    int *defs = nullptr;            // [ndef][DEFW]
    int *bph = nullptr;             // [ndef nc] 0-based phonon of bond cell + nc n, -1 on a bare bond
    double *bpar = nullptr;         // [NHPAR][ndef nc]
    double *xr = nullptr;           // [chain][Nph][L] the fields as the caller holds them
    double *f = nullptr;            // [NCC][ndef][chain][L][nc] the fields of one pair of vectors
    double2 *nu = nullptr;          // [NCC][ndef][chain][Lh][nc] their half spectra, then their cell-axis DFTs in place
    double2 *Y = nullptr;           // [np][chain][Lh][nc] per-frequency correlations of the listed pairs
    double *B = nullptr;            // [np][chain][L][nc]
    double *part = nullptr;         // [np][chain][L][NDELTA] one partial per time slice
    double *dl = nullptr;           // [np][chain][NDELTA] the δ terms of one pair of vectors, signed and normalised
};

SshBondChainsState *sbc_of(elph_handle_s *h) { return (SshBondChainsState *)h->ssh_bond_chains; }

int need_state(elph_handle_s *h) { return corr_need(h->ssh_bond_chains, "elph_ssh_bond_chains_create"); }

bool has_current(const SshBondChainsState *m) { return m->cr.req.np[0] > 0; }

// ---- the CurrentCurrent kernels of ssh_bondcorr.hip with the chain as the last grid axis; per: L nc, slice: Lh nc

// One thread per (cell, τ, definition) of chain blockIdx.y.  v: chain 0's vectors, chain c's c L N further on; xr: chain 0's field.
__global__ void __launch_bounds__(TPB) k_ccc_fields(double *__restrict__ f, ElphGreensPair v, const int *__restrict__ defs,
                                                    const double *__restrict__ bpar, const int *__restrict__ bph, const double *__restrict__ xr,
                                                    int N, int Nph, int L, int ns, int L1, int L2, int L3, int ndef, int nchains) {
    const size_t ch = blockIdx.y, o = ch * L * N, per = (size_t)L * (L1 * L2 * L3);
    cc_fields_at(f + ch * per, v.X1 + o, v.X2 + o, v.R1 + o, v.R2 + o, defs, CcModulated{bpar, bph, xr + ch * Nph * L, ndef * (L1 * L2 * L3), L}, N,
                 L, ns, L1, L2, L3, ndef, (long long)blockIdx.x * TPB + threadIdx.x, (size_t)nchains * per);
}

// One workgroup per (frequency, listed pair, chain).  LDS: 2 buffers of nc complex.
__global__ void __launch_bounds__(TPB) k_ccc_correlate(double2 *__restrict__ Y, const double2 *__restrict__ nu, CcReq rq, int Lh, int ndef, int L1,
                                                       int L2, int L3, const double2 *__restrict__ tw, double norm, int nchains) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3;
    const size_t ch = blockIdx.z, slice = (size_t)Lh * nc;
    cc_correlate_slice(Y + (((size_t)blockIdx.y * nchains + ch) * Lh + blockIdx.x) * nc, nu + ch * slice, rq, blockIdx.y, blockIdx.x, ndef, L1, L2, L3, tw,
                       norm, (size_t)nchains * slice, lds);
}

// One workgroup per (time slice, listed pair, chain).  X1, R1: vector 1 of chain 0's pair.
__global__ void __launch_bounds__(TPB) k_ccc_delta(double *__restrict__ part, CcReq rq, const double *__restrict__ X1, const double *__restrict__ R1,
                                                   const int *__restrict__ defs, const double *__restrict__ bpar, const int *__restrict__ bph,
                                                   const double *__restrict__ xr, int N, int Nph, int L, int ns, int L1, int L2, int L3, int ndef,
                                                   int nchains) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.z, o = ch * L * N;
    cc_delta_slice(part + ((size_t)blockIdx.y * nchains + ch) * L * NDELTA, rq, blockIdx.y, blockIdx.x, X1 + o, R1 + o, defs,
                   CcModulated{bpar, bph, xr + ch * Nph * L, ndef * (L1 * L2 * L3), L}, N, ns, L1, L2, L3, red);
}

// One thread per (δ term, chain, listed pair): dl and part are [pair][chain] blocks, np nchains of them.
__global__ void __launch_bounds__(TPB) k_ccc_delta_finish(double *__restrict__ dl, const double *__restrict__ part, int np, int nchains, int L, int nc) {
    cc_delta_finish_at(dl, part, np * nchains, L, nc, blockIdx.x * TPB + threadIdx.x);
}

// One thread per (τ, cell, listed pair) of chain blockIdx.z.  block: doubles of a chain's accumulator.
__global__ void __launch_bounds__(TPB) k_ccc_fold(CcReq rq, const double *__restrict__ B, const double *__restrict__ dl, const int *__restrict__ defs,
                                                  int L, int L1, int L2, int L3, int nchains, size_t block) {
    const size_t ch = blockIdx.z, per = (size_t)L * (L1 * L2 * L3);
    cc_fold_at(rq, (long long)blockIdx.x * TPB + threadIdx.x, B + ch * per, dl + ch * NDELTA, defs, L, L1, L2, L3, (size_t)nchains * per,
               (size_t)nchains * NDELTA, ch * block);
}

// CurrentCurrent of one pair of vectors v of every chain into m's accumulator
int ccc_accumulate_pair(elph_handle_s *h, SshBondChainsState *m, const ElphGreensView &g, const ElphGreensPair &v) {
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = m->ns, nc = m->nc, ndef = m->ndef, np = m->cr.req.np[0], nch = m->nchains;
    const int Nph = (int)m->Nph;
    const size_t shm = bc_lds_bytes(nc);
    const long long nfld = (long long)L * nc * ndef;
    const double norm = 1.0 / ((double)L * (double)nc * (double)nc);   // 1/(L Nc)² in all: the other 1/L is in the inverse τ table
    hipLaunchKernelGGL(k_ccc_fields, dim3((unsigned)((nfld + TPB - 1) / TPB), (unsigned)nch), dim3(TPB), 0, h->stream, m->f, v, m->defs, m->bpar, m->bph,
                       m->xr, N, Nph, L, ns, m->L1, m->L2, m->L3, ndef, nch);
    RC(elph_launch_check("k_ccc_fields"));
    RC(elph_dft_fwd_plain(h, m->nu, m->f, nc, NCC * ndef * nch));
    hipLaunchKernelGGL(k_bc_spatial_fwd, dim3((unsigned)Lh, (unsigned)(NCC * ndef * nch)), dim3(TPB), shm, h->stream, m->nu, Lh, m->L1, m->L2, m->L3,
                       g.tw);
    RC(elph_launch_check("k_bc_spatial_fwd(CurrentCurrent, chains)"));
    hipLaunchKernelGGL(k_ccc_correlate, dim3((unsigned)Lh, (unsigned)np, (unsigned)nch), dim3(TPB), shm, h->stream, m->Y, m->nu, m->cr.req, Lh, ndef,
                       m->L1, m->L2, m->L3, g.tw, norm, nch);
    RC(elph_launch_check("k_ccc_correlate"));
    RC(elph_dft_inv_plain(h, m->B, m->Y, nc, np * nch));
    hipLaunchKernelGGL(k_ccc_delta, dim3((unsigned)L, (unsigned)np, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, m->cr.req, v.X1, v.R1, m->defs,
                       m->bpar, m->bph, m->xr, N, Nph, L, ns, m->L1, m->L2, m->L3, ndef, nch);
    RC(elph_launch_check("k_ccc_delta"));
    hipLaunchKernelGGL(k_ccc_delta_finish, dim3((unsigned)(((long long)np * nch * NDELTA + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->dl, m->part, np,
                       nch, L, nc);
    RC(elph_launch_check("k_ccc_delta_finish"));
    hipLaunchKernelGGL(k_ccc_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), 1, (unsigned)nch), dim3(TPB), 0, h->stream, m->cr.req, m->B, m->dl,
                       m->defs, L, m->L1, m->L2, m->L3, nch, m->cr.total);
    return elph_launch_check("k_ccc_fold");
}

// Everything one accumulate queues on the handle's stream, the copy of the host's X first; the caller synchronises, whatever this returns.
int accumulate_launches(elph_handle_s *h, SshBondChainsState *m, const ElphGreensView &g, const double *X) {
    const int nch = m->nchains, nvc = g.nv / nch;
    const bool current = has_current(m);
    if (!current && !m->bond) return ELPH_OK;
    if (current && m->Nph > 0)
        HIPCHK(hipMemcpyAsync(m->xr, X, (size_t)nch * h->L * m->Nph * sizeof(double), hipMemcpyHostToDevice, h->stream));
    for (int i = 1; i < nvc; ++i)
        for (int j = i + 1; j <= nvc; ++j) {           // pairs of a chain's vectors; every launch serves all chains
            ElphGreensPair v;                          // its setup leaves G[Δ,0] of every chain's pair of vectors for the δ terms of the BondState
            RC(elph_i_greens_setup_chains_dev(h, m->gs, i, j, &v));
            if (m->bond) RC(bc_accumulate_pair_chains(h, m->bond, g, m->gs, v));
            if (current) RC(ccc_accumulate_pair(h, m, g, v));
        }
    return ELPH_OK;
}

}  // namespace

void elph_ssh_bond_chains_free(elph_handle_s *h) {
    SshBondChainsState *m = sbc_of(h);
    if (!m) return;
    bc_free(m->bond);
    corr_free({m->cr.pairs, m->cr.acc, m->defs, m->bph, m->bpar, m->xr, m->f, m->nu, m->Y, m->B, m->part, m->dl});
    elph_i_greens_chain_scratch_free(&m->gs);
    delete m;
    h->ssh_bond_chains = nullptr;
}

extern "C" int elph_ssh_bond_chains_create(elph_handle h, int nchains, int n_def, const int *o1, const int *o2, const int *v, int64_t Nbonds,
                                           const double *t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph,
                                           const double *alpha, const double *alpha2, const int *measure, const int *time_dependent,
                                           const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_ssh_bond_chains_free(h);
    RC(corr_refuse_model(h, WORDS.prefix, ELPH_MODEL_SSH));
    if (nchains < 1 || nchains != h->nchains) {
        elph_set_error("%s: created for %d chains, %d are resident in this handle", WORDS.prefix, nchains, h->nchains);
        return ELPH_E_ARG;
    }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    RC(bc_check(WORDS, g, n_def, o1, o2, v, measure, time_dependent, npairs));
    std::vector<int> defs;
    RC(bc_defs_table(defs, WORDS, g, n_def, o1, o2, v));
    const int L = (int)h->L, Lh = L / 2 + 1, nc = g.nc;
    CorrPlan<NBOND> bplan;                             // request bookkeeping before anything is allocated
    CorrPlan<1> cplan;
    RC(cc_split_plans(bplan, cplan, WORDS, measure, time_dependent, npairs, pairs, n_def, L, nc));
    const int np = cplan.req.np[0];
    const size_t nb = (size_t)n_def * nc;
    std::vector<int> bph;
    std::vector<double> bpar;
    if (np) RC(cc_check_params(h, WORDS.prefix, n_def, nc, Nbonds, t, bond_to_definition, bond_to_phonon, Nph, alpha, alpha2, bph, bpar));
    // the chain multiplies the slices of the cell-axis DFT (grid y) and the right-hand sides of the tau-DFTs (grid z)
    const long long nk = std::max<long long>((bplan.req.np[BONDBOND] ? 4 : 0) + (bplan.req.np[BONDPAIR] ? NFIELD - 4 : 0), np ? NCC : 0);
    if (nk * n_def * nchains > GRID_YZ_MAX) {
        elph_set_error("%s: %lld fields x %d bond definitions x %d chains = %lld slices exceed the grid's %lld", WORDS.prefix, nk, n_def, nchains,
                       nk * n_def * nchains, GRID_YZ_MAX);
        return ELPH_E_UNSUPPORTED;
    }
    const long long nlist = std::max(bplan.npairs, np);
    if (nlist * nchains > GRID_YZ_MAX) {
        elph_set_error("%s: %lld listed pairs x %d chains = %lld transforms exceed the grid's %lld", WORDS.prefix, nlist, nchains, nlist * nchains,
                       GRID_YZ_MAX);
        return ELPH_E_UNSUPPORTED;
    }
    SshBondChainsState *m = new SshBondChainsState;
    h->ssh_bond_chains = m;
    m->nchains = nchains; m->ns = g.ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = n_def; m->Nph = Nph;
    m->cr = cplan;
    const size_t nch = (size_t)nchains;
    CorrFirstError ok;
    if (bplan.npairs) ok(bc_make(&m->bond, h, WORDS, g, bplan, defs, n_def, nchains, k_bcc_correlate));
    if (ok.rc == ELPH_OK && (bplan.npairs || np)) ok(elph_i_greens_chain_scratch_alloc(h, nchains, &m->gs));
    if (ok.rc == ELPH_OK && np) {
        const size_t nf = nch * NCC * n_def, nP = nch * np;
        const bool allocated = ok(corr_alloc(&m->cr.pairs, m->cr.prs.size())) && ok(corr_alloc(&m->cr.acc, nch * m->cr.total)) &&
            ok(corr_alloc(&m->defs, defs.size())) && ok(corr_alloc(&m->bph, nb)) && ok(corr_alloc(&m->bpar, bpar.size())) &&
            ok(corr_alloc(&m->xr, nch * L * Nph)) && ok(corr_alloc(&m->f, nf * L * nc)) && ok(corr_alloc(&m->nu, nf * Lh * nc)) &&
            ok(corr_alloc(&m->Y, nP * Lh * nc)) && ok(corr_alloc(&m->B, nP * L * nc)) && ok(corr_alloc(&m->part, nP * L * NDELTA)) &&
            ok(corr_alloc(&m->dl, nP * NDELTA));
        if (allocated && ok(corr_up(m->defs, defs.data(), defs.size() * sizeof(int))) && ok(corr_up(m->bph, bph.data(), nb * sizeof(int))) &&
            ok(corr_up(m->bpar, bpar.data(), bpar.size() * sizeof(double))))
            ok(corr_upload(m->cr, WORDS.prefix));      // the pairs; zeroes chain 0's block and binds req to it
        if (ok.rc == ELPH_OK && hipMemset(m->cr.acc, 0, std::max<size_t>(nch * m->cr.total, 1) * sizeof(double)) != hipSuccess) {
            elph_set_error("%s: hipMemset failed", WORDS.prefix);
            ok(ELPH_E_HIP);
        }
        if (ok.rc == ELPH_OK && ok(bc_allow_lds(k_bc_spatial_fwd, WORDS, nc))) ok(bc_allow_lds(k_ccc_correlate, WORDS, nc));
    }
    if (ok.rc != ELPH_OK) elph_ssh_bond_chains_free(h);
    return ok.rc;
}

extern "C" int elph_ssh_bond_chains_accumulate(elph_handle h, const double *X) {
    CHECK_H(h);
    RC(need_state(h));
    SshBondChainsState *m = sbc_of(h);
    if (has_current(m) && !X && m->Nph > 0) { elph_set_error("%s: X is null", WORDS.prefix); return ELPH_E_ARG; }
    const int nch = m->nchains;
    if (h->nchains != nch) {
        elph_set_error("%s: created for %d chains, %d are resident in this handle now", WORDS.prefix, nch, h->nchains);
        return ELPH_E_STATE;
    }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (g.nv % nch) {
        elph_set_error("%s: the estimator's %d vectors are not a multiple of the %d resident chains", WORDS.prefix, g.nv, nch);
        return ELPH_E_STATE;
    }
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    const int rc = accumulate_launches(h, m, g, X);
    const hipError_t e = hipStreamSynchronize(h->stream);      // on every path: X (a host pointer) is not retained after return
    if (rc == ELPH_OK && e != hipSuccess) { elph_set_error("%s: hipStreamSynchronize -> %s", WORDS.prefix, hipGetErrorString(e)); return ELPH_E_HIP; }
    return rc;
}

extern "C" int elph_ssh_bond_chains_fetch(elph_handle h, int chain, double *BondBond, double *CurrentCurrent, double *BondPairGreens) {
    CHECK_H(h);
    RC(need_state(h));
    const SshBondChainsState *m = sbc_of(h);
    if (chain < 0 || chain >= m->nchains) { elph_set_error("%s: chain %d outside 0..%d", WORDS.prefix, chain, m->nchains - 1); return ELPH_E_ARG; }
    std::vector<double> host;
    if (m->bond) {
        CorrPlan<NBOND> one = m->bond->cr;             // the chain's block, laid out as the plan says
        one.acc = m->bond->cr.acc + (size_t)chain * m->bond->cr.total;
        double *outs[NBOND] = {BondBond, BondPairGreens};
        RC(corr_fetch(h, one, host, outs));
    }
    if (has_current(m)) {
        CorrPlan<1> one = m->cr;
        one.acc = m->cr.acc + (size_t)chain * m->cr.total;
        double *outs[1] = {CurrentCurrent};
        RC(corr_fetch(h, one, host, outs));
    }
    return ELPH_OK;
}

extern "C" int elph_ssh_bond_chains_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_state(h));
    const SshBondChainsState *m = sbc_of(h);
    if (m->bond) HIPCHK(hipMemsetAsync(m->bond->cr.acc, 0, std::max<size_t>((size_t)m->nchains * m->bond->cr.total, 1) * sizeof(double), h->stream));
    if (has_current(m)) HIPCHK(hipMemsetAsync(m->cr.acc, 0, std::max<size_t>((size_t)m->nchains * m->cr.total, 1) * sizeof(double), h->stream));
    return ELPH_OK;
}
