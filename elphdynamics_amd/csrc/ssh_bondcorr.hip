// ssh_bondcorr.hip — the inter-site correlations of the bond-phonon (SSH) model accumulated on the device, for one configuration or for
// EVERY chain resident in the handle at once (DESIGN.md "Measurements on the device"):
//   measure_BondBond!                Measurements.jl:1663-1785     the kernels of bondcorr_dev.h, shared with bondcorr.hip: the method
//   measure_BondPairGreens!          Measurements.jl:2390-2483     reads model.bond_definitions and nothing else of the model
//   measure_CurrentCurrent!(ssh)     Measurements.jl:2100-2384     this unit
//   translational_average!           Utilities.jl:49-60
// Notation of bondcorr.hip: f ⋆ g [Δτ, Δr] = 1/(L N_cells) Σ_{τ,i} f[τ + Δτ, i + Δr] g[τ, i], sh(f)[τ, i] = f[τ, i + v], x = M⁻¹r, a listed
// pair p = (n″, n′) with (d, c, r″) = (o₁, o₂, v) of n″ and (b, a, r′) = (o₁, o₂, v) of n′.  CurrentCurrent weights every factor by the
// modulated hopping of its bond definition, t′[τ, cell, n] = model.t′[τ, cell + N_cells n] (the reference's reshape of (Lτ, Nbonds) to
// (Lτ, L₁, L₂, L₃, n_def)), t′ = t − (α x + sign(x) α₂ x²) recomputed from the field, t′ = t on a bare bond.  Eight fields per definition
// (s = o₁, e = o₂) serve the eight translation averages:
//   A0 = t′·x₁[s]·sh(r₁[e])   A1 = t′·sh(x₁[e])·r₁[s]   A2 = t′·sh(x₂[e])·r₂[s]   A3 = t′·x₂[s]·sh(r₂[e])
//   A4 = t′·x₁[s]·sh(r₂[e])   A5 = t′·sh(x₂[e])·r₁[s]   A6 = t′·sh(r₁[e])·x₂[s]   A7 = t′·sh(x₁[e])·r₂[s]
//   J = 4 A0[n′]⋆A2[n″] − 4 A0[n′]⋆A3[n″] − 4 A1[n′]⋆A2[n″] − 4 A1[n′]⋆A3[n″]
//     − 2 A4[n′]⋆A5[n″] + 2 A6[n″]⋆A4[n′] + 2 A7[n′]⋆A5[n″] − 2 A7[n′]⋆A6[n″]
// combined in the spectrum: one inverse cell DFT and one inverse τ-transform per listed pair.  The code is mirrored as it executes, which
// differs from its comments in three places: the fourth term is subtracted (:2231, under a comment that says `J +=`); the sixth term
// averages the n″ field against the n′ field, in that order (:2256-2260); the b == c δ term reads M⁻¹r₁[:, b] where its comment names a
// (:2340).  Four δ terms at τ = 0, each a mean over all (τ, i) of a product of t′-weighted elements of vector 1, with u = t′[n′], w = t′[n″]:
//   a == c:  + 2 ⟨u x₁[b] · sh_l(w r₁[d])⟩                 at l = mod(r″ − r′, L)        (:2298-2313)
//   a == d:  − 2 ⟨u x₁[b] · sh_l(w sh_r″(r₁[c]))⟩          at l = mod(−r′, L)            (:2316-2331)
//   b == c:  − 2 ⟨u sh_r′(x₁[b]) · sh_l(w r₁[d])⟩          at l = r″ reduced mod L       (:2334-2349; unreduced the reference throws)
//   b == d:  + 2 ⟨u sh_r′(x₁[a]) · w sh_r″(r₁[c])⟩         at l = 0                      (:2352-2361)
// and the τ = β slice is the τ = 0 slice, δ terms included, mirrored in r (:2369-2379).
//
// The δ means have the one reduction order of measure.hip: a thread walks its cells in index order, the 64 lanes of a wave fold by
// halves, the waves are added in index order through LDS, one partial per time slice, the L partials added in slice order.  Everything
// else is one thread's sum in index order.  No floating-point atomics, no reduction split across workgroups: the same inputs give the
// same bits.  A workgroup reads one chain's vectors, field and tables only, so chain c's numbers depend on nothing of another chain.
//
// Layouts.  Vector v (0-based) of chain c is row v nchains + c of the estimator (greens.chain_vector), so the v-th vectors of all chains
// are one block [chain][ndim].  The fields arrive as X[chain][Nph][L] (the reference's layout per chain) and stay so on the device (xr):
// chain c's t′ reads xr + c Nph L.  Every buffer carries the chain between the definition (or listed pair) and the time axis:
//   f  [NCC][ndef][chain][L][nc]     nu [NCC][ndef][chain][Lh][nc]     Y [pair][chain][Lh][nc]     B [pair][chain][L][nc]
//   part [pair][chain][L][NDELTA]    dl [pair][chain][NDELTA]
// so the forward tau-DFT is one elph_dft_fwd_plain of NCC ndef nchains right-hand sides, the cell-axis DFT k_bc_spatial_fwd over as many
// slices, and the inverse one elph_dft_inv_plain of np nchains.  The CurrentCurrent accumulator is ONE allocation
// [chain][CurrentCurrent]; BondBond and BondPairGreens live in a BondState for nchains configurations (bondcorr_dev.h) with its own
// [chain][BondBond | BondPairGreens]: reset is one memset per allocation.  The δ terms of CurrentCurrent read vector 1 of the chain's
// own pair.  LDS per workgroup: bc_lds_bytes.
//
// ONE state, one kernel set and one host path serve both families of entry points; the chain is the last grid axis of every kernel and
// nchains = 1 is the single configuration.  elph_ssh_bond_* (the slot ssh_bond) keep a state for one chain, refuse a handle with several
// resident chains and run the estimator's pipeline in the estimator's own scratch, so that its tables and their doubled complex copies
// are left holding the last pair of vectors; elph_ssh_bond_chains_* (the slot ssh_bond_chains) measure every resident chain in scratch
// the state owns and leave the estimator's tables alone, even with one chain resident.  BondBond and BondPairGreens live in a BondState of
// bondcorr_dev.h (made when one of them is requested), CurrentCurrent in an accumulator and scratch of this unit's.  The bodies of the
// CurrentCurrent kernels are in currcorr_dev.h, shared under another hopping weight with currcorr.hip (the Holstein model's method,
// :1790-2098); the kernels here are thin wrappers over them with the weight CcModulated.

#include <vector>

#include "currcorr_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int NWAVE = MEAS_NWAVE;
const CorrWords WORDS = {"SSH bond correlations", "bond", "with no pair of bonds"};
const CorrWords WORDS_CHAINS = {"SSH chain bond correlations", "bond", "with no pair of bonds"};

struct SshBondState {
    int nchains = 1;
    BondState *bond = nullptr;      // BondBond, BondPairGreens of all chains (null: neither requested)
    ElphGreensChainScratch gs{};    // the estimator's pipeline for all chains (the _chains entry points; the others borrow the estimator's)
                                    // — those leave gs all null, so that freeing it frees nothing
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

SshBondState *sb_of(void *slot) { return (SshBondState *)slot; }
int need_ssh_bond(elph_handle_s *h) { return corr_need(h->ssh_bond, "elph_ssh_bond_create"); }
int need_chains(elph_handle_s *h) { return corr_need(h->ssh_bond_chains, "elph_ssh_bond_chains_create"); }
bool has_current(const SshBondState *m) { return m->cr.req.np[0] > 0; }

// ---- the CurrentCurrent kernels: the bodies of currcorr_dev.h under the modulated hopping, the chain the last grid axis; per: L nc,
// slice: Lh nc

// The eight fields of every definition (header), one thread per (cell, τ, definition) of chain blockIdx.y.  v: chain 0's vectors, chain c's
// c L N further on; xr: chain 0's field.
__global__ void __launch_bounds__(TPB) k_cc_fields(double *__restrict__ f, ElphGreensPair v, const int *__restrict__ defs,
                                                   const double *__restrict__ bpar, const int *__restrict__ bph, const double *__restrict__ xr,
                                                   int N, int Nph, int L, int ns, int L1, int L2, int L3, int ndef, int nchains) {
    const size_t ch = blockIdx.y, o = ch * L * N, per = (size_t)L * (L1 * L2 * L3);
    cc_fields_at(f + ch * per, v.X1 + o, v.X2 + o, v.R1 + o, v.R2 + o, defs, CcModulated{bpar, bph, xr + ch * Nph * L, ndef * (L1 * L2 * L3), L}, N,
                 L, ns, L1, L2, L3, ndef, (long long)blockIdx.x * TPB + threadIdx.x, (size_t)nchains * per);
}

// One workgroup per (frequency, listed pair, chain): the eight products of the spectra in the reference's order (term 6 with its
// operands swapped), inverse cell-axis DFT.  LDS: 2 buffers of nc complex.
__global__ void __launch_bounds__(TPB) k_cc_correlate(double2 *__restrict__ Y, const double2 *__restrict__ nu, CcReq rq, int Lh, int ndef, int L1,
                                                      int L2, int L3, const double2 *__restrict__ tw, double norm, int nchains) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3;
    const size_t ch = blockIdx.z, slice = (size_t)Lh * nc;
    cc_correlate_slice(Y + (((size_t)blockIdx.y * nchains + ch) * Lh + blockIdx.x) * nc, nu + ch * slice, rq, blockIdx.y, blockIdx.x, ndef, L1, L2, L3, tw,
                       norm, (size_t)nchains * slice, lds);
}

// One workgroup per (time slice, listed pair, chain): this slice's part of the four δ sums (header), zero where the orbitals differ.
// X1, R1: vector 1 of chain 0's pair.
__global__ void __launch_bounds__(TPB) k_cc_delta(double *__restrict__ part, CcReq rq, const double *__restrict__ X1, const double *__restrict__ R1,
                                                  const int *__restrict__ defs, const double *__restrict__ bpar, const int *__restrict__ bph,
                                                  const double *__restrict__ xr, int N, int Nph, int L, int ns, int L1, int L2, int L3, int ndef,
                                                  int nchains) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.z, o = ch * L * N;
    cc_delta_slice(part + ((size_t)blockIdx.y * nchains + ch) * L * NDELTA, rq, blockIdx.y, blockIdx.x, X1 + o, R1 + o, defs,
                   CcModulated{bpar, bph, xr + ch * Nph * L, ndef * (L1 * L2 * L3), L}, N, ns, L1, L2, L3, red);
}

// dl[p][chain][k] = ± 2 (the slices' partials in slice order) / (L nc), one thread per (δ term, chain, listed pair): dl and part are
// [pair][chain] blocks, np nchains of them.
__global__ void __launch_bounds__(TPB) k_cc_delta_finish(double *__restrict__ dl, const double *__restrict__ part, int np, int nchains, int L, int nc) {
    cc_delta_finish_at(dl, part, np * nchains, L, nc, blockIdx.x * TPB + threadIdx.x);
}

// One thread per (τ, cell, listed pair) of chain blockIdx.z: the δ terms at their τ = 0 cells, the τ = β slice J(β, r) = J(0, -r)
// (:2363-2380).  block: doubles of a chain's accumulator.
__global__ void __launch_bounds__(TPB) k_cc_fold(CcReq rq, const double *__restrict__ B, const double *__restrict__ dl, const int *__restrict__ defs,
                                                 int L, int L1, int L2, int L3, int nchains, size_t block) {
    const size_t ch = blockIdx.z, per = (size_t)L * (L1 * L2 * L3);
    cc_fold_at(rq, (long long)blockIdx.x * TPB + threadIdx.x, B + ch * per, dl + ch * NDELTA, defs, L, L1, L2, L3, (size_t)nchains * per,
               (size_t)nchains * NDELTA, ch * block);
}

// CurrentCurrent of one pair of vectors v of every chain into m's accumulator
int cc_accumulate_pair(elph_handle_s *h, SshBondState *m, const ElphGreensView &g, const ElphGreensPair &v) {
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = m->ns, nc = m->nc, ndef = m->ndef, np = m->cr.req.np[0], nch = m->nchains;
    const int Nph = (int)m->Nph;
    const size_t shm = bc_lds_bytes(nc);
    const long long nfld = (long long)L * nc * ndef;
    const double norm = 1.0 / ((double)L * (double)nc * (double)nc);   // 1/(L Nc)² in all: the other 1/L is in the inverse τ table
    hipLaunchKernelGGL(k_cc_fields, dim3((unsigned)((nfld + TPB - 1) / TPB), (unsigned)nch), dim3(TPB), 0, h->stream, m->f, v, m->defs, m->bpar, m->bph,
                       m->xr, N, Nph, L, ns, m->L1, m->L2, m->L3, ndef, nch);
    RC(elph_launch_check("k_cc_fields"));
    RC(elph_dft_fwd_plain(h, m->nu, m->f, nc, NCC * ndef * nch));
    hipLaunchKernelGGL(k_bc_spatial_fwd, dim3((unsigned)Lh, (unsigned)(NCC * ndef * nch)), dim3(TPB), shm, h->stream, m->nu, Lh, m->L1, m->L2, m->L3,
                       g.tw);
    RC(elph_launch_check("k_bc_spatial_fwd(CurrentCurrent)"));
    hipLaunchKernelGGL(k_cc_correlate, dim3((unsigned)Lh, (unsigned)np, (unsigned)nch), dim3(TPB), shm, h->stream, m->Y, m->nu, m->cr.req, Lh, ndef,
                       m->L1, m->L2, m->L3, g.tw, norm, nch);
    RC(elph_launch_check("k_cc_correlate"));
    RC(elph_dft_inv_plain(h, m->B, m->Y, nc, np * nch));
    hipLaunchKernelGGL(k_cc_delta, dim3((unsigned)L, (unsigned)np, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, m->cr.req, v.X1, v.R1, m->defs,
                       m->bpar, m->bph, m->xr, N, Nph, L, ns, m->L1, m->L2, m->L3, ndef, nch);
    RC(elph_launch_check("k_cc_delta"));
    hipLaunchKernelGGL(k_cc_delta_finish, dim3((unsigned)(((long long)np * nch * NDELTA + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->dl, m->part, np,
                       nch, L, nc);
    RC(elph_launch_check("k_cc_delta_finish"));
    hipLaunchKernelGGL(k_cc_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), 1, (unsigned)nch), dim3(TPB), 0, h->stream, m->cr.req, m->B, m->dl,
                       m->defs, L, m->L1, m->L2, m->L3, nch, m->cr.total);
    return elph_launch_check("k_cc_fold");
}

// Everything one accumulate queues on the handle's stream, the copy of the host's X first; the caller synchronises, whatever this returns.
// S: the scratch the estimator's pipeline runs in.
int sb_launches(elph_handle_s *h, SshBondState *m, const ElphGreensView &g, const ElphGreensChainScratch &S, const double *X) {
    const int nch = m->nchains, nvc = g.nv / nch;
    const bool current = has_current(m);
    if (!current && !m->bond) return ELPH_OK;
    if (current && m->Nph > 0)
        HIPCHK(hipMemcpyAsync(m->xr, X, (size_t)nch * h->L * m->Nph * sizeof(double), hipMemcpyHostToDevice, h->stream));
    for (int i = 1; i < nvc; ++i)
        for (int j = i + 1; j <= nvc; ++j) {           // pairs of a chain's vectors; every launch serves all chains
            ElphGreensPair v;                          // its setup leaves G[Δ,0] of every chain's pair of vectors for the δ terms of the BondState
            RC(elph_i_greens_setup_chains_dev(h, S, i, j, &v));
            if (m->bond) RC(bc_accumulate_pair(h, m->bond, g, S, v));
            if (current) RC(cc_accumulate_pair(h, m, g, v));
        }
    return ELPH_OK;
}

void sb_free(void *&slot) {
    SshBondState *m = sb_of(slot);
    if (!m) return;
    bc_free(m->bond);
    corr_free({m->cr.pairs, m->cr.acc, m->defs, m->bph, m->bpar, m->xr, m->f, m->nu, m->Y, m->B, m->part, m->dl});
    elph_i_greens_chain_scratch_free(&m->gs);
    delete m;
    slot = nullptr;
}

// The state of a request for nchains chains into the (freed) slot, after the entry point's refusals.  own_scratch: the state brings the
// scratch of the estimator's pipeline (the _chains entry points).
int sb_create(elph_handle_s *h, void *&slot, const CorrWords &W, int nchains, bool own_scratch, int n_def, const int *o1, const int *o2, const int *v,
              int64_t Nbonds, const double *t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph, const double *alpha,
              const double *alpha2, const int *measure, const int *time_dependent, const int *npairs, const int *pairs) {
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    RC(bc_check(W, g, n_def, o1, o2, v, measure, time_dependent, npairs));
    std::vector<int> defs;
    RC(bc_defs_table(defs, W, g, n_def, o1, o2, v));
    const int L = (int)h->L, Lh = L / 2 + 1, nc = g.nc;
    CorrPlan<NBOND> bplan;                             // request bookkeeping before anything is allocated
    CorrPlan<1> cplan;
    RC(cc_split_plans(bplan, cplan, W, measure, time_dependent, npairs, pairs, n_def, L, nc));
    const int np = cplan.req.np[0];
    const size_t nb = (size_t)n_def * nc;
    std::vector<int> bph;
    std::vector<double> bpar;
    if (np) RC(cc_check_params(h, W.prefix, n_def, nc, Nbonds, t, bond_to_definition, bond_to_phonon, Nph, alpha, alpha2, bph, bpar));
    RC(bc_check_grid(W, std::max<long long>(bc_fields_of(bplan), np ? NCC : 0), n_def, std::max(bplan.npairs, np), nchains));
    SshBondState *m = new SshBondState;
    slot = m;
    m->nchains = nchains; m->ns = g.ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = n_def; m->Nph = Nph;
    m->cr = cplan;
    const size_t nch = (size_t)nchains;
    CorrFirstError ok;
    if (bplan.npairs) ok(bc_make(&m->bond, h, W, g, bplan, defs, n_def, nchains));
    if (ok.rc == ELPH_OK && own_scratch && (bplan.npairs || np)) ok(elph_i_greens_chain_scratch_alloc(h, nchains, &m->gs));
    if (ok.rc == ELPH_OK && np) {
        const size_t nf = nch * NCC * n_def, nP = nch * np;
        const bool allocated = ok(corr_alloc(m->cr, nch)) && ok(corr_alloc(&m->defs, defs.size())) && ok(corr_alloc(&m->bph, nb)) &&
            ok(corr_alloc(&m->bpar, bpar.size())) && ok(corr_alloc(&m->xr, nch * L * Nph)) && ok(corr_alloc(&m->f, nf * L * nc)) &&
            ok(corr_alloc(&m->nu, nf * Lh * nc)) && ok(corr_alloc(&m->Y, nP * Lh * nc)) && ok(corr_alloc(&m->B, nP * L * nc)) &&
            ok(corr_alloc(&m->part, nP * L * NDELTA)) && ok(corr_alloc(&m->dl, nP * NDELTA));
        if (allocated && ok(corr_up(m->defs, defs.data(), defs.size() * sizeof(int))) && ok(corr_up(m->bph, bph.data(), nb * sizeof(int))) &&
            ok(corr_up(m->bpar, bpar.data(), bpar.size() * sizeof(double))))
            ok(corr_upload(m->cr, W.prefix, nch));
        if (ok.rc == ELPH_OK && ok(bc_allow_lds(k_bc_spatial_fwd, W, nc))) ok(bc_allow_lds(k_cc_correlate, W, nc));
    }
    if (ok.rc != ELPH_OK) sb_free(slot);
    return ok.rc;
}

// after the entry point's own checks: the estimator's vectors, the launches, one synchronisation
int sb_accumulate(elph_handle_s *h, SshBondState *m, const CorrWords &W, const ElphGreensChainScratch *S, const double *X) {
    ElphGreensView g;
    RC(corr_vectors(h, W.prefix, m->nchains, &g));
    return corr_synchronised(h, W.prefix, sb_launches(h, m, g, *S, X));
}

int sb_fetch(elph_handle_s *h, const SshBondState *m, int chain, double *BondBond, double *CurrentCurrent, double *BondPairGreens) {
    if (m->bond) RC(bc_fetch(h, m->bond, chain, BondBond, BondPairGreens));
    if (has_current(m)) {
        std::vector<double> host;
        double *outs[1] = {CurrentCurrent};
        RC(corr_fetch(h, m->cr, host, outs, chain));
    }
    return ELPH_OK;
}

int sb_reset(elph_handle_s *h, const SshBondState *m) {
    if (m->bond) RC(bc_reset(h, m->bond));
    if (has_current(m)) RC(corr_reset(h, m->cr, (size_t)m->nchains));
    return ELPH_OK;
}

}  // namespace

void elph_ssh_bond_free(elph_handle_s *h) { sb_free(h->ssh_bond); }
void elph_ssh_bond_chains_free(elph_handle_s *h) { sb_free(h->ssh_bond_chains); }

// ---- one configuration per handle: x[Nph][L]
extern "C" int elph_ssh_bond_create(elph_handle h, int n_def, const int *o1, const int *o2, const int *v, int64_t Nbonds, const double *t,
                                    const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph, const double *alpha,
                                    const double *alpha2, const int *measure, const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_ssh_bond_free(h);
    RC(corr_refuse_handle(h, WORDS.prefix, ELPH_MODEL_SSH));
    return sb_create(h, h->ssh_bond, WORDS, 1, false, n_def, o1, o2, v, Nbonds, t, bond_to_definition, bond_to_phonon, Nph, alpha, alpha2, measure,
                     time_dependent, npairs, pairs);
}

extern "C" int elph_ssh_bond_accumulate(elph_handle h, const double *x) {
    CHECK_H(h);
    RC(need_ssh_bond(h));
    RC(corr_refuse_chains(h, WORDS.prefix));
    SshBondState *m = sb_of(h->ssh_bond);
    if (has_current(m) && !x && m->Nph > 0) { elph_set_error("x is null"); return ELPH_E_ARG; }
    return sb_accumulate(h, m, WORDS, elph_i_greens_own_scratch(h), x);
}

extern "C" int elph_ssh_bond_fetch(elph_handle h, double *BondBond, double *CurrentCurrent, double *BondPairGreens) {
    CHECK_H(h);
    RC(need_ssh_bond(h));
    return sb_fetch(h, sb_of(h->ssh_bond), 0, BondBond, CurrentCurrent, BondPairGreens);
}

extern "C" int elph_ssh_bond_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_ssh_bond(h));
    return sb_reset(h, sb_of(h->ssh_bond));
}

// ---- every resident chain at once: X[nchains][Nph][L]
extern "C" int elph_ssh_bond_chains_create(elph_handle h, int nchains, int n_def, const int *o1, const int *o2, const int *v, int64_t Nbonds,
                                           const double *t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph,
                                           const double *alpha, const double *alpha2, const int *measure, const int *time_dependent,
                                           const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_ssh_bond_chains_free(h);
    RC(corr_refuse_model(h, WORDS_CHAINS.prefix, ELPH_MODEL_SSH));
    RC(corr_check_chain_count(h, WORDS_CHAINS.prefix, nchains));
    return sb_create(h, h->ssh_bond_chains, WORDS_CHAINS, nchains, true, n_def, o1, o2, v, Nbonds, t, bond_to_definition, bond_to_phonon, Nph, alpha,
                     alpha2, measure, time_dependent, npairs, pairs);
}

extern "C" int elph_ssh_bond_chains_accumulate(elph_handle h, const double *X) {
    CHECK_H(h);
    RC(need_chains(h));
    SshBondState *m = sb_of(h->ssh_bond_chains);
    if (has_current(m) && !X && m->Nph > 0) { elph_set_error("%s: X is null", WORDS_CHAINS.prefix); return ELPH_E_ARG; }
    RC(corr_same_chains(h, WORDS_CHAINS.prefix, m->nchains));
    return sb_accumulate(h, m, WORDS_CHAINS, &m->gs, X);
}

extern "C" int elph_ssh_bond_chains_fetch(elph_handle h, int chain, double *BondBond, double *CurrentCurrent, double *BondPairGreens) {
    CHECK_H(h);
    RC(need_chains(h));
    const SshBondState *m = sb_of(h->ssh_bond_chains);
    RC(corr_check_chain(WORDS_CHAINS.prefix, chain, m->nchains));
    return sb_fetch(h, m, chain, BondBond, CurrentCurrent, BondPairGreens);
}

extern "C" int elph_ssh_bond_chains_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_chains(h));
    return sb_reset(h, sb_of(h->ssh_bond_chains));
}
