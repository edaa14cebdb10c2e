// ssh_bondcorr.hip — the inter-site correlations of the bond-phonon (SSH) model accumulated on the device (DESIGN.md "Measurements on
// the device"):
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
// else is one thread's sum in index order.  No floating-point atomics: the same inputs give the same bits.
//
// State: the handle's slot ssh_bond.  BondBond and BondPairGreens live in a BondState of bondcorr_dev.h (made when one of them is
// requested), CurrentCurrent in an accumulator and scratch of this unit's.  The bodies of the CurrentCurrent kernels are in
// currcorr_dev.h, shared with ssh_bondcorr_chains.hip (every resident chain at once) and, under another hopping weight, with currcorr.hip
// (the Holstein model's method, :1790-2098); the kernels here are thin wrappers over them with the weight CcModulated.

#include <vector>

#include "currcorr_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int NWAVE = MEAS_NWAVE;
const CorrWords WORDS = {"SSH bond correlations", "bond", "with no pair of bonds"};

struct SshBondState {
    BondState *bond = nullptr;      // BondBond, BondPairGreens (null: neither requested)
    // CurrentCurrent (allocated when it is requested)
    int ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0;
    int64_t Nph = 0;
    CorrPlan<1> cr;                 // the request; cr.acc: [CurrentCurrent]
    int *defs = nullptr;            // [ndef][DEFW]
    int *bph = nullptr;             // [ndef nc] 0-based phonon of bond cell + nc n, -1 on a bare bond
    double *bpar = nullptr;         // [NHPAR][ndef nc]
    double *xr = nullptr;           // [Nph][L] the field as the caller holds it
    double *f = nullptr;            // [NCC][ndef][L][nc] the fields of one pair of vectors
    double2 *nu = nullptr;          // [NCC][ndef][Lh][nc] their half spectra, then their cell-axis DFTs in place
    double2 *Y = nullptr;           // [np][Lh][nc] per-frequency correlations of the listed pairs
    double *B = nullptr;            // [np][L][nc]
    double *part = nullptr;         // [np][L][NDELTA] one partial per time slice
    double *dl = nullptr;           // [np][NDELTA] the δ terms of one pair of vectors, signed and normalised
};

SshBondState *sb_of(elph_handle_s *h) { return (SshBondState *)h->ssh_bond; }

// ---- the CurrentCurrent kernels of one configuration: the bodies of currcorr_dev.h with the stride between definitions (pairs) equal to
// the block

// The eight fields of every definition (header), one thread per (cell, τ, definition).
__global__ void __launch_bounds__(TPB) k_cc_fields(double *__restrict__ f, const double *__restrict__ X1, const double *__restrict__ X2,
                                                   const double *__restrict__ R1, const double *__restrict__ R2, const int *__restrict__ defs,
                                                   const double *__restrict__ bpar, const int *__restrict__ bph, const double *__restrict__ xr,
                                                   int N, int L, int ns, int L1, int L2, int L3, int ndef) {
    cc_fields_at(f, X1, X2, R1, R2, defs, CcModulated{bpar, bph, xr, ndef * (L1 * L2 * L3), L}, N, L, ns, L1, L2, L3, ndef,
                 (long long)blockIdx.x * TPB + threadIdx.x, (size_t)L * (L1 * L2 * L3));
}

// One workgroup per (frequency, listed pair): the eight products of the spectra in the reference's order (term 6 with its operands
// swapped), inverse cell-axis DFT.  nu as in k_bc_correlate.  LDS: 2 buffers of nc complex.
__global__ void __launch_bounds__(TPB) k_cc_correlate(double2 *__restrict__ Y, const double2 *__restrict__ nu, CcReq rq, int Lh, int ndef, int L1,
                                                      int L2, int L3, const double2 *__restrict__ tw, double norm) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3;
    cc_correlate_slice(Y + ((size_t)blockIdx.y * Lh + blockIdx.x) * nc, nu, rq, blockIdx.y, blockIdx.x, ndef, L1, L2, L3, tw, norm, (size_t)Lh * nc, lds);
}

// One workgroup per (time slice, listed pair): this slice's part of the four δ sums (header), zero where the orbitals differ.
__global__ void __launch_bounds__(TPB) k_cc_delta(double *__restrict__ part, CcReq rq, const double *__restrict__ X1, const double *__restrict__ R1,
                                                  const int *__restrict__ defs, const double *__restrict__ bpar, const int *__restrict__ bph,
                                                  const double *__restrict__ xr, int N, int L, int ns, int L1, int L2, int L3, int ndef) {
    __shared__ double red[NWAVE];
    cc_delta_slice(part + (size_t)blockIdx.y * L * NDELTA, rq, blockIdx.y, blockIdx.x, X1, R1, defs,
                   CcModulated{bpar, bph, xr, ndef * (L1 * L2 * L3), L}, N, ns, L1, L2, L3, red);
}

// dl[p][k] = ± 2 (the slices' partials in slice order) / (L nc), one thread per (listed pair, δ term)
__global__ void __launch_bounds__(TPB) k_cc_delta_finish(double *__restrict__ dl, const double *__restrict__ part, int np, int L, int nc) {
    cc_delta_finish_at(dl, part, np, L, nc, blockIdx.x * TPB + threadIdx.x);
}

// One thread per (τ, cell, listed pair): the δ terms at their τ = 0 cells, the τ = β slice J(β, r) = J(0, -r) (:2363-2380).
__global__ void __launch_bounds__(TPB) k_cc_fold(CcReq rq, const double *__restrict__ B, const double *__restrict__ dl, const int *__restrict__ defs,
                                                 int L, int L1, int L2, int L3) {
    cc_fold_at(rq, (long long)blockIdx.x * TPB + threadIdx.x, B, dl, defs, L, L1, L2, L3, (size_t)L * (L1 * L2 * L3), NDELTA, 0);
}

int need_ssh_bond(elph_handle_s *h) { return corr_need(h->ssh_bond, "elph_ssh_bond_create"); }

bool has_current(const SshBondState *m) { return m->cr.req.np[0] > 0; }

// CurrentCurrent of one pair of vectors v into m's accumulator
int cc_accumulate_pair(elph_handle_s *h, SshBondState *m, const ElphGreensView &g, const ElphGreensPair &v) {
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = m->ns, nc = m->nc, ndef = m->ndef, np = m->cr.req.np[0];
    const size_t shm = bc_lds_bytes(nc);
    const long long nfld = (long long)L * nc * ndef;
    const double norm = 1.0 / ((double)L * (double)nc * (double)nc);   // 1/(L Nc)² in all: the other 1/L is in the inverse τ table
    hipLaunchKernelGGL(k_cc_fields, dim3((unsigned)((nfld + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->f, v.X1, v.X2, v.R1, v.R2, m->defs, m->bpar,
                       m->bph, m->xr, N, L, ns, m->L1, m->L2, m->L3, ndef);
    RC(elph_launch_check("k_cc_fields"));
    RC(elph_dft_fwd_plain(h, m->nu, m->f, nc, NCC * ndef));
    hipLaunchKernelGGL(k_bc_spatial_fwd, dim3((unsigned)Lh, (unsigned)(NCC * ndef)), dim3(TPB), shm, h->stream, m->nu, Lh, m->L1, m->L2, m->L3, g.tw);
    RC(elph_launch_check("k_bc_spatial_fwd(CurrentCurrent)"));
    hipLaunchKernelGGL(k_cc_correlate, dim3((unsigned)Lh, (unsigned)np), dim3(TPB), shm, h->stream, m->Y, m->nu, m->cr.req, Lh, ndef, m->L1, m->L2,
                       m->L3, g.tw, norm);
    RC(elph_launch_check("k_cc_correlate"));
    RC(elph_dft_inv_plain(h, m->B, m->Y, nc, np));
    hipLaunchKernelGGL(k_cc_delta, dim3((unsigned)L, (unsigned)np), dim3(TPB), 0, h->stream, m->part, m->cr.req, v.X1, v.R1, m->defs, m->bpar, m->bph,
                       m->xr, N, L, ns, m->L1, m->L2, m->L3, ndef);
    RC(elph_launch_check("k_cc_delta"));
    hipLaunchKernelGGL(k_cc_delta_finish, dim3((unsigned)((np * NDELTA + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->dl, m->part, np, L, nc);
    RC(elph_launch_check("k_cc_delta_finish"));
    hipLaunchKernelGGL(k_cc_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->cr.req, m->B, m->dl, m->defs, L,
                       m->L1, m->L2, m->L3);
    return elph_launch_check("k_cc_fold");
}

}  // namespace

void elph_ssh_bond_free(elph_handle_s *h) {
    SshBondState *m = sb_of(h);
    if (!m) return;
    bc_free(m->bond);
    corr_free({m->cr.pairs, m->cr.acc, m->defs, m->bph, m->bpar, m->xr, m->f, m->nu, m->Y, m->B, m->part, m->dl});
    delete m;
    h->ssh_bond = nullptr;
}

extern "C" int elph_ssh_bond_create(elph_handle h, int n_def, const int *o1, const int *o2, const int *v, int64_t Nbonds, const double *t,
                                    const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph, const double *alpha,
                                    const double *alpha2, const int *measure, const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_ssh_bond_free(h);
    RC(corr_refuse_handle(h, WORDS.prefix, ELPH_MODEL_SSH));
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
    SshBondState *m = new SshBondState;
    h->ssh_bond = m;
    m->ns = g.ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = n_def; m->Nph = Nph;
    m->cr = cplan;
    CorrFirstError ok;
    if (bplan.npairs) ok(bc_make(&m->bond, h, WORDS, g, bplan, defs, n_def, 1, k_bc_correlate));
    if (ok.rc == ELPH_OK && np) {
        const size_t nf = (size_t)NCC * n_def;
        const bool allocated = ok(corr_alloc(m->cr)) && ok(corr_alloc(&m->defs, defs.size())) && ok(corr_alloc(&m->bph, nb)) &&
            ok(corr_alloc(&m->bpar, bpar.size())) && ok(corr_alloc(&m->xr, (size_t)L * Nph)) && ok(corr_alloc(&m->f, nf * L * nc)) &&
            ok(corr_alloc(&m->nu, nf * Lh * nc)) && ok(corr_alloc(&m->Y, (size_t)np * Lh * nc)) && ok(corr_alloc(&m->B, (size_t)np * L * nc)) &&
            ok(corr_alloc(&m->part, (size_t)np * L * NDELTA)) && ok(corr_alloc(&m->dl, (size_t)np * NDELTA));
        if (allocated && ok(corr_up(m->defs, defs.data(), defs.size() * sizeof(int))) && ok(corr_up(m->bph, bph.data(), nb * sizeof(int))) &&
            ok(corr_up(m->bpar, bpar.data(), bpar.size() * sizeof(double))))
            ok(corr_upload(m->cr, WORDS.prefix));
        if (ok.rc == ELPH_OK && ok(bc_allow_lds(k_bc_spatial_fwd, WORDS, nc))) ok(bc_allow_lds(k_cc_correlate, WORDS, nc));
    }
    if (ok.rc != ELPH_OK) elph_ssh_bond_free(h);
    return ok.rc;
}

extern "C" int elph_ssh_bond_accumulate(elph_handle h, const double *x) {
    CHECK_H(h);
    RC(need_ssh_bond(h));
    RC(corr_refuse_chains(h, WORDS.prefix));
    SshBondState *m = sb_of(h);
    const bool current = has_current(m);
    if (current && !x && m->Nph > 0) { elph_set_error("x is null"); return ELPH_E_ARG; }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    if (!current && !m->bond) return ELPH_OK;
    if (current && m->Nph > 0) HIPCHK(hipMemcpyAsync(m->xr, x, (size_t)h->L * m->Nph * sizeof(double), hipMemcpyHostToDevice, h->stream));
    for (int i = 1; i < g.nv; ++i)
        for (int j = i + 1; j <= g.nv; ++j) {
            ElphGreensPair v;                          // its setup leaves G[Δ,0] of this pair of vectors for the δ terms of the BondState
            RC(elph_i_greens_pair_dev(h, i, j, &v));
            if (m->bond) RC(bc_accumulate_pair(h, m->bond, g, v));
            if (current) RC(cc_accumulate_pair(h, m, g, v));
        }
    HIPCHK(hipStreamSynchronize(h->stream));           // x (a host pointer) is not retained after return
    return ELPH_OK;
}

extern "C" int elph_ssh_bond_fetch(elph_handle h, double *BondBond, double *CurrentCurrent, double *BondPairGreens) {
    CHECK_H(h);
    RC(need_ssh_bond(h));
    SshBondState *m = sb_of(h);
    std::vector<double> host;
    if (m->bond) {
        double *outs[NBOND] = {BondBond, BondPairGreens};
        RC(corr_fetch(h, m->bond->cr, host, outs));
    }
    if (has_current(m)) {
        double *outs[1] = {CurrentCurrent};
        RC(corr_fetch(h, m->cr, host, outs));
    }
    return ELPH_OK;
}

extern "C" int elph_ssh_bond_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_ssh_bond(h));
    SshBondState *m = sb_of(h);
    if (m->bond) RC(corr_reset(h, m->bond->cr));
    if (has_current(m)) RC(corr_reset(h, m->cr));
    return ELPH_OK;
}
