// bondcorr.hip — the bond correlations of the Holstein model accumulated on the device (DESIGN.md "Measurements on the device"):
//   measure_BondBond!         Measurements.jl:1663-1785
//   measure_BondPairGreens!   Measurements.jl:2390-2483
//   translational_average!    Utilities.jl:49-60
// Unlike the on-site correlations (measure.hip) these are not folds of the estimator's four tables: each is a translation average
//   f ⋆ g [Δτ, Δr] = 1/(L N_cells) Σ_{τ,i} f[τ + Δτ, i + Δr] g[τ, i]          (periodic in L: no doubling of the time axis)
// of products of SHIFTED vectors, shift(f, r)[τ, i] = f[τ, i + r].  With a listed pair p = (n″, n′) of bond definitions,
// (d, c, r″) = (o₁, o₂, v) of n″ and (b, a, r′) = (o₁, o₂, v) of n′, and r, M⁻¹r the estimator's vectors (x = M⁻¹r below):
//   BondBond        B = 4 (x₁[b]·shift(r₁[a], r′)) ⋆ (x₂[d]·shift(r₂[c], r″)) − 2 (x₁[b]·shift(r₂[a], r′)) ⋆ (x₂[d]·shift(r₁[c], r″))
//   BondPairGreens  P = (shift(x₁[a], r′)·x₂[b]) ⋆ (shift(r₁[c], r″)·r₂[d])
// Every field depends on ONE definition (start orbital s = o₁, end orbital e = o₂, shift v), so a pair of vectors needs 6 n_def fields:
//   0: x₁[s]·shift(r₁[e])   1: x₂[s]·shift(r₂[e])   2: x₁[s]·shift(r₂[e])   3: x₂[s]·shift(r₁[e])   4: shift(x₁[e])·x₂[s]   5: shift(r₁[e])·r₂[s]
// with B = 4 F0[n′] ⋆ F1[n″] − 2 F2[n′] ⋆ F3[n″] (combined in the spectrum: one inverse transform) and P = F4[n′] ⋆ F5[n″].
// The fields are real: half spectra along τ (elph_dft_fwd_plain / elph_dft_inv_plain), the cell-axis DFTs of one frequency slice in
// LDS (cell_dft_dev.h, unit = 1), fft(g)[-ω,-k] = conj fft(g)[ω,k].
//
// No reduction is split across workgroups and there are no atomics: every output element is one thread's sum in index order, so the
// same inputs give the same bits.  Accumulators: real doubles in one allocation [BondBond | BondPairGreens], each
// [L0][L1][L2][L3][n_p] first index fastest, L0 = L + 1 (time-dependent, τ = β included) or 1 (equal-time).
//
// The kernels, their state and the launches of one pair of vectors are in bondcorr_dev.h, shared with ssh_bondcorr.hip (the same two
// correlations of the bond-phonon model) and bondcorr_chains.hip (every resident chain of a lockstep run at once); this unit holds the
// Holstein entry points of one configuration.

#include "bondcorr_dev.h"

namespace {

const char *const BOND_NAMES[NBOND] = {"BondBond", "BondPairGreens"};
const CorrWords WORDS = {"bond correlations", "bond", "with no pair of bonds"};

BondState *bs_of(elph_handle_s *h) { return (BondState *)h->bond; }

int need_bond(elph_handle_s *h) { return corr_need(h->bond, "elph_bond_create"); }

}  // namespace

void elph_bond_free(elph_handle_s *h) {
    bc_free(bs_of(h));
    h->bond = nullptr;
}

extern "C" int elph_bond_create(elph_handle h, int n_def, const int *o1, const int *o2, const int *v, const int *measure,
                                const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_bond_free(h);
    RC(corr_refuse_handle(h, WORDS.prefix));
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    RC(bc_check(WORDS, g, n_def, o1, o2, v, measure, time_dependent, npairs));
    std::vector<int> defs;
    RC(bc_defs_table(defs, WORDS, g, n_def, o1, o2, v));
    CorrPlan<NBOND> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, WORDS, BOND_NAMES, measure, time_dependent, npairs, pairs, n_def, (int)h->L, g.nc, 0));
    BondState *m = nullptr;
    const int rc = bc_make(&m, h, WORDS, g, plan, defs, n_def, 1, k_bc_correlate);
    h->bond = m;
    return rc;
}

extern "C" int elph_bond_accumulate(elph_handle h) {
    CHECK_H(h);
    RC(need_bond(h));
    RC(corr_refuse_chains(h, WORDS.prefix));
    BondState *m = bs_of(h);
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    for (int i = 1; i < g.nv && m->cr.npairs; ++i)
        for (int j = i + 1; j <= g.nv; ++j) {
            ElphGreensPair v;                          // its setup leaves G[Δ,0] of this pair of vectors for the δ terms
            RC(elph_i_greens_pair_dev(h, i, j, &v));
            RC(bc_accumulate_pair(h, m, g, v));
        }
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_bond_fetch(elph_handle h, double *BondBond, double *BondPairGreens) {
    CHECK_H(h);
    RC(need_bond(h));
    std::vector<double> host;
    double *outs[NBOND] = {BondBond, BondPairGreens};
    return corr_fetch(h, bs_of(h)->cr, host, outs);
}

extern "C" int elph_bond_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_bond(h));
    return corr_reset(h, bs_of(h)->cr);
}
