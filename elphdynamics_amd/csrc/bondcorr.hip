// bondcorr.hip — the bond correlations of the Holstein model accumulated on the device, for one configuration or for EVERY chain resident
// in the handle at once (DESIGN.md "Measurements on the device"):
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
// same inputs give the same bits.  A workgroup reads one chain's vectors and tables only, so chain c's numbers depend on nothing of
// another chain.  The correlations read the estimator's vectors and neither the field nor mu: accumulate takes no X.
//
// Layouts.  Vector v (0-based) of chain c is row v nchains + c of the estimator (greens.chain_vector), so the v-th vectors of all chains
// are one block [chain][ndim].  Every buffer carries the chain between the definition (or listed pair) and the time axis:
//   f  [NFIELD][ndef][chain][L][nc]      nu [NFIELD][ndef][chain][Lh][nc]      Y [pair][chain][Lh][nc]      B [pair][chain][L][nc]
// so the fields [k0, k1) stay one contiguous range, the forward tau-DFT is one elph_dft_fwd_plain of (k1 - k0) ndef nchains right-hand
// sides, the cell-axis DFT k_bc_spatial_fwd over as many slices, and the inverse one elph_dft_inv_plain of nP nchains.  Accumulators:
// real doubles in ONE allocation [chain][BondBond | BondPairGreens], each correlation [L0][L1][L2][L3][n_p] first index fastest, L0 = L + 1
// (time-dependent, τ = β included) or 1 (equal-time): reset is one memset, a chain's fetch one copy.  The delta terms read the tau = 0
// slice of table 0 (G[D,0]) of the chain's own pair of vectors, S.C + chain L n_s N in the pipeline's [table][chain][L][n_s N].
//
// The kernels, their state and the launches of one pair of vectors are in bondcorr_dev.h, shared with ssh_bondcorr.hip (the same two
// correlations of the bond-phonon model); the chain is the last grid axis of every kernel and nchains = 1 is the single configuration.
// This unit holds the Holstein entry points: elph_bond_* (the slot bond) keep a state for one chain, refuse a handle with several
// resident chains and run the estimator's pipeline in the estimator's own scratch, so that its tables and their doubled complex copies
// are left holding the last pair of vectors; elph_bond_chains_* (the slot bond_chains) measure every resident chain in scratch the state
// owns and leave the estimator's tables alone, even with one chain resident.

#include "bondcorr_dev.h"

namespace {

const char *const BOND_NAMES[NBOND] = {"BondBond", "BondPairGreens"};
const CorrWords WORDS = {"bond correlations", "bond", "with no pair of bonds"};
const CorrWords WORDS_CHAINS = {"chain bond correlations", "bond", "with no pair of bonds"};

struct HolsteinBondState {
    BondState *b = nullptr;         // buffers and accumulators of all chains (b->nchains)
    ElphGreensChainScratch gs{};    // the estimator's pipeline for all chains (the _chains entry points; the others borrow the estimator's)
                                    // — those leave gs all null, so that freeing it frees nothing
};

HolsteinBondState *hb_of(void *slot) { return (HolsteinBondState *)slot; }
int need_bond(elph_handle_s *h) { return corr_need(h->bond, "elph_bond_create"); }
int need_chains(elph_handle_s *h) { return corr_need(h->bond_chains, "elph_bond_chains_create"); }

void hb_free(void *&slot) {
    HolsteinBondState *s = hb_of(slot);
    if (!s) return;
    bc_free(s->b);
    elph_i_greens_chain_scratch_free(&s->gs);
    delete s;
    slot = nullptr;
}

// The state of a request for nchains chains into the (freed) slot, after the entry point's refusals.  own_scratch: the state brings the
// scratch of the estimator's pipeline (the _chains entry points).
int hb_create(elph_handle_s *h, void *&slot, const CorrWords &W, int nchains, bool own_scratch, int n_def, const int *o1, const int *o2, const int *v,
              const int *measure, const int *time_dependent, const int *npairs, const int *pairs) {
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    RC(bc_check(W, g, n_def, o1, o2, v, measure, time_dependent, npairs));
    std::vector<int> defs;
    RC(bc_defs_table(defs, W, g, n_def, o1, o2, v));
    CorrPlan<NBOND> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, W, BOND_NAMES, measure, time_dependent, npairs, pairs, n_def, (int)h->L, g.nc, 0));
    RC(bc_check_grid(W, bc_fields_of(plan), n_def, plan.npairs, nchains));
    HolsteinBondState *s = new HolsteinBondState;
    slot = s;
    CorrFirstError ok;
    if (ok(bc_make(&s->b, h, W, g, plan, defs, n_def, nchains)) && own_scratch) ok(elph_i_greens_chain_scratch_alloc(h, nchains, &s->gs));
    if (ok.rc != ELPH_OK) hb_free(slot);
    return ok.rc;
}

// after the entry point's own checks: the estimator's vectors, the launches of every pair of a chain's vectors in the scratch S, one
// synchronisation
int hb_accumulate(elph_handle_s *h, BondState *m, const CorrWords &W, const ElphGreensChainScratch *S) {
    ElphGreensView g;
    RC(corr_vectors(h, W.prefix, m->nchains, &g));
    const int nvc = g.nv / m->nchains;
    int rc = ELPH_OK;
    for (int i = 1; i < nvc && m->cr.npairs && rc == ELPH_OK; ++i)
        for (int j = i + 1; j <= nvc && rc == ELPH_OK; ++j) {      // pairs of a chain's vectors; every launch serves all chains
            ElphGreensPair v;                          // its setup leaves G[Δ,0] of every chain's pair of vectors for the δ terms
            rc = elph_i_greens_setup_chains_dev(h, *S, i, j, &v);
            if (rc == ELPH_OK) rc = bc_accumulate_pair(h, m, g, *S, v);
        }
    return corr_synchronised(h, W.prefix, rc);
}

}  // namespace

void elph_bond_free(elph_handle_s *h) { hb_free(h->bond); }
void elph_bond_chains_free(elph_handle_s *h) { hb_free(h->bond_chains); }

// ---- one configuration per handle
extern "C" int elph_bond_create(elph_handle h, int n_def, const int *o1, const int *o2, const int *v, const int *measure,
                                const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_bond_free(h);
    RC(corr_refuse_handle(h, WORDS.prefix));
    return hb_create(h, h->bond, WORDS, 1, false, n_def, o1, o2, v, measure, time_dependent, npairs, pairs);
}

extern "C" int elph_bond_accumulate(elph_handle h) {
    CHECK_H(h);
    RC(need_bond(h));
    RC(corr_refuse_chains(h, WORDS.prefix));
    return hb_accumulate(h, hb_of(h->bond)->b, WORDS, elph_i_greens_own_scratch(h));
}

extern "C" int elph_bond_fetch(elph_handle h, double *BondBond, double *BondPairGreens) {
    CHECK_H(h);
    RC(need_bond(h));
    return bc_fetch(h, hb_of(h->bond)->b, 0, BondBond, BondPairGreens);
}

extern "C" int elph_bond_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_bond(h));
    return bc_reset(h, hb_of(h->bond)->b);
}

// ---- every resident chain at once
extern "C" int elph_bond_chains_create(elph_handle h, int nchains, int n_def, const int *o1, const int *o2, const int *v, const int *measure,
                                       const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_bond_chains_free(h);
    RC(corr_refuse_model(h, WORDS_CHAINS.prefix));
    RC(corr_check_chain_count(h, WORDS_CHAINS.prefix, nchains));
    return hb_create(h, h->bond_chains, WORDS_CHAINS, nchains, true, n_def, o1, o2, v, measure, time_dependent, npairs, pairs);
}

extern "C" int elph_bond_chains_accumulate(elph_handle h) {
    CHECK_H(h);
    RC(need_chains(h));
    HolsteinBondState *s = hb_of(h->bond_chains);
    RC(corr_same_chains(h, WORDS_CHAINS.prefix, s->b->nchains));
    return hb_accumulate(h, s->b, WORDS_CHAINS, &s->gs);
}

extern "C" int elph_bond_chains_fetch(elph_handle h, int chain, double *BondBond, double *BondPairGreens) {
    CHECK_H(h);
    RC(need_chains(h));
    const BondState *m = hb_of(h->bond_chains)->b;
    RC(corr_check_chain(WORDS_CHAINS.prefix, chain, m->nchains));
    return bc_fetch(h, m, chain, BondBond, BondPairGreens);
}

extern "C" int elph_bond_chains_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_chains(h));
    return bc_reset(h, hb_of(h->bond_chains)->b);
}
