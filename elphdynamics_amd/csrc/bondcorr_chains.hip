// bondcorr_chains.hip — the bond correlations of bondcorr.hip for EVERY chain resident in the handle at once (DESIGN.md "Bond
// correlations of resident chains"): the chain is the last grid axis of every kernel, so the launches of one accumulate depend on the
// vectors per chain and on the request, not on the number of chains.
//   measure_BondBond!         Measurements.jl:1663-1785
//   measure_BondPairGreens!   Measurements.jl:2390-2483
// per chain, for every pair of ITS vectors.  What a thread or workgroup computes is bondcorr.hip's (the bodies of bondcorr_dev.h), and so
// is the rule of the reductions: every output element is one thread's sum in index order, no atomics, no reduction split across
// workgroups.  A workgroup reads one chain's vectors and tables only, so chain c's numbers depend on nothing of another chain.  The
// correlations read the estimator's vectors and neither the field nor mu: accumulate takes no X.
//
// Layouts.  Vector v (0-based) of chain c is row v nchains + c of the estimator (greens.chain_vector), so the v-th vectors of all chains
// are one block [chain][ndim].  Every buffer carries the chain between the definition (or listed pair) and the time axis:
//   f  [NFIELD][ndef][chain][L][nc]      nu [NFIELD][ndef][chain][Lh][nc]      Y [pair][chain][Lh][nc]      B [pair][chain][L][nc]
// so the fields [k0, k1) stay one contiguous range, the forward tau-DFT is one elph_dft_fwd_plain of (k1 - k0) ndef nchains right-hand
// sides, the cell-axis DFT k_bc_spatial_fwd as it is over as many slices, and the inverse one elph_dft_inv_plain of nP nchains.  The
// accumulator is ONE allocation [chain][BondBond | BondPairGreens], a chain's block laid out as elph_bond_fetch's: reset is one memset,
// a chain's fetch one copy.  The estimator's pipeline for one pair of vectors of all chains runs in scratch this state owns
// (elph_i_greens_setup_chains_dev): the delta terms read the tau = 0 slice of table 0 (G[D,0]) of the chain's own pair of vectors,
// S.C + chain L n_s N in its [table][chain][L][n_s N].  LDS per workgroup is bondcorr.hip's (bc_lds_bytes).

#include "bondcorr_dev.h"

namespace {

const char *const BOND_NAMES[NBOND] = {"BondBond", "BondPairGreens"};
const CorrWords WORDS = {"chain bond correlations", "bond", "with no pair of bonds"};
constexpr long long GRID_YZ_MAX = 65535;

struct BondChainsState {
    BondState *b = nullptr;         // buffers and accumulators of all chains (b->nchains)
    ElphGreensChainScratch gs{};    // the estimator's pipeline for all chains
};

BondChainsState *bcs_of(elph_handle_s *h) { return (BondChainsState *)h->bond_chains; }

int need_state(elph_handle_s *h) { return corr_need(h->bond_chains, "elph_bond_chains_create"); }

}  // namespace

void elph_bond_chains_free(elph_handle_s *h) {
    BondChainsState *s = bcs_of(h);
    if (!s) return;
    bc_free(s->b);
    elph_i_greens_chain_scratch_free(&s->gs);
    delete s;
    h->bond_chains = nullptr;
}

extern "C" int elph_bond_chains_create(elph_handle h, int nchains, int n_def, const int *o1, const int *o2, const int *v, const int *measure,
                                       const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_bond_chains_free(h);
    RC(corr_refuse_model(h, WORDS.prefix));
    if (nchains < 1 || nchains != h->nchains) {
        elph_set_error("%s: created for %d chains, %d are resident in this handle", WORDS.prefix, nchains, h->nchains);
        return ELPH_E_ARG;
    }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    RC(bc_check(WORDS, g, n_def, o1, o2, v, measure, time_dependent, npairs));
    std::vector<int> defs;
    RC(bc_defs_table(defs, WORDS, g, n_def, o1, o2, v));
    CorrPlan<NBOND> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, WORDS, BOND_NAMES, measure, time_dependent, npairs, pairs, n_def, (int)h->L, g.nc, 0));
    // the chain multiplies the slices of the cell-axis DFT (grid y) and the right-hand sides of the tau-DFTs (grid z)
    const long long nk = (plan.req.np[BONDBOND] ? 4 : 0) + (plan.req.np[BONDPAIR] ? NFIELD - 4 : 0);
    if (nk * n_def * nchains > GRID_YZ_MAX) {
        elph_set_error("%s: %lld fields x %d bond definitions x %d chains = %lld slices exceed the grid's %lld", WORDS.prefix, nk, n_def, nchains,
                       nk * n_def * nchains, GRID_YZ_MAX);
        return ELPH_E_UNSUPPORTED;
    }
    if ((long long)plan.npairs * nchains > GRID_YZ_MAX) {
        elph_set_error("%s: %d listed pairs x %d chains = %lld transforms exceed the grid's %lld", WORDS.prefix, plan.npairs, nchains,
                       (long long)plan.npairs * nchains, GRID_YZ_MAX);
        return ELPH_E_UNSUPPORTED;
    }
    BondChainsState *s = new BondChainsState;
    h->bond_chains = s;
    CorrFirstError ok;
    if (ok(bc_make(&s->b, h, WORDS, g, plan, defs, n_def, nchains, k_bcc_correlate))) ok(elph_i_greens_chain_scratch_alloc(h, nchains, &s->gs));
    if (ok.rc != ELPH_OK) elph_bond_chains_free(h);
    return ok.rc;
}

extern "C" int elph_bond_chains_accumulate(elph_handle h) {
    CHECK_H(h);
    RC(need_state(h));
    BondChainsState *s = bcs_of(h);
    BondState *m = s->b;
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
    const int nvc = g.nv / nch;
    int rc = ELPH_OK;
    for (int i = 1; i < nvc && m->cr.npairs && rc == ELPH_OK; ++i)
        for (int j = i + 1; j <= nvc && rc == ELPH_OK; ++j) {      // pairs of a chain's vectors; every launch serves all chains
            ElphGreensPair v;                          // its setup leaves G[Δ,0] of every chain's pair of vectors for the δ terms
            rc = elph_i_greens_setup_chains_dev(h, s->gs, i, j, &v);
            if (rc == ELPH_OK) rc = bc_accumulate_pair_chains(h, m, g, s->gs, v);
        }
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (rc == ELPH_OK && e != hipSuccess) { elph_set_error("%s: hipStreamSynchronize -> %s", WORDS.prefix, hipGetErrorString(e)); return ELPH_E_HIP; }
    return rc;
}

extern "C" int elph_bond_chains_fetch(elph_handle h, int chain, double *BondBond, double *BondPairGreens) {
    CHECK_H(h);
    RC(need_state(h));
    const BondState *m = bcs_of(h)->b;
    if (chain < 0 || chain >= m->nchains) { elph_set_error("%s: chain %d outside 0..%d", WORDS.prefix, chain, m->nchains - 1); return ELPH_E_ARG; }
    CorrPlan<NBOND> one = m->cr;                       // the chain's block, laid out as the plan says
    one.acc = m->cr.acc + (size_t)chain * m->cr.total;
    std::vector<double> host;
    double *outs[NBOND] = {BondBond, BondPairGreens};
    return corr_fetch(h, one, host, outs);
}

extern "C" int elph_bond_chains_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_state(h));
    const BondState *m = bcs_of(h)->b;
    HIPCHK(hipMemsetAsync(m->cr.acc, 0, std::max<size_t>((size_t)m->nchains * m->cr.total, 1) * sizeof(double), h->stream));
    return ELPH_OK;
}
