// corr_req.h — the request for a group of correlation functions, shared by measure.hip (on-site, N = 5), bondcorr.hip (bonds, N = 2),
// ssh_measure.hip (on-site and PhononGreens over phonon types, N = 5), ssh_bondcorr.hip (bonds, N = 2, and CurrentCurrent, N = 1) and
// currcorr.hip (N = 1): the record the kernels receive by value, the host's bookkeeping with its pure planner, and what every such group
// does with its one accumulator allocation [chain][lead doubles | the measured correlations]: bind, fetch, reset, free.  A correlation's
// accumulator is [L0][L1][L2][L3][n_p] doubles, first index fastest, L0 = L + 1 (time-dependent, tau = beta included) or 1 (equal-time).
// The plan is ONE chain's; a state for nchains chains holds nchains such blocks behind one another, and the kernels find a chain's block
// from the chain's grid index.  The state checks of the groups' two entry-point families are at the end.
#pragma once

#include <algorithm>
#include <vector>

#include "elph_internal.h"

template <int N>
struct CorrReq {                // by value into the kernels
    double *acc[N];
    const int *pairs[N];        // [np][2] 0-based
    int np[N], L0[N];           // np = 0: not measured
};

// the words in which the groups' messages differ
struct CorrWords {
    const char *prefix;         // "measurements" / "bond correlations" / "SSH measurements"
    const char *index;          // what a pair names: "orbital" / "bond"
    const char *no_pair;        // "with no orbital pair" / "with no pair of bonds"
    // one correlation of the group may count something else: its index in the request arrays (-1: none), what its pairs name
    // ("phonon type") and how a request without pairs reads
    int other = -1;
    const char *other_index = nullptr, *other_no_pair = nullptr;
};

template <int N>
struct CorrPlan {
    CorrReq<N> req{};           // np, L0 from corr_plan; acc, pairs from corr_upload
    std::vector<int> prs;       // every request's pairs, 0-based, concatenated
    size_t off[N] = {}, pair_off[N] = {};      // of a correlation in acc / of its pairs in prs
    size_t total = 0;           // doubles of acc: lead + the measured correlations
    size_t fold_max = 0;        // elements of the largest correlation
    int nc = 1, npairs = 0;     // cells; listed pairs of all requests
    int *pairs = nullptr;       // device: prs
    double *acc = nullptr;      // device: [chains][total] (at least one double)
    size_t count(int c) const { return (size_t)req.L0[c] * nc * req.np[c]; }
};

// measure / time_dependent / npairs / pairs (1-based, the requests' lists one after another) of a create call into P.  A pair's indices
// run over 1..limit (1..other_limit for the correlation w.other); `lead` doubles precede the first correlation.  Pure: no HIP call, so a
// bad request fails before anything is allocated.
template <int N>
int corr_plan(CorrPlan<N> &P, const CorrWords &w, const char *const *names, const int *measure, const int *time_dependent, const int *npairs,
              const int *pairs, int limit, int L, int nc, size_t lead, int other_limit = 0) {
    P = CorrPlan<N>();
    P.nc = nc;
    P.total = lead;
    size_t at = 0;
    for (int c = 0; c < N; ++c) {
        P.req.np[c] = 0; P.req.L0[c] = 1;
        if (!measure[c]) continue;
        const bool other = (c == w.other);
        const int lim = other ? other_limit : limit;
        if (npairs[c] < 1 || !pairs) { elph_set_error("%s: %s is requested %s", w.prefix, names[c], other ? w.other_no_pair : w.no_pair); return ELPH_E_ARG; }
        for (int p = 0; p < npairs[c]; ++p)
            for (int k = 0; k < 2; ++k) {
                const int o = pairs[2 * (at + p) + k];
                if (o < 1 || o > lim) {
                    elph_set_error("%s: %s pair %d names %s %d, outside 1..%d", w.prefix, names[c], p + 1, other ? w.other_index : w.index, o, lim);
                    return ELPH_E_ARG;
                }
                P.prs.push_back(o - 1);
            }
        P.pair_off[c] = 2 * at;
        at += (size_t)npairs[c];
        P.req.np[c] = npairs[c];
        P.req.L0[c] = time_dependent[c] ? L + 1 : 1;
        P.off[c] = P.total;
        P.total += P.count(c);
        P.fold_max = std::max(P.fold_max, P.count(c));
    }
    P.npairs = (int)at;
    return ELPH_OK;
}

template <class T>
int corr_alloc(T **p, size_t n) {
    HIPCHK(hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T)));
    return ELPH_OK;
}

inline int corr_up(void *dst, const void *src, size_t bytes) {
    if (bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return ELPH_OK;
}

// keeps the first error of a chain of calls; true while there is none
struct CorrFirstError {
    int rc = ELPH_OK;
    bool operator()(int r) { if (rc == ELPH_OK) rc = r; return rc == ELPH_OK; }
};

template <int N>
int corr_alloc(CorrPlan<N> &P, size_t chains = 1) {
    RC(corr_alloc(&P.pairs, P.prs.size()));
    return corr_alloc(&P.acc, chains * P.total);
}

// the pairs to the device, the accumulator of every chain zeroed, req bound to the pairs and to chain 0's block
template <int N>
int corr_upload(CorrPlan<N> &P, const char *prefix, size_t chains = 1) {
    RC(corr_up(P.pairs, P.prs.data(), P.prs.size() * sizeof(int)));
    if (hipMemset(P.acc, 0, std::max<size_t>(chains * P.total, 1) * sizeof(double)) != hipSuccess) { elph_set_error("%s: hipMemset failed", prefix); return ELPH_E_HIP; }
    for (int c = 0; c < N; ++c) {
        P.req.acc[c] = P.acc + P.off[c];
        P.req.pairs[c] = P.pairs + P.pair_off[c];
    }
    return ELPH_OK;
}

// one copy of a chain's block of the accumulator into host; every measured correlation with an output widened to interleaved complex
template <int N>
int corr_fetch(elph_handle_s *h, const CorrPlan<N> &P, std::vector<double> &host, double *const *outs, int chain = 0) {
    host.resize(std::max<size_t>(P.total, 1));
    HIPCHK(hipMemcpyAsync(host.data(), P.acc + (size_t)chain * P.total, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < N; ++c) {
        if (!outs[c] || !P.req.np[c]) continue;
        const double *src = host.data() + P.off[c];
        for (size_t i = 0, cnt = P.count(c); i < cnt; ++i) { outs[c][2 * i] = src[i]; outs[c][2 * i + 1] = 0.0; }
    }
    return ELPH_OK;
}

template <int N>
int corr_reset(elph_handle_s *h, const CorrPlan<N> &P, size_t chains = 1) {
    HIPCHK(hipMemsetAsync(P.acc, 0, std::max<size_t>(chains * P.total, 1) * sizeof(double), h->stream));
    return ELPH_OK;
}

inline void corr_free(std::initializer_list<void *> ptrs) {
    for (void *p : ptrs) if (p) (void)hipFree(p);
}

// What the creates of measure.hip check of their parameter arrays and bonds before anything is planned or allocated
// (prefix: the unit's word in the message); bs comes back as [2][nbonds] 0-based sites.
inline int corr_check_onsite_params(const elph_handle_s *h, const char *prefix, int nc, const double *omega, const double *omega4, const double *lambda,
                           const double *mu, double dtau, int64_t nbonds, int ndef, const int64_t *bond_sites, const double *bond_t,
                           const int *measure, const int *time_dependent, const int *npairs, std::vector<int> &bs) {
    if (!omega || !omega4 || !lambda || !mu || !measure || !time_dependent || !npairs) { elph_set_error("%s: a null parameter array", prefix); return ELPH_E_ARG; }
    if (!(dtau > 0.0)) { elph_set_error("%s: dtau = %g", prefix, dtau); return ELPH_E_ARG; }
    const int N = (int)h->N;
    if (ndef < 0 || nbonds != (int64_t)ndef * nc || (nbonds > 0 && (!bond_sites || !bond_t))) {
        elph_set_error("%s: %lld bonds are not %d bond definitions x %d cells (bond = (definition - 1) * ncells + cell)", prefix, (long long)nbonds,
                       ndef, nc);
        return ELPH_E_ARG;
    }
    bs.assign(2 * (size_t)nbonds, 0);
    for (int64_t b = 0; b < nbonds; ++b)
        for (int k = 0; k < 2; ++k) {
            const int64_t s = bond_sites[2 * b + k];
            if (s < 1 || s > N) { elph_set_error("%s: bond %lld joins site %lld, outside 1..%d", prefix, (long long)b + 1, (long long)s, N); return ELPH_E_ARG; }
            bs[(size_t)k * nbonds + b] = (int)(s - 1);
        }
    return ELPH_OK;
}

// What the creates of ssh_measure.hip check of their parameter arrays, bonds and phonons before anything is planned
// or allocated, and the bond tables they put on the device: bs [2][nbonds] 0-based sites, bph [nbonds] 0-based phonon (-1 on a bare bond),
// bpar [4][nbonds] t, omega, alpha, alpha2 (zeros on a bare bond), doff / dlist the bonds of every definition in bond order.  ndef comes
// back as 0 for a model without bonds.
struct CorrSshBonds {
    std::vector<int> bs, bph, doff, dlist;
    std::vector<double> bpar;
};

inline int corr_check_ssh_params(const elph_handle_s *h, const char *prefix, const double *mu, double dtau, int64_t nbonds, int &ndef,
                                 const int64_t *bond_sites, const double *bond_t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon,
                                 int64_t Nph, int nph, const double *omega, const double *alpha, const double *alpha2, const int *measure,
                                 const int *time_dependent, const int *npairs, CorrSshBonds &T) {
    if (!mu || !measure || !time_dependent || !npairs) { elph_set_error("%s: a null parameter array", prefix); return ELPH_E_ARG; }
    if (!(dtau > 0.0)) { elph_set_error("%s: dtau = %g", prefix, dtau); return ELPH_E_ARG; }
    const int N = (int)h->N, L = (int)h->L;
    if (ndef < 0 || nbonds < 0 || nbonds != h->nb || (nbonds > 0 && (ndef < 1 || nbonds < ndef || !bond_sites || !bond_t || !bond_to_definition || !bond_to_phonon))) {
        elph_set_error("%s: %lld bonds in %d bond definitions (the handle has %lld bonds), or a null bond array", prefix, (long long)nbonds, ndef,
                       (long long)h->nb);
        return ELPH_E_ARG;
    }
    if (nbonds == 0) ndef = 0;
    if (Nph < 0 || nph < 0 || Nph > 0x7fffffff / (int64_t)(L + 1) || (Nph > 0 && (!omega || !alpha || !alpha2))) {
        elph_set_error("%s: %lld phonons of %d types, or a null phonon array", prefix, (long long)Nph, nph);
        return ELPH_E_ARG;
    }
    T.bs.assign(2 * (size_t)nbonds, 0);
    T.bph.assign((size_t)nbonds, 0);
    T.doff.assign((size_t)ndef + 1, 0);
    T.dlist.assign((size_t)nbonds, 0);
    T.bpar.assign(4 * (size_t)nbonds, 0.0);
    for (int64_t b = 0; b < nbonds; ++b) {
        for (int k = 0; k < 2; ++k) {
            const int64_t s = bond_sites[2 * b + k];
            if (s < 1 || s > N) { elph_set_error("%s: bond %lld joins site %lld, outside 1..%d", prefix, (long long)b + 1, (long long)s, N); return ELPH_E_ARG; }
            T.bs[(size_t)k * nbonds + b] = (int)(s - 1);
        }
        const int64_t d = bond_to_definition[b], p = bond_to_phonon[b];
        if (d < 1 || d > ndef) { elph_set_error("%s: bond %lld belongs to definition %lld, outside 1..%d", prefix, (long long)b + 1, (long long)d, ndef); return ELPH_E_ARG; }
        if (p < 0 || p > Nph) { elph_set_error("%s: bond %lld carries phonon %lld, outside 0..%lld", prefix, (long long)b + 1, (long long)p, (long long)Nph); return ELPH_E_ARG; }
        ++T.doff[(size_t)d];
        T.bph[(size_t)b] = (int)p - 1;
        T.bpar[(size_t)b] = bond_t[b];
        if (p > 0) {
            T.bpar[(size_t)nbonds + b] = omega[p - 1];
            T.bpar[2 * (size_t)nbonds + b] = alpha[p - 1];
            T.bpar[3 * (size_t)nbonds + b] = alpha2[p - 1];
        }
    }
    for (int d = 0; d < ndef; ++d) T.doff[(size_t)d + 1] += T.doff[(size_t)d];
    std::vector<int> at(T.doff.begin(), T.doff.end() - 1);
    for (int64_t b = 0; b < nbonds; ++b) T.dlist[(size_t)at[(size_t)bond_to_definition[b] - 1]++] = (int)b;
    return ELPH_OK;
}

// PhononGreens over phonon types needs the field to reshape to (Ltau, L1, L2, L3, nph) and a frequency slice to fit in LDS
inline int corr_check_phonongreens(const char *prefix, int nph, int64_t Nph, int L1, int L2, int L3, size_t lds_bytes) {
    const int nc = L1 * L2 * L3;
    if (nph < 1 || Nph != (int64_t)nph * nc) {
        elph_set_error("%s: PhononGreens needs Nph = nph x ncells phonons; %lld phonons are not %d types x %d cells (the "
                       "reference's reshape of the field to (Ltau, L1, L2, L3, nph) fails)", prefix, (long long)Nph, nph, nc);
        return ELPH_E_UNSUPPORTED;
    }
    if (lds_bytes > 160 * 1024) {
        elph_set_error("%s: PhononGreens: a frequency slice of the %d x %d x %d lattice (%d cells) does not fit in 160 KB of LDS", prefix, L1, L2, L3, nc);
        return ELPH_E_UNSUPPORTED;
    }
    return ELPH_OK;
}

// ---- the state checks of the groups' entry points
inline int corr_need(const void *state, const char *create) {
    if (!state) { elph_set_error("%s has not been called", create); return ELPH_E_STATE; }
    return ELPH_OK;
}

inline int corr_refuse_chains(const elph_handle_s *h, const char *prefix) {
    if (h->nchains > 1) {
        elph_set_error("%s: %d chains are resident in this handle; one configuration per handle is measured", prefix, h->nchains);
        return ELPH_E_UNSUPPORTED;
    }
    return ELPH_OK;
}

// kind: the model the group measures
inline int corr_refuse_model(const elph_handle_s *h, const char *prefix, int kind = ELPH_MODEL_HOLSTEIN) {
    if (h->kind != kind) {
        if (kind == ELPH_MODEL_HOLSTEIN) elph_set_error("%s: the SSH model is not supported (Holstein only)", prefix);
        else elph_set_error("%s: the Holstein model is not supported (SSH only)", prefix);
        return ELPH_E_UNSUPPORTED;
    }
    if (h->shard || h->is_slab) { elph_set_error("%s: sharded and slab handles are not supported", prefix); return ELPH_E_UNSUPPORTED; }
    return ELPH_OK;
}

inline int corr_refuse_handle(const elph_handle_s *h, const char *prefix, int kind = ELPH_MODEL_HOLSTEIN) {
    RC(corr_refuse_model(h, prefix, kind));
    return corr_refuse_chains(h, prefix);
}

// ---- what the _chains entry points ask where the single-configuration ones refuse resident chains
inline int corr_check_chain_count(const elph_handle_s *h, const char *prefix, int nchains) {
    if (nchains < 1 || nchains != h->nchains) {
        elph_set_error("%s: created for %d chains, %d are resident in this handle", prefix, nchains, h->nchains);
        return ELPH_E_ARG;
    }
    return ELPH_OK;
}

inline int corr_same_chains(const elph_handle_s *h, const char *prefix, int nchains) {
    if (h->nchains != nchains) {
        elph_set_error("%s: created for %d chains, %d are resident in this handle now", prefix, nchains, h->nchains);
        return ELPH_E_STATE;
    }
    return ELPH_OK;
}

inline int corr_check_chain(const char *prefix, int chain, int nchains) {
    if (chain < 0 || chain >= nchains) { elph_set_error("%s: chain %d outside 0..%d", prefix, chain, nchains - 1); return ELPH_E_ARG; }
    return ELPH_OK;
}

// ---- the two ends of every accumulate
// the estimator as the accumulate of a state for nchains chains needs it: nv / nchains vectors per chain, set
inline int corr_vectors(elph_handle_s *h, const char *prefix, int nchains, ElphGreensView *g) {
    RC(elph_i_greens_view(h, g));
    if (g->nv % nchains) {
        elph_set_error("%s: the estimator's %d vectors are not a multiple of the %d resident chains", prefix, g->nv, nchains);
        return ELPH_E_STATE;
    }
    if (!g->have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    return ELPH_OK;
}

// rc of the launches, after a synchronisation on every path: a host pointer the launches copy from is not retained after return
inline int corr_synchronised(elph_handle_s *h, const char *prefix, int rc) {
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (rc == ELPH_OK && e != hipSuccess) { elph_set_error("%s: hipStreamSynchronize -> %s", prefix, hipGetErrorString(e)); return ELPH_E_HIP; }
    return rc;
}
