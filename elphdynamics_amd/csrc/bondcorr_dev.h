// bondcorr_dev.h — what the bond-correlation units share (bondcorr.hip: Holstein, ssh_bondcorr.hip: bond phonons, currcorr.hip): the
// kernels of
//   measure_BondBond!         Measurements.jl:1663-1785
//   measure_BondPairGreens!   Measurements.jl:2390-2483
// which read model.bond_definitions and nothing else of the model, their state, and the host steps around them (the definitions'
// table, create, the launches of one pair of vectors).  The chain is the last grid axis of every kernel and nchains = 1 is the single
// configuration; the formulas and layouts are in bondcorr.hip's header.
#pragma once

#include <vector>

#include "cell_dft_dev.h"
#include "corr_req.h"
#include "elph_internal.h"

namespace {

constexpr int BC_TPB = CELL_DFT_TPB;
constexpr int NBOND = 2;
enum { BONDBOND = 0, BONDPAIR = 1 };
constexpr int NFIELD = 6;       // per definition; 0..3 serve BondBond, 4..5 BondPairGreens
constexpr int DEFW = 8;         // ints per definition: s, e (0-based orbitals), v mod L (3), v as given (3)

using BondReq = CorrReq<NBOND>;          // pairs (n″, n′)

struct BondState {
    int ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0;
    int nchains = 1;                // configurations the buffers serve: 1, or every resident chain
    int k0 = 0, k1 = 0;             // the fields [k0, k1) are transformed
    int *defs = nullptr;            // [ndef][DEFW]
    CorrPlan<NBOND> cr;             // ONE configuration's plan; cr.acc: [chain][BondBond | BondPairGreens], cr.req bound to chain 0
    double *f = nullptr;            // [NFIELD][ndef][chain][L][nc] the fields of one pair of vectors
    double2 *nu = nullptr;          // [NFIELD][ndef][chain][Lh][nc] their half spectra, then their cell-axis DFTs in place
    double2 *Y = nullptr;           // [nP][chain][Lh][nc] per-frequency correlations of the listed pairs, BondBond's first
    double *B = nullptr;            // [nP][chain][L][nc]
};

size_t bc_lds_bytes(int nc) { return 2 * (size_t)nc * sizeof(double2); }

// cell + (s1, s2, s3) on the periodic grid; 0 <= s_k < L_k
__device__ __forceinline__ int cell_plus(int cell, int s1, int s2, int s3, int L1, int L2, int L3) {
    const int l1 = cell % L1, l2 = (cell / L1) % L2, l3 = cell / (L1 * L2);
    return ((l1 + s1) % L1) + L1 * (((l2 + s2) % L2) + L2 * ((l3 + s3) % L3));
}

__device__ __forceinline__ int shifted_cell(int cell, const int *dv, int L1, int L2, int L3) {
    return cell_plus(cell, dv[2], dv[3], dv[4], L1, L2, L3);
}

// ---- what one thread or workgroup does in each kernel.  The buffers carry the chain between the definition (or listed pair) and the
// time axis — f: [NFIELD][ndef][chain][L][nc], nu the same with Lh, Y: [pair][chain][Lh][nc], B: [pair][chain][L][nc] — so a body takes
// its chain's block of definition (pair) 0 and the distance between two definitions (pairs); with one configuration that distance is
// the block itself.

// The six fields of every definition (header of bondcorr.hip) for idx = (cell, τ, definition), first fastest: gathers inside one time
// slice of layout S.  f: the chain's block of field 0 of definition 0; dstride: doubles between two definitions.
__device__ __forceinline__ void bc_fields_at(double *__restrict__ f, const double *__restrict__ X1, const double *__restrict__ X2,
                                             const double *__restrict__ R1, const double *__restrict__ R2, const int *__restrict__ defs, int N,
                                             int L, int ns, int L1, int L2, int L3, int ndef, long long idx, size_t dstride) {
    const int nc = L1 * L2 * L3;
    const long long per = (long long)L * nc;
    if (idx >= per * ndef) return;
    const int cell = (int)(idx % nc), t = (int)((idx / nc) % L), n = (int)(idx / per);
    const int *dv = defs + n * DEFW;
    const size_t is = (size_t)t * N + (size_t)cell * ns + dv[0];
    const size_t ie = (size_t)t * N + (size_t)shifted_cell(cell, dv, L1, L2, L3) * ns + dv[1];
    const double x1s = X1[is], x2s = X2[is], r2s = R2[is], x1e = X1[ie], r1e = R1[ie], r2e = R2[ie];
    const size_t fs = (size_t)ndef * dstride, o = (size_t)n * dstride + (size_t)t * nc + cell;
    f[o] = x1s * r1e;
    f[fs + o] = x2s * r2e;
    f[2 * fs + o] = x1s * r2e;
    f[3 * fs + o] = x2s * r1e;
    f[4 * fs + o] = x1e * x2s;
    f[5 * fs + o] = r1e * r2s;
}

// Frequency k of listed pair p (BondBond's pairs first): the product of the spectra (BondBond's two terms combined), inverse cell-axis
// DFT, into the slice y.  nu: the chain's spectra of field 0 of definition 0; field `kind` of definition n sits (kind * ndef + n) * dstride
// further on.  lds: 2 buffers of nc complex.
__device__ __forceinline__ void bc_correlate_slice(double2 *__restrict__ y, const double2 *__restrict__ nu, const BondReq &rq, int p, int k, int ndef,
                                                   int L1, int L2, int L3, const double2 *__restrict__ tw, double norm, size_t dstride, double2 *lds) {
    const int nc = L1 * L2 * L3;
    const int which = (p < rq.np[BONDBOND]) ? BONDBOND : BONDPAIR;
    if (which == BONDPAIR) p -= rq.np[BONDBOND];
    const int n2 = rq.pairs[which][2 * p], n1 = rq.pairs[which][2 * p + 1];       // n″, n′
    auto field = [&](int kind, int n) { return nu + ((size_t)kind * ndef + n) * dstride + (size_t)k * nc; };
    double2 *P = lds, *Q = lds + nc;
    if (which == BONDBOND) {
        const double2 *f0 = field(0, n1), *f1 = field(1, n2), *f2 = field(2, n1), *f3 = field(3, n2);
        for (int q = threadIdx.x; q < nc; q += BC_TPB) {
            const double2 a = f0[q], b = f1[q], c = f2[q], d = f3[q];             // a·conj(b), c·conj(d)
            P[q] = make_double2((4.0 * (a.x * b.x + a.y * b.y) - 2.0 * (c.x * d.x + c.y * d.y)) * norm,
                                (4.0 * (a.y * b.x - a.x * b.y) - 2.0 * (c.y * d.x - c.x * d.y)) * norm);
        }
    } else {
        const double2 *f4 = field(4, n1), *f5 = field(5, n2);
        for (int q = threadIdx.x; q < nc; q += BC_TPB) {
            const double2 a = f4[q], b = f5[q];
            P[q] = make_double2((a.x * b.x + a.y * b.y) * norm, (a.y * b.x - a.x * b.y) * norm);
        }
    }
    __syncthreads();
    const double2 *Pf = dft_cells<true>(P, Q, 1, L1, L2, L3, tw);
    for (int q = threadIdx.x; q < nc; q += BC_TPB) y[q] = Pf[q];
}

// Element idx = (τ, cell, listed pair) of correlation `which`: the δ terms and the τ = β slice (Measurements.jl:1750-1781, :2457-2479)
// added to the accumulator at idx + acc_off.  B: the chain's block of listed pair 0, pstride doubles between two pairs.  G0: the τ = 0
// slice of the estimator's G[Δ,0] of this pair of vectors, measure_GΔ0(l, o₁, o₂, 0) = G0[(o₂ - 1) + n_s ((o₁ - 1) + n_s cell(l))]
// (header of measure.hip).
__device__ __forceinline__ void bc_fold_at(const BondReq &rq, int which, long long idx, const double *__restrict__ B, const double *__restrict__ G0,
                                           const int *__restrict__ defs, int L, int ns, int L1, int L2, int L3, size_t pstride, size_t acc_off) {
    const int np = rq.np[which], L0 = rq.L0[which], nc = L1 * L2 * L3;
    if (idx >= (long long)L0 * nc * np) return;
    const int tau = (int)(idx % L0), cell = (int)((idx / L0) % nc), p = (int)(idx / ((long long)L0 * nc));
    const int *d2 = defs + rq.pairs[which][2 * p] * DEFW, *d1 = defs + rq.pairs[which][2 * p + 1] * DEFW;
    const int d = d2[0], c = d2[1], b = d1[0], a = d1[1];
    const int l1 = cell % L1, l2 = (cell / L1) % L2, l3 = cell / (L1 * L2);
    const bool beta = (tau == L);
    const double *Bp = B + ((size_t)(which == BONDPAIR ? rq.np[BONDBOND] : 0) + p) * pstride;
    double v;
    if (which == BONDBOND) {
        // B(β, r) = B(0, -r) with its δ term
        const int rc = beta ? ((L1 - l1) % L1) + L1 * (((L2 - l2) % L2) + L2 * ((L3 - l3) % L3)) : cell;
        v = Bp[(size_t)(beta ? 0 : tau) * nc + rc];
        if (a == d && (beta || tau == 0)) {
            // l = mod(-r′ - r″, L); the shifts are stored reduced, so 2 L - s′ - s″ is positive
            const int m1 = (2 * L1 - d1[2] - d2[2]) % L1, m2 = (2 * L2 - d1[3] - d2[3]) % L2, m3 = (2 * L3 - d1[4] - d2[4]) % L3;
            const int lc = m1 + L1 * (m2 + L2 * m3);
            if (rc == lc) v += 2.0 * G0[b + ns * (c + ns * lc)];                   // measure_GΔ0(l, c, b, 0)
        }
    } else {
        v = Bp[(size_t)(beta ? 0 : tau) * nc + cell];
        if (beta) {
            const bool d_ac = (a == c), d_bd = (b == d), d_r0 = (cell == 0);
            const bool d_rr = d1[5] == d2[5] && d1[6] == d2[6] && d1[7] == d2[7];                        // δ(r′, r″), as given
            // δ(r″, mod(r′ + l, L)): r″ as given against the reduced sum, as the reference writes it
            const bool d_rl = d2[5] == (d1[2] + l1) % L1 && d2[6] == (d1[3] + l2) % L2 && d2[7] == (d1[4] + l3) % L3;
            if (d_ac && d_rr && d_bd && d_r0) v += 1.0;
            if (d_bd && d_r0) {
                const int m1 = (d1[2] + l1 + L1 - d2[2]) % L1, m2 = (d1[3] + l2 + L2 - d2[3]) % L2, m3 = (d1[4] + l3 + L3 - d2[4]) % L3;
                v -= G0[a + ns * (c + ns * (m1 + L1 * (m2 + L2 * m3)))];           // measure_GΔ0(mod(r′ + l - r″), c, a, 0)
            }
            if (d_ac && d_rl) v -= G0[b + ns * (d + ns * cell)];                   // measure_GΔ0(l, d, b, 0)
        }
    }
    rq.acc[which][acc_off + idx] += v;
}

// ---- the kernels: the chain is the last grid axis; per: L nc, slice: Lh nc

// One workgroup per (frequency, slice of Lh frequencies): the cell-axis DFT of one frequency slice, in place; a slice is a field of a
// definition of a chain.  LDS: 2 buffers of nc complex.
__global__ void __launch_bounds__(BC_TPB) k_bc_spatial_fwd(double2 *__restrict__ nu, int Lh, int L1, int L2, int L3,
                                                           const double2 *__restrict__ tw) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3;
    double2 *s = nu + ((size_t)blockIdx.y * Lh + blockIdx.x) * nc;
    for (int q = threadIdx.x; q < nc; q += BC_TPB) lds[q] = s[q];
    __syncthreads();
    const double2 *F = dft_cells<false>(lds, lds + nc, 1, L1, L2, L3, tw);
    for (int q = threadIdx.x; q < nc; q += BC_TPB) s[q] = F[q];
}

// One thread per (cell, tau, definition) of chain blockIdx.y.  X1 .. R2: chain 0's vectors, chain c's c L N further on.
__global__ void __launch_bounds__(BC_TPB) k_bc_fields(double *__restrict__ f, ElphGreensPair v, const int *__restrict__ defs, int N, int L, int ns,
                                                      int L1, int L2, int L3, int ndef, int nchains) {
    const size_t ch = blockIdx.y, o = ch * L * N, per = (size_t)L * (L1 * L2 * L3);
    bc_fields_at(f + ch * per, v.X1 + o, v.X2 + o, v.R1 + o, v.R2 + o, defs, N, L, ns, L1, L2, L3, ndef, (long long)blockIdx.x * BC_TPB + threadIdx.x,
                 (size_t)nchains * per);
}

// One workgroup per (frequency, listed pair, chain).  LDS: 2 buffers of nc complex.
__global__ void __launch_bounds__(BC_TPB) k_bc_correlate(double2 *__restrict__ Y, const double2 *__restrict__ nu, BondReq rq, int Lh, int ndef, int L1,
                                                         int L2, int L3, const double2 *__restrict__ tw, double norm, int nchains) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3;
    const size_t ch = blockIdx.z, slice = (size_t)Lh * nc;
    bc_correlate_slice(Y + (((size_t)blockIdx.y * nchains + ch) * Lh + blockIdx.x) * nc, nu + ch * slice, rq, blockIdx.y, blockIdx.x, ndef, L1, L2, L3, tw,
                       norm, (size_t)nchains * slice, lds);
}

// One thread per (tau, cell, listed pair) of correlation blockIdx.y of chain blockIdx.z.  C0: table 0 of chain 0; block: doubles of a
// chain's accumulators.
__global__ void __launch_bounds__(BC_TPB) k_bc_fold(BondReq rq, const double *__restrict__ B, const double *__restrict__ C0,
                                                    const int *__restrict__ defs, int N, int L, int ns, int L1, int L2, int L3, int nchains,
                                                    size_t block) {
    const size_t ch = blockIdx.z, per = (size_t)L * (L1 * L2 * L3);
    bc_fold_at(rq, blockIdx.y, (long long)blockIdx.x * BC_TPB + threadIdx.x, B + ch * per, C0 + ch * L * ns * N, defs, L, ns, L1, L2, L3,
               (size_t)nchains * per, ch * block);
}

// ---- host

// model.bond_definitions (o₁, o₂ 1-based, v in unit cells) into the [n_def][DEFW] table the kernels read; w: the unit's words.
int bc_defs_table(std::vector<int> &defs, const CorrWords &w, const ElphGreensView &g, int n_def, const int *o1, const int *o2, const int *v) {
    const int dims[3] = {g.L1, g.L2, g.L3};
    defs.assign((size_t)n_def * DEFW, 0);
    for (int n = 0; n < n_def; ++n) {
        const int oo[2] = {o1[n], o2[n]};
        for (int k = 0; k < 2; ++k) {
            if (oo[k] < 1 || oo[k] > g.ns) {
                elph_set_error("%s: bond definition %d names orbital %d, outside 1..%d", w.prefix, n + 1, oo[k], g.ns);
                return ELPH_E_ARG;
            }
            defs[(size_t)n * DEFW + k] = oo[k] - 1;
        }
        for (int k = 0; k < 3; ++k) {
            const int r = v[3 * n + k];
            defs[(size_t)n * DEFW + 2 + k] = ((r % dims[k]) + dims[k]) % dims[k];
            defs[(size_t)n * DEFW + 5 + k] = r;
        }
    }
    return ELPH_OK;
}

// the argument and LDS checks every bond-correlation create starts with
int bc_check(const CorrWords &w, const ElphGreensView &g, int n_def, const int *o1, const int *o2, const int *v, const int *measure,
             const int *time_dependent, const int *npairs) {
    if (n_def < 1 || !o1 || !o2 || !v || !measure || !time_dependent || !npairs) {
        elph_set_error("%s: %d bond definitions, or a null array", w.prefix, n_def);
        return ELPH_E_ARG;
    }
    if (bc_lds_bytes(g.nc) > 160 * 1024) {
        elph_set_error("%s: a frequency slice of the %d x %d x %d lattice (%d cells) does not fit in 160 KB of LDS", w.prefix, g.L1, g.L2, g.L3,
                       g.nc);
        return ELPH_E_UNSUPPORTED;
    }
    return ELPH_OK;
}

// this unit's copy of a kernel that takes bc_lds_bytes of dynamic LDS
template <class K>
int bc_allow_lds(K kernel, const CorrWords &w, int nc) {
    const int lds = (int)bc_lds_bytes(nc);
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
        elph_set_error("%s: %d bytes of LDS were refused", w.prefix, lds);
        return ELPH_E_HIP;
    }
    return ELPH_OK;
}

void bc_free(BondState *m) {
    if (!m) return;
    corr_free({m->defs, m->cr.pairs, m->cr.acc, m->f, m->nu, m->Y, m->B});
    delete m;
}

// The chain multiplies the slices of the cell-axis DFT (grid y) and the right-hand sides of the tau-DFTs (grid z): nk fields per
// definition and nlist listed pairs must fit the grid.  Refuses only what would fail at launch.
int bc_check_grid(const CorrWords &w, long long nk, int n_def, long long nlist, int nchains) {
    constexpr long long GRID_YZ_MAX = 65535;
    if (nk * n_def * nchains > GRID_YZ_MAX) {
        elph_set_error("%s: %lld fields x %d bond definitions x %d chains = %lld slices exceed the grid's %lld", w.prefix, nk, n_def, nchains,
                       nk * n_def * nchains, GRID_YZ_MAX);
        return ELPH_E_UNSUPPORTED;
    }
    if (nlist * nchains > GRID_YZ_MAX) {
        elph_set_error("%s: %lld listed pairs x %d chains = %lld transforms exceed the grid's %lld", w.prefix, nlist, nchains, nlist * nchains,
                       GRID_YZ_MAX);
        return ELPH_E_UNSUPPORTED;
    }
    return ELPH_OK;
}

// the fields per definition a BondBond / BondPairGreens plan transforms
long long bc_fields_of(const CorrPlan<NBOND> &plan) { return (plan.req.np[BONDBOND] ? 4 : 0) + (plan.req.np[BONDPAIR] ? NFIELD - 4 : 0); }

// The state of a planned request for nchains configurations: allocations, the definitions and pairs on the device, zeroed accumulators,
// the LDS of this unit's k_bc_spatial_fwd and k_bc_correlate.  *out stays null on failure.
int bc_make(BondState **out, elph_handle_s *h, const CorrWords &w, const ElphGreensView &g, const CorrPlan<NBOND> &plan, const std::vector<int> &defs,
            int n_def, int nchains) {
    const int L = (int)h->L, Lh = L / 2 + 1, nc = g.nc;
    BondState *m = new BondState;
    m->cr = plan;
    m->ns = g.ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = n_def; m->nchains = nchains;
    m->k0 = plan.req.np[BONDBOND] ? 0 : 4;
    m->k1 = plan.req.np[BONDPAIR] ? NFIELD : 4;
    const size_t nch = (size_t)nchains, nP = nch * plan.npairs, nf = nch * NFIELD * n_def;
    CorrFirstError ok;
    const bool allocated = ok(corr_alloc(&m->defs, defs.size())) && ok(corr_alloc(m->cr, nch)) && ok(corr_alloc(&m->f, nf * L * nc)) &&
        ok(corr_alloc(&m->nu, nf * Lh * nc)) && ok(corr_alloc(&m->Y, nP * Lh * nc)) && ok(corr_alloc(&m->B, nP * L * nc));
    if (allocated && ok(corr_up(m->defs, defs.data(), defs.size() * sizeof(int)))) ok(corr_upload(m->cr, w.prefix, nch));
    if (ok.rc == ELPH_OK && ok(bc_allow_lds(k_bc_spatial_fwd, w, nc))) ok(bc_allow_lds(k_bc_correlate, w, nc));
    if (ok.rc != ELPH_OK) { bc_free(m); return ok.rc; }
    *out = m;
    return ELPH_OK;
}

// BondBond and BondPairGreens of one pair of vectors v of every chain (m->nchains), after its elph_i_greens_setup_chains_dev into S, into
// m's accumulators [chain][BondBond | BondPairGreens].
int bc_accumulate_pair(elph_handle_s *h, BondState *m, const ElphGreensView &g, const ElphGreensChainScratch &S, const ElphGreensPair &v) {
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = m->ns, nc = m->nc, ndef = m->ndef, nch = m->nchains;
    const int nP = m->cr.npairs, nk = m->k1 - m->k0;
    const size_t shm = bc_lds_bytes(nc);
    const long long nfld = (long long)L * nc * ndef;
    const double norm = 1.0 / ((double)L * (double)nc * (double)nc);   // 1/(L Nc)² in all: the other 1/L is in the inverse τ table
    hipLaunchKernelGGL(k_bc_fields, dim3((unsigned)((nfld + BC_TPB - 1) / BC_TPB), (unsigned)nch), dim3(BC_TPB), 0, h->stream, m->f, v, m->defs, N, L, ns,
                       m->L1, m->L2, m->L3, ndef, nch);
    RC(elph_launch_check("k_bc_fields"));
    double2 *nu = m->nu + (size_t)m->k0 * ndef * nch * Lh * nc;
    RC(elph_dft_fwd_plain(h, nu, m->f + (size_t)m->k0 * ndef * nch * L * nc, nc, nk * ndef * nch));
    hipLaunchKernelGGL(k_bc_spatial_fwd, dim3((unsigned)Lh, (unsigned)(nk * ndef * nch)), dim3(BC_TPB), shm, h->stream, nu, Lh, m->L1, m->L2, m->L3, g.tw);
    RC(elph_launch_check("k_bc_spatial_fwd"));
    hipLaunchKernelGGL(k_bc_correlate, dim3((unsigned)Lh, (unsigned)nP, (unsigned)nch), dim3(BC_TPB), shm, h->stream, m->Y, m->nu, m->cr.req, Lh, ndef,
                       m->L1, m->L2, m->L3, g.tw, norm, nch);
    RC(elph_launch_check("k_bc_correlate"));
    RC(elph_dft_inv_plain(h, m->B, m->Y, nc, nP * nch));
    hipLaunchKernelGGL(k_bc_fold, dim3((unsigned)((m->cr.fold_max + BC_TPB - 1) / BC_TPB), NBOND, (unsigned)nch), dim3(BC_TPB), 0, h->stream, m->cr.req,
                       m->B, S.C, m->defs, N, L, ns, m->L1, m->L2, m->L3, nch, m->cr.total);
    return elph_launch_check("k_bc_fold");
}

// a chain's [BondBond | BondPairGreens] to the host / the accumulators of all chains zeroed
int bc_fetch(elph_handle_s *h, const BondState *m, int chain, double *BondBond, double *BondPairGreens) {
    std::vector<double> host;
    double *outs[NBOND] = {BondBond, BondPairGreens};
    return corr_fetch(h, m->cr, host, outs, chain);
}

int bc_reset(elph_handle_s *h, const BondState *m) { return corr_reset(h, m->cr, (size_t)m->nchains); }

}  // namespace
