// currcorr_dev.h — what the two CurrentCurrent units share (ssh_bondcorr.hip: the SSH model; currcorr.hip: the Holstein model; each for
// one configuration or every resident chain): the bodies of the kernels of
//   measure_CurrentCurrent!(ssh)        Measurements.jl:2100-2384
//   measure_CurrentCurrent!(holstein)   Measurements.jl:1790-2098
// and the checks of the bond and phonon parameters the create calls make.  One text of each kernel body; the formulas, the eight fields
// A0 .. A7 and the four δ terms are in ssh_bondcorr.hip's header.  The two methods differ in the hopping that weights every factor and
// in nothing else, so the bodies that weight take the weight of (bond, slice) as a policy W, `double W::operator()(int bond, int t)`:
// CcModulated for the SSH model, CcLastSlice for the Holstein model.
// One difference between the units is deliberate and lies outside the bodies: cc_fold_at adds into whatever block rq.acc names.  The SSH
// unit binds it to the accumulator itself; currcorr.hip binds it to a second block that it zeroes per accumulate and adds to the
// accumulator once (k_cur_add), because its contract promises that the same accumulate twice is EXACTLY twice the first, where the SSH
// unit promises that up to rounding (its tests hold 4 eps).  Do not align one with the other without changing that contract and its
// tests.
// As in bondcorr_dev.h the buffers carry the chain between the definition (or listed pair) and the time axis — f: [NCC][ndef][chain][L][nc],
// nu the same with Lh, Y: [pair][chain][Lh][nc], B: [pair][chain][L][nc], part: [pair][chain][L][NDELTA], dl: [pair][chain][NDELTA] — so a
// body takes its chain's block of definition (pair) 0 and the distance between two definitions (pairs); with one configuration that
// distance is the block itself.
#pragma once

#include <vector>

#include "bondcorr_dev.h"
#include "meas_dev.h"

namespace {

static_assert(MEAS_TPB == BC_TPB, "dft_cells walks the workgroup of cc_correlate_slice");
constexpr int NCC = 8;                // fields per definition (header of ssh_bondcorr.hip)
constexpr int NDELTA = 4;             // δ terms: a == c, a == d, b == c, b == d
constexpr int NHPAR = 3;              // per bond: t, alpha, alpha2 (zeros on a bare bond)

using CcReq = CorrReq<1>;

// The SSH model's weight: t′ of bond `bond` = cell + nc n on slice t, the modulated hopping recomputed from the field.  bpar [NHPAR][nb],
// bph [nb], xr [Nph][L]: the tables of cc_check_params and the (chain's) field.
struct CcModulated {
    const double *__restrict__ bpar;
    const int *__restrict__ bph;
    const double *__restrict__ xr;
    int nb, L;
    __device__ __forceinline__ double operator()(int bond, int t) const {
        const int ph = bph[bond];
        const double t0 = bpar[bond];
        return ph < 0 ? t0 : t_modulated(t0, bpar[nb + bond], bpar[2 * nb + bond], xr[(size_t)ph * L + t]);
    }
};

// The Holstein model's weight, as the reference executes it: the static model.t of bond `bond` = cell + nc n on the LAST time slice and
// 1 on every other one (Measurements.jl:1868-1871 and its twins: `for τ in Lₜ` visits Lₜ alone).  t0 [nb].
struct CcLastSlice {
    const double *__restrict__ t0;
    int L;
    __device__ __forceinline__ double operator()(int bond, int t) const { return t == L - 1 ? t0[bond] : 1.0; }
};

// The displacements l of the four δ terms (header) from the reduced shifts of n′ (d1) and n″ (d2).
__device__ __forceinline__ void cc_delta_shifts(int l[NDELTA][3], const int *d1, const int *d2, int L1, int L2, int L3) {
    const int dims[3] = {L1, L2, L3};
    for (int k = 0; k < 3; ++k) {
        l[0][k] = (d2[2 + k] + dims[k] - d1[2 + k]) % dims[k];
        l[1][k] = (dims[k] - d1[2 + k]) % dims[k];
        l[2][k] = d2[2 + k];
        l[3][k] = 0;
    }
}

// The eight fields of every definition for idx = (cell, τ, definition), first fastest.  f: the chain's block of field 0 of definition 0;
// dstride: doubles between two definitions; X1 .. R2: the chain's vectors; w: the (chain's) weight.
template <class W>
__device__ __forceinline__ void cc_fields_at(double *__restrict__ f, const double *__restrict__ X1, const double *__restrict__ X2,
                                             const double *__restrict__ R1, const double *__restrict__ R2, const int *__restrict__ defs,
                                             const W &w, int N, int L, int ns, int L1, int L2, int L3, int ndef, long long idx,
                                             size_t dstride) {
    const int nc = L1 * L2 * L3;
    const long long per = (long long)L * nc;
    if (idx >= per * ndef) return;
    const int cell = (int)(idx % nc), t = (int)((idx / nc) % L), n = (int)(idx / per);
    const int *dv = defs + n * DEFW;
    const size_t is = (size_t)t * N + (size_t)cell * ns + dv[0];
    const size_t ie = (size_t)t * N + (size_t)shifted_cell(cell, dv, L1, L2, L3) * ns + dv[1];
    const double x1s = X1[is], x2s = X2[is], r1s = R1[is], r2s = R2[is], x1e = X1[ie], x2e = X2[ie], r1e = R1[ie], r2e = R2[ie];
    const double tp = w(n * nc + cell, t);
    const size_t fs = (size_t)ndef * dstride, o = (size_t)n * dstride + (size_t)t * nc + cell;
    f[o] = (x1s * r1e) * tp;
    f[fs + o] = (x1e * r1s) * tp;
    f[2 * fs + o] = (x2e * r2s) * tp;
    f[3 * fs + o] = (x2s * r2e) * tp;
    f[4 * fs + o] = (x1s * r2e) * tp;
    f[5 * fs + o] = (x2e * r1s) * tp;
    f[6 * fs + o] = (r1e * x2s) * tp;
    f[7 * fs + o] = (x1e * r2s) * tp;
}

// Frequency k of listed pair p: the eight products of the spectra in the reference's order (term 6 with its operands swapped), inverse
// cell-axis DFT, into the slice y.  nu: the chain's spectra of field 0 of definition 0; field `kind` of definition n sits
// (kind * ndef + n) * dstride further on.  lds: 2 buffers of nc complex.
__device__ __forceinline__ void cc_correlate_slice(double2 *__restrict__ y, const double2 *__restrict__ nu, const CcReq &rq, int p, int k, int ndef,
                                                   int L1, int L2, int L3, const double2 *__restrict__ tw, double norm, size_t dstride, double2 *lds) {
    const int nc = L1 * L2 * L3;
    const int n2 = rq.pairs[0][2 * p], n1 = rq.pairs[0][2 * p + 1];               // n″, n′
    auto field = [&](int kind, int n) { return nu + ((size_t)kind * ndef + n) * dstride + (size_t)k * nc; };
    const double2 *A0 = field(0, n1), *A1 = field(1, n1), *A4 = field(4, n1), *A7 = field(7, n1);
    const double2 *B2 = field(2, n2), *B3 = field(3, n2), *B5 = field(5, n2), *B6 = field(6, n2);
    double2 *P = lds, *Q = lds + nc;
    for (int q = threadIdx.x; q < nc; q += BC_TPB) {
        const double2 a0 = A0[q], a1 = A1[q], a4 = A4[q], a7 = A7[q], b2 = B2[q], b3 = B3[q], b5 = B5[q], b6 = B6[q];
        double re = 0.0, im = 0.0;
        auto add = [&](double w, const double2 &u, const double2 &v) {           // w · u·conj(v)
            re += w * (u.x * v.x + u.y * v.y);
            im += w * (u.y * v.x - u.x * v.y);
        };
        add(4.0, a0, b2);
        add(-4.0, a0, b3);
        add(-4.0, a1, b2);
        add(-4.0, a1, b3);
        add(-2.0, a4, b5);
        add(2.0, b6, a4);
        add(2.0, a7, b5);
        add(-2.0, a7, b6);
        P[q] = make_double2(re * norm, im * norm);
    }
    __syncthreads();
    const double2 *Pf = dft_cells<true>(P, Q, 1, L1, L2, L3, tw);
    for (int q = threadIdx.x; q < nc; q += BC_TPB) y[q] = Pf[q];
}

// Time slice t of listed pair p: this slice's part of the four δ sums (header), zero where the orbitals differ, into part[t][NDELTA].
// part: the [L][NDELTA] block of this pair (of this chain); X1, R1: the chain's vector 1; w: the (chain's) weight.  red: MEAS_NWAVE
// doubles of LDS.
template <class W>
__device__ __forceinline__ void cc_delta_slice(double *__restrict__ part, const CcReq &rq, int p, int t, const double *__restrict__ X1,
                                               const double *__restrict__ R1, const int *__restrict__ defs, const W &w, int N, int ns, int L1,
                                               int L2, int L3, double *red) {
    const int nc = L1 * L2 * L3;
    const int n2 = rq.pairs[0][2 * p], n1 = rq.pairs[0][2 * p + 1];
    const int *d2 = defs + n2 * DEFW, *d1 = defs + n1 * DEFW;
    const int d = d2[0], c = d2[1], b = d1[0], a = d1[1];
    const bool on[NDELTA] = {a == c, a == d, b == c, b == d};
    int l[NDELTA][3];
    cc_delta_shifts(l, d1, d2, L1, L2, L3);
    const double *x1 = X1 + (size_t)t * N, *r1 = R1 + (size_t)t * N;
    double s[NDELTA] = {0.0, 0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < nc; j += MEAS_TPB) {
        const double u = w(n1 * nc + j, t);
        const int jp = shifted_cell(j, d1, L1, L2, L3);                           // j + r′
        if (on[0]) {
            const int jl = cell_plus(j, l[0][0], l[0][1], l[0][2], L1, L2, L3);
            s[0] += (x1[j * ns + b] * u) * (r1[jl * ns + d] * w(n2 * nc + jl, t));
        }
        if (on[1]) {
            const int jl = cell_plus(j, l[1][0], l[1][1], l[1][2], L1, L2, L3);
            s[1] += (x1[j * ns + b] * u) * (r1[shifted_cell(jl, d2, L1, L2, L3) * ns + c] * w(n2 * nc + jl, t));
        }
        if (on[2]) {
            const int jl = cell_plus(j, l[2][0], l[2][1], l[2][2], L1, L2, L3);
            s[2] += (x1[jp * ns + b] * u) * (r1[jl * ns + d] * w(n2 * nc + jl, t));
        }
        if (on[3])
            s[3] += (x1[jp * ns + a] * u) * (r1[shifted_cell(j, d2, L1, L2, L3) * ns + c] * w(n2 * nc + j, t));
    }
    for (int k = 0; k < NDELTA; ++k) {
        const double tot = block_sum(s[k], red);
        if (threadIdx.x == 0) part[(size_t)t * NDELTA + k] = tot;
    }
}

// dl[q] = ± 2 (the slices' partials in slice order) / (L nc) for q = (δ term, block), first fastest; a block is a listed pair (of a
// chain): dl [nblocks][NDELTA], part [nblocks][L][NDELTA].
__device__ __forceinline__ void cc_delta_finish_at(double *__restrict__ dl, const double *__restrict__ part, int nblocks, int L, int nc, int q) {
    if (q >= nblocks * NDELTA) return;
    const int p = q / NDELTA, k = q % NDELTA;
    double s = 0.0;
    for (int t = 0; t < L; ++t) s += part[((size_t)p * L + t) * NDELTA + k];
    const double v = 2 * s / ((double)L * (double)nc);
    dl[q] = (k == 1 || k == 2) ? -v : v;
}

// Element idx = (τ, cell, listed pair): the δ terms at their τ = 0 cells, the τ = β slice J(β, r) = J(0, -r) (:2363-2380), added to the
// accumulator at idx + acc_off.  B, dl: the chain's blocks of listed pair 0, pstride / dlstride doubles between two pairs.
__device__ __forceinline__ void cc_fold_at(const CcReq &rq, long long idx, const double *__restrict__ B, const double *__restrict__ dl,
                                           const int *__restrict__ defs, int L, int L1, int L2, int L3, size_t pstride, size_t dlstride,
                                           size_t acc_off) {
    const int np = rq.np[0], L0 = rq.L0[0], nc = L1 * L2 * L3;
    if (idx >= (long long)L0 * nc * np) return;
    const int tau = (int)(idx % L0), cell = (int)((idx / L0) % nc), p = (int)(idx / ((long long)L0 * nc));
    const bool beta = (tau == L);
    const int l1 = cell % L1, l2 = (cell / L1) % L2, l3 = cell / (L1 * L2);
    const int rc = beta ? ((L1 - l1) % L1) + L1 * (((L2 - l2) % L2) + L2 * ((L3 - l3) % L3)) : cell;
    double v = B[(size_t)p * pstride + (size_t)(beta ? 0 : tau) * nc + rc];
    if (beta || tau == 0) {
        const int *d2 = defs + rq.pairs[0][2 * p] * DEFW, *d1 = defs + rq.pairs[0][2 * p + 1] * DEFW;
        const int d = d2[0], c = d2[1], b = d1[0], a = d1[1];
        const bool on[NDELTA] = {a == c, a == d, b == c, b == d};
        int l[NDELTA][3];
        cc_delta_shifts(l, d1, d2, L1, L2, L3);
        for (int k = 0; k < NDELTA; ++k)                                          // in the reference's order
            if (on[k] && rc == l[k][0] + L1 * (l[k][1] + L2 * l[k][2])) v += dl[(size_t)p * dlstride + k];
    }
    rq.acc[0][acc_off + idx] += v;
}

// ---- host

// CurrentCurrent needs model.t (t′) to reshape to (.., L1, L2, L3, n_def): what every create call answers where it does not.
inline int cc_check_bond_count(const char *prefix, int n_def, int nc, int64_t Nbonds) {
    if (Nbonds == (int64_t)n_def * nc) return ELPH_OK;
    elph_set_error("%s: CurrentCurrent needs Nbonds = n_def x ncells bonds; %lld bonds are not %d definitions x %d cells (the reference's "
                   "reshape of t' to (Ltau, L1, L2, L3, n_def) fails)", prefix, (long long)Nbonds, n_def, nc);
    return ELPH_E_UNSUPPORTED;
}

// What elph_ssh_bond_create and elph_ssh_bond_chains_create check of the bonds and phonons of a CurrentCurrent request before anything
// is allocated, and the tables they put on the device: bph [n_def nc] 0-based phonon of bond cell + nc n (-1 on a bare bond), bpar
// [NHPAR][n_def nc] t, alpha, alpha2 (zeros on a bare bond).
inline int cc_check_params(const elph_handle_s *h, const char *prefix, int n_def, int nc, int64_t Nbonds, const double *t,
                           const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph, const double *alpha, const double *alpha2,
                           std::vector<int> &bph, std::vector<double> &bpar) {
    const int L = (int)h->L;
    const size_t nb = (size_t)n_def * nc;
    if (Nbonds < 0 || Nbonds != h->nb || !t || !bond_to_definition || !bond_to_phonon || Nph < 0 || Nph > 0x7fffffff / (int64_t)(L + 1) ||
        (Nph > 0 && (!alpha || !alpha2))) {
        elph_set_error("%s: CurrentCurrent: %lld bonds (the handle has %lld) carrying %lld phonons, or a null bond or phonon array", prefix,
                       (long long)Nbonds, (long long)h->nb, (long long)Nph);
        return ELPH_E_ARG;
    }
    RC(cc_check_bond_count(prefix, n_def, nc, Nbonds));
    bph.assign(nb, -1);
    bpar.assign((size_t)NHPAR * nb, 0.0);
    for (size_t b = 0; b < nb; ++b) {
        const int64_t d = bond_to_definition[b], p = bond_to_phonon[b];
        if (d < 1 || d > n_def) { elph_set_error("%s: bond %lld belongs to definition %lld, outside 1..%d", prefix, (long long)b + 1, (long long)d, n_def); return ELPH_E_ARG; }
        if (p < 0 || p > Nph) { elph_set_error("%s: bond %lld carries phonon %lld, outside 0..%lld", prefix, (long long)b + 1, (long long)p, (long long)Nph); return ELPH_E_ARG; }
        bpar[b] = t[b];
        if (p > 0) {
            bph[b] = (int)p - 1;
            bpar[nb + b] = alpha[p - 1];
            bpar[2 * nb + b] = alpha2[p - 1];
        }
    }
    return ELPH_OK;
}

// The request arrays of the two SSH bond creates come as [BondBond, CurrentCurrent, BondPairGreens], the pair lists of the measured ones
// one after another: split into the plan of the BondState and the plan of CurrentCurrent (pure: a bad request fails before anything is
// allocated).
constexpr int CC_NREQ = 3;
enum { CC_REQ_BONDBOND = 0, CC_REQ_CURRENT = 1, CC_REQ_BONDPAIR = 2 };

inline int cc_split_plans(CorrPlan<NBOND> &bplan, CorrPlan<1> &cplan, const CorrWords &w, const int *measure, const int *time_dependent,
                          const int *npairs, const int *pairs, int n_def, int L, int nc) {
    static const char *const BOND_NAMES[NBOND] = {"BondBond", "BondPairGreens"};
    static const char *const CC_NAMES[1] = {"CurrentCurrent"};
    size_t at[CC_NREQ + 1] = {0, 0, 0, 0};
    for (int c = 0; c < CC_NREQ; ++c) at[c + 1] = at[c] + (size_t)((measure[c] && npairs[c] > 0) ? npairs[c] : 0);
    std::vector<int> bpairs;
    if (pairs) {
        bpairs.assign(pairs + 2 * at[CC_REQ_BONDBOND], pairs + 2 * at[CC_REQ_BONDBOND + 1]);
        bpairs.insert(bpairs.end(), pairs + 2 * at[CC_REQ_BONDPAIR], pairs + 2 * at[CC_REQ_BONDPAIR + 1]);
    }
    const int bm[NBOND] = {measure[CC_REQ_BONDBOND], measure[CC_REQ_BONDPAIR]};
    const int bt[NBOND] = {time_dependent[CC_REQ_BONDBOND], time_dependent[CC_REQ_BONDPAIR]};
    const int bn[NBOND] = {npairs[CC_REQ_BONDBOND], npairs[CC_REQ_BONDPAIR]};
    RC(corr_plan(bplan, w, BOND_NAMES, bm, bt, bn, pairs ? bpairs.data() : nullptr, n_def, L, nc, 0));
    return corr_plan(cplan, w, CC_NAMES, measure + CC_REQ_CURRENT, time_dependent + CC_REQ_CURRENT, npairs + CC_REQ_CURRENT,
                     pairs ? pairs + 2 * at[CC_REQ_CURRENT] : nullptr, n_def, L, nc, 0);
}

}  // namespace
