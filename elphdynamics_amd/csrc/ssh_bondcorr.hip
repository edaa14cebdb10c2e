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
// requested), CurrentCurrent in an accumulator and scratch of this unit's.

#include <vector>

#include "bondcorr_dev.h"
#include "meas_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int NWAVE = MEAS_NWAVE;
static_assert(TPB == BC_TPB, "dft_cells walks the workgroup of k_cc_correlate");
constexpr int NREQ = 3;               // the entry points' request order
enum { REQ_BONDBOND = 0, REQ_CURRENT = 1, REQ_BONDPAIR = 2 };
const char *const BOND_NAMES[NBOND] = {"BondBond", "BondPairGreens"};
const char *const CC_NAMES[1] = {"CurrentCurrent"};
const CorrWords WORDS = {"SSH bond correlations", "bond", "with no pair of bonds"};
constexpr int NCC = 8;                // fields per definition (header)
constexpr int NDELTA = 4;             // δ terms: a == c, a == d, b == c, b == d
constexpr int NHPAR = 3;              // per bond: t, alpha, alpha2 (zeros on a bare bond)

using CcReq = CorrReq<1>;

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

// t′ of bond `bond` = cell + nc n on slice t
__device__ __forceinline__ double cc_hopping(const double *__restrict__ bpar, const int *__restrict__ bph, const double *__restrict__ xr,
                                             int nb, int L, int bond, int t) {
    const int ph = bph[bond];
    const double t0 = bpar[bond];
    return ph < 0 ? t0 : t_modulated(t0, bpar[nb + bond], bpar[2 * nb + bond], xr[(size_t)ph * L + t]);
}

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

// The eight fields of every definition (header), one thread per (cell, τ, definition).
__global__ void __launch_bounds__(TPB) k_cc_fields(double *__restrict__ f, const double *__restrict__ X1, const double *__restrict__ X2,
                                                   const double *__restrict__ R1, const double *__restrict__ R2, const int *__restrict__ defs,
                                                   const double *__restrict__ bpar, const int *__restrict__ bph, const double *__restrict__ xr,
                                                   int N, int L, int ns, int L1, int L2, int L3, int ndef) {
    const int nc = L1 * L2 * L3;
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long per = (long long)L * nc;
    if (idx >= per * ndef) return;
    const int cell = (int)(idx % nc), t = (int)((idx / nc) % L), n = (int)(idx / per);
    const int *dv = defs + n * DEFW;
    const size_t is = (size_t)t * N + (size_t)cell * ns + dv[0];
    const size_t ie = (size_t)t * N + (size_t)shifted_cell(cell, dv, L1, L2, L3) * ns + dv[1];
    const double x1s = X1[is], x2s = X2[is], r1s = R1[is], r2s = R2[is], x1e = X1[ie], x2e = X2[ie], r1e = R1[ie], r2e = R2[ie];
    const double tp = cc_hopping(bpar, bph, xr, ndef * nc, L, n * nc + cell, t);
    const size_t fs = (size_t)ndef * per, o = (size_t)n * per + (size_t)t * nc + cell;
    f[o] = (x1s * r1e) * tp;
    f[fs + o] = (x1e * r1s) * tp;
    f[2 * fs + o] = (x2e * r2s) * tp;
    f[3 * fs + o] = (x2s * r2e) * tp;
    f[4 * fs + o] = (x1s * r2e) * tp;
    f[5 * fs + o] = (x2e * r1s) * tp;
    f[6 * fs + o] = (r1e * x2s) * tp;
    f[7 * fs + o] = (x1e * r2s) * tp;
}

// One workgroup per (frequency, listed pair): the eight products of the spectra in the reference's order (term 6 with its operands
// swapped), inverse cell-axis DFT.  nu as in k_bc_correlate.  LDS: 2 buffers of nc complex.
__global__ void __launch_bounds__(TPB) k_cc_correlate(double2 *__restrict__ Y, const double2 *__restrict__ nu, CcReq rq, int Lh, int ndef, int L1,
                                                      int L2, int L3, const double2 *__restrict__ tw, double norm) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3, k = blockIdx.x, p = blockIdx.y;
    const int n2 = rq.pairs[0][2 * p], n1 = rq.pairs[0][2 * p + 1];               // n″, n′
    const size_t slice = (size_t)Lh * nc;
    auto field = [&](int kind, int n) { return nu + ((size_t)kind * ndef + n) * slice + (size_t)k * nc; };
    const double2 *A0 = field(0, n1), *A1 = field(1, n1), *A4 = field(4, n1), *A7 = field(7, n1);
    const double2 *B2 = field(2, n2), *B3 = field(3, n2), *B5 = field(5, n2), *B6 = field(6, n2);
    double2 *P = lds, *Q = lds + nc;
    for (int q = threadIdx.x; q < nc; q += TPB) {
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
    double2 *y = Y + ((size_t)p * Lh + k) * nc;
    for (int q = threadIdx.x; q < nc; q += TPB) y[q] = Pf[q];
}

// One workgroup per (time slice, listed pair): this slice's part of the four δ sums (header), zero where the orbitals differ.
__global__ void __launch_bounds__(TPB) k_cc_delta(double *__restrict__ part, CcReq rq, const double *__restrict__ X1, const double *__restrict__ R1,
                                                  const int *__restrict__ defs, const double *__restrict__ bpar, const int *__restrict__ bph,
                                                  const double *__restrict__ xr, int N, int L, int ns, int L1, int L2, int L3, int ndef) {
    __shared__ double red[NWAVE];
    const int nc = L1 * L2 * L3, nb = ndef * nc, t = blockIdx.x, p = blockIdx.y;
    const int n2 = rq.pairs[0][2 * p], n1 = rq.pairs[0][2 * p + 1];
    const int *d2 = defs + n2 * DEFW, *d1 = defs + n1 * DEFW;
    const int d = d2[0], c = d2[1], b = d1[0], a = d1[1];
    const bool on[NDELTA] = {a == c, a == d, b == c, b == d};
    int l[NDELTA][3];
    cc_delta_shifts(l, d1, d2, L1, L2, L3);
    const double *x1 = X1 + (size_t)t * N, *r1 = R1 + (size_t)t * N;
    double s[NDELTA] = {0.0, 0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < nc; j += TPB) {
        const double u = cc_hopping(bpar, bph, xr, nb, L, n1 * nc + j, t);
        const int jp = shifted_cell(j, d1, L1, L2, L3);                           // j + r′
        if (on[0]) {
            const int jl = cell_plus(j, l[0][0], l[0][1], l[0][2], L1, L2, L3);
            s[0] += (x1[j * ns + b] * u) * (r1[jl * ns + d] * cc_hopping(bpar, bph, xr, nb, L, n2 * nc + jl, t));
        }
        if (on[1]) {
            const int jl = cell_plus(j, l[1][0], l[1][1], l[1][2], L1, L2, L3);
            s[1] += (x1[j * ns + b] * u) * (r1[shifted_cell(jl, d2, L1, L2, L3) * ns + c] * cc_hopping(bpar, bph, xr, nb, L, n2 * nc + jl, t));
        }
        if (on[2]) {
            const int jl = cell_plus(j, l[2][0], l[2][1], l[2][2], L1, L2, L3);
            s[2] += (x1[jp * ns + b] * u) * (r1[jl * ns + d] * cc_hopping(bpar, bph, xr, nb, L, n2 * nc + jl, t));
        }
        if (on[3])
            s[3] += (x1[jp * ns + a] * u) * (r1[shifted_cell(j, d2, L1, L2, L3) * ns + c] * cc_hopping(bpar, bph, xr, nb, L, n2 * nc + j, t));
    }
    for (int k = 0; k < NDELTA; ++k) {
        const double tot = block_sum(s[k], red);
        if (threadIdx.x == 0) part[((size_t)p * L + t) * NDELTA + k] = tot;
    }
}

// dl[p][k] = ± 2 (the slices' partials in slice order) / (L nc), one thread per (listed pair, δ term)
__global__ void __launch_bounds__(TPB) k_cc_delta_finish(double *__restrict__ dl, const double *__restrict__ part, int np, int L, int nc) {
    const int q = blockIdx.x * TPB + threadIdx.x;
    if (q >= np * NDELTA) return;
    const int p = q / NDELTA, k = q % NDELTA;
    double s = 0.0;
    for (int t = 0; t < L; ++t) s += part[((size_t)p * L + t) * NDELTA + k];
    const double v = 2 * s / ((double)L * (double)nc);
    dl[q] = (k == 1 || k == 2) ? -v : v;
}

// One thread per (τ, cell, listed pair): the δ terms at their τ = 0 cells, the τ = β slice J(β, r) = J(0, -r) (:2363-2380).
__global__ void __launch_bounds__(TPB) k_cc_fold(CcReq rq, const double *__restrict__ B, const double *__restrict__ dl, const int *__restrict__ defs,
                                                 int L, int L1, int L2, int L3) {
    const int np = rq.np[0], L0 = rq.L0[0], nc = L1 * L2 * L3;
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (long long)L0 * nc * np) return;
    const int tau = (int)(idx % L0), cell = (int)((idx / L0) % nc), p = (int)(idx / ((long long)L0 * nc));
    const bool beta = (tau == L);
    const int l1 = cell % L1, l2 = (cell / L1) % L2, l3 = cell / (L1 * L2);
    const int rc = beta ? ((L1 - l1) % L1) + L1 * (((L2 - l2) % L2) + L2 * ((L3 - l3) % L3)) : cell;
    double v = B[((size_t)p * L + (beta ? 0 : tau)) * nc + rc];
    if (beta || tau == 0) {
        const int *d2 = defs + rq.pairs[0][2 * p] * DEFW, *d1 = defs + rq.pairs[0][2 * p + 1] * DEFW;
        const int d = d2[0], c = d2[1], b = d1[0], a = d1[1];
        const bool on[NDELTA] = {a == c, a == d, b == c, b == d};
        int l[NDELTA][3];
        cc_delta_shifts(l, d1, d2, L1, L2, L3);
        for (int k = 0; k < NDELTA; ++k)                                          // in the reference's order
            if (on[k] && rc == l[k][0] + L1 * (l[k][1] + L2 * l[k][2])) v += dl[p * NDELTA + k];
    }
    rq.acc[0][idx] += v;
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
    // the request arrays come as [BondBond, CurrentCurrent, BondPairGreens], the pair lists of the measured ones one after another: split
    // into the two plans (pure: a bad request fails before anything is allocated)
    size_t at[NREQ + 1] = {0, 0, 0, 0};
    for (int c = 0; c < NREQ; ++c) at[c + 1] = at[c] + (size_t)((measure[c] && npairs[c] > 0) ? npairs[c] : 0);
    std::vector<int> bpairs;
    if (pairs) {
        bpairs.assign(pairs + 2 * at[REQ_BONDBOND], pairs + 2 * at[REQ_BONDBOND + 1]);
        bpairs.insert(bpairs.end(), pairs + 2 * at[REQ_BONDPAIR], pairs + 2 * at[REQ_BONDPAIR + 1]);
    }
    const int bm[NBOND] = {measure[REQ_BONDBOND], measure[REQ_BONDPAIR]}, bt[NBOND] = {time_dependent[REQ_BONDBOND], time_dependent[REQ_BONDPAIR]};
    const int bn[NBOND] = {npairs[REQ_BONDBOND], npairs[REQ_BONDPAIR]};
    CorrPlan<NBOND> bplan;
    RC(corr_plan(bplan, WORDS, BOND_NAMES, bm, bt, bn, pairs ? bpairs.data() : nullptr, n_def, L, nc, 0));
    CorrPlan<1> cplan;
    RC(corr_plan(cplan, WORDS, CC_NAMES, measure + REQ_CURRENT, time_dependent + REQ_CURRENT, npairs + REQ_CURRENT,
                 pairs ? pairs + 2 * at[REQ_CURRENT] : nullptr, n_def, L, nc, 0));
    const int np = cplan.req.np[0];
    const size_t nb = (size_t)n_def * nc;
    std::vector<int> bph;
    std::vector<double> bpar;
    if (np) {
        if (Nbonds < 0 || Nbonds != h->nb || !t || !bond_to_definition || !bond_to_phonon || Nph < 0 || Nph > 0x7fffffff / (int64_t)(L + 1) ||
            (Nph > 0 && (!alpha || !alpha2))) {
            elph_set_error("%s: CurrentCurrent: %lld bonds (the handle has %lld) carrying %lld phonons, or a null bond or phonon array", WORDS.prefix,
                           (long long)Nbonds, (long long)h->nb, (long long)Nph);
            return ELPH_E_ARG;
        }
        if ((size_t)Nbonds != nb) {
            elph_set_error("%s: CurrentCurrent needs Nbonds = n_def x ncells bonds; %lld bonds are not %d definitions x %d cells (the reference's "
                           "reshape of t' to (Ltau, L1, L2, L3, n_def) fails)", WORDS.prefix, (long long)Nbonds, n_def, nc);
            return ELPH_E_UNSUPPORTED;
        }
        bph.assign(nb, -1);
        bpar.assign((size_t)NHPAR * nb, 0.0);
        for (size_t b = 0; b < nb; ++b) {
            const int64_t d = bond_to_definition[b], p = bond_to_phonon[b];
            if (d < 1 || d > n_def) { elph_set_error("%s: bond %lld belongs to definition %lld, outside 1..%d", WORDS.prefix, (long long)b + 1, (long long)d, n_def); return ELPH_E_ARG; }
            if (p < 0 || p > Nph) { elph_set_error("%s: bond %lld carries phonon %lld, outside 0..%lld", WORDS.prefix, (long long)b + 1, (long long)p, (long long)Nph); return ELPH_E_ARG; }
            bpar[b] = t[b];
            if (p > 0) {
                bph[b] = (int)p - 1;
                bpar[nb + b] = alpha[p - 1];
                bpar[2 * nb + b] = alpha2[p - 1];
            }
        }
    }
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
