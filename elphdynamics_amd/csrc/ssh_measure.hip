// ssh_measure.hip — the measurements of the bond-phonon (SSH) model accumulated on the device (DESIGN.md "Measurements on the device"):
//   make_measurements!             Measurements.jl:545-566   (without its update!: the estimator's vectors are there already)
//     make_global_measurements!    :845-861, :1283-1312      density, Nsqr, mu
//     make_onsite_measurements!    :978-1024                 density, double_occ, mu per orbital
//     make_intersite_measurements! :1072-1155                x, x2, x4, phonon_pe, phonon_ke, elph_energy, el_ke, sign_switch per bond definition
//     measure_Greens! / _DenDen! / _SpinSpin! / _PairGreens!  :1469-1596   the folds of meas_dev.h, shared with measure.hip
//     measure_PhononGreens!        :2488-2541                the field's translation average over phonon types
//   reset_measurements!            :698-758
// One allocation holds [scalars | Greens | DenDen | SpinSpin | PairGreens | PhononGreens], all real doubles (corr_req.h).
//
// Bonds come in the reference's order (model.t, bond_to_definition, bond_to_phonon; sites neighbor_table[:, checkerboard_perm[bond]]).
// The bonds of one definition are walked in bond order through a list made at create, so a definition may own any number of bonds; the
// normalisation is the reference's V = (Nbonds / nbonds) Ltau.  The modulated hopping t' = t - (alpha x + sign(x) alpha2 x^2)
// (SSHModels.jl:531-533) is recomputed from the field, t' = t on a bare bond.
//
// Reductions have the ONE order of measure.hip: a thread walks its cells / bonds in index order, the 64 lanes of a wave fold by halves,
// the waves are added in index order through LDS, each workgroup (= one time slice) writes one partial, a single workgroup adds the L
// partials in slice order.  No floating-point atomics.  What depends on the field alone (x ... phonon_ke, sign_switch, PhononGreens) is
// computed once per accumulate and added once per pair of vectors.  One accumulate adds its pairs of vectors up from zero in a buffer of
// its own (cur) and adds that to the accumulators once at the end: two accumulations of the same inputs are twice one, to the bit.
//
// The field is (Ltau, Nph) in the reference, phonon slowest; here layout S with Nph columns: x[tau * Nph + phonon], and for
// PhononGreens phonon = cell + ncells * type (the reference's reshape to (Ltau, L1, L2, L3, nph)).  PhononGreens of the pair (b1, b2) is
//   1/(L Nc) sum_{tau, cell} x_b2[tau + dtau, cell + dcell] x_b1[tau, cell]
// spectrally: plain half spectra along tau of all Nph columns, then per (frequency, listed pair) the cell-axis DFTs of the two types in
// LDS (cell_dft_dev.h, unit = 1), their product, the inverse cell-axis DFT, and one inverse tau-transform of all listed pairs — in
// scratch this unit owns (the estimator's is sized for n_s orbitals, and nph > n_s is the normal case).

#include <vector>

#include "cell_dft_dev.h"
#include "corr_req.h"
#include "elph_internal.h"
#include "meas_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int NWAVE = MEAS_NWAVE;
static_assert(TPB == CELL_DFT_TPB, "dft_cells walks the workgroup of k_sm_ph");
constexpr int NCORR = 5;
const char *const CORR_NAMES[NCORR] = {"Greens", "DenDen", "SpinSpin", "PairGreens", "PhononGreens"};
constexpr int PHONONGREENS = 4;       // 0..3: the folds of meas_dev.h
const CorrWords WORDS = {"SSH measurements", "orbital", "with no orbital pair", PHONONGREENS, "phonon type", "with no pair of phonon types"};
constexpr int NONSITE = 3;            // density, double_occ, mu
constexpr int NINTER = 8;             // x, x2, x4, phonon_pe, phonon_ke, elph_energy, el_ke, sign_switch
constexpr int NXONLY = 6;             // x, x2, x4, phonon_pe, phonon_ke, sign_switch: functions of the field alone
constexpr int NBPAR = 4;              // per bond: t, omega, alpha, alpha2 (zeros on a bare bond)

struct SshMeasState {
    int ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0, nph = 0;
    int64_t nbonds = 0, Nph = 0;
    double dtau = 0.0, mu_mean = 0.0, V = 1.0;
    int *bs = nullptr;              // [2][nbonds] 0-based sites of every bond, the reference's bond order
    int *bph = nullptr;             // [nbonds] 0-based phonon of the bond, -1 on a bare bond
    double *bpar = nullptr;         // [NBPAR][nbonds]
    int *doff = nullptr;            // [ndef + 1] offsets into dlist
    int *dlist = nullptr;           // [nbonds] the bonds of every definition, in bond order
    double *muo = nullptr;          // [ns] mean of mu over the sites of an orbital
    CorrPlan<NCORR> cr;             // the requests; cr.acc: [nsc | the measured correlations]
    int nsc = 0;
    double *cur = nullptr;          // [cr.total] this accumulate's sums, laid out as cr.acc
    CorrReq<NCORR> rq_cur{};        // cr.req with its accumulators in cur
    double *xr = nullptr;           // [Nph][L] the field as the caller holds it
    double *x = nullptr;            // [L][Nph] the field, layout S
    double *xs = nullptr;           // [NXONLY][ndef] the field-only terms of this accumulate, normalised
    double *part = nullptr;         // [L][max(nq, NXONLY * ndef)] one partial per workgroup
    double2 *nu = nullptr;          // [Lh][Nph] the field's half spectra          (PhononGreens requested)
    double2 *Y = nullptr;           // [nP][Lh][nc] per-frequency correlations of the listed pairs
    double *B = nullptr;            // [nP][L][nc] the translation averages of this accumulate
};

SshMeasState *sm_of(elph_handle_s *h) { return (SshMeasState *)h->ssh_meas; }

size_t ph_lds_bytes(int nc) { return 4 * (size_t)nc * sizeof(double2); }

// The field-only terms (Measurements.jl:1127-1147), one workgroup per time slice: part[t][d * NXONLY + k].
__global__ void __launch_bounds__(TPB) k_sm_x(double *__restrict__ part, const double *__restrict__ x, const double *__restrict__ bpar,
                                              const int *__restrict__ bph, const int *__restrict__ doff, const int *__restrict__ dlist, int Nph,
                                              int L, int ndef, long long nbonds, double dtau) {
    __shared__ double red[NWAVE];
    const int t = blockIdx.x, tn = (t + 1 == L) ? 0 : t + 1;
    const double *xt = x + (size_t)t * Nph, *xn = x + (size_t)tn * Nph;
    const double *bt = bpar, *om = bpar + nbonds, *al = bpar + 2 * nbonds, *al2 = bpar + 3 * nbonds;
    for (int d = 0; d < ndef; ++d) {
        double a[NXONLY] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = doff[d] + threadIdx.x; j < doff[d + 1]; j += TPB) {
            const int b = dlist[j], ph = bph[b];
            if (ph < 0) continue;
            const double xi = xt[ph], dx = xn[ph] - xi, x2 = xi * xi;
            a[0] += xi;
            a[1] += x2;
            a[2] += x2 * x2;
            a[3] += om[b] * om[b] * x2 / 2;
            a[4] += 0.5 / dtau - dx * dx / (dtau * dtau) / 2;
            a[5] += (sign_of(bt[b]) != sign_of(t_modulated(bt[b], al[b], al2[b], xi))) ? 1.0 : 0.0;
        }
        for (int k = 0; k < NXONLY; ++k) {
            const double s = block_sum(a[k], red);
            if (threadIdx.x == 0) part[(size_t)t * NXONLY * ndef + d * NXONLY + k] = s;
        }
    }
}

// xs[k][d] = (sum of the slices' partials in slice order) / V
__global__ void __launch_bounds__(TPB) k_sm_x_finish(double *__restrict__ xs, const double *__restrict__ part, int L, int ndef, double V) {
    const int nq = NXONLY * ndef;
    for (int q = threadIdx.x; q < nq; q += TPB) {
        double s = 0.0;
        for (int t = 0; t < L; ++t) s += part[(size_t)t * nq + q];
        const int d = q / NXONLY, k = q % NXONLY;
        xs[k * ndef + d] = s / V;
    }
}

// The terms of one pair of vectors that need the estimate (:1011-1016, :1121-1150, :1287-1288), one workgroup per slice.
// part[t][q]: q = 2 o + {density, double_occ}; 2 n_s + {dot(M^-1 r1, r1), dot(M^-1 r2, r2)}; 2 n_s + 2 + 2 d + {el_ke, elph_energy}.
__global__ void __launch_bounds__(TPB) k_sm_pair(double *__restrict__ part, const double *__restrict__ X1, const double *__restrict__ X2,
                                                 const double *__restrict__ R1, const double *__restrict__ R2, const double *__restrict__ x,
                                                 const int *__restrict__ bs, const double *__restrict__ bpar, const int *__restrict__ bph,
                                                 const int *__restrict__ doff, const int *__restrict__ dlist, int N, int Nph, int ns, int nc,
                                                 int ndef, long long nbonds) {
    __shared__ double red[NWAVE];
    const int t = blockIdx.x, nq = 2 * ns + 2 + 2 * ndef;
    const size_t o0 = (size_t)t * N;
    const double *a1 = X1 + o0, *a2 = X2 + o0, *b1 = R1 + o0, *b2 = R2 + o0, *xt = x + (size_t)t * Nph;
    const double *bt = bpar, *al = bpar + 2 * nbonds, *al2 = bpar + 3 * nbonds;
    double *out = part + (size_t)t * nq;
    double d1 = 0.0, d2 = 0.0;
    for (int o = 0; o < ns; ++o) {
        double den = 0.0, docc = 0.0, g1s = 0.0, g2s = 0.0;
        for (int c = threadIdx.x; c < nc; c += TPB) {
            const int i = c * ns + o;
            const double G1 = a1[i] * b1[i], G2 = a2[i] * b2[i];
            den += (1.0 - G1) + (1.0 - G2);
            docc += (1.0 - G1) * (1.0 - G2);
            g1s += G1;
            g2s += G2;
        }
        double s = block_sum(den, red);
        if (threadIdx.x == 0) out[2 * o] = s;
        s = block_sum(docc, red);
        if (threadIdx.x == 0) out[2 * o + 1] = s;
        d1 += block_sum(g1s, red);                     // thread 0: orbitals in index order
        d2 += block_sum(g2s, red);
    }
    if (threadIdx.x == 0) { out[2 * ns] = d1; out[2 * ns + 1] = d2; }
    for (int d = 0; d < ndef; ++d) {
        double ke = 0.0, eph = 0.0;
        for (int j = doff[d] + threadIdx.x; j < doff[d + 1]; j += TPB) {
            const int b = dlist[j], ph = bph[b];
            const int s1 = bs[b], s2 = bs[nbonds + b];
            // h = -(G1 + G2 + G3 + G4)
            const double mh = a1[s1] * b1[s2] + a1[s2] * b1[s1] + a2[s1] * b2[s2] + a2[s2] * b2[s1];
            double tp = bt[b];
            if (ph >= 0) {
                const double xi = xt[ph];
                tp = t_modulated(tp, al[b], al2[b], xi);
                eph -= al[b] * mh * xi;                // alpha h x
            }
            ke += tp * mh;                             // -t' h
        }
        double s = block_sum(ke, red);
        if (threadIdx.x == 0) out[2 * ns + 2 + 2 * d] = s;
        s = block_sum(eph, red);
        if (threadIdx.x == 0) out[2 * ns + 2 + 2 * d + 1] = s;
    }
}

// One workgroup: the slices' partials in slice order, the tau = 0 slice of G[D,0] G[0,D] for Nsqr, then every scalar accumulator of
// this pair.  acc: [density, Nsqr, mu | NONSITE x n_s | NINTER x ndef].
__global__ void __launch_bounds__(TPB) k_sm_finish(double *__restrict__ acc, const double *__restrict__ part, const double *__restrict__ xs,
                                                   const double *__restrict__ muo, const double *__restrict__ C3, int N, int L, int ns, int nc,
                                                   int ndef, double mu_mean, double V) {
    extern __shared__ double tot[];                    // [nq] + red[NWAVE]
    const int nq = 2 * ns + 2 + 2 * ndef, ncol = ns * N;
    double *red = tot + nq;
    for (int q = threadIdx.x; q < nq; q += TPB) {
        double s = 0.0;
        for (int t = 0; t < L; ++t) s += part[(size_t)t * nq + q];
        tot[q] = s;
    }
    double g = 0.0;
    for (int i = threadIdx.x; i < ncol; i += TPB) g += C3[i];
    const double sumG = block_sum(g, red);             // (its barriers also publish tot)
    const double norm = (double)nc * (double)L;
    if (threadIdx.x == 0) {
        const double Nd = (double)N;
        const double Tr1 = tot[2 * ns] / L, Tr2 = tot[2 * ns + 1] / L;
        const double N1 = 2 * (Nd - Tr1), N2 = 2 * (Nd - Tr2);
        acc[0] += (N1 + N2) / (2 * Nd);
        acc[1] += N1 * N2 + Tr1 + Tr2 - 2 * (Nd / ns) * sumG;
        acc[2] += mu_mean;
    }
    double *on = acc + 3;
    for (int o = threadIdx.x; o < ns; o += TPB) {
        on[0 * ns + o] += tot[2 * o] / norm;
        on[1 * ns + o] += tot[2 * o + 1] / norm;
        on[2 * ns + o] += muo[o];
    }
    double *in = acc + 3 + NONSITE * ns;
    for (int d = threadIdx.x; d < ndef; d += TPB) {
        for (int k = 0; k < 5; ++k) in[k * ndef + d] += xs[k * ndef + d];
        in[5 * ndef + d] += tot[2 * ns + 2 + 2 * d + 1] / V;
        in[6 * ndef + d] += tot[2 * ns + 2 + 2 * d] / V;
        in[7 * ndef + d] += xs[5 * ndef + d];
    }
}

// One workgroup per (frequency, listed pair of phonon types): the cell-axis DFTs of the two types' spectra, their product with
// fft(g)[-w,-k] = conj fft(g)[w,k], the inverse cell-axis DFT.  LDS: 4 buffers of nc complex.
__global__ void __launch_bounds__(TPB) k_sm_ph(double2 *__restrict__ Y, const double2 *__restrict__ nu, const int *__restrict__ pairs, int Lh,
                                               int Nph, int L1, int L2, int L3, const double2 *__restrict__ tw, double norm) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3, k = blockIdx.x, p = blockIdx.y;
    const int t1 = pairs[2 * p], t2 = pairs[2 * p + 1];
    const double2 *f = nu + (size_t)k * Nph + (size_t)t2 * nc, *g = nu + (size_t)k * Nph + (size_t)t1 * nc;
    double2 *A = lds, *TA = lds + nc, *B = lds + 2 * nc, *TB = lds + 3 * nc;
    for (int q = threadIdx.x; q < nc; q += TPB) { A[q] = f[q]; B[q] = g[q]; }
    __syncthreads();
    const double2 *Af = dft_cells<false>(A, TA, 1, L1, L2, L3, tw);
    const double2 *Bf = dft_cells<false>(B, TB, 1, L1, L2, L3, tw);
    double2 *P = (Af == A) ? TA : A, *Q = (Bf == B) ? TB : B;
    for (int q = threadIdx.x; q < nc; q += TPB) {
        const double2 a = Af[q], b = Bf[q];            // a·conj(b)
        P[q] = make_double2((a.x * b.x + a.y * b.y) * norm, (a.y * b.x - a.x * b.y) * norm);
    }
    __syncthreads();
    const double2 *Pf = dft_cells<true>(P, Q, 1, L1, L2, L3, tw);
    double2 *y = Y + ((size_t)p * Lh + k) * nc;
    for (int q = threadIdx.x; q < nc; q += TPB) y[q] = Pf[q];
}

// One thread per (tau, cell, listed pair) of correlation blockIdx.y.  C: the estimator's four real tables of this pair of vectors; B: the
// translation averages of the listed phonon-type pairs; slice L is slice 0.
__global__ void __launch_bounds__(TPB) k_sm_fold(CorrReq<NCORR> rq, const double *__restrict__ C, const double *__restrict__ B, int N, int L, int ns,
                                                 int L1, int L2, int L3) {
    const int which = blockIdx.y, np = rq.np[which], L0 = rq.L0[which], nc = L1 * L2 * L3;
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= (long long)L0 * nc * np) return;
    const int tau = (int)(idx % L0), cell = (int)((idx / L0) % nc);
    const int p = (int)(idx / ((long long)L0 * nc));
    double v;
    if (which == PHONONGREENS)
        v = B[((size_t)p * L + (tau == L ? 0 : tau)) * nc + cell];
    else
        v = meas_fold(which, C, N, L, ns, L1, L2, L3, tau, cell, rq.pairs[which][2 * p], rq.pairs[which][2 * p + 1]);
    rq.acc[which][idx] += v;
}

// acc += cur, one thread per element
__global__ void __launch_bounds__(TPB) k_sm_add(double *__restrict__ acc, const double *__restrict__ cur, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) acc[i] += cur[i];
}

int need_ssh_meas(elph_handle_s *h) { return corr_need(h->ssh_meas, "elph_ssh_meas_create"); }

}  // namespace

void elph_i_ssh_meas_free(elph_handle_s *h) {
    SshMeasState *m = sm_of(h);
    if (!m) return;
    corr_free({m->bs, m->bph, m->bpar, m->doff, m->dlist, m->muo, m->cr.pairs, m->cr.acc, m->cur, m->xr, m->x, m->xs, m->part, m->nu, m->Y, m->B});
    delete m;
    h->ssh_meas = nullptr;
}

extern "C" int elph_ssh_meas_free(elph_handle h) {
    CHECK_H(h);
    elph_i_ssh_meas_free(h);
    return ELPH_OK;
}

extern "C" int elph_ssh_meas_create(elph_handle h, const double *mu, double dtau, int64_t nbonds, int ndef, const int64_t *bond_sites,
                                    const double *bond_t, const int64_t *bond_to_definition, const int64_t *bond_to_phonon, int64_t Nph,
                                    int nph, const double *omega, const double *alpha, const double *alpha2, const int *measure,
                                    const int *time_dependent, const int *npairs, const int *pairs) {
    CHECK_H(h);
    elph_i_ssh_meas_free(h);
    RC(corr_refuse_handle(h, WORDS.prefix, ELPH_MODEL_SSH));
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (!mu || !measure || !time_dependent || !npairs) { elph_set_error("SSH measurements: a null parameter array"); return ELPH_E_ARG; }
    if (!(dtau > 0.0)) { elph_set_error("SSH measurements: dtau = %g", dtau); return ELPH_E_ARG; }
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = g.ns, nc = g.nc;
    if (ndef < 0 || nbonds < 0 || nbonds != h->nb || (nbonds > 0 && (ndef < 1 || nbonds < ndef || !bond_sites || !bond_t || !bond_to_definition || !bond_to_phonon))) {
        elph_set_error("SSH measurements: %lld bonds in %d bond definitions (the handle has %lld bonds), or a null bond array", (long long)nbonds, ndef,
                       (long long)h->nb);
        return ELPH_E_ARG;
    }
    if (nbonds == 0) ndef = 0;
    if (Nph < 0 || nph < 0 || Nph > 0x7fffffff / (int64_t)(L + 1) || (Nph > 0 && (!omega || !alpha || !alpha2))) {
        elph_set_error("SSH measurements: %lld phonons of %d types, or a null phonon array", (long long)Nph, nph);
        return ELPH_E_ARG;
    }
    std::vector<int> bs(2 * (size_t)nbonds), bph((size_t)nbonds), doff((size_t)ndef + 1, 0), dlist((size_t)nbonds);
    std::vector<double> bpar((size_t)NBPAR * nbonds, 0.0);
    for (int64_t b = 0; b < nbonds; ++b) {
        for (int k = 0; k < 2; ++k) {
            const int64_t s = bond_sites[2 * b + k];
            if (s < 1 || s > N) { elph_set_error("SSH measurements: bond %lld joins site %lld, outside 1..%d", (long long)b + 1, (long long)s, N); return ELPH_E_ARG; }
            bs[(size_t)k * nbonds + b] = (int)(s - 1);
        }
        const int64_t d = bond_to_definition[b], p = bond_to_phonon[b];
        if (d < 1 || d > ndef) { elph_set_error("SSH measurements: bond %lld belongs to definition %lld, outside 1..%d", (long long)b + 1, (long long)d, ndef); return ELPH_E_ARG; }
        if (p < 0 || p > Nph) { elph_set_error("SSH measurements: bond %lld carries phonon %lld, outside 0..%lld", (long long)b + 1, (long long)p, (long long)Nph); return ELPH_E_ARG; }
        ++doff[(size_t)d];
        bph[(size_t)b] = (int)p - 1;
        bpar[(size_t)b] = bond_t[b];
        if (p > 0) {
            bpar[(size_t)nbonds + b] = omega[p - 1];
            bpar[2 * (size_t)nbonds + b] = alpha[p - 1];
            bpar[3 * (size_t)nbonds + b] = alpha2[p - 1];
        }
    }
    for (int d = 0; d < ndef; ++d) doff[(size_t)d + 1] += doff[(size_t)d];
    {
        std::vector<int> at(doff.begin(), doff.end() - 1);
        for (int64_t b = 0; b < nbonds; ++b) dlist[(size_t)at[(size_t)bond_to_definition[b] - 1]++] = (int)b;
    }
    const int nsc = 3 + NONSITE * ns + NINTER * ndef;
    CorrPlan<NCORR> plan;                              // request bookkeeping before anything is allocated
    RC(corr_plan(plan, WORDS, CORR_NAMES, measure, time_dependent, npairs, pairs, ns, L, nc, (size_t)nsc, nph));
    const int nP = plan.req.np[PHONONGREENS];
    if (nP) {
        if (nph < 1 || Nph != (int64_t)nph * nc) {
            elph_set_error("SSH measurements: PhononGreens needs Nph = nph x ncells phonons; %lld phonons are not %d types x %d cells (the "
                           "reference's reshape of the field to (Ltau, L1, L2, L3, nph) fails)", (long long)Nph, nph, nc);
            return ELPH_E_UNSUPPORTED;
        }
        if (ph_lds_bytes(nc) > 160 * 1024) {
            elph_set_error("SSH measurements: PhononGreens: a frequency slice of the %d x %d x %d lattice (%d cells) does not fit in 160 KB of LDS",
                           g.L1, g.L2, g.L3, nc);
            return ELPH_E_UNSUPPORTED;
        }
    }
    SshMeasState *m = new SshMeasState;
    h->ssh_meas = m;
    m->cr = plan;
    m->ns = ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = ndef; m->nph = nph; m->nbonds = nbonds; m->Nph = Nph;
    m->dtau = dtau; m->nsc = nsc;
    m->V = ndef ? (double)(nbonds / ndef) * (double)L : 1.0;           // div(Nbonds, nbonds) * Ltau, :1094
    double mus = 0.0;
    for (int i = 0; i < N; ++i) mus += mu[i];
    m->mu_mean = mus / N;                              // mean(model.mu), :858
    std::vector<double> muo((size_t)ns, 0.0);          // sum over the cells and slices of mu[site] / (Nc L), :1018
    for (int o = 0; o < ns; ++o) {
        for (int c = 0; c < nc; ++c) muo[(size_t)o] += mu[(size_t)c * ns + o];
        muo[(size_t)o] /= nc;
    }
    const int nq = std::max(2 * ns + 2 + 2 * ndef, NXONLY * ndef);
    const size_t nx = (size_t)L * (size_t)Nph;
    CorrFirstError ok;
    const bool allocated = ok(corr_alloc(&m->bs, bs.size())) && ok(corr_alloc(&m->bph, bph.size())) && ok(corr_alloc(&m->bpar, bpar.size())) &&
        ok(corr_alloc(&m->doff, doff.size())) && ok(corr_alloc(&m->dlist, dlist.size())) && ok(corr_alloc(&m->muo, muo.size())) &&
        ok(corr_alloc(m->cr)) && ok(corr_alloc(&m->cur, m->cr.total)) && ok(corr_alloc(&m->xr, nx)) && ok(corr_alloc(&m->x, nx)) && ok(corr_alloc(&m->xs, (size_t)NXONLY * ndef)) &&
        ok(corr_alloc(&m->part, (size_t)L * nq)) &&
        (nP == 0 || (ok(corr_alloc(&m->nu, (size_t)Lh * Nph)) && ok(corr_alloc(&m->Y, (size_t)nP * Lh * nc)) && ok(corr_alloc(&m->B, (size_t)nP * L * nc))));
    if (!allocated) { elph_i_ssh_meas_free(h); return ok.rc; }
    ok(corr_up(m->bs, bs.data(), bs.size() * sizeof(int)));
    ok(corr_up(m->bph, bph.data(), bph.size() * sizeof(int)));
    ok(corr_up(m->bpar, bpar.data(), bpar.size() * sizeof(double)));
    ok(corr_up(m->doff, doff.data(), doff.size() * sizeof(int)));
    ok(corr_up(m->dlist, dlist.data(), dlist.size() * sizeof(int)));
    ok(corr_up(m->muo, muo.data(), muo.size() * sizeof(double)));
    if (ok.rc == ELPH_OK) ok(corr_upload(m->cr, WORDS.prefix));
    m->rq_cur = m->cr.req;
    for (int c = 0; c < NCORR; ++c) m->rq_cur.acc[c] = m->cur + m->cr.off[c];
    const int lds = (int)ph_lds_bytes(nc);
    if (ok.rc == ELPH_OK && nP && hipFuncSetAttribute((const void *)k_sm_ph, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
        elph_set_error("SSH measurements: %d bytes of LDS were refused", lds);
        ok(ELPH_E_HIP);
    }
    if (ok.rc != ELPH_OK) elph_i_ssh_meas_free(h);
    return ok.rc;
}

extern "C" int elph_ssh_meas_accumulate(elph_handle h, const double *x) {
    CHECK_H(h);
    RC(need_ssh_meas(h));
    RC(corr_refuse_chains(h, WORDS.prefix));
    SshMeasState *m = sm_of(h);
    if (!x && m->Nph > 0) { elph_set_error("x is null"); return ELPH_E_ARG; }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = m->ns, nc = m->nc, nv = g.nv, ndef = m->ndef, Nph = (int)m->Nph;
    const int nP = m->cr.req.np[PHONONGREENS];
    const size_t total = std::max<size_t>(m->cr.total, 1);
    HIPCHK(hipMemsetAsync(m->cur, 0, total * sizeof(double), h->stream));
    if (Nph > 0) {
        HIPCHK(hipMemcpyAsync(m->xr, x, (size_t)L * Nph * sizeof(double), hipMemcpyHostToDevice, h->stream));
        RC(elph_launch_r2s(h, m->x, m->xr, 1, Nph));
    }
    // what depends on the field alone: once per call, added once per pair below (the reference's loop recomputes it per pair)
    if (ndef) {
        hipLaunchKernelGGL(k_sm_x, dim3((unsigned)L), dim3(TPB), 0, h->stream, m->part, m->x, m->bpar, m->bph, m->doff, m->dlist, Nph, L, ndef,
                           (long long)m->nbonds, m->dtau);
        RC(elph_launch_check("k_sm_x"));
        hipLaunchKernelGGL(k_sm_x_finish, dim3(1), dim3(TPB), 0, h->stream, m->xs, m->part, L, ndef, m->V);
        RC(elph_launch_check("k_sm_x_finish"));
    }
    if (nP) {
        RC(elph_dft_fwd_plain(h, m->nu, m->x, Nph, 1));
        const double norm = 1.0 / ((double)L * (double)nc * (double)nc);       // 1/(L Nc)² in all: the other 1/L is in the inverse τ table
        hipLaunchKernelGGL(k_sm_ph, dim3((unsigned)Lh, (unsigned)nP), dim3(TPB), ph_lds_bytes(nc), h->stream, m->Y, m->nu,
                           m->cr.req.pairs[PHONONGREENS], Lh, Nph, m->L1, m->L2, m->L3, g.tw, norm);
        RC(elph_launch_check("k_sm_ph"));
        RC(elph_dft_inv_plain(h, m->B, m->Y, nc, nP));
    }
    const int nq = 2 * ns + 2 + 2 * ndef;
    const size_t shm = ((size_t)nq + NWAVE) * sizeof(double);
    const size_t tab = (size_t)L * ns * N;
    for (int i = 1; i < nv; ++i)
        for (int j = i + 1; j <= nv; ++j) {
            ElphGreensPair v;
            RC(elph_i_greens_pair_dev(h, i, j, &v));
            hipLaunchKernelGGL(k_sm_pair, dim3((unsigned)L), dim3(TPB), 0, h->stream, m->part, v.X1, v.X2, v.R1, v.R2, m->x, m->bs, m->bpar, m->bph,
                               m->doff, m->dlist, N, Nph, ns, nc, ndef, (long long)m->nbonds);
            RC(elph_launch_check("k_sm_pair"));
            hipLaunchKernelGGL(k_sm_finish, dim3(1), dim3(TPB), shm, h->stream, m->cur, m->part, m->xs, m->muo, g.C + 3 * tab, N, L, ns, nc, ndef,
                               m->mu_mean, m->V);
            RC(elph_launch_check("k_sm_finish"));
            if (m->cr.fold_max) {
                hipLaunchKernelGGL(k_sm_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), NCORR), dim3(TPB), 0, h->stream, m->rq_cur, g.C, m->B, N, L,
                                   ns, m->L1, m->L2, m->L3);
                RC(elph_launch_check("k_sm_fold"));
            }
        }
    hipLaunchKernelGGL(k_sm_add, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->cr.acc, m->cur, (long long)m->cr.total);
    RC(elph_launch_check("k_sm_add"));
    HIPCHK(hipStreamSynchronize(h->stream));           // x (a host pointer) is not retained after return
    return ELPH_OK;
}

extern "C" int elph_ssh_meas_fetch(elph_handle h, double *scalars, double *Greens, double *DenDen, double *SpinSpin, double *PairGreens,
                                   double *PhononGreens) {
    CHECK_H(h);
    RC(need_ssh_meas(h));
    SshMeasState *m = sm_of(h);
    std::vector<double> host;
    double *outs[NCORR] = {Greens, DenDen, SpinSpin, PairGreens, PhononGreens};
    RC(corr_fetch(h, m->cr, host, outs));
    if (scalars)
        for (int i = 0; i < m->nsc; ++i) scalars[i] = host[(size_t)i];
    return ELPH_OK;
}

extern "C" int elph_ssh_meas_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_ssh_meas(h));
    return corr_reset(h, sm_of(h)->cr);
}
