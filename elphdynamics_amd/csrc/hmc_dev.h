// hmc_dev.h — what the three units of the resident dynamics share: hmc.hip (the state, the shared steps, the HMC trajectory),
// langevin.hip and special_updates.hip.  The state record and the host helpers that more than one of them calls (defined in hmc.hip
// unless inline); every kernel is defined in one unit only and reached from the others through its launcher below.
#pragma once

#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>
#include "elph_internal.h"
#include "rng_dev.h"

namespace hmc {

constexpr int TPB = 256;
inline unsigned nblk(long long n) { return (unsigned)((n + TPB - 1) / TPB); }

struct HmcState {
    int nch = 1;                 // chains advanced in lockstep (one phonon configuration, one trajectory each)
    bool ssh = false;            // SSH: the fields are bond phonons (nf = Nph columns), Λ ≡ 1
    int nf = 0;                  // phonon columns: nsites (Holstein) or Nph (SSH); field vectors are [tau][column]
    // per chain: [nch][nf*L], layout S (tau-major) inside a chain
    double *x = nullptr, *v = nullptr, *x0 = nullptr, *v0 = nullptr, *dS = nullptr, *y = nullptr;
    double *R2 = nullptr;        // [2][nch][ndim] R±
    double *phi = nullptr;       // [2][nch][ndim] ϕ±
    double *faM = nullptr;       // FourierAccelerator.M in layout S ([k][site]), shared by the chains
    double *par = nullptr;       // [2N] ω, ω₄   (λ, λ₂, μ are h->d_lam)
    double *part = nullptr;      // [2 nch][L] partial sums
    double dtau = 0.0;
    bool have_state = false;
    // SSH phonon types of the same name share their fields (SSHModels.jl:480-502): primary column of each column, the next
    // member of its class (-1 ends the list) and the weight 1 (primary) / 0 of each column in Sb and K
    bool shared = false;
    int *prim = nullptr, *next = nullptr;
    double *wcol = nullptr;
    std::vector<int> prim_host;
    // a sharded lattice with bond phonons (elph_shard_hmc_set_columns): the slab's phonon columns in the numbering of the whole lattice, which of
    // them this rank owns (weight 1 / 0, device copy in wown) — sums over fields count owned columns, the force of the others comes from their owners
    double *wown = nullptr;
    std::vector<int> gcol;
    std::vector<double> wown_host;
    int ngcol = 0;
    // optional generator for the random inputs the caller leaves NULL (elph_hmc_set_rng)
    bool rng_on = false;
    uint64_t rng_seed = 0, rng_batches = 0;
    // scratch of the special updates, made on first use: one allocation, carved by special_scratch (special_updates.hip)
    void *sp_buf = nullptr;
    size_t sp_cap = 0;
};

inline HmcState *state_of(elph_handle_s *h) { return static_cast<HmcState *>(h->hmc); }
// The precondition of an entry point: *st = the handle's state, ELPH_E_STATE when there is none or — with_field — no field in it yet
int state_ready(elph_handle_s *h, HmcState **st, bool with_field = false);
int chk(const char *what);      // the last launch: ELPH_E_HIP naming `what` when it failed

// Random inputs.  An input the caller leaves NULL is drawn from the handle's generator (elph_hmc_set_rng).  Batch k (from 1) of a handle seeded with s is
// the counter-based stream of sm64(s, k) (rng_dev.h) and equals synth.randn / synth.uniform01 of that seed; elph_hmc_rng_batches counts
// them.  The batches of a call, in the order they are taken — part of the contract: tests replay them by number.
//   elph_hmc_update[_chains]          R, R₊, R₋, [kpm_randn: Nt + 2 set-ups], u
//   elph_hmc_special_move[_chains]    R₊, R₋, [kpm_randn: 1 set-up], u
//   elph_hmc_special_update_chains    per move: the draw, R₊, R₋, [kpm_randn: 1 set-up], u       (the draw and u are read on the device)
//   elph_langevin_evolve              eta, [kpm_randn: 2 set-ups], g1, g2                          (g2: beyond Euler)
// Only an input that is NULL takes a batch, [kpm_randn] only with a preconditioner.  Vectors (R, R±, eta, g) are made on the device
// (randn_vectors), kpm_randn and u on the host (given_or_drawn).

// seed of the next batch: output number (batches drawn so far + 1) of SplitMix64 started at the handle's seed
inline uint64_t next_batch_seed(HmcState *st) { return sm64(st->rng_seed, ++st->rng_batches); }

// the refusal of random inputs left NULL on a handle without a generator
inline int need_randoms(const HmcState *st, bool all_given, const char *names) {
    if (!all_given && !st->rng_on) { elph_set_error("%s are required unless elph_hmc_set_rng was called", names); return ELPH_E_ARG; }
    return ELPH_OK;
}

// A host-side random input of n numbers, given or drawn: *p stays when the caller gave it, otherwise `own` takes the next batch — standard
// normals (the Arnoldi start vectors kpm_randn) or uniforms (the Metropolis numbers u) — and *p points at it
inline int given_or_drawn(HmcState *st, const double **p, std::vector<double> &own, size_t n, bool normal) {
    if (*p) return ELPH_OK;
    RC(need_randoms(st, false, "random inputs"));
    const uint64_t seed = next_batch_seed(st);
    const size_t m = (n + 1) / 2;
    own.resize(n);
    *p = own.data();
    if (!normal) { for (size_t k = 0; k < n; ++k) own[k] = u01(seed, k); return ELPH_OK; }
    auto fill = [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; ++k) {
            const double r = sqrt(-2.0 * log(u01(seed, k))), th = 6.283185307179586476925 * u01(seed, m + k);
            own[2 * k] = r * cos(th);
            if (2 * k + 1 < n) own[2 * k + 1] = r * sin(th);
        }
    };
    // counter-based: any split gives the same numbers.  ~20 ns per normal on one core; 64 chains x (Nt + 2) set-ups need 10^6
    const size_t nthr = std::min<size_t>({(size_t)16, m / 16384 + 1, (size_t)std::max(1u, std::thread::hardware_concurrency())});
    if (nthr <= 1) { fill(0, m); return ELPH_OK; }
    std::vector<std::thread> pool;
    for (size_t t = 0; t < nthr; ++t) pool.emplace_back(fill, m * t / nthr, m * (t + 1) / nthr);
    for (auto &th : pool) th.join();
    return ELPH_OK;
}

// nvec vectors into dstS (layout S): uploaded when the caller gives them, otherwise the next batch, drawn on the device (no PCIe, no host
// generator).  ncols = 0: site vectors, otherwise field vectors of that many columns
int randn_vectors(elph_handle_s *h, HmcState *st, double *dstS, const double *host, int nvec, int ncols = 0);

int update_model(elph_handle_s *h, HmcState *st);      // update_model! of every chain from the resident fields
// refresh_ϕ!  (HMC.jl:665-692) of every chain: R± (given or the next two batches, R₊ first) into st->R2, ϕ± = Λ⁻¹ Mᵀ R± into st->phi
int refresh_phi(elph_handle_s *h, HmcState *st, const double *Rp, const double *Rm);
int calc_OinvLphi(elph_handle_s *h, HmcState *st, int use_precond, double power, const double *kpm_randn, int64_t *kpm_calls,
                  int64_t *iters, int *flag);
int fa(elph_handle_s *h, HmcState *st, double *out, const double *in, double power);      // fourier_accelerate! of every chain's field vector
int alias_sum(elph_handle_s *h, HmcState *st, double *F);                                  // shared fields: a class's members get the class sum
// dS (+)= dS_b/dx of every chain (calc_dSbdx!); lam_shift: the λ table of the particle-hole shifted action (Langevin), or nullptr
int add_dsb(elph_handle_s *h, HmcState *st, double *dS, int accumulate, const double *lam_shift = nullptr);

// Sums over the lattice are per-slice partials on the device, [rows][L], added in slice order — on the host by sum_rows, in
// special_updates.hip by k_sp_accept.  dot_parts: row k = a_k · b_k of `count` consecutive vectors of n elements (st->part holds 2 nch
// rows); sb_parts: row c = S_b/Δτ of chain c (calc_Sb, PhononAction.jl:11-66).  On a shard both count this rank's own columns.
int dot_parts(elph_handle_s *h, HmcState *st, double *part, const double *a, const double *b, long long n, int count, bool site_vectors = true);
int sb_parts(elph_handle_s *h, HmcState *st, double *part);
inline void sum_rows(const double *p, int rows, int per_row, double *out) {
    for (int r = 0; r < rows; ++r) {
        double s = 0.0;
        for (int q = 0; q < per_row; ++q) s += p[(size_t)r * per_row + q];
        out[r] = s;
    }
}
// the host forms, through st->part: the rows summed and — a shard — added over the ranks.  dots_host: out[count]; calc_Sb: S_b, out[nch]
int dots_host(elph_handle_s *h, HmcState *st, const double *a, const double *b, long long n, int count, double *out, bool site_vectors = true);
int calc_Sb(elph_handle_s *h, HmcState *st, double *out);

}  // namespace hmc
