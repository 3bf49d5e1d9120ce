// Parallel-tempered ensembles (lcf_tempered_*): K rungs of inverse temperature betas[0] = 1 > ... > betas[K-1] >= 0, each
// an ensemble of its own that makes the stretch move on prior * L^beta, and swaps between neighbouring rungs after every
// step.  A driver beside the sampler: the colourings and the draws come from the sampler's generators (rung k under
// seed + k * 0x9E3779B97F4A7C15), the likelihood of a half-step's K * ceil(W / 2) proposals from ONE call of
// lcf_log_likelihood_dev on the engine's stream.  Per half-step: k_t_propose, the likelihood's launches, k_t_accept;
// per step one k_t_swap more, which also stores the step.  One stream, stream order is all the synchronisation.
// An adapting run (lcf_tempered_run_adaptive) launches k_t_adapt behind the k_t_swap of every odd step: the ladder moves
// on the device, from the swap counts since the last adaptation, and the host reads nothing until the run has ended.
// k_t_stone reduces the stored ln L to the stepping-stone partials of every (pair, batch).
// Moves (lcf_tempered_set_moves): a handle with a list of moves launches k_t_propose_moves in place of k_t_propose, which
// makes the step's move of every rung (stretch, differential evolution or snooker) and leaves the move's log proposal
// factor in FAC for k_t_accept.  Without a list nothing changes: the same kernels, the same numbers.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lcf_internal.h"

namespace {

struct DevTempered {
    int n_temps, n_walkers, n_half, n_dim;
    uint32_t key0, key1;             // of the swap draws: the run's own seed
    const double* betas;             // [n_temps]
    double *X, *LL, *LPR;            // [n_temps][n_walkers][n_dim], [n_temps][n_walkers] x 2: position, ln L, ln prior
    double *Q, *QLL, *QPR;           // [n_temps][n_half][n_dim], [n_temps][n_half] x 2: the proposals of a half-step
    long long* nacc;                 // [n_temps][n_walkers] accepted moves, by slot
    unsigned long long *swap_acc, *swap_prop;   // [n_temps - 1] per pair (k, k + 1)
    int* err;                        // 1: a proposal inside the prior had a NaN likelihood
};

// The moves of lcf_tempered_set_moves, by value to k_t_propose_moves.
struct DevMoves {
    int n;                           // 0: none set (the stretch move through k_t_propose)
    int kind[LCF_MAX_MOVES];         // LCF_MOVE_*
    double cum[LCF_MAX_MOVES];       // cumulative weights, the last exactly 1
    double p0[LCF_MAX_MOVES];        // DE: sigma; snooker: gammas
    double p1[LCF_MAX_MOVES];        // DE: gamma0
};

// ln prior of n rows.
__global__ void k_t_prior(const DevProblem pb, int n, const double* __restrict__ P, double* __restrict__ out) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    out[w] = walker_log_prior(pb, P + (size_t)w * pb.n_dim);
}

// Half-step, first part: the proposals of every rung and their log-priors, one thread per (rung, slot).  `draws`: the
// records of this half-step of rung 0; rung k's lie rung_stride records further per rung.  The slot an odd ensemble
// leaves empty in half 1 (wid = -1) gets a copy of the rung's walker 0: its likelihood is evaluated and ignored.
__global__ void k_t_propose(const DevProblem pb, const DevTempered tp, const DrawRec* __restrict__ draws,
                            long long rung_stride) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tp.n_temps * tp.n_half) return;
    const int k = idx / tp.n_half, i = idx - k * tp.n_half;
    const DrawRec d = draws[(size_t)k * rung_stride + i];
    const double* Xk = tp.X + (size_t)k * tp.n_walkers * tp.n_dim;
    double* q = tp.Q + (size_t)idx * tp.n_dim;
    if (d.wid < 0) {
        for (int c = 0; c < tp.n_dim; ++c) q[c] = Xk[c];
        tp.QPR[idx] = -INFINITY;
        return;
    }
    const double* x = Xk + (size_t)d.wid * tp.n_dim;
    const double* partner = Xk + (size_t)d.pid * tp.n_dim;
    for (int c = 0; c < tp.n_dim; ++c) q[c] = partner[c] - (partner[c] - x[c]) * d.z;
    tp.QPR[idx] = walker_log_prior(pb, q);
}

// Index into a complement of n walkers from a uniform draw.
__device__ inline int pick(double u, int n) { return min((int)(u * (double)n), n - 1); }

// k_t_propose for a handle with moves.  Rung k makes ONE kind of move in both halves of step `step`: the first m with
// um < cum[m], um from Philox(0, step, 4, 0) under the rung's key (seed + k 0x9E3779B97F4A7C15), so a wave diverges only
// where it spans two rungs.  The active walker and ln u stay the draw record's; a stretch move takes its partner and z
// too.  The others draw from P2 = Philox(wid, step, half, 2) and P3 = Philox(wid, step, half, 3) under the same key, and
// their partners c[j] from the complementary colour in the order of the step's permutation (`perm`: rung 0's row of this
// step, rung k's perm_stride entries further per rung):
//   DE       j1 = pick(ua, n), j2 = pick(ub, n - 1) bumped past j1; g = sqrt(-2 ln uc) cos(2 pi ud);
//            q = x + gamma0 (1 + sigma g) (c[j1] - c[j2]); factor 0.
//   snooker  j0, j1 likewise, j2 = pick(uc, n - 2) bumped past the smaller, then the larger of them; z = c[j0],
//            d = x - z, u = d / |d|, q = x + u gammas (u.c[j1] - u.c[j2]); factor (n_dim - 1) (ln |q - z| - ln |d|);
//            |d| = 0 or |q - z| = 0: q = x with log-prior -inf, never accepted.
// FAC gets the factor (a stretch move's (n_dim - 1) ln z); kinds_row (or null) the kind rung k made, [n_temps].
__global__ void k_t_propose_moves(const DevProblem pb, const DevTempered tp, const DevMoves mv,
                                  const DrawRec* __restrict__ draws, long long rung_stride, const int* __restrict__ perm,
                                  long long perm_stride, long long step, int half, double* __restrict__ FAC,
                                  int* __restrict__ kinds_row) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tp.n_temps * tp.n_half) return;
    const int k = idx / tp.n_half, i = idx - k * tp.n_half;
    const DrawRec d = draws[(size_t)k * rung_stride + i];
    const double* Xk = tp.X + (size_t)k * tp.n_walkers * tp.n_dim;
    double* q = tp.Q + (size_t)idx * tp.n_dim;
    const unsigned long long sk =
        (((unsigned long long)tp.key1 << 32) | tp.key0) + (unsigned long long)k * 0x9E3779B97F4A7C15ull;
    const uint32_t k0 = (uint32_t)(sk & 0xffffffffu), k1 = (uint32_t)(sk >> 32);
    uint32_t r[4];
    philox4x32(0u, (uint32_t)step, 4u, 0u, k0, k1, r);
    const double um = u01(r[0], r[1]);
    int m = 0;
    while (m < mv.n - 1 && !(um < mv.cum[m])) ++m;
    const int kind = mv.kind[m];
    if (kinds_row && i == 0 && half == 0) kinds_row[k] = kind;
    if (d.wid < 0) {
        for (int c = 0; c < tp.n_dim; ++c) q[c] = Xk[c];
        tp.QPR[idx] = -INFINITY;
        FAC[idx] = 0.;
        return;
    }
    const double* x = Xk + (size_t)d.wid * tp.n_dim;
    if (kind == LCF_MOVE_STRETCH) {
        const double* partner = Xk + (size_t)d.pid * tp.n_dim;
        for (int c = 0; c < tp.n_dim; ++c) q[c] = partner[c] - (partner[c] - x[c]) * d.z;
        tp.QPR[idx] = walker_log_prior(pb, q);
        FAC[idx] = d.zl;
        return;
    }
    // the complementary colour: colour 0 is the first n_half entries of the permutation and moves in half 0
    const int n = half == 0 ? tp.n_walkers - tp.n_half : tp.n_half;
    const int* other = perm + (size_t)k * perm_stride + (half == 0 ? tp.n_half : 0);
    uint32_t p2[4], p3[4];
    philox4x32((uint32_t)d.wid, (uint32_t)step, (uint32_t)half, 2u, k0, k1, p2);
    philox4x32((uint32_t)d.wid, (uint32_t)step, (uint32_t)half, 3u, k0, k1, p3);
    const double ua = u01(p2[0], p2[1]), ub = u01(p2[2], p2[3]), uc = u01(p3[0], p3[1]), ud = u01(p3[2], p3[3]);
    const int ja = pick(ua, n);
    int jb = pick(ub, n - 1);
    jb += jb >= ja ? 1 : 0;
    const double* ca = Xk + (size_t)other[ja] * tp.n_dim;
    const double* cb = Xk + (size_t)other[jb] * tp.n_dim;
    if (kind == LCF_MOVE_DE) {
        const double g = sqrt(-2. * log(uc)) * cos(6.283185307179586 * ud);
        const double scale = mv.p1[m] * (1. + mv.p0[m] * g);
        for (int c = 0; c < tp.n_dim; ++c) q[c] = x[c] + scale * (ca[c] - cb[c]);
        tp.QPR[idx] = walker_log_prior(pb, q);
        FAC[idx] = 0.;
        return;
    }
    // snooker: ca is z, cb is z1
    int jc = pick(uc, n - 2);
    jc += jc >= min(ja, jb) ? 1 : 0;
    jc += jc >= max(ja, jb) ? 1 : 0;
    const double* cc = Xk + (size_t)other[jc] * tp.n_dim;
    double dd = 0.;
    for (int c = 0; c < tp.n_dim; ++c) {
        const double t = x[c] - ca[c];
        dd += t * t;
    }
    const double norm = sqrt(dd);
    double qn = 0.;
    if (norm > 0.) {
        double a1 = 0., a2 = 0.;
        for (int c = 0; c < tp.n_dim; ++c) {
            const double u = (x[c] - ca[c]) / norm;
            a1 += u * cb[c];
            a2 += u * cc[c];
        }
        const double proj = a1 - a2;
        double qq = 0.;
        for (int c = 0; c < tp.n_dim; ++c) {
            const double u = (x[c] - ca[c]) / norm;
            const double v = x[c] + u * mv.p0[m] * proj;
            const double t = v - ca[c];
            q[c] = v;
            qq += t * t;
        }
        qn = sqrt(qq);
    }
    if (!(norm > 0.) || !(qn > 0.)) {
        for (int c = 0; c < tp.n_dim; ++c) q[c] = x[c];
        tp.QPR[idx] = -INFINITY;
        FAC[idx] = 0.;
        return;
    }
    tp.QPR[idx] = walker_log_prior(pb, q);
    FAC[idx] = (double)(tp.n_dim - 1) * (log(qn) - log(norm));
}

// Half-step, last part: accept iff the proposal's prior is finite, its likelihood is above -inf and
// (n_dim - 1) ln z + beta (ln L(q) - ln L(x)) + (ln prior(q) - ln prior(x)) > ln u.  beta = 0 takes no product at all.
// `fac` (a handle with moves; else null): the log proposal factor of k_t_propose_moves in place of (n_dim - 1) ln z.
__global__ void k_t_accept(const DevTempered tp, const DrawRec* __restrict__ draws, long long rung_stride,
                           const double* __restrict__ fac) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tp.n_temps * tp.n_half) return;
    const int k = idx / tp.n_half, i = idx - k * tp.n_half;
    const DrawRec d = draws[(size_t)k * rung_stride + i];
    if (d.wid < 0) return;
    const double lq = tp.QLL[idx], pq = tp.QPR[idx];
    if (!(pq > -INFINITY && pq < INFINITY)) return;   // outside the prior (whatever its likelihood, a NaN included)
    if (lq != lq) {
        *tp.err = 1;
        return;
    }
    if (!(lq > -INFINITY)) return;
    const size_t w = (size_t)k * tp.n_walkers + d.wid;
    const double beta = tp.betas[k];
    const double dl = beta > 0. ? beta * (lq - tp.LL[w]) : 0.;
    const double factor = fac ? fac[idx] : d.zl;
    if (!(factor + dl + (pq - tp.LPR[w]) > d.lnu)) return;
    double* x = tp.X + w * tp.n_dim;
    const double* q = tp.Q + (size_t)idx * tp.n_dim;
    for (int c = 0; c < tp.n_dim; ++c) x[c] = q[c];
    tp.LL[w] = lq;
    tp.LPR[w] = pq;
    tp.nacc[w] += 1;
}

// After both halves of step `step`: the pairs (k, k + 1) with k = step (mod 2) swap slot by slot, then the step is
// stored (chain != null: row `row` of chain[.][n_temps][n_walkers][n_dim] and chain_ll[.][n_temps][n_walkers]).  One
// thread per (rung, slot); the thread of a pair's lower rung does the pair, the upper rung's does nothing.  Row `row` of
// chain_betas[.][n_temps] gets the ladder the step was sampled under (an adaptation comes behind this launch).
__global__ void k_t_swap(const DevTempered tp, long long step, double* __restrict__ chain, double* __restrict__ chain_ll,
                         double* __restrict__ chain_betas, long long row) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tp.n_temps * tp.n_walkers) return;
    if (chain && idx < tp.n_temps) chain_betas[(size_t)row * tp.n_temps + idx] = tp.betas[idx];
    const int k = idx / tp.n_walkers, i = idx - k * tp.n_walkers;
    const int parity = (int)(step & 1);
    if (k >= 1 && ((k - 1) & 1) == parity) return;            // the upper rung of a pair
    const bool lower = (k & 1) == parity && k + 1 < tp.n_temps;
    const size_t w0 = (size_t)idx, w1 = w0 + tp.n_walkers;
    if (lower) {
        uint32_t r[4];
        philox4x32((uint32_t)i, (uint32_t)step, 3u, (uint32_t)k, tp.key0, tp.key1, r);
        const double lnu = log(u01(r[0], r[1]));
        const double l0 = tp.LL[w0], l1 = tp.LL[w1];
        if ((tp.betas[k] - tp.betas[k + 1]) * (l1 - l0) > lnu) {
            double* a = tp.X + w0 * tp.n_dim;
            double* b = tp.X + w1 * tp.n_dim;
            for (int c = 0; c < tp.n_dim; ++c) {
                const double t = a[c];
                a[c] = b[c];
                b[c] = t;
            }
            tp.LL[w0] = l1;
            tp.LL[w1] = l0;
            const double p0 = tp.LPR[w0];
            tp.LPR[w0] = tp.LPR[w1];
            tp.LPR[w1] = p0;
            atomicAdd(&tp.swap_acc[k], 1ull);
        }
        if (i == 0) tp.swap_prop[k] += (unsigned long long)tp.n_walkers;   // (the pair's only writer in this launch)
    }
    if (!chain) return;
    const size_t per_step = (size_t)tp.n_temps * tp.n_walkers;
    for (int j = 0; j <= (lower ? 1 : 0); ++j) {
        const size_t w = j ? w1 : w0;
        const double* x = tp.X + w * tp.n_dim;
        double* o = chain + ((size_t)row * per_step + w) * tp.n_dim;
        for (int c = 0; c < tp.n_dim; ++c) o[c] = x[c];
        chain_ll[(size_t)row * per_step + w] = tp.LL[w];
    }
}

// Mean ln L of every rung over the stored steps discard .. n_steps - 1 and all walkers, one workgroup per rung, in a
// fixed order: thread t adds the elements t, t + 256, ... (step-major), then a tree over the 256 sums.
__global__ __launch_bounds__(256) void k_t_mean(const double* __restrict__ chain_ll, long long n_steps, int n_temps,
                                                int n_walkers, long long discard, double* __restrict__ out) {
    __shared__ double part[256];
    const int k = blockIdx.x, t = threadIdx.x;
    const long long n = (n_steps - discard) * n_walkers;
    double s = 0.;
    for (long long e = t; e < n; e += 256) {
        const long long st = discard + e / n_walkers;
        s += chain_ll[((size_t)st * n_temps + k) * n_walkers + (size_t)(e % n_walkers)];
    }
    part[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) part[t] += part[t + h];
        __syncthreads();
    }
    if (t == 0) out[k] = part[0] / (double)n;
}

// The ladder after the swaps of an odd step (one workgroup of 64 threads; n_temps <= 64).  Nothing happens unless every
// pair was offered since the last adaptation.  A_k: the fraction of pair k's swaps accepted since then;
// kappa = lag / (t + lag) / time; dT_k = (1 / beta_{k+1} - 1 / beta_k) exp(kappa (A_k - A_{k+1})) for k = 0 .. K - 3, by
// the lanes; then ONE lane, left to right: T_0 = 1, T_{k+1} = T_k + dT_k, beta_{k+1} = 1 / T_{k+1}.  beta_0 and
// beta_{K-1} (= 0: the last gap is no free variable) are never written.  Then seen := the counts.
__global__ __launch_bounds__(64) void k_t_adapt(int n_temps, double* __restrict__ betas,
                                                const unsigned long long* __restrict__ swap_acc,
                                                const unsigned long long* __restrict__ swap_prop,
                                                unsigned long long* __restrict__ seen_acc,
                                                unsigned long long* __restrict__ seen_prop, double lag, double time,
                                                long long t_adapt) {
    __shared__ double A[64], dT[64];
    __shared__ int closed;
    const int t = threadIdx.x, pairs = n_temps - 1;
    if (t == 0) closed = 0;
    __syncthreads();
    unsigned long long acc = 0, prop = 0;
    if (t < pairs) {
        acc = swap_acc[t];
        prop = swap_prop[t];
        const unsigned long long dp = prop - seen_prop[t];
        if (dp == 0)
            closed = 1;   // (every writer writes the same value)
        else
            A[t] = (double)(acc - seen_acc[t]) / (double)dp;
    }
    __syncthreads();
    if (closed) return;   // (uniform: read behind the barrier)
    const double kappa = lag / ((double)t_adapt + lag) / time;
    if (t < pairs - 1) dT[t] = (1. / betas[t + 1] - 1. / betas[t]) * exp(kappa * (A[t] - A[t + 1]));
    __syncthreads();
    if (t == 0) {
        double T = 1.;
        for (int k = 0; k < pairs - 1; ++k) {
            T += dT[k];
            betas[k + 1] = 1. / T;
        }
    }
    if (t < pairs) {
        seen_acc[t] = acc;
        seen_prop[t] = prop;
    }
}

// Stepping stones: one workgroup per (pair k, batch b) over ln L of rung k + 1, the stored steps s0 + (b n) / B ..
// s0 + ((b + 1) n) / B - 1 (n = n_steps - s0) and all walkers, in the fixed order of k_t_mean: thread t takes the
// elements t, t + 256, ..., then a tree.  Two passes: the maximum m, then sum exp((beta_k - beta_{k+1}) (ln L - m)).
// Idle threads hold the identities (-inf, 0); a batch whose maximum is -inf has sum 0.  The ladder is row s0 of
// chain_betas.  out: max, sum, count, each [n_temps - 1][n_batches].
__global__ __launch_bounds__(256) void k_t_stone(const double* __restrict__ chain_ll, const double* __restrict__ chain_betas,
                                                 long long n_steps, int n_temps, int n_walkers, long long s0, int n_batches,
                                                 double* __restrict__ out) {
    __shared__ double part[256];
    const int k = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const long long nk = n_steps - s0;
    const long long lo = s0 + ((long long)b * nk) / n_batches, hi = s0 + ((long long)(b + 1) * nk) / n_batches;
    const long long n = (hi - lo) * n_walkers;
    const double db = chain_betas[(size_t)s0 * n_temps + k] - chain_betas[(size_t)s0 * n_temps + k + 1];
    const auto at = [&](long long e) {
        return chain_ll[((size_t)(lo + e / n_walkers) * n_temps + (k + 1)) * n_walkers + (size_t)(e % n_walkers)];
    };
    double m = -INFINITY;
    for (long long e = t; e < n; e += 256) m = fmax(m, at(e));
    part[t] = m;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) part[t] = fmax(part[t], part[t + h]);
        __syncthreads();
    }
    m = part[0];
    __syncthreads();
    double s = 0.;
    if (m > -INFINITY)
        for (long long e = t; e < n; e += 256) s += exp(db * (at(e) - m));
    part[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) part[t] += part[t + h];
        __syncthreads();
    }
    if (t == 0) {
        const size_t o = (size_t)k * n_batches + b, plane = (size_t)(n_temps - 1) * n_batches;
        out[o] = m;
        out[plane + o] = part[0];
        out[2 * plane + o] = (double)n;
    }
}

}  // namespace

struct lcf_tempered {
    lcf_engine* e = nullptr;
    int device = 0;
    DevTempered dt{};
    double a = 2.;
    std::vector<void*> owned;
    // the state-independent draws of a run come in blocks of blk_cap steps (one buffer: the generation of the next block
    // is enqueued behind the last reader of this one)
    int64_t blk_cap = 0;
    int* d_perm = nullptr;          // [n_temps][blk_cap][n_walkers]
    DrawRec* d_draws = nullptr;     // [n_temps][blk_cap][2][n_half]
    GenItem* d_items = nullptr;     // [n_temps]
    double* d_mean = nullptr;       // [n_temps]
    double *chain = nullptr, *chain_ll = nullptr;
    double* chain_betas = nullptr;  // [chain_cap][n_temps]: the ladder every stored step was sampled under
    int64_t chain_cap = 0, chain_steps = 0;
    bool has_state = false;
    // adaptation (k_t_adapt): the ladder dt.betas points to, writable, and the swap counts at the last adaptation
    double* d_betas = nullptr;                                       // [n_temps]
    unsigned long long *seen_acc = nullptr, *seen_prop = nullptr;    // [n_temps - 1] used
    bool ends_at_prior = false;     // betas[n_temps - 1] == 0 (never written after create)
    bool window_open = false;       // the last run adapted: the next adapting run goes on in its window
    double* d_stone = nullptr;      // [3][n_temps - 1][stone_cap] of k_t_stone
    int64_t stone_cap = 0;
    // moves (lcf_tempered_set_moves)
    DevMoves mv{};
    double* d_fac = nullptr;        // [n_temps][n_half] log proposal factors of a half-step, beside QLL / QPR
    int* chain_kinds = nullptr;     // [chain_cap][n_temps]: the kind of move every stored step made (zero: stretch)
    bool kinds_written = false;     // a run with moves has stored kinds: a run without clears its rows

    ~lcf_tempered() {
        hipSetDevice(device);
        for (void* p : owned) hipFree(p);
        if (chain) hipFree(chain);
        if (chain_ll) hipFree(chain_ll);
        if (chain_betas) hipFree(chain_betas);
        if (chain_kinds) hipFree(chain_kinds);
        if (d_stone) hipFree(d_stone);
    }
    size_t rows() const { return (size_t)dt.n_temps * dt.n_walkers; }
};

namespace {

unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

// Room for `steps` stored steps, the first `keep` of the present chain kept.  The size is checked against the device's
// free memory before anything is allocated.
lcf_status reserve_chain(lcf_tempered* t, int64_t steps, int64_t keep) {
    if (steps <= t->chain_cap) return LCF_OK;
    const size_t per_step = t->rows();
    const size_t nd = t->dt.n_dim, K = t->dt.n_temps;
    if ((double)steps * (double)per_step * (double)(nd + 1) * 8. > 9e18)
        return fail(LCF_ERR_OUT_OF_MEMORY, "the chain of the run does not fit in an address space");
    int64_t cap = steps;
    size_t free_b = 0, total_b = 0;
    LCF_HIP(hipStreamSynchronize(t->e->stream));
    LCF_HIP(hipMemGetInfo(&free_b, &total_b));
    const auto bytes = [&](int64_t s) { return (size_t)s * (per_step * (nd + 1) + 2 * K) * sizeof(double); };
    if (keep > 0 && bytes(std::max(steps, 2 * t->chain_cap)) <= free_b / 2) cap = std::max(steps, 2 * t->chain_cap);
    if (bytes(cap) > free_b)
        return fail(LCF_ERR_OUT_OF_MEMORY, "the chain of the run needs " + std::to_string(bytes(cap)) + " bytes of device memory, " +
                                               std::to_string(free_b) + " are free");
    double *c = nullptr, *l = nullptr, *b = nullptr;
    int* m = nullptr;
    LCF_HIP(hipMalloc((void**)&c, (size_t)cap * per_step * nd * sizeof(double)));
    hipError_t err = hipMalloc((void**)&l, (size_t)cap * per_step * sizeof(double));
    if (!err) err = hipMalloc((void**)&b, (size_t)cap * K * sizeof(double));
    if (!err) err = hipMalloc((void**)&m, (size_t)cap * K * sizeof(int));
    if (err) {
        hipFree(c);
        if (l) hipFree(l);
        if (b) hipFree(b);
        return fail(err == hipErrorOutOfMemory ? LCF_ERR_OUT_OF_MEMORY : LCF_ERR_HIP, hipGetErrorString(err));
    }
    err = hipMemset(m, 0, (size_t)cap * K * sizeof(int));
    if (!err && keep > 0) err = hipMemcpy(m, t->chain_kinds, (size_t)keep * K * sizeof(int), hipMemcpyDeviceToDevice);
    if (err) {
        hipFree(c);
        hipFree(l);
        hipFree(b);
        hipFree(m);
        return fail(LCF_ERR_HIP, hipGetErrorString(err));
    }
    if (keep > 0) {
        err = hipMemcpy(c, t->chain, (size_t)keep * per_step * nd * sizeof(double), hipMemcpyDeviceToDevice);
        if (!err) err = hipMemcpy(l, t->chain_ll, (size_t)keep * per_step * sizeof(double), hipMemcpyDeviceToDevice);
        if (!err) err = hipMemcpy(b, t->chain_betas, (size_t)keep * K * sizeof(double), hipMemcpyDeviceToDevice);
        if (err) {
            hipFree(c);
            hipFree(l);
            hipFree(b);
            hipFree(m);
            return fail(LCF_ERR_HIP, hipGetErrorString(err));
        }
    }
    if (t->chain) hipFree(t->chain);
    if (t->chain_ll) hipFree(t->chain_ll);
    if (t->chain_betas) hipFree(t->chain_betas);
    if (t->chain_kinds) hipFree(t->chain_kinds);
    t->chain_kinds = m;
    t->chain = c;
    t->chain_ll = l;
    t->chain_betas = b;
    t->chain_cap = cap;
    return LCF_OK;
}

}  // namespace

extern "C" {

lcf_status lcf_tempered_create(lcf_engine* e, int32_t n_temps, const double* betas, int32_t n_walkers, uint64_t seed,
                               double a, lcf_tempered** out) {
    if (!e || !out || !betas) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const int nd = e->dp.n_dim;
    if (n_temps < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "n_temps must be >= 1");
    if (n_temps > 64) return fail(LCF_ERR_UNSUPPORTED, "at most 64 rungs");
    if (n_walkers < 2 * nd) return fail(LCF_ERR_INVALID_ARGUMENT, "n_walkers must be at least twice the number of dimensions");
    if (n_walkers > 16384) return fail(LCF_ERR_UNSUPPORTED, "at most 16384 walkers per rung");
    if (!(a > 1.)) return fail(LCF_ERR_INVALID_ARGUMENT, "stretch scale a must be > 1");
    if (betas[0] != 1.) return fail(LCF_ERR_INVALID_ARGUMENT, "betas must start at 1");
    for (int k = 0; k < n_temps; ++k)
        if (!(betas[k] >= 0.) || (k > 0 && !(betas[k] <= betas[k - 1])))   // (equal neighbours: every swap is accepted)
            return fail(LCF_ERR_INVALID_ARGUMENT, "betas must descend and stay >= 0");
    LCF_HIP(hipSetDevice(e->device));
    auto* t = new lcf_tempered();
    t->e = e;
    t->device = e->device;
    t->a = a;
    DevTempered& dt = t->dt;
    dt.n_temps = n_temps;
    dt.n_walkers = n_walkers;
    dt.n_half = (n_walkers + 1) / 2;
    dt.n_dim = nd;
    dt.key0 = (uint32_t)(seed & 0xffffffffu);
    dt.key1 = (uint32_t)(seed >> 32);
    const size_t K = n_temps, nw = K * n_walkers, nh = K * dt.n_half;
    // about 2^19 draw records (28 MiB) per block of steps
    t->blk_cap = std::max<int64_t>(1, std::min<int64_t>(256, (int64_t)(1 << 19) / (int64_t)nw));
    lcf_status st;
    double*& d_betas = t->d_betas;
#define AL(p, n) if ((st = dalloc(&p, n, t->owned)) != LCF_OK) { delete t; return st; }
    AL(d_betas, K); AL(dt.X, nw * nd); AL(dt.LL, nw); AL(dt.LPR, nw); AL(dt.nacc, nw);
    AL(dt.Q, nh * nd); AL(dt.QLL, nh); AL(dt.QPR, nh);
    AL(dt.swap_acc, K); AL(dt.swap_prop, K); AL(dt.err, 1);
    AL(t->d_perm, nw * t->blk_cap); AL(t->d_draws, 2 * nh * t->blk_cap); AL(t->d_items, K); AL(t->d_mean, K);
    AL(t->seen_acc, K); AL(t->seen_prop, K); AL(t->d_fac, nh);
#undef AL
    dt.betas = d_betas;
    t->ends_at_prior = betas[n_temps - 1] == 0.;
    std::vector<GenItem> items(K);
    for (size_t k = 0; k < K; ++k) {
        const uint64_t sk = seed + (uint64_t)k * 0x9E3779B97F4A7C15ull;   // (mod 2^64)
        GenItem& it = items[k];
        std::memset(&it, 0, sizeof(it));
        it.key0 = (uint32_t)(sk & 0xffffffffu);
        it.key1 = (uint32_t)(sk >> 32);
        it.n_dim = nd;
        it.a = a;
        it.perm[0] = t->d_perm + k * (size_t)t->blk_cap * n_walkers;
        it.draws[0] = t->d_draws + k * (size_t)t->blk_cap * 2 * dt.n_half;
    }
    hipError_t err = hipMemcpy(t->d_items, items.data(), K * sizeof(GenItem), hipMemcpyHostToDevice);
    if (!err) err = hipMemcpy(d_betas, betas, K * sizeof(double), hipMemcpyHostToDevice);
    if (!err) err = hipMemset(dt.nacc, 0, nw * sizeof(long long));
    if (!err) err = hipMemset(dt.swap_acc, 0, K * sizeof(unsigned long long));
    if (!err) err = hipMemset(dt.swap_prop, 0, K * sizeof(unsigned long long));
    if (!err) err = hipMemset(t->seen_acc, 0, K * sizeof(unsigned long long));
    if (!err) err = hipMemset(t->seen_prop, 0, K * sizeof(unsigned long long));
    if (!err) err = hipMemset(dt.err, 0, sizeof(int));
    if (err) {
        delete t;
        return fail(LCF_ERR_HIP, hipGetErrorString(err));
    }
    // the likelihood's scratch, once: the start state is the largest block this driver ever evaluates
    if ((st = e->reserve((int64_t)nw)) != LCF_OK) {
        delete t;
        return st;
    }
    *out = t;
    return LCF_OK;
}

void lcf_tempered_destroy(lcf_tempered* t) { delete t; }

lcf_status lcf_tempered_set_state(lcf_tempered* t, const double* coords) {
    if (!t || !coords) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    lcf_engine* e = t->e;
    const DevTempered& dt = t->dt;
    const size_t nw = t->rows();
    LCF_HIP(hipSetDevice(e->device));
    LCF_HIP(hipStreamSynchronize(e->stream));
    t->has_state = false;
    LCF_HIP(hipMemcpyAsync(dt.X, coords, nw * dt.n_dim * sizeof(double), hipMemcpyHostToDevice, e->stream));
    if (lcf_status st = lcf_log_likelihood_dev(e, (int64_t)nw, dt.X, dt.LL, e->stream)) return st;
    hipLaunchKernelGGL(k_t_prior, dim3(blocks_for(nw)), dim3(256), 0, e->stream, e->dp, (int)nw, dt.X, dt.LPR);
    LCF_HIP(hipGetLastError());
    LCF_HIP(hipMemsetAsync(dt.nacc, 0, nw * sizeof(long long), e->stream));
    LCF_HIP(hipMemsetAsync(dt.swap_acc, 0, dt.n_temps * sizeof(unsigned long long), e->stream));
    LCF_HIP(hipMemsetAsync(dt.swap_prop, 0, dt.n_temps * sizeof(unsigned long long), e->stream));
    LCF_HIP(hipMemsetAsync(t->seen_acc, 0, dt.n_temps * sizeof(unsigned long long), e->stream));   // (the window too)
    LCF_HIP(hipMemsetAsync(t->seen_prop, 0, dt.n_temps * sizeof(unsigned long long), e->stream));
    LCF_HIP(hipMemsetAsync(dt.err, 0, sizeof(int), e->stream));
    std::vector<double> ll(nw), lpr(nw);
    LCF_HIP(hipMemcpyAsync(ll.data(), dt.LL, nw * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    LCF_HIP(hipMemcpyAsync(lpr.data(), dt.LPR, nw * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    LCF_HIP(hipStreamSynchronize(e->stream));
    for (size_t w = 0; w < nw; ++w) {
        if (!std::isfinite(lpr[w]))
            return fail(LCF_ERR_STATE, "start row " + std::to_string(w % dt.n_walkers) + " of rung " +
                                           std::to_string(w / dt.n_walkers) + " is outside the prior");
        if (std::isnan(ll[w]))
            return fail(LCF_ERR_NAN_LOGPROB, "the likelihood of start row " + std::to_string(w % dt.n_walkers) + " of rung " +
                                                 std::to_string(w / dt.n_walkers) + " is NaN");
    }
    t->has_state = true;
    return LCF_OK;
}

lcf_status lcf_tempered_get_state(lcf_tempered* t, double* coords, double* lnL, double* lnpr) {
    if (!t) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (!t->has_state) return fail(LCF_ERR_STATE, "lcf_tempered_set_state must be called first");
    const DevTempered& dt = t->dt;
    const size_t nw = t->rows();
    LCF_HIP(hipSetDevice(t->device));
    LCF_HIP(hipStreamSynchronize(t->e->stream));
    if (coords) LCF_HIP(hipMemcpy(coords, dt.X, nw * dt.n_dim * sizeof(double), hipMemcpyDeviceToHost));
    if (lnL) LCF_HIP(hipMemcpy(lnL, dt.LL, nw * sizeof(double), hipMemcpyDeviceToHost));
    if (lnpr) LCF_HIP(hipMemcpy(lnpr, dt.LPR, nw * sizeof(double), hipMemcpyDeviceToHost));
    return LCF_OK;
}

}  // extern "C"

namespace {

// The run of lcf_tempered_run (adapt = false) and of lcf_tempered_run_adaptive.
lcf_status run_steps(lcf_tempered* t, int64_t first_step, int64_t n_steps, int32_t store, bool adapt, double lag,
                     double time, int64_t t0) {
    if (!t || n_steps < 0 || first_step < 0 || store < 0 || store > 2) return fail(LCF_ERR_INVALID_ARGUMENT, "bad argument");
    // (the step is a 32-bit counter word of the generators; far below anything that could overflow the sums below)
    if (first_step > (1LL << 40) || n_steps > (1LL << 40)) return fail(LCF_ERR_INVALID_ARGUMENT, "step numbers beyond 2^40");
    const DevTempered& dt = t->dt;
    if (adapt) {
        if (dt.n_temps < 3 || !t->ends_at_prior)
            return fail(LCF_ERR_INVALID_ARGUMENT, "an adaptive ladder needs at least 3 rungs and a last rung at beta = 0");
        if (!(lag > 0.) || !(time > 0.) || !std::isfinite(lag) || !std::isfinite(time) || t0 < 0 || t0 > (1LL << 40))
            return fail(LCF_ERR_INVALID_ARGUMENT, "adaptation needs finite lag > 0 and time > 0, and 0 <= t0 <= 2^40");
    }
    if (!t->has_state) return fail(LCF_ERR_STATE, "lcf_tempered_set_state must be called first");
    lcf_engine* e = t->e;
    LCF_HIP(hipSetDevice(e->device));
    int64_t row0 = 0;
    if (store) {
        row0 = store == 2 ? t->chain_steps : 0;
        if (lcf_status st = reserve_chain(t, row0 + n_steps, row0)) return st;
        t->chain_steps = row0;
    }
    hipStream_t st = e->stream;
    if (adapt && !t->window_open) {   // after a frozen run (or none): the window starts here
        const size_t pb = (size_t)(dt.n_temps - 1) * sizeof(unsigned long long);
        LCF_HIP(hipMemcpyAsync(t->seen_acc, dt.swap_acc, pb, hipMemcpyDeviceToDevice, st));
        LCF_HIP(hipMemcpyAsync(t->seen_prop, dt.swap_prop, pb, hipMemcpyDeviceToDevice, st));
    }
    t->window_open = adapt;
    const size_t n_prop = (size_t)dt.n_temps * dt.n_half;
    const long long rung_stride = (long long)t->blk_cap * 2 * dt.n_half;
    const DevMoves& mv = t->mv;
    const long long perm_stride = (long long)t->blk_cap * dt.n_walkers;
    const double* fac = mv.n ? t->d_fac : nullptr;
    if (store && mv.n) t->kinds_written = true;
    if (store && !mv.n && t->kinds_written && n_steps > 0)   // (rows a run with moves may have left: stretch moves now)
        LCF_HIP(hipMemsetAsync(t->chain_kinds + (size_t)row0 * dt.n_temps, 0, (size_t)n_steps * dt.n_temps * sizeof(int), st));
    for (int64_t k0 = 0; k0 < n_steps; k0 += t->blk_cap) {
        const int64_t len = std::min<int64_t>(t->blk_cap, n_steps - k0);
        if (lcf_status r = generate_multi(t->d_items, dt.n_temps, dt.n_walkers, dt.n_half, first_step + k0, len, 0, -1, st))
            return r;
        for (int64_t j = 0; j < len; ++j) {
            for (int half = 0; half < 2; ++half) {
                const DrawRec* draws = t->d_draws + (size_t)(2 * j + half) * dt.n_half;
                if (mv.n)
                    hipLaunchKernelGGL(k_t_propose_moves, dim3(blocks_for(n_prop)), dim3(256), 0, st, e->dp, dt, mv, draws,
                                       rung_stride, t->d_perm + (size_t)j * dt.n_walkers, perm_stride,
                                       (long long)(first_step + k0 + j), half, t->d_fac,
                                       store ? t->chain_kinds + (size_t)(row0 + k0 + j) * dt.n_temps : nullptr);
                else
                    hipLaunchKernelGGL(k_t_propose, dim3(blocks_for(n_prop)), dim3(256), 0, st, e->dp, dt, draws, rung_stride);
                if (lcf_status r = lcf_log_likelihood_dev(e, (int64_t)n_prop, dt.Q, dt.QLL, st)) return r;
                hipLaunchKernelGGL(k_t_accept, dim3(blocks_for(n_prop)), dim3(256), 0, st, dt, draws, rung_stride, fac);
            }
            const int64_t step = first_step + k0 + j;
            hipLaunchKernelGGL(k_t_swap, dim3(blocks_for(t->rows())), dim3(256), 0, st, dt, (long long)step,
                               store ? t->chain : nullptr, store ? t->chain_ll : nullptr, store ? t->chain_betas : nullptr,
                               (long long)(row0 + k0 + j));
            if (adapt && (step & 1))
                hipLaunchKernelGGL(k_t_adapt, dim3(1), dim3(64), 0, st, dt.n_temps, t->d_betas, dt.swap_acc, dt.swap_prop,
                                   t->seen_acc, t->seen_prop, lag, time, (long long)(t0 + k0 + j + 1));
        }
        LCF_HIP(hipGetLastError());
    }
    int err = 0;
    LCF_HIP(hipMemcpyAsync(&err, dt.err, sizeof(int), hipMemcpyDeviceToHost, st));
    LCF_HIP(hipStreamSynchronize(st));
    // (a run that met a NaN stores nothing: the chain stays what it was before the run, or empty when it was replaced)
    if (err) return fail(LCF_ERR_NAN_LOGPROB, "a proposal inside the prior had a NaN likelihood");
    if (store) t->chain_steps = row0 + n_steps;
    return LCF_OK;
}

}  // namespace

extern "C" {

lcf_status lcf_tempered_run(lcf_tempered* t, int64_t first_step, int64_t n_steps, int32_t store) {
    return run_steps(t, first_step, n_steps, store, false, 0., 0., 0);
}

lcf_status lcf_tempered_run_adaptive(lcf_tempered* t, int64_t first_step, int64_t n_steps, int32_t store, double lag,
                                     double time, int64_t t0) {
    return run_steps(t, first_step, n_steps, store, true, lag, time, t0);
}

lcf_status lcf_tempered_set_moves(lcf_tempered* t, int32_t n_moves, const int32_t* kinds, const double* cum_weights,
                                  const double* params) {
    if (!t) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (n_moves < 0 || n_moves > LCF_MAX_MOVES)
        return fail(LCF_ERR_INVALID_ARGUMENT, "n_moves must be from 0 to " + std::to_string(LCF_MAX_MOVES));
    if (n_moves > 0 && (!kinds || !cum_weights || !params)) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    DevMoves mv{};
    mv.n = n_moves;
    const int complement = t->dt.n_walkers - t->dt.n_half;   // the smaller colour: what the first half draws partners from
    for (int m = 0; m < n_moves; ++m) {
        const double p0 = params[2 * m], p1 = params[2 * m + 1], w = cum_weights[m];
        const std::string at = "move " + std::to_string(m) + ": ";
        if (!(w > 0.) || !(w <= 1.) || (m > 0 && !(w >= cum_weights[m - 1])))
            return fail(LCF_ERR_INVALID_ARGUMENT, at + "cum_weights must ascend within (0, 1]");
        switch (kinds[m]) {
            case LCF_MOVE_STRETCH:
                break;
            case LCF_MOVE_DE:
                if (!(p0 >= 0.) || !std::isfinite(p0)) return fail(LCF_ERR_INVALID_ARGUMENT, at + "sigma must be finite and >= 0");
                if (!(p1 > 0.) || !std::isfinite(p1)) return fail(LCF_ERR_INVALID_ARGUMENT, at + "gamma0 must be finite and > 0");
                if (complement < 2)
                    return fail(LCF_ERR_INVALID_ARGUMENT, at + "the DE move needs 2 partners in either colour: at least 4 walkers");
                break;
            case LCF_MOVE_SNOOKER:
                if (!(p0 > 0.) || !std::isfinite(p0)) return fail(LCF_ERR_INVALID_ARGUMENT, at + "gammas must be finite and > 0");
                if (complement < 3)
                    return fail(LCF_ERR_INVALID_ARGUMENT, at + "the snooker move needs 3 partners in either colour: at least 6 walkers");
                break;
            default:
                return fail(LCF_ERR_INVALID_ARGUMENT, at + "unknown kind " + std::to_string(kinds[m]));
        }
        mv.kind[m] = kinds[m];
        mv.cum[m] = w;
        mv.p0[m] = p0;
        mv.p1[m] = p1;
    }
    if (n_moves > 0 && cum_weights[n_moves - 1] != 1.)
        return fail(LCF_ERR_INVALID_ARGUMENT, "cum_weights must end at exactly 1");
    LCF_HIP(hipSetDevice(t->device));
    LCF_HIP(hipStreamSynchronize(t->e->stream));
    t->mv = mv;
    return LCF_OK;
}

lcf_status lcf_tempered_get_move_history(lcf_tempered* t, int32_t* kinds) {
    if (!t || !kinds) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (t->chain_steps == 0) return fail(LCF_ERR_STATE, "no chain is stored");
    LCF_HIP(hipSetDevice(t->device));
    LCF_HIP(hipStreamSynchronize(t->e->stream));
    LCF_HIP(hipMemcpy(kinds, t->chain_kinds, (size_t)t->chain_steps * t->dt.n_temps * sizeof(int32_t), hipMemcpyDeviceToHost));
    return LCF_OK;
}

lcf_status lcf_tempered_get_betas(lcf_tempered* t, double* betas) {
    if (!t || !betas) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    LCF_HIP(hipSetDevice(t->device));
    LCF_HIP(hipStreamSynchronize(t->e->stream));
    LCF_HIP(hipMemcpy(betas, t->d_betas, (size_t)t->dt.n_temps * sizeof(double), hipMemcpyDeviceToHost));
    return LCF_OK;
}

lcf_status lcf_tempered_get_beta_history(lcf_tempered* t, double* betas) {
    if (!t || !betas) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (t->chain_steps == 0) return fail(LCF_ERR_STATE, "no chain is stored");
    LCF_HIP(hipSetDevice(t->device));
    LCF_HIP(hipStreamSynchronize(t->e->stream));
    LCF_HIP(hipMemcpy(betas, t->chain_betas, (size_t)t->chain_steps * t->dt.n_temps * sizeof(double), hipMemcpyDeviceToHost));
    return LCF_OK;
}

lcf_status lcf_tempered_stepping_stones(lcf_tempered* t, int64_t discard, int32_t n_batches, double* max, double* sum,
                                        double* count) {
    if (!t || !max || !sum || !count) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (t->dt.n_temps < 2) return fail(LCF_ERR_INVALID_ARGUMENT, "stepping stones need at least 2 rungs");
    if (t->chain_steps == 0) return fail(LCF_ERR_STATE, "no chain is stored");
    if (discard < 0 || discard >= t->chain_steps) return fail(LCF_ERR_INVALID_ARGUMENT, "discard leaves no stored step");
    if (n_batches < 1 || n_batches > t->chain_steps - discard)
        return fail(LCF_ERR_INVALID_ARGUMENT, "n_batches must be from 1 to the number of stored steps kept");
    if (n_batches > 65535) return fail(LCF_ERR_UNSUPPORTED, "at most 65535 batches");
    const DevTempered& dt = t->dt;
    const size_t plane = (size_t)(dt.n_temps - 1) * n_batches;
    hipStream_t st = t->e->stream;
    LCF_HIP(hipSetDevice(t->device));
    if (n_batches > t->stone_cap) {
        LCF_HIP(hipStreamSynchronize(st));
        if (t->d_stone) hipFree(t->d_stone);
        t->d_stone = nullptr;
        t->stone_cap = 0;
        LCF_HIP(hipMalloc((void**)&t->d_stone, 3 * plane * sizeof(double)));
        t->stone_cap = n_batches;
    }
    hipLaunchKernelGGL(k_t_stone, dim3((unsigned)(dt.n_temps - 1), (unsigned)n_batches), dim3(256), 0, st, t->chain_ll,
                       t->chain_betas, (long long)t->chain_steps, dt.n_temps, dt.n_walkers, (long long)discard,
                       (int)n_batches, t->d_stone);
    LCF_HIP(hipGetLastError());
    LCF_HIP(hipMemcpyAsync(max, t->d_stone, plane * sizeof(double), hipMemcpyDeviceToHost, st));
    LCF_HIP(hipMemcpyAsync(sum, t->d_stone + plane, plane * sizeof(double), hipMemcpyDeviceToHost, st));
    LCF_HIP(hipMemcpyAsync(count, t->d_stone + 2 * plane, plane * sizeof(double), hipMemcpyDeviceToHost, st));
    LCF_HIP(hipStreamSynchronize(st));
    return LCF_OK;
}

lcf_status lcf_tempered_get_chain(lcf_tempered* t, double* chain, double* lnL) {
    if (!t) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (t->chain_steps == 0) return fail(LCF_ERR_STATE, "no chain is stored");
    const size_t n = (size_t)t->chain_steps * t->rows();
    LCF_HIP(hipSetDevice(t->device));
    LCF_HIP(hipStreamSynchronize(t->e->stream));
    if (chain) LCF_HIP(hipMemcpy(chain, t->chain, n * t->dt.n_dim * sizeof(double), hipMemcpyDeviceToHost));
    if (lnL) LCF_HIP(hipMemcpy(lnL, t->chain_ll, n * sizeof(double), hipMemcpyDeviceToHost));
    return LCF_OK;
}

lcf_status lcf_tempered_get_counts(lcf_tempered* t, int64_t* n_accepted, int64_t* swaps_accepted, int64_t* swaps_proposed) {
    if (!t) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    const DevTempered& dt = t->dt;
    const size_t pairs = (size_t)dt.n_temps - 1;
    LCF_HIP(hipSetDevice(t->device));
    LCF_HIP(hipStreamSynchronize(t->e->stream));
    if (n_accepted) LCF_HIP(hipMemcpy(n_accepted, dt.nacc, t->rows() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (swaps_accepted && pairs) LCF_HIP(hipMemcpy(swaps_accepted, dt.swap_acc, pairs * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (swaps_proposed && pairs) LCF_HIP(hipMemcpy(swaps_proposed, dt.swap_prop, pairs * sizeof(int64_t), hipMemcpyDeviceToHost));
    return LCF_OK;
}

lcf_status lcf_tempered_mean_loglike(lcf_tempered* t, int64_t discard, double* out) {
    if (!t || !out) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (t->chain_steps == 0) return fail(LCF_ERR_STATE, "no chain is stored");
    if (discard < 0 || discard >= t->chain_steps) return fail(LCF_ERR_INVALID_ARGUMENT, "discard leaves no stored step");
    const DevTempered& dt = t->dt;
    hipStream_t st = t->e->stream;
    LCF_HIP(hipSetDevice(t->device));
    hipLaunchKernelGGL(k_t_mean, dim3((unsigned)dt.n_temps), dim3(256), 0, st, t->chain_ll, (long long)t->chain_steps,
                       dt.n_temps, dt.n_walkers, (long long)discard, t->d_mean);
    LCF_HIP(hipGetLastError());
    LCF_HIP(hipMemcpyAsync(out, t->d_mean, dt.n_temps * sizeof(double), hipMemcpyDeviceToHost, st));
    LCF_HIP(hipStreamSynchronize(st));
    return LCF_OK;
}

}  // extern "C"
