// Parallel-tempered ensembles (lcf_tempered_*): K rungs of inverse temperature betas[0] = 1 > ... > betas[K-1] >= 0, each
// an ensemble of its own that makes the stretch move on prior * L^beta, and swaps between neighbouring rungs after every
// step.  A driver beside the sampler: the colourings and the draws come from the sampler's generators (rung k under
// seed + k * 0x9E3779B97F4A7C15), the likelihood of a half-step's K * ceil(W / 2) proposals from ONE call of
// lcf_log_likelihood_dev on the engine's stream.  Per half-step: k_t_propose, the likelihood's launches, k_t_accept;
// per step one k_t_swap more, which also stores the step.  One stream, stream order is all the synchronisation.
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

// Half-step, last part: accept iff the proposal's prior is finite, its likelihood is above -inf and
// (n_dim - 1) ln z + beta (ln L(q) - ln L(x)) + (ln prior(q) - ln prior(x)) > ln u.  beta = 0 takes no product at all.
__global__ void k_t_accept(const DevTempered tp, const DrawRec* __restrict__ draws, long long rung_stride) {
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
    if (!(d.zl + dl + (pq - tp.LPR[w]) > d.lnu)) return;
    double* x = tp.X + w * tp.n_dim;
    const double* q = tp.Q + (size_t)idx * tp.n_dim;
    for (int c = 0; c < tp.n_dim; ++c) x[c] = q[c];
    tp.LL[w] = lq;
    tp.LPR[w] = pq;
    tp.nacc[w] += 1;
}

// After both halves of step `step`: the pairs (k, k + 1) with k = step (mod 2) swap slot by slot, then the step is
// stored (chain != null: row `row` of chain[.][n_temps][n_walkers][n_dim] and chain_ll[.][n_temps][n_walkers]).  One
// thread per (rung, slot); the thread of a pair's lower rung does the pair, the upper rung's does nothing.
__global__ void k_t_swap(const DevTempered tp, long long step, double* __restrict__ chain, double* __restrict__ chain_ll,
                         long long row) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tp.n_temps * tp.n_walkers) return;
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
    int64_t chain_cap = 0, chain_steps = 0;
    bool has_state = false;

    ~lcf_tempered() {
        hipSetDevice(device);
        for (void* p : owned) hipFree(p);
        if (chain) hipFree(chain);
        if (chain_ll) hipFree(chain_ll);
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
    const size_t nd = t->dt.n_dim;
    if ((double)steps * (double)per_step * (double)(nd + 1) * 8. > 9e18)
        return fail(LCF_ERR_OUT_OF_MEMORY, "the chain of the run does not fit in an address space");
    int64_t cap = steps;
    size_t free_b = 0, total_b = 0;
    LCF_HIP(hipStreamSynchronize(t->e->stream));
    LCF_HIP(hipMemGetInfo(&free_b, &total_b));
    const auto bytes = [&](int64_t s) { return (size_t)s * per_step * (nd + 1) * sizeof(double); };
    if (keep > 0 && bytes(std::max(steps, 2 * t->chain_cap)) <= free_b / 2) cap = std::max(steps, 2 * t->chain_cap);
    if (bytes(cap) > free_b)
        return fail(LCF_ERR_OUT_OF_MEMORY, "the chain of the run needs " + std::to_string(bytes(cap)) + " bytes of device memory, " +
                                               std::to_string(free_b) + " are free");
    double *c = nullptr, *l = nullptr;
    LCF_HIP(hipMalloc((void**)&c, (size_t)cap * per_step * nd * sizeof(double)));
    if (hipError_t err = hipMalloc((void**)&l, (size_t)cap * per_step * sizeof(double))) {
        hipFree(c);
        return fail(err == hipErrorOutOfMemory ? LCF_ERR_OUT_OF_MEMORY : LCF_ERR_HIP, hipGetErrorString(err));
    }
    if (keep > 0) {
        hipError_t err = hipMemcpy(c, t->chain, (size_t)keep * per_step * nd * sizeof(double), hipMemcpyDeviceToDevice);
        if (!err) err = hipMemcpy(l, t->chain_ll, (size_t)keep * per_step * sizeof(double), hipMemcpyDeviceToDevice);
        if (err) {
            hipFree(c);
            hipFree(l);
            return fail(LCF_ERR_HIP, hipGetErrorString(err));
        }
    }
    if (t->chain) hipFree(t->chain);
    if (t->chain_ll) hipFree(t->chain_ll);
    t->chain = c;
    t->chain_ll = l;
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
    double* d_betas = nullptr;
#define AL(p, n) if ((st = dalloc(&p, n, t->owned)) != LCF_OK) { delete t; return st; }
    AL(d_betas, K); AL(dt.X, nw * nd); AL(dt.LL, nw); AL(dt.LPR, nw); AL(dt.nacc, nw);
    AL(dt.Q, nh * nd); AL(dt.QLL, nh); AL(dt.QPR, nh);
    AL(dt.swap_acc, K); AL(dt.swap_prop, K); AL(dt.err, 1);
    AL(t->d_perm, nw * t->blk_cap); AL(t->d_draws, 2 * nh * t->blk_cap); AL(t->d_items, K); AL(t->d_mean, K);
#undef AL
    dt.betas = d_betas;
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

lcf_status lcf_tempered_run(lcf_tempered* t, int64_t first_step, int64_t n_steps, int32_t store) {
    if (!t || n_steps < 0 || first_step < 0 || store < 0 || store > 2) return fail(LCF_ERR_INVALID_ARGUMENT, "bad argument");
    // (the step is a 32-bit counter word of the generators; far below anything that could overflow the sums below)
    if (first_step > (1LL << 40) || n_steps > (1LL << 40)) return fail(LCF_ERR_INVALID_ARGUMENT, "step numbers beyond 2^40");
    if (!t->has_state) return fail(LCF_ERR_STATE, "lcf_tempered_set_state must be called first");
    lcf_engine* e = t->e;
    const DevTempered& dt = t->dt;
    LCF_HIP(hipSetDevice(e->device));
    int64_t row0 = 0;
    if (store) {
        row0 = store == 2 ? t->chain_steps : 0;
        if (lcf_status st = reserve_chain(t, row0 + n_steps, row0)) return st;
        t->chain_steps = row0;
    }
    hipStream_t st = e->stream;
    const size_t n_prop = (size_t)dt.n_temps * dt.n_half;
    const long long rung_stride = (long long)t->blk_cap * 2 * dt.n_half;
    for (int64_t k0 = 0; k0 < n_steps; k0 += t->blk_cap) {
        const int64_t len = std::min<int64_t>(t->blk_cap, n_steps - k0);
        if (lcf_status r = generate_multi(t->d_items, dt.n_temps, dt.n_walkers, dt.n_half, first_step + k0, len, 0, -1, st))
            return r;
        for (int64_t j = 0; j < len; ++j) {
            for (int half = 0; half < 2; ++half) {
                const DrawRec* draws = t->d_draws + (size_t)(2 * j + half) * dt.n_half;
                hipLaunchKernelGGL(k_t_propose, dim3(blocks_for(n_prop)), dim3(256), 0, st, e->dp, dt, draws, rung_stride);
                if (lcf_status r = lcf_log_likelihood_dev(e, (int64_t)n_prop, dt.Q, dt.QLL, st)) return r;
                hipLaunchKernelGGL(k_t_accept, dim3(blocks_for(n_prop)), dim3(256), 0, st, dt, draws, rung_stride);
            }
            hipLaunchKernelGGL(k_t_swap, dim3(blocks_for(t->rows())), dim3(256), 0, st, dt, (long long)(first_step + k0 + j),
                               store ? t->chain : nullptr, store ? t->chain_ll : nullptr, (long long)(row0 + k0 + j));
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
