// Chain history on gfx950: the numbers of the chain plots of lightcurve_mcmc(..., show=True) (reference
// fitting.py:135-158) -- per kept step the order statistics of the ensemble behind its percentiles and the number of
// walkers that moved, and the (step bin, value bin) raster of every walker's trace -- from a stored chain
// [step][walker][dim] and its log-probabilities [step][walker], read where they lie.
//
//   k_history_steps   workgroup = one kept step.  Lanes are the ELEMENTS of the step's row block (n_w * n_dim
//                     consecutive doubles) for the moved test: the 64-bit pattern of every element against the one a
//                     stored step before, a walker with any difference flagged in LDS, the flags counted with a wave
//                     ballot / popcount and one integer add per wave.  Then column by column (the log-probability
//                     last): the walkers' order-preserving keys (corner_key; every NaN above +inf, the padding above
//                     every NaN) in LDS, a bitonic sort on the power of two at or above n_w, and the 2 n_q order
//                     statistics around h = (n_valid - 1) q / 100 picked.  The host interpolates between them.
//   k_history_raster  workgroup = (step bin, chunk of its samples), lanes = (step, walker) samples.  A lane finds the
//                     value bin of every column of its row (corner_bin, the rule of k_corner_hist) and adds to 32-bit
//                     counters in LDS, merged into the 64-bit counters in device memory with integer atomics.
//
// All results are integers or copies of input values: nothing depends on the order in which workgroups arrive or on the
// chunks, there is no floating-point atomic and no workgroup waits for another.  Every LDS index is checked against the
// size of its array before it is used.  (DESIGN.md "Chain history".)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <vector>

#include "lcf.h"
#include "lcf_corner.h"
#include "lcf_host.h"

using namespace lcf;

namespace {

constexpr int kMaxDim = 16;
constexpr int kMaxWalkers = 16384;
constexpr int kMaxQ = 16;
constexpr int kMaxVBins = 256;
constexpr int kMaxTBins = 4096;
constexpr int kMaxThreads = 1024;
constexpr int kRasterThreads = 1024;
constexpr long long kMaxChunk = 1LL << 30;                       // samples of a workgroup: a 32-bit counter cannot overflow
constexpr unsigned long long kNanKey = 0xfffffffffffffffeull;    // above the key of +inf (0xfff0...): NaNs sort last
constexpr unsigned long long kPadKey = 0xffffffffffffffffull;    // above every NaN: the padding stays behind them
constexpr unsigned int kNoBin = ~0u;

struct HistorySeg {
    const double* chain;     // stored step t, walker w: chain + (t * n_w + w) * n_dim
    const double* lp;        // [step][walker], or nullptr
    long long n_w, n_keep, discard, thin;
    int n_dim, n_pad;        // n_pad: the power of two at or above n_w
    // steps pass
    unsigned long long* stat;   // [n_keep][n_dim + 1][2 n_q] keys: lo, hi per percentile
    long long* n_valid;         // [n_keep][n_dim + 1]
    long long* n_moved;         // [n_keep]
    // raster pass
    const double* edges;        // [n_dim][v_bins + 1]
    unsigned long long* counts; // [n_dim][t_bins][v_bins]
    long long chunk;            // samples per workgroup
};

// work[2 * blockIdx.x] = segment, work[2 * blockIdx.x + 1] = kept step.  Dynamic LDS: lds_keys 64-bit keys (at least the
// segment's n_pad); qf[n_q] = q / 100.
__global__ __launch_bounds__(kMaxThreads) void k_history_steps(const HistorySeg* __restrict__ segs,
                                                               const int* __restrict__ work,
                                                               const double* __restrict__ qf, int n_q, int lds_keys) {
    extern __shared__ unsigned long long key[];
    __shared__ unsigned int s_count;
    const HistorySeg sg = segs[work[2 * blockIdx.x]];
    const long long k = work[2 * blockIdx.x + 1];
    const int tid = threadIdx.x, nt = blockDim.x, nd = sg.n_dim;
    const int n_w = (int)sg.n_w, n_pad = sg.n_pad;
    if (n_pad > lds_keys || n_w > n_pad) return;   // (the host sized the LDS for every segment: never taken)
    const long long t = sg.discard + k * sg.thin;
    const double* cur = sg.chain + t * sg.n_w * nd;

    // ---- moves: rows of stored step t against those of t - 1, 64-bit patterns
    if (t >= 1) {
        unsigned int* flag = reinterpret_cast<unsigned int*>(key);   // n_w words in the n_pad keys
        for (int w = tid; w < n_w; w += nt) flag[w] = 0u;
        if (tid == 0) s_count = 0u;
        __syncthreads();
        const double* prev = cur - sg.n_w * nd;
        const int n_el = n_w * nd;
        for (int e = tid; e < n_el; e += nt) {
            const int w = e / nd;
            if (__double_as_longlong(cur[e]) != __double_as_longlong(prev[e]) && w < n_pad) flag[w] = 1u;
        }
        __syncthreads();
        for (int base = 0; base < n_w; base += nt) {   // (every lane of a wave takes every trip: the ballot is whole)
            const int w = base + tid;
            const unsigned long long mask = __ballot(w < n_w && flag[min(w, n_pad - 1)] != 0u);
            if ((tid & 63) == 0 && mask) atomicAdd(&s_count, (unsigned int)__popcll(mask));
        }
        __syncthreads();
        if (tid == 0) sg.n_moved[k] = (long long)s_count;
    } else if (tid == 0) {
        sg.n_moved[k] = -1;   // (the predecessor of stored step 0 is not in the chain)
    }

    // ---- bands: column by column, the log-probability as column n_dim
    for (int c = 0; c <= nd; ++c) {
        unsigned long long* out = sg.stat + ((size_t)k * (nd + 1) + c) * 2 * n_q;
        if (c == nd && !sg.lp) {
            if (tid < 2 * n_q) out[tid] = kNanKey;
            if (tid == 0) sg.n_valid[k * (nd + 1) + c] = 0;
            break;
        }
        __syncthreads();   // (the flags, or the keys of the column before, have been read)
        if (tid == 0) s_count = 0u;
        __syncthreads();
        const double* src = c < nd ? cur + c : sg.lp + t * sg.n_w;
        const int ld = c < nd ? nd : 1;
        for (int base = 0; base < n_pad; base += nt) {
            const int w = base + tid;
            unsigned long long kk = kPadKey;
            bool nan = false;
            if (w < n_w) {
                const double v = src[(size_t)w * ld];
                nan = v != v;
                kk = nan ? kNanKey : corner_key((unsigned long long)__double_as_longlong(v));
            }
            if (w < n_pad) key[w] = kk;
            const unsigned long long mask = __ballot(nan);
            if ((tid & 63) == 0 && mask) atomicAdd(&s_count, (unsigned int)__popcll(mask));
        }
        // bitonic sort, ascending
        for (int size = 2; size <= n_pad; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (int p = tid; p < n_pad / 2; p += nt) {
                    const int i = 2 * p - (p & (stride - 1)), j = i + stride;
                    if (j >= n_pad) continue;
                    const unsigned long long a = key[i], b = key[j];
                    if ((a > b) == ((i & size) == 0)) {
                        key[i] = b;
                        key[j] = a;
                    }
                }
            }
        __syncthreads();
        const long long n = n_w - (long long)s_count;
        if (tid < 2 * n_q) {
            unsigned long long pick = kNanKey;
            if (n > 0) {
                const double h = (double)(n - 1) * qf[tid >> 1];
                long long lo = (long long)floor(h);
                lo = min(max(lo, 0LL), n - 1);
                const long long at = (tid & 1) ? min(lo + 1, n - 1) : lo;
                if (at < n_pad) pick = key[at];
            }
            out[tid] = pick;
        }
        if (tid == 0) sg.n_valid[k * (nd + 1) + c] = n;
    }
}

// work[3 * blockIdx.x] = segment, [.. + 1] = step bin, [.. + 2] = chunk of the bin's samples.
__global__ __launch_bounds__(kRasterThreads) void k_history_raster(const HistorySeg* __restrict__ segs,
                                                                   const int* __restrict__ work, int t_bins,
                                                                   int v_bins) {
    __shared__ unsigned int cnt[kMaxDim * kMaxVBins];
    const HistorySeg sg = segs[work[3 * blockIdx.x]];
    const int tid = threadIdx.x, nd = sg.n_dim, n_cnt = nd * v_bins;
    if (n_cnt > kMaxDim * kMaxVBins) return;   // (the host checked the limits: never taken)
    const long long bin = work[3 * blockIdx.x + 1];
    for (int i = tid; i < n_cnt; i += kRasterThreads) cnt[i] = 0u;
    __syncthreads();
    // kept steps k of the bin: (k * t_bins) / n_keep == bin, that is k0 <= k < k1
    const long long k0 = (bin * sg.n_keep + t_bins - 1) / t_bins, k1 = ((bin + 1) * sg.n_keep + t_bins - 1) / t_bins;
    const long long n = (k1 - k0) * sg.n_w;
    const long long s0 = (long long)work[3 * blockIdx.x + 2] * sg.chunk, s1 = min(n, s0 + sg.chunk);
    for (long long s = s0 + tid; s < s1; s += kRasterThreads) {
        const long long k = k0 + s / sg.n_w, w = s % sg.n_w;
        const double* row = sg.chain + ((sg.discard + k * sg.thin) * sg.n_w + w) * nd;
        for (int d = 0; d < nd; ++d) {
            const unsigned int j = corner_bin<kNoBin>(sg.edges + (size_t)d * (v_bins + 1), v_bins, row[d]);
            if (j < (unsigned int)v_bins) atomicAdd(&cnt[d * v_bins + (int)j], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < n_cnt; i += kRasterThreads) {
        const unsigned int v = cnt[i];
        if (v) atomicAdd(&sg.counts[((size_t)(i / v_bins) * t_bins + bin) * v_bins + i % v_bins], (unsigned long long)v);
    }
}

// What needs no device: the limits of both passes.
lcf_status check_chains(const ChainView* in, int32_t n, int64_t discard, int64_t thin) {
    if (!in || n < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (discard < 0 || thin < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "need discard >= 0 and thin >= 1");
    for (int32_t g = 0; g < n; ++g) {
        if (in[g].n_dim < 1 || in[g].n_dim > kMaxDim)
            return fail(LCF_ERR_INVALID_ARGUMENT, "need 1 <= n_dim <= 16 columns");
        if (!in[g].chain || in[g].n_t < 1 || in[g].n_w < 1)
            return fail(LCF_ERR_INVALID_ARGUMENT, "need at least one step and one walker");
        if (in[g].n_w > kMaxWalkers) return fail(LCF_ERR_UNSUPPORTED, "need n_w <= 16384 walkers");
        if (discard >= in[g].n_t) return fail(LCF_ERR_INVALID_ARGUMENT, "discard leaves no chain");
        if (in[g].n_t > (1LL << 40) / (in[g].n_w * in[g].n_dim))
            return fail(LCF_ERR_INVALID_ARGUMENT, "too many steps");
    }
    return LCF_OK;
}

lcf_status check_history_percentiles(const double* q, int32_t n_q) {
    if (!q) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    return check_percentiles(q, n_q, kMaxQ, "need 1 <= n_q <= 16 percentiles");
}

lcf_status check_raster(const ChainView* in, int32_t n, int64_t discard, int64_t thin, int32_t t_bins,
                        const double* edges, int32_t v_bins) {
    if (!edges) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (v_bins < 1 || v_bins > kMaxVBins) return fail(LCF_ERR_INVALID_ARGUMENT, "need 1 <= v_bins <= 256");
    if (t_bins < 1 || t_bins > kMaxTBins) return fail(LCF_ERR_INVALID_ARGUMENT, "need 1 <= t_bins <= min(n_keep, 4096)");
    size_t col = 0;
    for (int32_t g = 0; g < n; ++g) {
        if (t_bins > kept_steps(in[g], discard, thin).n)
            return fail(LCF_ERR_INVALID_ARGUMENT, "need 1 <= t_bins <= min(n_keep, 4096)");
        for (int d = 0; d < in[g].n_dim; ++d, ++col) {
            const double* e = edges + col * (v_bins + 1);
            for (int i = 0; i <= v_bins; ++i)
                if (!std::isfinite(e[i]) || (i > 0 && e[i] < e[i - 1]))
                    return fail(LCF_ERR_INVALID_ARGUMENT, "edges must be finite and ascending");
            if (!(e[0] < e[v_bins])) return fail(LCF_ERR_INVALID_ARGUMENT, "the first edge must be below the last");
        }
    }
    return LCF_OK;
}

std::vector<HistorySeg> history_segments(const ChainView* in, int32_t n, int64_t discard, int64_t thin) {
    std::vector<HistorySeg> segs(n, HistorySeg{});
    for (int32_t g = 0; g < n; ++g) {
        HistorySeg& a = segs[g];
        a.chain = in[g].chain;
        a.lp = in[g].log_prob;
        a.n_w = in[g].n_w;
        a.n_keep = kept_steps(in[g], discard, thin).n;
        a.discard = discard;
        a.thin = thin;
        a.n_dim = in[g].n_dim;
        a.n_pad = 1;
        while (a.n_pad < a.n_w) a.n_pad <<= 1;
    }
    return segs;
}

// Both runs: per entry of `in` a whole chain [n_t][n_w][n_dim] (ld = n_dim) and its log-probabilities, if any, in device
// memory.  Inputs and outputs (host) hold the entries' parts one after another, as lcf_samplers_chain_history /
// lcf_samplers_chain_raster describe them.
lcf_status history_steps_run(int32_t device, const ChainView* in, int32_t n, int64_t discard, int64_t thin,
                             const double* q, int32_t n_q, double* stat_lo, double* stat_hi, int64_t* n_valid,
                             int64_t* n_moved) {
    if (!stat_lo || !stat_hi || !n_valid || !n_moved) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = check_chains(in, n, discard, thin)) return st;
    if (lcf_status st = check_history_percentiles(q, n_q)) return st;
    int n_cu = 1;
    if (lcf_status st = use_device(device, &n_cu)) return st;
    std::vector<HistorySeg> segs = history_segments(in, n, discard, thin);
    size_t cells = 0, steps = 0;
    int n_pad = 1;
    for (const HistorySeg& a : segs) {
        cells += (size_t)a.n_keep * (a.n_dim + 1);
        steps += (size_t)a.n_keep;
        n_pad = std::max(n_pad, a.n_pad);
    }
    if (steps > (1u << 30)) return fail(LCF_ERR_INVALID_ARGUMENT, "too many steps");
    DevBuf mem;
    unsigned long long* d_stat;
    long long *d_valid, *d_moved;
    double* d_qf;
    lcf_status st;
    std::vector<double> qf(q, q + n_q);
    for (double& v : qf) v = v / 100.;   // (the device multiplies only: h = (n_valid - 1) * (q / 100), NumPy's order)
    if ((st = mem.alloc(&d_stat, cells * 2 * n_q)) || (st = mem.alloc(&d_valid, cells)) ||
        (st = mem.alloc(&d_moved, steps)) || (st = mem.put(&d_qf, qf.data(), qf.size())))
        return st;
    std::vector<int> work;
    work.reserve(2 * steps);
    size_t cell = 0, step = 0;
    for (int32_t g = 0; g < n; ++g) {
        HistorySeg& a = segs[g];
        a.stat = d_stat + cell * 2 * n_q;
        a.n_valid = d_valid + cell;
        a.n_moved = d_moved + step;
        cell += (size_t)a.n_keep * (a.n_dim + 1);
        step += (size_t)a.n_keep;
        for (long long k = 0; k < a.n_keep; ++k) {
            work.push_back(g);
            work.push_back((int)k);
        }
    }
    HistorySeg* d_segs;
    int* d_work;
    if ((st = mem.put(&d_segs, segs.data(), segs.size())) || (st = mem.put(&d_work, work.data(), work.size()))) return st;
    // a lane per pair of the sort, whole waves; 16384 walkers: 128 KiB of keys, granted to the kernel once
    const int threads = std::min(kMaxThreads, std::max(64, n_pad / 2));
    const size_t lds = (size_t)n_pad * sizeof(unsigned long long);
    LCF_HIP(prepare_kernel(k_history_steps, lds));
    hipLaunchKernelGGL(k_history_steps, dim3((unsigned)steps), dim3(threads), lds, 0, d_segs, d_work, d_qf, (int)n_q,
                       n_pad);
    LCF_HIP(hipGetLastError());
    std::vector<unsigned long long> stat(cells * 2 * n_q);
    LCF_HIP(hipMemcpy(stat.data(), d_stat, stat.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    static_assert(sizeof(long long) == sizeof(int64_t), "the counters are copied as they are");
    LCF_HIP(hipMemcpy(n_valid, d_valid, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(n_moved, d_moved, steps * sizeof(int64_t), hipMemcpyDeviceToHost));
    // [cell][2 n_q] keys -> per segment [n_q][n_keep][n_dim + 1] values
    cell = 0;
    for (const HistorySeg& a : segs) {
        const size_t n_cell = (size_t)a.n_keep * (a.n_dim + 1);
        for (size_t c = 0; c < n_cell; ++c)
            for (int i = 0; i < n_q; ++i) {
                const bool any = n_valid[cell + c] > 0;
                const size_t to = cell * n_q + (size_t)i * n_cell + c;
                stat_lo[to] = any ? corner_value(stat[((cell + c) * n_q + i) * 2]) : NAN;
                stat_hi[to] = any ? corner_value(stat[((cell + c) * n_q + i) * 2 + 1]) : NAN;
            }
        cell += n_cell;
    }
    return LCF_OK;
}

lcf_status history_raster_run(int32_t device, const ChainView* in, int32_t n, int64_t discard, int64_t thin,
                              int32_t t_bins, const double* edges, int32_t v_bins, int64_t* counts) {
    if (!counts) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = check_chains(in, n, discard, thin)) return st;
    if (lcf_status st = check_raster(in, n, discard, thin, t_bins, edges, v_bins)) return st;
    int n_cu = 1;
    if (lcf_status st = use_device(device, &n_cu)) return st;
    std::vector<HistorySeg> segs = history_segments(in, n, discard, thin);
    size_t cols = 0;
    for (const HistorySeg& a : segs) cols += a.n_dim;
    const size_t per_col = (size_t)t_bins * v_bins;
    DevBuf mem;
    double* d_edges;
    unsigned long long* d_counts;
    lcf_status st;
    if ((st = mem.put(&d_edges, edges, cols * (v_bins + 1))) || (st = mem.alloc(&d_counts, cols * per_col))) return st;
    LCF_HIP(hipMemset(d_counts, 0, cols * per_col * sizeof(unsigned long long)));
    // Two workgroups per CU over all segments and step bins, a bin's samples in whole sweeps of a workgroup and at most
    // kMaxChunk.  LCF_HISTORY_CHUNK (tests): that many samples instead.
    const char* env = std::getenv("LCF_HISTORY_CHUNK");
    const long long forced = env ? std::atoll(env) : 0;
    const long long per_bin = std::max<long long>(1, 2LL * n_cu / ((long long)n * t_bins));
    std::vector<int> work;
    size_t col = 0;
    for (int32_t g = 0; g < n; ++g) {
        HistorySeg& a = segs[g];
        a.edges = d_edges + col * (v_bins + 1);
        a.counts = d_counts + col * per_col;
        col += a.n_dim;
        const long long widest = ((a.n_keep + t_bins - 1) / t_bins) * a.n_w, unit = kRasterThreads;
        a.chunk = ((widest + per_bin - 1) / per_bin + unit - 1) / unit * unit;
        if (forced >= 1) a.chunk = forced;
        a.chunk = std::min(std::max<long long>(a.chunk, 1), kMaxChunk);
        for (long long b = 0; b < t_bins; ++b) {
            const long long k0 = (b * a.n_keep + t_bins - 1) / t_bins, k1 = ((b + 1) * a.n_keep + t_bins - 1) / t_bins;
            for (long long c = 0; c * a.chunk < (k1 - k0) * a.n_w; ++c) {
                work.push_back(g);
                work.push_back((int)b);
                work.push_back((int)c);
            }
        }
        if (work.size() / 3 > (1u << 30)) return fail(LCF_ERR_INVALID_ARGUMENT, "too many samples");
    }
    HistorySeg* d_segs;
    int* d_work;
    if ((st = mem.put(&d_segs, segs.data(), segs.size())) || (st = mem.put(&d_work, work.data(), work.size()))) return st;
    if (!work.empty()) {
        hipLaunchKernelGGL(k_history_raster, dim3((unsigned)(work.size() / 3)), dim3(kRasterThreads), 0, 0, d_segs, d_work,
                           (int)t_bins, (int)v_bins);
        LCF_HIP(hipGetLastError());
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are copied as they are");
    LCF_HIP(hipMemcpy(counts, d_counts, cols * per_col * sizeof(int64_t), hipMemcpyDeviceToHost));
    return LCF_OK;
}

}  // namespace

extern "C" {

lcf_status lcf_chain_history(int32_t device, const double* chain, const double* log_prob, int64_t n_t, int32_t n_w,
                             int32_t n_dim, int64_t discard, int64_t thin, const double* q, int32_t n_q, double* stat_lo,
                             double* stat_hi, int64_t* n_valid, int64_t* n_moved) {
    if (!stat_lo || !stat_hi || !n_valid || !n_moved) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    const ChainView host{chain, log_prob, n_t, n_w, n_dim, n_dim};
    if (lcf_status st = check_chains(&host, 1, discard, thin)) return st;
    if (lcf_status st = check_history_percentiles(q, n_q)) return st;
    DevBuf mem;
    ChainView in;
    if (lcf_status st = upload_chain(device, host, mem, &in)) return st;
    return history_steps_run(device, &in, 1, discard, thin, q, n_q, stat_lo, stat_hi, n_valid, n_moved);
}

lcf_status lcf_samplers_chain_history(lcf_sampler** s, int32_t n, int64_t discard, int64_t thin, const double* q,
                                      int32_t n_q, double* stat_lo, double* stat_hi, int64_t* n_valid,
                                      int64_t* n_moved) {
    std::vector<ChainView> in;
    int32_t device = 0;
    if (lcf_status st = stored_chains(s, n, discard, thin, &in, &device)) return st;
    return history_steps_run(device, in.data(), n, discard, thin, q, n_q, stat_lo, stat_hi, n_valid, n_moved);
}

lcf_status lcf_chain_raster(int32_t device, const double* chain, int64_t n_t, int32_t n_w, int32_t n_dim,
                            int64_t discard, int64_t thin, int32_t t_bins, const double* edges, int32_t v_bins,
                            int64_t* counts) {
    if (!counts) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    const ChainView host{chain, nullptr, n_t, n_w, n_dim, n_dim};
    if (lcf_status st = check_chains(&host, 1, discard, thin)) return st;
    if (lcf_status st = check_raster(&host, 1, discard, thin, t_bins, edges, v_bins)) return st;
    DevBuf mem;
    ChainView in;
    if (lcf_status st = upload_chain(device, host, mem, &in)) return st;
    return history_raster_run(device, &in, 1, discard, thin, t_bins, edges, v_bins, counts);
}

lcf_status lcf_samplers_chain_raster(lcf_sampler** s, int32_t n, int64_t discard, int64_t thin, int32_t t_bins,
                                     const double* edges, int32_t v_bins, int64_t* counts) {
    std::vector<ChainView> in;
    int32_t device = 0;
    if (lcf_status st = stored_chains(s, n, discard, thin, &in, &device)) return st;
    return history_raster_run(device, in.data(), n, discard, thin, t_bins, edges, v_bins, counts);
}

}  // extern "C"
