// Corner histograms on gfx950: what corner.corner counts for lightcurve_corner (reference fitting.py:241-253) -- the
// marginal histogram of every column of a chain and the joint histogram of every pair of columns -- over ALL samples,
// read where they lie (a stored chain [step][walker][dim] in place, discard / thin as a row offset and stride).
//
//   k_corner_range  per column the minimum and maximum of the non-NaN values and the number of NaNs.  Lanes are
//                   ELEMENTS (sample, column), consecutive lanes consecutive doubles of a row, and a lane's stride is
//                   a multiple of n_dim, so a lane stays with one column and keeps its running minimum, maximum (as
//                   order-preserving 64-bit keys: IEEE bits, sign folded -- the key of lcf_predict.hip) and NaN count
//                   in registers.  The lanes of a wave hold different columns, so a column's lanes meet in LDS
//                   (64-bit integer min / max, 32-bit add), then one 64-bit integer atomic min, max and add per
//                   column and workgroup in device memory.
//   k_corner_hist   workgroup = (chunk of samples, group of pairs), lanes = samples.  A lane reads its row once,
//                   v = x[d] - shift[d], finds the bin of every column once (a multiply-and-truncate guess corrected
//                   against the edge table) and keeps the n_dim bin numbers as bytes of two 64-bit registers -- no
//                   per-lane array, no scratch.  Then one ds_add per column (group 0) and per pair of the group into
//                   32-bit counters in LDS, merged into the 64-bit counters in device memory with integer atomics.
//
// All counts are integers and the extremes are integer minima / maxima: no result depends on the order in which
// workgroups arrive, on the chunks or on the pair groups; there is no floating-point atomic and no workgroup waits
// for another.  Every counter index is checked against the bins and the group before it is used.  (DESIGN.md "Corner
// histograms".)
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
constexpr int kMaxBins = 128;
constexpr int kCornerThreads = 1024;           // lanes of a workgroup (16 waves): two workgroups are a CU's 32 waves
constexpr int kCornerLdsBytes = 64 * 1024;     // counters of a histogram workgroup: two workgroups in a CU's 160 KiB
constexpr long long kMaxChunk = 1LL << 30;     // samples of a workgroup: a 32-bit counter cannot overflow
constexpr unsigned long long kNoKey = ~0ull;   // (no double has the key 0 or ~0: both would be NaNs)
constexpr unsigned int kNoBin = 0xffu;

struct CornerSeg {
    const double* base;          // sample s = the row at base + (s / n_w) * step_stride + (s % n_w) * ld
    long long n, n_w, step_stride;
    long long chunk;             // samples per workgroup
    int ld, n_dim;
    // range pass
    unsigned long long *kmin, *kmax, *n_nan;   // [n_dim]
    // histogram pass
    const double *shift, *edges;               // [n_dim], [n_dim][bins + 1]
    unsigned long long *h1, *h2;               // [n_dim][bins], [n_pairs][bins][bins]
    int bins, n_pairs, group_pairs;
};

__device__ __forceinline__ const double* corner_row(const CornerSeg& sg, long long s) {
    if (sg.n_w == sg.n) return sg.base + s * sg.ld;   // (one block of rows: a host array, or a chain with thin = 1)
    return sg.base + (s / sg.n_w) * sg.step_stride + (s % sg.n_w) * sg.ld;
}

// work[2 * blockIdx.x] = segment, work[2 * blockIdx.x + 1] = chunk of its samples.
__global__ __launch_bounds__(kCornerThreads) void k_corner_range(const CornerSeg* __restrict__ segs,
                                                                 const int* __restrict__ work) {
    __shared__ unsigned long long s_min[kMaxDim], s_max[kMaxDim];
    __shared__ unsigned int s_nan[kMaxDim];
    const CornerSeg sg = segs[work[2 * blockIdx.x]];
    const int tid = threadIdx.x, nd = sg.n_dim;
    if (tid < kMaxDim) {
        s_min[tid] = kNoKey;
        s_max[tid] = 0ull;
        s_nan[tid] = 0u;
    }
    __syncthreads();
    const int per = kCornerThreads / nd;   // samples of one sweep of the workgroup; lanes >= per * nd idle
    const int d = tid % nd;
    if (tid < per * nd) {
        const long long s0 = (long long)work[2 * blockIdx.x + 1] * sg.chunk, s1 = min(sg.n, s0 + sg.chunk);
        unsigned long long kmin = kNoKey, kmax = 0ull;
        unsigned int nan = 0u;
        for (long long s = s0 + tid / nd; s < s1; s += per) {
            const double v = corner_row(sg, s)[d];
            if (v != v) {
                ++nan;
            } else {
                const unsigned long long k = corner_key((unsigned long long)__double_as_longlong(v));
                kmin = min(kmin, k);
                kmax = max(kmax, k);
            }
        }
        if (kmin != kNoKey) {
            atomicMin(&s_min[d], kmin);
            atomicMax(&s_max[d], kmax);
        }
        if (nan) atomicAdd(&s_nan[d], nan);
    }
    __syncthreads();
    if (tid < nd) {
        if (s_min[tid] != kNoKey) {
            atomicMin(&sg.kmin[tid], s_min[tid]);
            atomicMax(&sg.kmax[tid], s_max[tid]);
        }
        if (s_nan[tid]) atomicAdd(&sg.n_nan[tid], (unsigned long long)s_nan[tid]);
    }
}

// byte d of the packed bin numbers (d is wave-uniform)
__device__ __forceinline__ unsigned int corner_byte(unsigned long long lo, unsigned long long hi, int d) {
    return (unsigned int)((d < 8 ? lo >> (8 * d) : hi >> (8 * (d - 8))) & 0xffull);
}

// work[3 * blockIdx.x] = segment, [.. + 1] = chunk of its samples, [.. + 2] = group of its pairs.  Dynamic LDS:
// n_dim * bins counters of the columns (used by group 0), then bins^2 per pair of the group.
__global__ __launch_bounds__(kCornerThreads) void k_corner_hist(const CornerSeg* __restrict__ segs,
                                                                const int* __restrict__ work, int lds_counters) {
    extern __shared__ unsigned int cnt[];
    const CornerSeg sg = segs[work[3 * blockIdx.x]];
    const int tid = threadIdx.x, nd = sg.n_dim, bins = sg.bins, nb2 = bins * bins;
    const int group = work[3 * blockIdx.x + 2];
    const int p0 = group * sg.group_pairs, p1 = min(sg.n_pairs, p0 + sg.group_pairs);
    const int n_marg = nd * bins, n_cnt = n_marg + max(p1 - p0, 0) * nb2;
    if (n_cnt > lds_counters) return;   // (the host sized the LDS for every group: never taken)
    for (int k = tid; k < n_cnt; k += kCornerThreads) cnt[k] = 0u;
    __syncthreads();

    int a0 = 1;   // the pair p0 is (a0, b0), b0 < a0
    while (a0 * (a0 + 1) / 2 <= p0) ++a0;
    const int b0 = p0 - a0 * (a0 - 1) / 2;
    const long long s0 = (long long)work[3 * blockIdx.x + 1] * sg.chunk, s1 = min(sg.n, s0 + sg.chunk);
    for (long long s = s0 + tid; s < s1; s += kCornerThreads) {
        const double* row = corner_row(sg, s);
        unsigned long long lo = 0ull, hi = 0ull;   // the row's bin numbers, a byte per column
        for (int d = 0; d < nd; ++d) {
            const unsigned int bin = corner_bin<kNoBin>(sg.edges + (size_t)d * (bins + 1), bins, row[d] - sg.shift[d]);
            if (group == 0 && bin < (unsigned int)bins) atomicAdd(&cnt[d * bins + (int)bin], 1u);
            if (d < 8)
                lo |= (unsigned long long)bin << (8 * d);
            else
                hi |= (unsigned long long)bin << (8 * (d - 8));
        }
        for (int p = p0, a = a0, b = b0; p < p1; ++p) {
            const unsigned int ia = corner_byte(lo, hi, a), ib = corner_byte(lo, hi, b);
            if (ia < (unsigned int)bins && ib < (unsigned int)bins)
                atomicAdd(&cnt[n_marg + (p - p0) * nb2 + (int)ib * bins + (int)ia], 1u);
            if (++b == a) {
                ++a;
                b = 0;
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < n_cnt; k += kCornerThreads) {
        const unsigned int v = cnt[k];
        if (!v) continue;
        if (k < n_marg)
            atomicAdd(&sg.h1[k], (unsigned long long)v);
        else
            atomicAdd(&sg.h2[(size_t)p0 * nb2 + (k - n_marg)], (unsigned long long)v);
    }
}

// What needs no device: the limits of both passes.
lcf_status check_samples(const ChainView* in, int32_t n) {
    if (!in || n < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    for (int32_t g = 0; g < n; ++g) {
        if (in[g].n_dim < 1 || in[g].n_dim > kMaxDim)
            return fail(LCF_ERR_INVALID_ARGUMENT, "need 1 <= n_dim <= 16 columns");
        if (!in[g].chain || in[g].n_t < 1 || in[g].n_w < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "need at least one sample");
        if (in[g].ld < in[g].n_dim) return fail(LCF_ERR_INVALID_ARGUMENT, "ld is smaller than n_dim");
    }
    return LCF_OK;
}

// Samples per workgroup such that `per_seg` workgroups cover n samples: whole sweeps of a workgroup, at most kMaxChunk.
long long corner_chunk(long long n, long long per_seg) {
    const long long unit = kCornerThreads;
    const long long chunk = ((n + per_seg - 1) / per_seg + unit - 1) / unit * unit;
    return std::min(std::max(chunk, unit), kMaxChunk);
}

// What both passes need of every entry: the walkers of its kept steps as samples.
std::vector<CornerSeg> corner_segments(const ChainView* in, int32_t n, int64_t discard, int64_t thin) {
    std::vector<CornerSeg> segs(n, CornerSeg{});
    for (int32_t g = 0; g < n; ++g) {
        const KeptSteps k = kept_steps(in[g], discard, thin);
        CornerSeg& a = segs[g];
        a.base = k.base;
        a.n = k.samples;
        a.n_w = in[g].n_w;
        a.step_stride = k.step_stride;
        if (a.n_w >= a.n || a.step_stride == a.n_w * in[g].ld) a.n_w = a.n;   // one block of rows
        a.ld = in[g].ld;
        a.n_dim = in[g].n_dim;
    }
    return segs;
}

// Both runs: per entry of `in` the walkers of its kept steps, in device memory.  Inputs and outputs (host) hold the
// entries' parts one after another, as lcf_samplers_chain_range / lcf_samplers_chain_hist describe them.
lcf_status corner_range_run(int32_t device, const ChainView* in, int32_t n, int64_t discard, int64_t thin, double* lo,
                            double* hi, int64_t* n_nan) {
    if (!lo || !hi || !n_nan) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = check_samples(in, n)) return st;
    int n_cu = 1;
    if (lcf_status st = use_device(device, &n_cu)) return st;
    std::vector<CornerSeg> segs = corner_segments(in, n, discard, thin);
    size_t cols = 0;
    for (const CornerSeg& a : segs) cols += a.n_dim;
    // per column: minimum key, maximum key, NaN count
    std::vector<unsigned long long> res(3 * cols, 0ull);
    std::fill(res.begin(), res.begin() + cols, kNoKey);
    DevBuf mem;
    unsigned long long* d_res;
    lcf_status st;
    if ((st = mem.put(&d_res, res.data(), res.size()))) return st;
    std::vector<int> work;
    size_t col = 0;
    for (int32_t g = 0; g < n; ++g) {
        CornerSeg& a = segs[g];
        a.kmin = d_res + col;
        a.kmax = d_res + cols + col;
        a.n_nan = d_res + 2 * cols + col;
        col += a.n_dim;
        a.chunk = corner_chunk(a.n, std::max(1, 4 * n_cu / n));
        for (long long c = 0; c * a.chunk < a.n; ++c) {
            work.push_back(g);
            work.push_back((int)c);
        }
    }
    CornerSeg* d_segs;
    int* d_work;
    if ((st = mem.put(&d_segs, segs.data(), segs.size())) || (st = mem.put(&d_work, work.data(), work.size()))) return st;
    hipLaunchKernelGGL(k_corner_range, dim3((unsigned)(work.size() / 2)), dim3(kCornerThreads), 0, 0, d_segs, d_work);
    LCF_HIP(hipGetLastError());
    LCF_HIP(hipMemcpy(res.data(), d_res, res.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < cols; ++k) {
        const bool any = res[k] != kNoKey;
        lo[k] = any ? corner_value(res[k]) : NAN;
        hi[k] = any ? corner_value(res[cols + k]) : NAN;
        n_nan[k] = (int64_t)res[2 * cols + k];
    }
    return LCF_OK;
}

lcf_status corner_hist_run(int32_t device, const ChainView* in, int32_t n, int64_t discard, int64_t thin,
                           const double* shift, const double* edges, int32_t bins, int64_t* hist1d, int64_t* hist2d) {
    if (!shift || !edges || !hist1d) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (bins < 1 || bins > kMaxBins) return fail(LCF_ERR_INVALID_ARGUMENT, "need 1 <= bins <= 128");
    if (lcf_status st = check_samples(in, n)) return st;
    size_t cols = 0, pairs = 0;
    for (int32_t g = 0; g < n; ++g) {
        cols += in[g].n_dim;
        pairs += (size_t)in[g].n_dim * (in[g].n_dim - 1) / 2;
    }
    if (pairs && !hist2d) return fail(LCF_ERR_INVALID_ARGUMENT, "hist2d is null and there are pairs of columns");
    for (size_t d = 0; d < cols; ++d) {
        const double* e = edges + d * (bins + 1);
        if (!std::isfinite(shift[d])) return fail(LCF_ERR_INVALID_ARGUMENT, "shift must be finite");
        for (int i = 0; i <= bins; ++i)
            if (!std::isfinite(e[i]) || (i > 0 && e[i] < e[i - 1]))
                return fail(LCF_ERR_INVALID_ARGUMENT, "edges must be finite and ascending");
        if (!(e[0] < e[bins])) return fail(LCF_ERR_INVALID_ARGUMENT, "the first edge must be below the last");
    }
    int n_cu = 1;
    if (lcf_status st = use_device(device, &n_cu)) return st;

    // Pairs per group: what fits the LDS budget beside the columns' counters, but at least one pair (128 bins: 64 KiB
    // a pair; the launch is then granted more than the default).  LCF_CORNER_GROUP_PAIRS (tests): fewer.
    const size_t nb2 = (size_t)bins * bins;
    const char* env = std::getenv("LCF_CORNER_GROUP_PAIRS");
    const long long forced = env ? std::atoll(env) : 0;
    std::vector<CornerSeg> segs = corner_segments(in, n, discard, thin);
    size_t lds_counters = 0;
    long long n_work = 0;
    for (int32_t g = 0; g < n; ++g) {
        CornerSeg& a = segs[g];
        a.bins = bins;
        a.n_pairs = a.n_dim * (a.n_dim - 1) / 2;
        const size_t marg = (size_t)a.n_dim * bins;
        long long gp = std::max<long long>(1, ((long long)(kCornerLdsBytes / 4) - (long long)marg) / (long long)nb2);
        if (forced >= 1) gp = std::min(gp, forced);
        a.group_pairs = (int)std::min<long long>(gp, std::max(a.n_pairs, 1));
        lds_counters = std::max(lds_counters, marg + (size_t)std::min(a.group_pairs, a.n_pairs) * nb2);
        // two workgroups per CU over all segments and groups: a workgroup's merge stays small next to its samples
        const int groups = std::max(1, (a.n_pairs + a.group_pairs - 1) / a.group_pairs);
        a.chunk = corner_chunk(a.n, std::max<long long>(1, 2LL * n_cu / ((long long)n * groups)));
        n_work += (a.n + a.chunk - 1) / a.chunk * groups;
    }
    if (n_work > (1LL << 30)) return fail(LCF_ERR_INVALID_ARGUMENT, "too many samples");

    DevBuf mem;
    double *d_shift, *d_edges;
    unsigned long long *d_h1, *d_h2;
    lcf_status st;
    if ((st = mem.put(&d_shift, shift, cols)) || (st = mem.put(&d_edges, edges, cols * (bins + 1))) ||
        (st = mem.alloc(&d_h1, cols * bins)) || (st = mem.alloc(&d_h2, pairs * nb2)))
        return st;
    LCF_HIP(hipMemset(d_h1, 0, std::max<size_t>(cols * bins, 1) * sizeof(unsigned long long)));
    LCF_HIP(hipMemset(d_h2, 0, std::max<size_t>(pairs * nb2, 1) * sizeof(unsigned long long)));
    std::vector<int> work;
    work.reserve((size_t)n_work * 3);
    size_t col = 0, pair = 0;
    for (int32_t g = 0; g < n; ++g) {
        CornerSeg& a = segs[g];
        a.shift = d_shift + col;
        a.edges = d_edges + col * (bins + 1);
        a.h1 = d_h1 + col * bins;
        a.h2 = d_h2 + pair * nb2;
        col += a.n_dim;
        pair += a.n_pairs;
        const int groups = std::max(1, (a.n_pairs + a.group_pairs - 1) / a.group_pairs);
        for (long long c = 0; c * a.chunk < a.n; ++c)
            for (int gr = 0; gr < groups; ++gr) {
                work.push_back(g);
                work.push_back((int)c);
                work.push_back(gr);
            }
    }
    CornerSeg* d_segs;
    int* d_work;
    if ((st = mem.put(&d_segs, segs.data(), segs.size())) || (st = mem.put(&d_work, work.data(), work.size()))) return st;
    const size_t lds = lds_counters * sizeof(unsigned int);
    LCF_HIP(prepare_kernel(k_corner_hist, lds));
    hipLaunchKernelGGL(k_corner_hist, dim3((unsigned)(work.size() / 3)), dim3(kCornerThreads), lds, 0, d_segs, d_work,
                       (int)lds_counters);
    LCF_HIP(hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are copied as they are");
    LCF_HIP(hipMemcpy(hist1d, d_h1, cols * bins * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (pairs) LCF_HIP(hipMemcpy(hist2d, d_h2, pairs * nb2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return LCF_OK;
}

// n host samples P[n][ld] as one step of n walkers, on `device` for as long as `mem` lives.
lcf_status uploaded_samples(int32_t device, const double* P, int64_t n, int32_t ld, int32_t n_dim, DevBuf& mem,
                            ChainView* in) {
    if (!P || n < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "need at least one sample");
    if (n_dim < 1 || n_dim > kMaxDim) return fail(LCF_ERR_INVALID_ARGUMENT, "need 1 <= n_dim <= 16 columns");
    if (ld < n_dim) return fail(LCF_ERR_INVALID_ARGUMENT, "ld is smaller than n_dim");
    if (n > (1LL << 40) / ld) return fail(LCF_ERR_INVALID_ARGUMENT, "too many samples");
    return upload_chain(device, ChainView{P, nullptr, 1, n, ld, n_dim}, mem, in);
}

}  // namespace

extern "C" {

lcf_status lcf_chain_range(int32_t device, const double* P, int64_t n, int32_t ld, int32_t n_dim, double* lo,
                           double* hi, int64_t* n_nan) {
    if (!lo || !hi || !n_nan) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    DevBuf mem;
    ChainView in;
    if (lcf_status st = uploaded_samples(device, P, n, ld, n_dim, mem, &in)) return st;
    return corner_range_run(device, &in, 1, 0, 1, lo, hi, n_nan);
}

lcf_status lcf_samplers_chain_range(lcf_sampler** s, int32_t n, int64_t discard, int64_t thin, double* lo, double* hi,
                                    int64_t* n_nan) {
    if (!lo || !hi || !n_nan) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<ChainView> in;
    int32_t device = 0;
    if (lcf_status st = stored_chains(s, n, discard, thin, &in, &device)) return st;
    return corner_range_run(device, in.data(), n, discard, thin, lo, hi, n_nan);
}

lcf_status lcf_chain_hist(int32_t device, const double* P, int64_t n, int32_t ld, int32_t n_dim, const double* shift,
                          const double* edges, int32_t bins, int64_t* hist1d, int64_t* hist2d) {
    if (!shift || !edges || !hist1d) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (bins < 1 || bins > kMaxBins) return fail(LCF_ERR_INVALID_ARGUMENT, "need 1 <= bins <= 128");
    DevBuf mem;
    ChainView in;
    if (lcf_status st = uploaded_samples(device, P, n, ld, n_dim, mem, &in)) return st;
    return corner_hist_run(device, &in, 1, 0, 1, shift, edges, bins, hist1d, hist2d);
}

lcf_status lcf_samplers_chain_hist(lcf_sampler** s, int32_t n, int64_t discard, int64_t thin, const double* shift,
                                   const double* edges, int32_t bins, int64_t* hist1d, int64_t* hist2d) {
    std::vector<ChainView> in;
    int32_t device = 0;
    if (lcf_status st = stored_chains(s, n, discard, thin, &in, &device)) return st;
    return corner_hist_run(device, in.data(), n, discard, thin, shift, edges, bins, hist1d, hist2d);
}

}  // extern "C"
