// Integrated autocorrelation time of stored chains on gfx950: emcee's estimator (autocorr.integrated_time with its
// auto_window), with the autocorrelation computed only for the lags the window search needs.
//
//   k_acf_moments  the mean of every series (one per walker and parameter), a workgroup per 64 series, its waves
//                  summing equal t-chunks of x_t - x_0 that are then combined in a fixed order
//   k_acf_lags     for a slab of lags [lo, hi): sum_t y_t y_{t+tau} of every series, y = x - mean.  One lane per series
//                  (consecutive lanes read consecutive doubles of a chain row), a workgroup per 64 series and kLagK
//                  consecutive lags, its kLagWaves waves one t-chunk each; every lane keeps y_{t+tau0 .. t+tau0+K-1}
//                  in a register window that the unrolled loop refills in place (one new element per t), so a t costs
//                  two loads and K fused multiply-adds.  The chunks' partial sums are combined in LDS in chunk order.
//   k_acf_reduce   f[d][tau] = (sum over walkers, in walker order, of acf_w[tau] / acf_w[0]) / n_w, emcee's order.
//
// The host drives slabs [0, 64), [64, 128), [128, 256), ... (a slab is at most kSlabMax lags) and after each one
// extends taus = 2 cumsum(f) - 1 and looks for the window; it stops when every parameter's window is decided or n_t
// is reached.  Every sum runs in an order fixed by the series' n_t alone, so a series gives bitwise the same tau
// whichever entry point, slab sequence or population it is computed in.  No atomics.  (DESIGN.md "Autocorrelation
// time".)
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "lcf.h"
#include "lcf_host.h"

using namespace lcf;

namespace {

constexpr int kTile = 64;          // series per workgroup (one wave's lanes)
constexpr int kMomWaves = 16;      // t-chunks of the mean
constexpr int kLagWaves = 8;       // t-chunks of the lag sums
constexpr int kLagK = 16;          // lags per lane (register window)
constexpr int kFirstSlab = 64;
constexpr int kSlabMax = 512;

struct AcfSeg {
    const double* base;      // element t of series s at base[t * stride + s]
    long long stride;        // doubles between consecutive elements (thin * n_w * n_d)
    long long n_t;
    int n_ser, n_w, n_d;     // n_ser = n_w * n_d
    int ser0;                // first series in the global series numbering (mean / acf0 / scratch rows)
    int row0;                // first (segment, parameter) row of the f output
    int tile0;               // first tile of 64 series
};

__device__ __forceinline__ long long chunk_lo(long long n_t, int c, int n_c) { return n_t * c / n_c; }

__global__ __launch_bounds__(kTile * kMomWaves) void k_acf_moments(const AcfSeg* __restrict__ segs,
                                                                  const int* __restrict__ tile_seg,
                                                                  double* __restrict__ mean) {
    __shared__ double part[kMomWaves][kTile];
    const int lane = threadIdx.x & (kTile - 1), wave = threadIdx.x / kTile;
    const AcfSeg sg = segs[tile_seg[blockIdx.x]];
    const int s = (blockIdx.x - sg.tile0) * kTile + lane;
    // mean = x_0 + sum_t (x_t - x_0) / n_t: exactly x_0 for a constant series, whose y is then exactly 0
    double sum = 0., x0 = 0.;
    if (s < sg.n_ser) {
        const long long t1 = chunk_lo(sg.n_t, wave + 1, kMomWaves);
        const double* p = sg.base + s;
        x0 = p[0];
#pragma unroll 8
        for (long long t = chunk_lo(sg.n_t, wave, kMomWaves); t < t1; ++t) sum += p[t * sg.stride] - x0;
    }
    part[wave][lane] = sum;
    __syncthreads();
    if (wave == 0 && s < sg.n_ser) {
        double m = part[0][lane];
        for (int w = 1; w < kMomWaves; ++w) m += part[w][lane];
        mean[sg.ser0 + s] = x0 + m / (double)sg.n_t;
    }
}

// blockIdx.x = tile index into tile_seg * groups + lag group; out[(ser0 + s) * width + tau - lo] for tau in [lo, hi).
__global__ __launch_bounds__(kTile * kLagWaves) void k_acf_lags(const AcfSeg* __restrict__ segs,
                                                               const int* __restrict__ tile_seg,
                                                               const double* __restrict__ mean, long long lo,
                                                               long long hi, int groups, double* __restrict__ out) {
    __shared__ double part[kLagWaves - 1][kLagK][kTile];
    const int lane = threadIdx.x & (kTile - 1), wave = threadIdx.x / kTile;
    const int tile = tile_seg[blockIdx.x / groups * 2 + 1];
    const AcfSeg sg = segs[tile_seg[blockIdx.x / groups * 2]];
    const long long tau0 = lo + (long long)(blockIdx.x % groups) * kLagK;
    const int s = (tile - sg.tile0) * kTile + lane;
    const bool live = s < sg.n_ser && tau0 < sg.n_t;
    double acc[kLagK];
#pragma unroll
    for (int k = 0; k < kLagK; ++k) acc[k] = 0.;
    if (live) {
        const double mu = mean[sg.ser0 + s];
        const double* p = sg.base + s;
        const long long n_t = sg.n_t, st = sg.stride;
        const long long t0 = chunk_lo(n_t, wave, kLagWaves);
        const long long t1 = min(chunk_lo(n_t, wave + 1, kLagWaves), n_t - tau0);   // (no product beyond n_t - tau0)
        if (t0 < t1) {
            // win[(j + k) % K] = y_{t + tau0 + k} at sub-step j of a block of K consecutive t
            double win[kLagK];
#pragma unroll
            for (int k = 0; k < kLagK; ++k) {
                const long long u = t0 + tau0 + k;
                win[k] = u < n_t ? p[u * st] - mu : 0.;
            }
            for (long long tb = t0; tb < t1; tb += kLagK) {
#pragma unroll
                for (int j = 0; j < kLagK; ++j) {
                    const long long t = tb + j;
                    const double yt = t < t1 ? p[t * st] - mu : 0.;
#pragma unroll
                    for (int k = 0; k < kLagK; ++k) acc[k] = fma(yt, win[(j + k) % kLagK], acc[k]);
                    const long long u = t + tau0 + kLagK;
                    win[j] = u < n_t ? p[u * st] - mu : 0.;
                }
            }
        }
    }
    if (wave > 0)
#pragma unroll
        for (int k = 0; k < kLagK; ++k) part[wave - 1][k][lane] = acc[k];
    __syncthreads();
    if (wave == 0 && live) {
        const long long width = hi - lo;
        double* o = out + (long long)(sg.ser0 + s) * width + (tau0 - lo);
#pragma unroll
        for (int k = 0; k < kLagK; ++k) {
            double a = acc[k];
            for (int w = 1; w < kLagWaves; ++w) a += part[w - 1][k][lane];
            if (tau0 + k < hi) o[k] = a;
        }
    }
}

// blockIdx.y = entry of row_seg: (segment, parameter d) as 2 ints; lanes over tau.  f[r][tau - lo] for r = that entry.
// den: acf_w[0] of series q at den[q * den_stride] (the first slab's own lag 0, later acf0); the first slab also
// keeps acf_w[0] in acf0 for the later ones.
__global__ __launch_bounds__(kTile) void k_acf_reduce(const AcfSeg* __restrict__ segs, const int* __restrict__ row_seg,
                                                     const double* __restrict__ lags, long long lo, long long hi,
                                                     const double* __restrict__ den, long long den_stride,
                                                     double* __restrict__ acf0, double* __restrict__ f) {
    const AcfSeg sg = segs[row_seg[2 * blockIdx.y]];
    const int d = row_seg[2 * blockIdx.y + 1];
    const long long width = hi - lo;
    const long long tau = lo + (long long)blockIdx.x * kTile + threadIdx.x;
    if (tau >= hi || tau >= sg.n_t) return;
    double sum = 0.;
    for (int w = 0; w < sg.n_w; ++w) {
        const long long q = sg.ser0 + (long long)w * sg.n_d + d;
        const double a0 = den[q * den_stride];
        if (acf0 && tau == 0) acf0[q] = a0;
        sum += lags[q * width + (tau - lo)] / a0;
    }
    f[(long long)blockIdx.y * width + (tau - lo)] = sum / (double)sg.n_w;
}

// A device buffer that grows with the slab width (reallocated, contents not kept).
struct Grow {
    double* p = nullptr;
    size_t cap = 0;
    ~Grow() {
        if (p) hipFree(p);
    }
    lcf_status need(size_t n) {
        if (n <= cap) return LCF_OK;
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
        LCF_HIP(hipMalloc((void**)&p, n * sizeof(double)));
        cap = n;
        return LCF_OK;
    }
};

// emcee's auto_window over a growing prefix of taus: window = argmin(m) if any(m) else n_t - 1, m[k] = k < c taus[k].
struct Window {
    long long n_t = 0, next = 0, first_false = -1, window = -1;
    double cs = 0., tau0 = 0., tau_ff = 0., tau = 0.;
    bool any_true = false, done = false;
    void feed(double fk, double c) {
        const long long k = next++;
        cs += fk;
        const double taus = 2. * cs - 1.;
        if (k == 0) tau0 = taus;
        if ((double)k < c * taus)
            any_true = true;
        else if (first_false < 0) {
            first_false = k;
            tau_ff = taus;
        }
        if (any_true && first_false >= 0) {
            finish(first_false, tau_ff);
        } else if (next == n_t) {
            if (!any_true) finish(n_t - 1, taus);
            // every m[k] true: argmin is 0.  That needs taus[n_t - 1] > 0, and in exact arithmetic the normalised
            // autocorrelations of a mean-subtracted series sum to taus[n_t - 1] = 0, so no honest chain comes here
            // and no test does.
            else finish(0, tau0);
        }
    }
    void finish(long long w, double t) {
        window = w;
        tau = t;
        done = true;
    }
};

// One series per walker and parameter of every view's kept steps, where they lie in device memory.  tau / window
// receive n_dim entries per view, in order.
lcf_status autocorr_run(int32_t device, const ChainView* in, int32_t n, int64_t discard, int64_t thin, double c,
                        double* tau, int64_t* window) {
    if (lcf_status st = use_device(device)) return st;
    std::vector<AcfSeg> segs(n);
    std::vector<int> tile_seg;   // segment of every tile of 64 series
    std::vector<Window> win;     // one per (segment, parameter) row
    int ser = 0, rows = 0, tiles = 0;
    long long max_t = 0;
    for (int g = 0; g < n; ++g) {
        AcfSeg& a = segs[g];
        const KeptSteps k = kept_steps(in[g], discard, thin);
        a.base = k.base;
        a.stride = k.stride;
        a.n_t = k.n;
        a.n_w = (int)in[g].n_w;
        a.n_d = in[g].n_dim;
        a.n_ser = a.n_w * a.n_d;
        a.ser0 = ser;
        a.row0 = rows;
        a.tile0 = tiles;
        const int nt = (a.n_ser + kTile - 1) / kTile;
        for (int k = 0; k < nt; ++k) tile_seg.push_back(g);
        ser += a.n_ser;
        rows += a.n_d;
        tiles += nt;
        max_t = std::max(max_t, a.n_t);
        for (int d = 0; d < a.n_d; ++d) {
            Window w;
            w.n_t = a.n_t;
            win.push_back(w);
        }
    }
    DevBuf b;
    AcfSeg* dsegs;
    int *dtiles, *dlive, *drows;
    double *dmean, *dacf0;
    lcf_status st;
    if ((st = b.alloc(&dsegs, n)) || (st = b.alloc(&dtiles, tiles)) || (st = b.alloc(&dlive, 2 * tiles)) ||
        (st = b.alloc(&drows, 2 * rows)) || (st = b.alloc(&dmean, ser)) || (st = b.alloc(&dacf0, ser)))
        return st;
    LCF_HIP(hipMemcpy(dsegs, segs.data(), n * sizeof(AcfSeg), hipMemcpyHostToDevice));
    LCF_HIP(hipMemcpy(dtiles, tile_seg.data(), tiles * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_acf_moments, dim3(tiles), dim3(kTile * kMomWaves), 0, 0, dsegs, dtiles, dmean);
    LCF_HIP(hipGetLastError());

    Grow lags, f;   // [series][width] lag sums of the slab, [row][width] its f
    std::vector<int> live, row_list;
    std::vector<double> fh;
    for (long long lo = 0, width = kFirstSlab; lo < max_t; lo += width, width = std::min<long long>(lo, kSlabMax)) {
        // the (segment, d) rows still undecided, and the tiles of their segments as (segment, tile) pairs
        live.clear();
        row_list.clear();
        for (int g = 0; g < n; ++g) {
            bool any = false;
            for (int d = 0; d < segs[g].n_d; ++d)
                if (!win[segs[g].row0 + d].done) {
                    any = true;
                    row_list.push_back(g);
                    row_list.push_back(d);
                }
            for (int k = 0; any && k < (segs[g].n_ser + kTile - 1) / kTile; ++k) {
                live.push_back(g);
                live.push_back(segs[g].tile0 + k);
            }
        }
        if (row_list.empty()) break;
        const long long hi = lo + width;
        const int n_rows = (int)row_list.size() / 2, n_tiles = (int)live.size() / 2;
        const int groups = (int)((width + kLagK - 1) / kLagK);
        if ((st = lags.need((size_t)ser * width)) || (st = f.need((size_t)n_rows * width))) return st;
        LCF_HIP(hipMemcpy(dlive, live.data(), live.size() * sizeof(int), hipMemcpyHostToDevice));
        LCF_HIP(hipMemcpy(drows, row_list.data(), row_list.size() * sizeof(int), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_acf_lags, dim3((unsigned)(n_tiles * groups)), dim3(kTile * kLagWaves), 0, 0, dsegs, dlive,
                           dmean, lo, hi, groups, lags.p);
        LCF_HIP(hipGetLastError());
        const bool first = lo == 0;   // (lag 0 of the first slab is every series' acf_w[0])
        hipLaunchKernelGGL(k_acf_reduce, dim3((unsigned)((width + kTile - 1) / kTile), (unsigned)n_rows), dim3(kTile), 0,
                           0, dsegs, drows, lags.p, lo, hi, first ? (const double*)lags.p : (const double*)dacf0,
                           first ? width : 1LL, first ? dacf0 : nullptr, f.p);
        LCF_HIP(hipGetLastError());
        fh.resize((size_t)n_rows * width);
        LCF_HIP(hipMemcpy(fh.data(), f.p, fh.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int r = 0; r < n_rows; ++r) {
            const AcfSeg& a = segs[row_list[2 * r]];
            Window& w = win[a.row0 + row_list[2 * r + 1]];
            const double* fr = fh.data() + (size_t)r * width;
            if (first && std::isnan(fr[0])) {   // a constant (or non-finite) walker: every f[tau] is NaN
                w.finish(a.n_t - 1, NAN);
                continue;
            }
            for (long long t = lo; t < hi && t < a.n_t && !w.done; ++t) w.feed(fr[t - lo], c);
        }
    }
    for (int r = 0; r < rows; ++r) {
        tau[r] = win[r].tau;
        window[r] = win[r].window;
    }
    return LCF_OK;
}

}  // namespace

extern "C" {

lcf_status lcf_autocorr_time(int32_t device, const double* chain, int64_t n_t, int32_t n_w, int32_t n_d, double c,
                             double* tau, int64_t* window) {
    if (!chain || !tau || !window) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (n_t < 1 || n_w < 1 || n_d < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "need n_t, n_w, n_d >= 1");
    if ((int64_t)n_w * n_d > (1 << 30)) return fail(LCF_ERR_INVALID_ARGUMENT, "n_w * n_d too large");
    if (!std::isfinite(c)) return fail(LCF_ERR_INVALID_ARGUMENT, "c must be finite");
    DevBuf mem;
    ChainView in;
    if (lcf_status st = upload_chain(device, ChainView{chain, nullptr, n_t, n_w, n_d, n_d}, mem, &in)) return st;
    return autocorr_run(device, &in, 1, 0, 1, c, tau, window);
}

lcf_status lcf_samplers_autocorr_time(lcf_sampler** s, int32_t n, int64_t discard, int64_t thin, double c,
                                      double* tau, int64_t* window) {
    if (!tau || !window) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (!std::isfinite(c)) return fail(LCF_ERR_INVALID_ARGUMENT, "c must be finite");
    std::vector<ChainView> in;
    int32_t device = 0;
    if (lcf_status st = stored_chains(s, n, discard, thin, &in, &device)) return st;
    return autocorr_run(device, in.data(), n, discard, thin, c, tau, window);
}

}  // extern "C"
