// Posterior-predictive quantiles on gfx950: for every grid point (observation time x filter) the percentiles, over ALL
// samples of a chain, of the model light curve -- np.nanpercentile(Y, q, axis=samples) with Y[point][sample] never
// stored.  The value of a (sample, point) pair is recomputed in every pass; device memory beyond the chain is the
// samples' derived coefficients (64 bytes each) plus a per-time block that does not depend on the number of samples.
//
// Every value becomes an order-preserving 64-bit key (IEEE bits, sign folded), NaNs are dropped, and the wanted order
// statistics are found by radix selection on the key, most significant bits first:
//   k_pq_coef     walker_coefficients of every sample, once, [8][n] (consecutive lanes = consecutive samples)
//   k_pq_pass     workgroup = (one time, all its filters, a chunk of samples), lanes = samples: thermal state once per
//                 (sample, time), then the filters.  mode 0: histogram of the keys' top bits per point; mode 1: per
//                 search (point, percentile) the histogram of the next bits among the keys that carry the search's
//                 prefix; mode 2: the keys with the prefix go to the search's buffer, the smallest key above them is kept.
//                 Histograms are 32-bit counters in LDS (ds_add), merged into device memory with integer atomic adds.
//   k_pq_pick     per search: the bin that holds the wanted rank -> longer prefix, rank inside it, number of keys left
//   k_pq_finish   per search: bitonic sort of the (at most kPqCap) collected keys in LDS, order statistics rank and
//                 rank + 1 (the latter possibly the kept successor), NumPy's linear interpolation
// The host repeats mode 1 until every search holds at most kPqCap keys or its prefix is a whole key (ties: the answer is
// that key).  All counts are integers and the collected keys are sorted, so no result depends on the order in which
// workgroups arrive, on the sample chunks or on how the times are tiled over the workspace; there is no floating-point
// atomic and no workgroup waits for another.  (DESIGN.md "Posterior-predictive quantiles".)
//
// The thermal form (DESIGN.md "Thermal bands and validity") runs the same searches on what the band sums are made from:
//   k_th_sample   walker_coefficients and the validity window (t_min, t_max) of every sample, once, [8][n] and [2][n]
//   k_th_pass     the geometry and modes of k_pq_pass with three "filters" per time -- T, R_bb = sqrt(R_bb^2) and
//                 L_bol = 4 pi sigma_SB R_bb^2 T^4 of ONE linear-space thermal_state, the values of
//                 lcf_temperature_radius -- and no band sum, filter descriptor or exp table.  In mode 0 it also counts,
//                 per time, the samples with T < T_floor and those with t_min <= t <= t_max: wave ballot + popcount,
//                 a sum per workgroup in LDS, one 64-bit integer atomic per workgroup and counter.
//
// The luminosity form (DESIGN.md "Luminosity bands and peaks") is for the central-engine models, whose value is a
// 64-node quadrature -- a wavefront -- and too dear to recompute in every pass: every (sample, time) pair of a tile is
// evaluated ONCE into its key, keys[tile time][n] (k_lq_eval, lcf_central.hip, beside the quadrature), and
//   k_kq_pass     the geometry and modes of k_pq_pass with one series per time, over the stored keys: lanes = samples,
//                 coalesced 8-byte reads, NaN keys dropped.  In mode 0 it also counts, per time, the samples whose L
//                 is exactly +0 (not exploded yet), as k_th_pass counts its two.
//   k_lq_peak     lane = sample: walks the tile's times in ascending order and keeps the sample's largest non-NaN L
//                 and the first time it is attained (strict >).  Tiles follow each other on one stream, so the first
//                 occurrence wins whatever the tiling.
// The custom form (DESIGN.md "Bands of a custom model") stores keys as well: the program of a custom model evaluates
// its state function once per (sample, time) and writes the keys of every filter's light curve, T, R and L
// (lcf_custom_keys, lcf_custom_kernel.h), keys[tile time][series][n].  A (time, series) pair is a selection unit --
// what a time is to k_kq_pass, which reads the keys as it reads the luminosity form's -- and a tile is whole times.
// The colour form (DESIGN.md "Colour bands and peaks") recomputes, as the light-curve form does, but its selection units
// are colours, not filters:
//   k_cq_pass     the geometry and modes of k_pq_pass: thermal state once per (sample, time), every filter of the grid
//                 ONCE into LDS as [filter][lane], then per colour (a, b) the value
//                 (m0_a - m0_b) - 2.5 log10(Y_a / Y_b) -- NaN unless both are finite and > 0 -- as series c of the time.
//   k_cq_peak     lane = sample: walks the tile's times in ascending order, recomputes the filters' values and keeps
//                 per filter the sample's largest non-NaN value and the first time it is attained (strict >), in LDS
//                 as [filter][lane]; read from and written to device memory across tiles, as k_lq_peak's are.
// The template form (DESIGN.md "Bands and features of a template fit") is for an engine with a second component attached
// (lcf_engine_set_template): per (sample, time, filter) the base model's value B -- pq_point -- and the template term
// Tm = r_f S_f((t - t_max - dt_f) (1 / s)), with Y = B + Tm the operations of k_template in its order.
//   k_tq_pass     the geometry and modes of k_pq_pass: thermal state once per (sample, time), then per filter B and Tm;
//                 the series of a time are component x filter (Y, B, Tm: those the caller's mask names).  The knots and
//                 the cubic coefficients of every filter are staged in LDS where they fit beside the histograms (lanes
//                 are samples: their spline intervals diverge).  In mode 0 it also counts, per (time, filter), the
//                 samples whose B is exactly +0 (the shock has not started), as k_kq_pass counts its dark ones.
//   k_tq_features lane = sample, one launch over all samples: per filter the times are walked once in ascending order
//                 for the largest non-NaN B and Tm (first occurrence, strict >) and the first time with Tm > B, then the
//                 times between the two peaks for the smallest non-NaN Y (the dip), B and Tm recomputed.
// k_pq_pick and k_pq_finish serve all forms; the host driver (quantile_run) differs in the launches only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "lcf.h"
#include "lcf_device.h"
#include "lcf_host.h"
#include "lcf_internal.h"
#include "lcf_keys.h"
#include "lcf_template.h"

using namespace lcf;

namespace {

constexpr int kPqThreads = 512;            // lanes of a pass workgroup (8 waves)
constexpr int kPqCap = 2048;               // keys a search sorts in LDS
constexpr int kPqHistBytes = 48 * 1024;    // LDS histogram counters of a pass workgroup
constexpr int kPqMaxSearch = 512;          // filters x percentiles of one call
constexpr int kPqMinBits = 4, kPqMaxBits = 11;
constexpr unsigned long long kNoKey = ~0ull;

struct PqSearch {
    unsigned long long prefix;   // the top `pbits` bits shared by the keys still in question
    unsigned long long succ;     // smallest key above all of them (mode 2)
    long long rank;              // wanted order statistic among the keys with the prefix
    long long count;             // keys with the prefix
    double gamma;                // weight of order statistic rank + 1
    int pbits;                   // -1: the point has no valid value
    unsigned int fill;           // keys collected so far (mode 2)
    int active;                  // still more than kPqCap keys and bits left: another histogram pass
    int collect;                 // at most kPqCap keys: they are collected and sorted
};

struct PqArgs {
    const double* base;          // sample s = the row at base + (s / n_w) * step_stride + (s % n_w) * ld
    long long n, n_w, step_stride;
    int ld;
    const double* coef;          // [kNCoef][n]
    const int* orig;             // [n_epochs][n_filters]: the point's index in the caller's order, -1 = no such point
    int ep0;                     // first time of the tile
    int n_q, component, mode, shift, bits;
    long long chunk;             // samples per workgroup
    unsigned int* hist;          // mode 0: [tile time][filter][1 << bits], mode 1: [search][1 << bits]
    PqSearch* search;            // [tile time][filter][percentile]
    unsigned long long* buf;     // [search][kPqCap]
};

// (pq_key / pq_value -- doubles ordered as unsigned integers -- are in lcf_keys.h: k_lq_eval writes them too)

// ln S_f(e^u) from the filter's interpolant in device memory (the form of the likelihood kernels: interval of the
// coordinate r, Horner's rule on 8 coefficients)
__device__ __forceinline__ double pq_interp(const DevProblem& pb, int filt, double r) {
    const int j = (int)r;
    const double s = fma(__builtin_amdgcn_fract(r), 2., -1.);
    const double2* q = reinterpret_cast<const double2*>(pb.itab + filt * pb.itab_m * 8 + 8 * j);
    const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    double g = fma(q0.x, s, q0.y);
    g = fma(g, s, q1.x);
    g = fma(g, s, q1.y);
    g = fma(g, s, q2.x);
    g = fma(g, s, q2.y);
    g = fma(g, s, q3.x);
    return fma(g, s, q3.y);
}

// Band sum over the shortest table that is valid at 1/T, chosen per LANE (lanes are samples here: a value must not
// depend on which samples share a wave).
__device__ __forceinline__ double pq_band_sum(const DevProblem& pb, const FiltDesc& fd, double invT, const ExpTab et) {
    int off = fd.off, cnt = fd.cnt;
    if (pb.use_ctab && fd.ccnt > 0 && invT <= fd.inv_tmin) off = fd.coff, cnt = fd.ccnt;
    if (pb.use_ctab && fd.hcnt > 0 && invT <= fd.inv_tmin2) off = fd.hoff, cnt = fd.hcnt;
    if (cnt <= 0) return 0.;
    const double2* tab = pb.tab + off;
    if (pb.variant == 0) return band_sum_ref(tab, cnt, invT);
    const double amax = fmax(tab[0].x, tab[cnt - 1].x);
    if (amax * invT < 170.) return band_sum_main(tab, cnt, invT * kInvLn2N, et);
    return band_sum_safe(tab, cnt, -(invT * kInvLn2N), et);
}

// The model at (sample, time t_in, filter f) from the thermal state (x, p) in the encoding of thermal_state_log.
// component 1 (companion-shocking models): the SiFTO term alone.
template <int MODEL>
__device__ __forceinline__ double pq_point(const DevProblem& pb, const double* __restrict__ c,
                                           const double* __restrict__ prow, double t_in, int f, double x, double p,
                                           const ExpTab et, int component) {
    const int model = MODEL ? MODEL : pb.model;
    const bool companion = model >= kCompanion && model <= kCompanion3;
    const FiltDesc fd = pb.f_desc[f];
    double y = 0.;
    if (!(companion && component == 1)) {
        double invT = 0., pref = 0.;
        bool done = false;
        if (__double2hiint(x) >= 0) {   // log-space state: x = interval coordinate of ln T, p = ln R_bb^2
            // (ShockCooling4 also needs the band sum at 0.74 T: ln 0.74 / h intervals lower)
            const double r_low = model == kShockCooling4 ? x - 0.3011050927839216 * pb.itab_inv_h : x;
            if (r_low >= (double)fd.r_min) {
                double L = pq_interp(pb, f, x);
                if (model == kShockCooling4)   // min(blackbody, suppressed blackbody at 0.74 T), models.py:629-631
                    L = fmin(L, pq_interp(pb, f, x - 0.3011050927839216 * pb.itab_inv_h) + 1.2044203711356864);
                y = exp_scaled<false>(fma(L, kInvLn2N, p * kInvLn2N), et);
                done = true;
            } else {   // outside this filter's proved range: the sample tables, in linear space
                invT = exp(-fma(x, 1. / pb.itab_inv_h, pb.itab_u0));
                pref = exp(p);
            }
        } else {
            invT = -x;
            pref = p;
        }
        if (!done) {
            double S = 0.;
            if (invT > 0.) {
                if (model == kShockCooling3) {   // the sample's reddening, sample by sample over the full table
                    for (int k = 0; k < fd.cnt; ++k) {
                        const double2 aw = pb.tab[fd.off + k];
                        S += aw.y * exp2(-c[6] * pb.tab_ext[fd.off + k]) / expm1(aw.x * invT);
                    }
                } else {
                    S = pq_band_sum(pb, fd, invT, et);
                    if (model == kShockCooling4)
                        S = fmin(S, pq_band_sum(pb, fd, invT * (1. / 0.74), et) * (1. / (0.74 * 0.74 * 0.74 * 0.74)));
                }
            }
            y = (pref != pref) ? pref : pref * S;   // (pref may be NaN, or 0 with 1/T == 0)
        }
        if (model == kShockCooling3) y *= c[5];   // models.py:495
    }
    if (companion) {   // models.py:909-917, 977-980, 1040-1045
        const double kfac = c[5] * (fd.kpar >= 0 ? prow[fd.kpar] : 1.);
        const double sfac = fd.spar >= 0 ? prow[fd.spar] : 1.;
        const double dt = fd.dtpar >= 0 ? prow[fd.dtpar] : 0.;
        const double u = (t_in - c[3] - dt) * (1. / c[4]);
        double tmpl;
        if (pb.knot_h > 0.)
            tmpl = spline_eval_uniform(pb, reinterpret_cast<const double2*>(pb.spl) + f * (pb.n_knots - 1) * 2, u);
        else
            tmpl = spline_eval(pb.knots, pb.n_knots, pb.spl + (size_t)f * (pb.n_knots - 1) * 4, u, pb.knot_inv_h);
        y = component == 1 ? tmpl * sfac : y * kfac + tmpl * sfac;
    }
    return y;
}

__device__ __forceinline__ const double* pq_row(const PqArgs& a, long long s) {
    return a.base + (s / a.n_w) * a.step_stride + (s % a.n_w) * a.ld;
}

// What both pass kernels do with the values of a point.  Per search in LDS: prefix, successor, prefix bits, collect
// flag; behind them the histogram counters.
struct PqLds {
    unsigned long long *prefix, *succ;
    int *pbits, *col;
    unsigned int* hist;
};

// The searches' LDS at `at` (8-byte aligned): counters zeroed, the tile time's searches loaded (modes 1, 2).  The caller
// synchronises.
__device__ __forceinline__ PqLds pq_lds_setup(const PqArgs& a, void* at, const PqSearch* search, int ns, int n_hist,
                                              int tid) {
    PqLds s;
    s.prefix = reinterpret_cast<unsigned long long*>(at);
    s.succ = s.prefix + ns;
    s.pbits = reinterpret_cast<int*>(s.succ + ns);
    s.col = s.pbits + ns;
    s.hist = reinterpret_cast<unsigned int*>(s.col + ns);
    for (int k = tid; k < n_hist; k += kPqThreads) s.hist[k] = 0u;
    if (a.mode != 0)
        for (int k = tid; k < ns; k += kPqThreads) {
            const PqSearch sr = search[k];
            s.prefix[k] = sr.prefix;
            s.succ[k] = kNoKey;
            s.pbits[k] = (a.mode == 1 ? sr.active != 0 : sr.pbits > 0) ? sr.pbits : -1;
            s.col[k] = sr.collect;
        }
    return s;
}

// The value v of (this lane's sample, series f of the workgroup's time) enters the histograms (modes 0, 1) or the
// searches' buffers and successors (mode 2).
__device__ __forceinline__ void pq_consume(const PqArgs& a, const PqLds& s, PqSearch* search, int ns, int f, double v,
                                           int lane, unsigned int mask) {
    const bool valid = v == v;
    const unsigned long long key = pq_key(v);
    if (a.mode == 0) {
        // (the values of a point mostly share their exponent: lanes with the same bin add once, together)
        const int bin = (int)(key >> a.shift);
        unsigned long long m = __builtin_amdgcn_ballot_w64(valid);
        while (m) {
            const int leader = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(m));
            const int b0 = __builtin_amdgcn_readlane(bin, leader);
            const unsigned long long peers = __builtin_amdgcn_ballot_w64(valid && bin == b0);
            if (lane == leader) atomicAdd(&s.hist[(f << a.bits) + b0], (unsigned int)__popcll(peers));
            m &= ~peers;
        }
    } else if (valid) {
        for (int j = 0; j < a.n_q; ++j) {
            const int k = f * a.n_q + j, pbits = s.pbits[k];
            if (pbits < 0) continue;
            const unsigned long long pre = s.prefix[k];
            if (a.mode == 1) {   // (every active search has the same 64 - shift - bits prefix bits)
                // One ds_add per lane.  (Measured and not kept: a round of the sharing above in front of it --
                // the first refinement, whose keys still crowd into a few bins, 76 -> 66 ms, the second, whose
                // keys are spread, 46 -> 60 ms at 2 048 000 samples x 6000 points.)
                if ((key >> (a.shift + a.bits)) == pre)
                    atomicAdd(&s.hist[(k << a.bits) + (int)((unsigned int)(key >> a.shift) & mask)], 1u);
            } else {
                const unsigned long long head = pbits >= 64 ? key : key >> (64 - pbits);
                if (head == pre) {
                    if (s.col[k]) {
                        const unsigned int at = atomicAdd(&search[k].fill, 1u);
                        if (at < (unsigned int)kPqCap) a.buf[((size_t)blockIdx.x * ns + k) * kPqCap + at] = key;
                    }
                } else if (head > pre && key < s.succ[k]) {
                    atomicMin(&s.succ[k], key);
                }
            }
        }
    }
}

// After the workgroup's last value (and a barrier): its histogram, or its successors, join the tile time's.
__device__ __forceinline__ void pq_merge(const PqArgs& a, const PqLds& s, PqSearch* search, int ns, int n_hist, int tid) {
    if (a.mode == 2) {
        for (int k = tid; k < ns; k += kPqThreads)
            if (s.succ[k] != kNoKey) atomicMin(&search[k].succ, s.succ[k]);
    } else {
        unsigned int* g = a.hist + (size_t)blockIdx.x * n_hist;
        for (int k = tid; k < n_hist; k += kPqThreads) {
            const unsigned int v = s.hist[k];
            if (v) atomicAdd(&g[k], v);
        }
    }
}

__global__ __launch_bounds__(256) void k_pq_coef(const DevProblem pb, const PqArgs a, double* __restrict__ coef) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n) return;
    double c[kNCoef];
    walker_coefficients(pb, pq_row(a, s), c);
    for (int i = 0; i < kNCoef; ++i) coef[(long long)i * a.n + s] = c[i];
}

// blockIdx.x = time of the tile, blockIdx.y = chunk of samples.  Dynamic LDS: exp table | per search prefix, successor,
// prefix bits, collect flag | histogram counters.
template <int MODEL>
__global__ __launch_bounds__(kPqThreads) void k_pq_pass(const DevProblem pb, const PqArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int nf = pb.n_filters, ns = nf * a.n_q;
    double* exptab = reinterpret_cast<double*>(smem);

    const int model = MODEL ? MODEL : pb.model;
    const bool companion = model >= kCompanion && model <= kCompanion3;
    const int tid = threadIdx.x, lane = tid & 63;
    const int ep = a.ep0 + blockIdx.x;
    const int n_hist = a.mode == 0 ? nf << a.bits : a.mode == 1 ? ns << a.bits : 0;
    PqSearch* search = a.search + (size_t)blockIdx.x * ns;
    for (int k = tid; k < kExpTabSize; k += kPqThreads) exptab[k] = pb.exp2tab[k];
    const PqLds lds = pq_lds_setup(a, exptab + kExpTabSize, search, ns, n_hist, tid);
    __syncthreads();

    const ExpTab et{exptab};
    const double t_in = pb.epoch_t[ep];
    const int* orig = a.orig + (size_t)ep * nf;
    const bool log_state = pb.variant != 0 && pb.use_itab && model != kShockCooling3;
    const bool sifto_only = companion && a.component == 1;
    const unsigned int mask = (1u << a.bits) - 1u;
    const long long s0 = (long long)blockIdx.y * a.chunk, s1 = min(a.n, s0 + a.chunk);
    for (long long sb = s0; sb < s1; sb += kPqThreads) {
        const long long s = sb + tid;
        if (s >= s1) continue;
        double c[kNCoef];
#pragma unroll
        for (int i = 0; i < kNCoef; ++i) c[i] = a.coef[(long long)i * a.n + s];
        const double* prow = companion ? pq_row(a, s) : a.base;
        double x = -0., p = 0.;
        if (!sifto_only) {
            if (log_state) {
                thermal_state_log<MODEL>(pb, c, t_in, x, p, et);
            } else {
                double T, invT, pref;
                thermal_state<MODEL>(pb, c, t_in, T, invT, pref);
                encode_linear(invT, pref, x, p);
            }
        }
        for (int f = 0; f < nf; ++f) {
            if (orig[f] < 0) continue;
            pq_consume(a, lds, search, ns, f, pq_point<MODEL>(pb, c, prow, t_in, f, x, p, et, a.component), lane, mask);
        }
    }
    __syncthreads();
    pq_merge(a, lds, search, ns, n_hist, tid);
}

// ---- the colour form: the filters of a time once, the colours between them as its series -----------------------------
constexpr int kCqMaxFilters = 16;          // filters of a colour call: 4 KiB of LDS each in a pass workgroup
constexpr int kCqPeakThreads = 256;
constexpr size_t kCqLdsPerCU = 160 * 1024; // LDS of a gfx950 CU: what a pass workgroup's words must stay under

struct CqArgs {
    const int* pairs;            // [n_c][2]: the colour's two filters of the engine
    const double* dzp;           // [n_c]: m0_a - m0_b
    int n_c;
};

struct CqPeak {
    double* best;                // [n_filters][n] largest non-NaN value so far (meaningless while at is -1)
    int* at;                     // [n_filters][n] the first epoch it was attained at, -1: none yet
    int n_ep;                    // times of the tile
};

// The thermal state of (sample, time) in the encoding pq_point reads: what k_pq_pass computes in front of its filters.
template <int MODEL>
__device__ __forceinline__ void cq_state(const DevProblem& pb, const double* __restrict__ c, double t_in, bool log_state,
                                         const ExpTab et, double& x, double& p) {
    x = -0.;
    p = 0.;
    if (log_state) {
        thermal_state_log<MODEL>(pb, c, t_in, x, p, et);
    } else {
        double T, invT, pref;
        thermal_state<MODEL>(pb, c, t_in, T, invT, pref);
        encode_linear(invT, pref, x, p);
    }
}

// The colour of two model values in magnitudes; NaN unless both are finite and positive (not exploded yet: 0; NaN; a
// negative SiFTO tail).  Two roundings, as the NumPy expression has.
__device__ __forceinline__ double cq_color(double ya, double yb, double dzp) {
    const bool ok = ya > 0. && yb > 0. && ya < INFINITY && yb < INFINITY;
    return ok ? __dsub_rn(dzp, __dmul_rn(2.5, log10(ya / yb))) : qnan();
}

// blockIdx.x = time of the tile, blockIdx.y = chunk of samples.  Dynamic LDS: exp table | the filters' values of every
// lane, [filter][lane] (a lane reads what it wrote: no barrier) | per search prefix, successor, prefix bits, collect
// flag | histogram counters.
template <int MODEL>
__global__ __launch_bounds__(kPqThreads) void k_cq_pass(const DevProblem pb, const PqArgs a, const CqArgs cq) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int nf = pb.n_filters, nc = cq.n_c, ns = nc * a.n_q;
    double* exptab = reinterpret_cast<double*>(smem);
    double* yv = exptab + kExpTabSize;

    const int model = MODEL ? MODEL : pb.model;
    const bool companion = model >= kCompanion && model <= kCompanion3;
    const int tid = threadIdx.x, lane = tid & 63;
    const int ep = a.ep0 + blockIdx.x;
    const int n_hist = a.mode == 0 ? nc << a.bits : a.mode == 1 ? ns << a.bits : 0;
    PqSearch* search = a.search + (size_t)blockIdx.x * ns;
    for (int k = tid; k < kExpTabSize; k += kPqThreads) exptab[k] = pb.exp2tab[k];
    const PqLds lds = pq_lds_setup(a, yv + (size_t)nf * kPqThreads, search, ns, n_hist, tid);
    __syncthreads();

    const ExpTab et{exptab};
    const double t_in = pb.epoch_t[ep];
    const bool log_state = pb.variant != 0 && pb.use_itab && model != kShockCooling3;
    const unsigned int mask = (1u << a.bits) - 1u;
    const long long s0 = (long long)blockIdx.y * a.chunk, s1 = min(a.n, s0 + a.chunk);
    for (long long sb = s0; sb < s1; sb += kPqThreads) {
        const long long s = sb + tid;
        if (s >= s1) continue;
        double c[kNCoef];
#pragma unroll
        for (int i = 0; i < kNCoef; ++i) c[i] = a.coef[(long long)i * a.n + s];
        const double* prow = companion ? pq_row(a, s) : a.base;
        double x, p;
        cq_state<MODEL>(pb, c, t_in, log_state, et, x, p);
        for (int f = 0; f < nf; ++f) yv[f * kPqThreads + tid] = pq_point<MODEL>(pb, c, prow, t_in, f, x, p, et, 0);
        for (int k = 0; k < nc; ++k) {
            const double ya = yv[cq.pairs[2 * k] * kPqThreads + tid], yb = yv[cq.pairs[2 * k + 1] * kPqThreads + tid];
            pq_consume(a, lds, search, ns, k, cq_color(ya, yb, cq.dzp[k]), lane, mask);
        }
    }
    __syncthreads();
    pq_merge(a, lds, search, ns, n_hist, tid);
}

// blockIdx.x = chunk of kCqPeakThreads samples, lanes = samples.  Dynamic LDS: best[filter][lane] | at[filter][lane].
template <int MODEL>
__global__ __launch_bounds__(kCqPeakThreads) void k_cq_peak(const DevProblem pb, const PqArgs a, const CqPeak pk) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double exptab[kExpTabSize];
    const int nf = pb.n_filters;
    double* best = reinterpret_cast<double*>(smem);
    int* at = reinterpret_cast<int*>(best + (size_t)nf * kCqPeakThreads);

    const int model = MODEL ? MODEL : pb.model;
    const bool companion = model >= kCompanion && model <= kCompanion3;
    const int tid = threadIdx.x;
    for (int k = tid; k < kExpTabSize; k += kCqPeakThreads) exptab[k] = pb.exp2tab[k];
    __syncthreads();
    const long long s = (long long)blockIdx.x * kCqPeakThreads + tid;
    if (s >= a.n) return;

    const ExpTab et{exptab};
    const bool log_state = pb.variant != 0 && pb.use_itab && model != kShockCooling3;
    double c[kNCoef];
#pragma unroll
    for (int i = 0; i < kNCoef; ++i) c[i] = a.coef[(long long)i * a.n + s];
    const double* prow = companion ? pq_row(a, s) : a.base;
    for (int f = 0; f < nf; ++f) {
        best[f * kCqPeakThreads + tid] = pk.best[(long long)f * a.n + s];
        at[f * kCqPeakThreads + tid] = pk.at[(long long)f * a.n + s];
    }
    for (int i = 0; i < pk.n_ep; ++i) {
        const int ep = a.ep0 + i;
        const double t_in = pb.epoch_t[ep];
        double x, p;
        cq_state<MODEL>(pb, c, t_in, log_state, et, x, p);
        for (int f = 0; f < nf; ++f) {
            const double v = pq_point<MODEL>(pb, c, prow, t_in, f, x, p, et, 0);
            const int k = f * kCqPeakThreads + tid;
            if (v == v && (at[k] < 0 || v > best[k])) {   // (as k_lq_peak: the first occurrence wins)
                best[k] = v;
                at[k] = ep;
            }
        }
    }
    for (int f = 0; f < nf; ++f) {
        pk.best[(long long)f * a.n + s] = best[f * kCqPeakThreads + tid];
        pk.at[(long long)f * a.n + s] = at[f * kCqPeakThreads + tid];
    }
}

// ---- the template form: base, template term and their sum as the series of a (time, filter) -------------------------
constexpr int kTqMaxFilters = 16;          // filters of a template call: a dark counter each in a pass workgroup
constexpr int kTqFeatThreads = 256;
constexpr int kTqValues = 3, kTqIndices = 4;   // per (filter, sample): y_peak_base, y_peak_template, y_dip | their indices, i_cross
enum { kTqTotal = LCF_TEMPLATE_MASK_TOTAL, kTqBase = LCF_TEMPLATE_MASK_BASE, kTqTemplate = LCF_TEMPLATE_MASK_TEMPLATE };

struct TqArgs {
    TemplateDev tp;
    int mask, n_comp;                // the components that are ranked (kTq*), and how many
    int stage;                       // the knots and coefficients are read from LDS
    unsigned long long* n_dark;      // [n_epochs][n_filters] samples whose B is exactly +0
};

struct TqFeatures {
    double* values;                  // [kTqValues][n_filters][n]
    int* indices;                    // [kTqIndices][n_filters][n]: epochs, -1 = none
};

// The knots and every filter's coefficients behind `at` (doubles): n_knots + n_filters (n_knots - 1) 4 of them.  The
// caller synchronises.
__device__ __forceinline__ void tq_stage(const TemplateDev& tp, int nf, double* at, int tid, int threads) {
    const int nk = tp.n_knots, nc = nf * (nk - 1) * 4;
    for (int k = tid; k < nk; k += threads) at[k] = tp.knots[k];
    for (int k = tid; k < nc; k += threads) at[nk + k] = tp.coef[k];
}

// The template term of (row p, filter f) at time t_in: the operations of k_template, in its order.
__device__ __forceinline__ double tq_term(const TemplateDev& tp, const double* __restrict__ knots,
                                          const double* __restrict__ coef, const double* __restrict__ p, int f,
                                          double t_in, double t_max, double inv_s) {
    const int fp = tp.fac[f], op = tp.off[f];
    const double fac = fp >= 0 ? p[fp] : 1.;
    const double dt = op >= 0 ? p[op] : 0.;
    const double x = (t_in - t_max - dt) * inv_s;
    return __dmul_rn(fac, spline_eval(knots, tp.n_knots, coef + (size_t)f * (tp.n_knots - 1) * 4, x, tp.inv_h));
}

// blockIdx.x = time of the tile, blockIdx.y = chunk of samples.  Dynamic LDS: exp table | dark counters [kTqMaxFilters]
// | knots and coefficients (tq.stage) | per search prefix, successor, prefix bits, collect flag | histogram counters.
template <int MODEL>
__global__ __launch_bounds__(kPqThreads) void k_tq_pass(const DevProblem pb, const PqArgs a, const TqArgs tq) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int nf = pb.n_filters, nk = tq.tp.n_knots, ns = tq.n_comp * nf * a.n_q;
    double* exptab = reinterpret_cast<double*>(smem);
    unsigned int* s_dark = reinterpret_cast<unsigned int*>(exptab + kExpTabSize);
    double* l_knots = exptab + kExpTabSize + kTqMaxFilters / 2;
    double* l_coef = l_knots + nk;
    double* words = tq.stage ? l_coef + (size_t)nf * (nk - 1) * 4 : l_knots;

    const int model = MODEL ? MODEL : pb.model;
    const int tid = threadIdx.x, lane = tid & 63;
    const int ep = a.ep0 + blockIdx.x;
    const int n_hist = a.mode == 0 ? (tq.n_comp * nf) << a.bits : a.mode == 1 ? ns << a.bits : 0;
    PqSearch* search = a.search + (size_t)blockIdx.x * ns;
    for (int k = tid; k < kExpTabSize; k += kPqThreads) exptab[k] = pb.exp2tab[k];
    if (tid < kTqMaxFilters) s_dark[tid] = 0u;
    if (tq.stage) tq_stage(tq.tp, nf, l_knots, tid, kPqThreads);
    const PqLds lds = pq_lds_setup(a, words, search, ns, n_hist, tid);
    __syncthreads();

    const ExpTab et{exptab};
    const double t_in = pb.epoch_t[ep];
    const bool log_state = pb.variant != 0 && pb.use_itab && model != kShockCooling3;
    const unsigned int mask = (1u << a.bits) - 1u;
    const long long s0 = (long long)blockIdx.y * a.chunk, s1 = min(a.n, s0 + a.chunk);
    for (long long sb = s0; sb < s1; sb += kPqThreads) {
        const long long s = sb + tid;
        if (s >= s1) continue;
        double c[kNCoef];
#pragma unroll
        for (int i = 0; i < kNCoef; ++i) c[i] = a.coef[(long long)i * a.n + s];
        const double* prow = pq_row(a, s);
        const double t_max = prow[tq.tp.i_tmax];
        const double inv_s = 1. / prow[tq.tp.i_s];
        double x, p;
        cq_state<MODEL>(pb, c, t_in, log_state, et, x, p);
        for (int f = 0; f < nf; ++f) {
            const double B = pq_point<MODEL>(pb, c, prow, t_in, f, x, p, et, 0);
            const double Tm = tq.stage ? tq_term(tq.tp, l_knots, l_coef, prow, f, t_in, t_max, inv_s)
                                       : tq_term(tq.tp, tq.tp.knots, tq.tp.coef, prow, f, t_in, t_max, inv_s);
            if (a.mode == 0) {   // (wave-uniform: one LDS add per wave and filter)
                const unsigned long long dark = __builtin_amdgcn_ballot_w64(__double_as_longlong(B) == 0LL);
                if (dark && lane == (int)__builtin_ctzll(dark)) atomicAdd(&s_dark[f], (unsigned int)__popcll(dark));
            }
            int k = 0;
            if (tq.mask & kTqTotal) pq_consume(a, lds, search, ns, k++ * nf + f, __dadd_rn(B, Tm), lane, mask);
            if (tq.mask & kTqBase) pq_consume(a, lds, search, ns, k++ * nf + f, B, lane, mask);
            if (tq.mask & kTqTemplate) pq_consume(a, lds, search, ns, k * nf + f, Tm, lane, mask);
        }
    }
    __syncthreads();
    pq_merge(a, lds, search, ns, n_hist, tid);
    if (a.mode == 0 && tid < nf && s_dark[tid]) atomicAdd(&tq.n_dark[(size_t)ep * nf + tid], (unsigned long long)s_dark[tid]);
}

// blockIdx.x = chunk of kTqFeatThreads samples, lanes = samples; every time of the grid, whatever the tiling of the
// passes.  Filters outermost, the running state of one filter in registers; the thermal state is recomputed per filter.
// Dynamic LDS: knots and coefficients (tq.stage).
template <int MODEL>
__global__ __launch_bounds__(kTqFeatThreads) void k_tq_features(const DevProblem pb, const PqArgs a, const TqArgs tq,
                                                               const TqFeatures ft) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double exptab[kExpTabSize];
    const int nf = pb.n_filters, nk = tq.tp.n_knots, n_ep = pb.n_epochs;
    double* l_knots = reinterpret_cast<double*>(smem);
    double* l_coef = l_knots + nk;

    const int model = MODEL ? MODEL : pb.model;
    const int tid = threadIdx.x;
    for (int k = tid; k < kExpTabSize; k += kTqFeatThreads) exptab[k] = pb.exp2tab[k];
    if (tq.stage) tq_stage(tq.tp, nf, l_knots, tid, kTqFeatThreads);
    __syncthreads();
    const long long s = (long long)blockIdx.x * kTqFeatThreads + tid;
    if (s >= a.n) return;

    const ExpTab et{exptab};
    const bool log_state = pb.variant != 0 && pb.use_itab && model != kShockCooling3;
    double c[kNCoef];
#pragma unroll
    for (int i = 0; i < kNCoef; ++i) c[i] = a.coef[(long long)i * a.n + s];
    const double* prow = pq_row(a, s);
    const double t_max = prow[tq.tp.i_tmax];
    const double inv_s = 1. / prow[tq.tp.i_s];
    const size_t plane = (size_t)nf * a.n;
    for (int f = 0; f < nf; ++f) {
        double best_b = 0., best_t = 0., best_y = 0.;
        int at_b = -1, at_t = -1, at_x = -1, at_y = -1;
        for (int i = 0; i < n_ep; ++i) {
            const double t_in = pb.epoch_t[i];
            double x, p;
            cq_state<MODEL>(pb, c, t_in, log_state, et, x, p);
            const double B = pq_point<MODEL>(pb, c, prow, t_in, f, x, p, et, 0);
            const double Tm = tq.stage ? tq_term(tq.tp, l_knots, l_coef, prow, f, t_in, t_max, inv_s)
                                       : tq_term(tq.tp, tq.tp.knots, tq.tp.coef, prow, f, t_in, t_max, inv_s);
            if (B == B && (at_b < 0 || B > best_b)) best_b = B, at_b = i;   // (as k_lq_peak: the first occurrence wins)
            if (Tm == Tm && (at_t < 0 || Tm > best_t)) best_t = Tm, at_t = i;
            if (at_x < 0 && Tm > B) at_x = i;
        }
        if (at_b >= 0 && at_b < at_t)
            for (int i = at_b; i <= at_t; ++i) {
                const double t_in = pb.epoch_t[i];
                double x, p;
                cq_state<MODEL>(pb, c, t_in, log_state, et, x, p);
                const double B = pq_point<MODEL>(pb, c, prow, t_in, f, x, p, et, 0);
                const double Tm = tq.stage ? tq_term(tq.tp, l_knots, l_coef, prow, f, t_in, t_max, inv_s)
                                           : tq_term(tq.tp, tq.tp.knots, tq.tp.coef, prow, f, t_in, t_max, inv_s);
                const double Y = __dadd_rn(B, Tm);
                if (Y == Y && (at_y < 0 || Y < best_y)) best_y = Y, at_y = i;
            }
        const size_t o = (size_t)f * a.n + s;
        ft.values[o] = best_b;
        ft.values[plane + o] = best_t;
        ft.values[2 * plane + o] = best_y;
        ft.indices[o] = at_b;
        ft.indices[plane + o] = at_t;
        ft.indices[2 * plane + o] = at_x;
        ft.indices[3 * plane + o] = at_y;
    }
}

// ---- the thermal form: T, R_bb, L_bol as the three series of a time, and the validity counters -----------------------
constexpr int kThSeries = 3;
constexpr double kThSigmaSB = 2.744452656619892e+28;   // W (1000 Rsun)^-2 kK^-4: kSigmaSB of lcf_bolo.hip
constexpr double kThFourPi = 12.566370614359172;

struct ThArgs {
    double* win;                     // [2][n]: t_min, t_max of every sample
    double T_floor;
    unsigned long long* n_cold;      // [n_epochs] samples with T < T_floor
    unsigned long long* n_inside;    // [n_epochs] samples with t_min <= t <= t_max
};

// max / min that keep a NaN, as np.maximum / np.minimum do (models.py:287, 657)
__device__ __forceinline__ double th_max(double a, double b) { return a != a ? a : b != b ? b : fmax(a, b); }
__device__ __forceinline__ double th_min(double a, double b) { return a != a ? a : b != b ? b : fmin(a, b); }

// The times between which the model of parameter row p holds, kappa = 1: the t_min / t_max methods of the reference
// (models.py:276-298, 414-430, 499-504, 634-657, 830-845).  c: the row's walker_coefficients.  A NaN means "never".
__device__ inline void th_window(const DevProblem& pb, const double* __restrict__ p, const double* __restrict__ c,
                                 double& t_lo, double& t_hi) {
    const double* k = pb.consts;
    const double t0 = c[0];
    switch (pb.model) {
        case kShockCooling:
        case kShockCooling3: {
            const double v = p[0], f = p[2], R = p[3];
            t_lo = 0.2 * R / v * th_max(0.5, pow(R, 0.4) * pow(f, -0.2) * pow(v, -0.7)) + t0;
            t_hi = 7.4 * pow(R, 0.55) + t0;
            break;
        }
        case kShockCooling2:   // (no lower bound; 8.12 kK = 0.7 eV; epsilon_T = 2 epsilon_1 - 0.5)
            t_lo = -INFINITY;
            t_hi = pow(8.12 / p[0], 1. / (2. * k[3] - 0.5)) + t0;
            break;
        case kShockCooling4: {   // (19.5 ** sqrt(...): the reference's, kept; k[6] = 19.5, k[1] = a)
            const double v = p[0], M = p[1], f = p[2], R = p[3];
            t_lo = 0.012 * R + t0;
            t_hi = th_min(6.86 * pow(R, 0.56) * pow(v, 0.16) * pow(f, -0.06), pow(k[6], sqrt(M / v)) / k[1]) + t0;
            break;
        }
        case kCompanion:
        case kCompanion2:
        case kCompanion3:   // the template's first and last epoch at the sample's stretch, about its t_peak
            t_lo = c[3] + c[4] * pb.knot0;
            t_hi = c[3] + c[4] * pb.knot_last;
            break;
        default:
            t_lo = t_hi = qnan();
            break;
    }
}

__global__ __launch_bounds__(256) void k_th_sample(const DevProblem pb, const PqArgs a, double* __restrict__ coef,
                                                   double* __restrict__ win) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n) return;
    const double* p = pq_row(a, s);
    double c[kNCoef], t_lo, t_hi;
    walker_coefficients(pb, p, c);
    th_window(pb, p, c, t_lo, t_hi);
    for (int i = 0; i < kNCoef; ++i) coef[(long long)i * a.n + s] = c[i];
    win[s] = t_lo;
    win[a.n + s] = t_hi;
}

// blockIdx.x = time of the tile, blockIdx.y = chunk of samples.  Dynamic LDS: per search prefix, successor, prefix
// bits, collect flag | histogram counters.
template <int MODEL>
__global__ __launch_bounds__(kPqThreads) void k_th_pass(const DevProblem pb, const PqArgs a, const ThArgs th) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ unsigned int s_count[2];
    const int ns = kThSeries * a.n_q;
    const int tid = threadIdx.x, lane = tid & 63;
    const int ep = a.ep0 + blockIdx.x;
    const int n_hist = a.mode == 0 ? kThSeries << a.bits : a.mode == 1 ? ns << a.bits : 0;
    PqSearch* search = a.search + (size_t)blockIdx.x * ns;
    const PqLds lds = pq_lds_setup(a, smem, search, ns, n_hist, tid);
    if (tid < 2) s_count[tid] = 0u;
    __syncthreads();

    const double t_in = pb.epoch_t[ep];
    const unsigned int mask = (1u << a.bits) - 1u;
    const long long s0 = (long long)blockIdx.y * a.chunk, s1 = min(a.n, s0 + a.chunk);
    unsigned int cold = 0u, inside = 0u;   // of this wave's samples (wave-uniform)
    for (long long sb = s0; sb < s1; sb += kPqThreads) {
        const long long s = sb + tid;
        if (s >= s1) continue;
        double c[kNCoef];
#pragma unroll
        for (int i = 0; i < kNCoef; ++i) c[i] = a.coef[(long long)i * a.n + s];
        double T, invT, pref;
        thermal_state<MODEL>(pb, c, t_in, T, invT, pref);   // (what mode 2 of k_points evaluates)
        const double R = sqrt(pref), T2 = T * T;
        const double v[kThSeries] = {T, R, kThFourPi * (R * R) * kThSigmaSB * (T2 * T2)};
        if (a.mode == 0) {
            const double t_lo = th.win[s], t_hi = th.win[a.n + s];
            cold += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(T < th.T_floor));
            inside += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(t_lo <= t_in && t_in <= t_hi));
        }
#pragma unroll
        for (int f = 0; f < kThSeries; ++f) pq_consume(a, lds, search, ns, f, v[f], lane, mask);
    }
    if (a.mode == 0 && lane == 0) {
        atomicAdd(&s_count[0], cold);
        atomicAdd(&s_count[1], inside);
    }
    __syncthreads();
    pq_merge(a, lds, search, ns, n_hist, tid);
    if (a.mode == 0 && tid == 0) {
        atomicAdd(&th.n_cold[ep], (unsigned long long)s_count[0]);
        atomicAdd(&th.n_inside[ep], (unsigned long long)s_count[1]);
    }
}

// ---- the luminosity form: one series per time, its keys evaluated once and stored -------------------------------------
constexpr unsigned long long kKeyPlusZero = 0x8000000000000000ull;   // pq_key(+0.)

struct KqArgs {
    const unsigned long long* keys;   // [tile time][n]
    unsigned long long* n_dark;       // [n_epochs] samples whose L is exactly +0
};

// blockIdx.x = time of the tile, blockIdx.y = chunk of samples.  Dynamic LDS: per search prefix, successor, prefix
// bits, collect flag | histogram counters.
__global__ __launch_bounds__(kPqThreads) void k_kq_pass(const PqArgs a, const KqArgs kq) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ unsigned int s_dark;
    const int ns = a.n_q;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n_hist = a.mode == 0 ? 1 << a.bits : a.mode == 1 ? ns << a.bits : 0;
    PqSearch* search = a.search + (size_t)blockIdx.x * ns;
    const PqLds lds = pq_lds_setup(a, smem, search, ns, n_hist, tid);
    if (tid == 0) s_dark = 0u;
    __syncthreads();

    const unsigned long long* keys = kq.keys + (size_t)blockIdx.x * a.n;
    const unsigned int mask = (1u << a.bits) - 1u;
    const long long s0 = (long long)blockIdx.y * a.chunk, s1 = min(a.n, s0 + a.chunk);
    unsigned int dark = 0u;   // of this wave's samples (wave-uniform)
    for (long long sb = s0; sb < s1; sb += kPqThreads) {
        const long long s = sb + tid;
        if (s >= s1) continue;
        const unsigned long long key = keys[s];
        if (a.mode == 0) dark += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(key == kKeyPlusZero));
        pq_consume(a, lds, search, ns, 0, pq_value(key), lane, mask);   // (a NaN is dropped there)
    }
    if (a.mode == 0 && lane == 0) atomicAdd(&s_dark, dark);
    __syncthreads();
    pq_merge(a, lds, search, ns, n_hist, tid);
    if (a.mode == 0 && tid == 0) atomicAdd(&kq.n_dark[a.ep0 + blockIdx.x], (unsigned long long)s_dark);
}

struct LqPeak {
    const unsigned long long* keys;   // [tile time][n]
    long long n;
    int ep0, n_ep;
    double* best;                     // [n] largest non-NaN L so far (meaningless while at is -1)
    int* at;                          // [n] the first epoch it was attained at, -1: none yet
};

__global__ __launch_bounds__(256) void k_lq_peak(const LqPeak a) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n) return;
    double best = a.best[s];
    int at = a.at[s];
    for (int i = 0; i < a.n_ep; ++i) {
        const double v = pq_value(a.keys[(size_t)i * a.n + s]);
        if (v == v && (at < 0 || v > best)) {   // (as values, not keys: -0 does not lose to a later +0, np.nanargmax)
            best = v;
            at = a.ep0 + i;
        }
    }
    a.best[s] = best;
    a.at[s] = at;
}

struct PqPick {
    const unsigned int* hist;
    PqSearch* search;
    const int* orig;             // of the tile's first time
    const double* qf;            // [n_q] percentiles / 100
    long long* n_valid;          // [n_points]
    unsigned int* n_active;
    int n_q, bits, mode;
};

// One workgroup per search of the tile.  mode 0: the point's histogram of the top bits -> n_valid, the wanted rank
// h = (n_valid - 1) q / 100 (NumPy's virtual index, default method) and its bin; mode 1: the search's own histogram.
__global__ __launch_bounds__(256) void k_pq_pick(const PqPick a) {
    __shared__ unsigned long long part[256];
    const int g = blockIdx.x, j = g % a.n_q, pf = g / a.n_q, tid = threadIdx.x;
    PqSearch* sr = a.search + g;
    if (a.mode == 1 && !sr->active) return;
    const int nb = 1 << a.bits, seg = (nb + 255) / 256;
    const unsigned int* row = a.hist + ((size_t)(a.mode == 0 ? pf : g) << a.bits);
    unsigned long long sum = 0;
    for (int b = tid * seg; b < min(nb, (tid + 1) * seg); ++b) sum += row[b];
    part[tid] = sum;
    __syncthreads();
    if (tid != 0) return;
    long long rank;
    int pbits;
    unsigned long long prefix;
    if (a.mode == 0) {
        unsigned long long total = 0;
        for (int t = 0; t < 256; ++t) total += part[t];
        const int o = a.orig[pf];
        if (j == 0 && o >= 0) a.n_valid[o] = (long long)total;
        sr->succ = kNoKey;
        sr->fill = 0u;
        if (total == 0) {
            sr->prefix = 0;
            sr->rank = sr->count = 0;
            sr->gamma = 0.;
            sr->pbits = -1;
            sr->active = sr->collect = 0;
            return;
        }
        const double h = (double)(long long)(total - 1) * a.qf[j], lo = floor(h);
        rank = (long long)lo;
        sr->gamma = h - lo;
        pbits = 0;
        prefix = 0;
    } else {
        rank = sr->rank;
        pbits = sr->pbits;
        prefix = sr->prefix;
    }
    unsigned long long cum = 0;
    int t = 0;
    while (t < 255 && cum + part[t] <= (unsigned long long)rank) cum += part[t++];
    int b = min(t * seg, nb - 1);
    while (b < nb - 1 && cum + row[b] <= (unsigned long long)rank) cum += row[b++];
    const long long count = row[b];
    pbits += a.bits;
    sr->prefix = (prefix << a.bits) | (unsigned long long)b;
    sr->pbits = pbits;
    sr->rank = rank - (long long)cum;
    sr->count = count;
    sr->active = count > kPqCap && pbits < 64;
    sr->collect = count <= kPqCap;
    if (sr->active) atomicAdd(a.n_active, 1u);
}

// One workgroup per search: sort what was collected, take the order statistics, interpolate as NumPy's _lerp does.
__global__ __launch_bounds__(256) void k_pq_finish(const PqSearch* __restrict__ search,
                                                   const unsigned long long* __restrict__ buf,
                                                   const int* __restrict__ orig, int n_q, long long n_points,
                                                   double* __restrict__ out) {
    __shared__ unsigned long long keys[kPqCap];
    const int g = blockIdx.x, j = g % n_q, o = orig[g / n_q], tid = threadIdx.x;
    if (o < 0) return;
    const PqSearch sr = search[g];
    double* dst = out + (long long)j * n_points + o;
    if (sr.pbits < 0) {
        if (tid == 0) *dst = qnan();
        return;
    }
    unsigned long long k_lo, k_hi;
    if (sr.collect) {
        const int n = (int)min((long long)kPqCap, min(sr.count, (long long)sr.fill));
        int np2 = 2;
        while (np2 < n) np2 <<= 1;
        for (int i = tid; i < np2; i += 256) keys[i] = i < n ? buf[(size_t)g * kPqCap + i] : kNoKey;
        __syncthreads();
        for (int k = 2; k <= np2; k <<= 1)
            for (int d = k >> 1; d > 0; d >>= 1) {
                for (int i = tid; i < np2; i += 256) {
                    const int l = i ^ d;
                    if (l > i) {
                        const unsigned long long x = keys[i], y = keys[l];
                        if ((x > y) == ((i & k) == 0)) {
                            keys[i] = y;
                            keys[l] = x;
                        }
                    }
                }
                __syncthreads();
            }
        if (tid != 0) return;
        const int r = (int)min(sr.rank, (long long)max(n - 1, 0));
        k_lo = keys[r];
        k_hi = r + 1 < n ? keys[r + 1] : sr.succ;
    } else {   // more than kPqCap keys and every bit decided: they all are the key `prefix`
        if (tid != 0) return;
        k_lo = sr.prefix;
        k_hi = sr.rank + 1 < sr.count ? sr.prefix : sr.succ;
    }
    const double lo = pq_value(k_lo);
    if (sr.gamma == 0.) {   // the result is an evaluated value itself
        *dst = lo;
        return;
    }
    const double hi = pq_value(k_hi), t = sr.gamma, diff = __dsub_rn(hi, lo);
    *dst = t >= 0.5 ? __dsub_rn(hi, __dmul_rn(diff, __dsub_rn(1., t))) : __dadd_rn(lo, __dmul_rn(diff, t));
}

int hist_bits(long long n_hist, int max_bits) {
    int b = kPqMinBits;
    while (b < max_bits && (n_hist << (b + 1)) * 4 <= kPqHistBytes) ++b;
    return b;
}

// What the two forms do differently on the host: the launch that prepares the samples and the pass launch.
struct PqForm {
    int nf;                // series per time: the filters, T / R_bb / L_bol, or L
    size_t sample_bytes;   // device memory per sample ...
    size_t time_bytes;     // ... and per time of the whole grid, beyond what every form needs
    size_t tile_bytes = 0; // ... and per time of a TILE, beyond the searches' (the stored keys)
    size_t call_bytes = 0; // ... and per call (the colour form's pairs and zero-point differences)
    int gran = 1;          // a tile is a whole multiple of this many "times" (the custom form's units of one time)
    size_t lds_head;       // dynamic LDS of a pass in front of the searches' words and the histograms
    bool coef = true;      // the samples' walker_coefficients are wanted ([kNCoef][n], part of sample_bytes)
    int tile = 0;          // times per tile, set by quantile_run in front of prepare
    virtual lcf_status prepare(DevBuf& mem, PqArgs& a, double* d_coef) = 0;   // ... and whatever else the passes read
    virtual lcf_status pass(const PqArgs& a, int n_ep, size_t lds) = 0;
    virtual ~PqForm() {}
};

template <class Kernel, class... Extra>
lcf_status launch_pass(Kernel kernel, const DevProblem& dp, const PqArgs& a, int n_ep, size_t lds, Extra... extra) {
    const unsigned chunks = (unsigned)((a.n + a.chunk - 1) / a.chunk);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_ep, chunks), dim3(kPqThreads), lds, 0, dp, a, extra...);
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

struct LightCurveForm : PqForm {
    const DevProblem& dp;
    explicit LightCurveForm(const DevProblem& d) : dp(d) {
        nf = d.n_filters;
        sample_bytes = kNCoef * sizeof(double);
        time_bytes = 0;
        lds_head = kExpTabSize * sizeof(double);
    }
    lcf_status prepare(DevBuf&, PqArgs& a, double* d_coef) override {
        hipLaunchKernelGGL(k_pq_coef, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, 0, dp, a, d_coef);
        LCF_HIP(hipGetLastError());
        return LCF_OK;
    }
    lcf_status pass(const PqArgs& a, int n_ep, size_t lds) override {
        if (dp.model == kShockCooling) return launch_pass(k_pq_pass<kShockCooling>, dp, a, n_ep, lds);
        return launch_pass(k_pq_pass<0>, dp, a, n_ep, lds);
    }
};

struct ThermalForm : PqForm {
    const DevProblem& dp;
    ThArgs th{};
    ThermalForm(const DevProblem& d, double T_floor) : dp(d) {
        nf = kThSeries;
        sample_bytes = (kNCoef + 2) * sizeof(double);   // + t_min, t_max
        time_bytes = 2 * sizeof(unsigned long long);    // the two counters
        lds_head = 0;
        th.T_floor = T_floor;
    }
    lcf_status prepare(DevBuf& mem, PqArgs& a, double* d_coef) override {
        lcf_status st;
        if ((st = mem.alloc(&th.win, (size_t)a.n * 2)) || (st = mem.alloc(&th.n_cold, (size_t)dp.n_epochs * 2))) return st;
        th.n_inside = th.n_cold + dp.n_epochs;
        LCF_HIP(hipMemset(th.n_cold, 0, (size_t)dp.n_epochs * 2 * sizeof(unsigned long long)));
        hipLaunchKernelGGL(k_th_sample, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, 0, dp, a, d_coef, th.win);
        LCF_HIP(hipGetLastError());
        return LCF_OK;
    }
    lcf_status pass(const PqArgs& a, int n_ep, size_t lds) override {
        if (dp.model == kShockCooling) return launch_pass(k_th_pass<kShockCooling>, dp, a, n_ep, lds, th);
        return launch_pass(k_th_pass<0>, dp, a, n_ep, lds, th);
    }
};

// Every (sample, time) value is evaluated once per tile, in front of the tile's first pass; the passes read the keys.
struct LuminosityForm : PqForm {
    const DevProblem& dp;
    const ChainView& in;
    const int64_t discard, thin;
    const bool peak;
    int n_cus = 1;
    unsigned long long* keys = nullptr;
    KqArgs kq{};
    LqPeak pk{};
    LuminosityForm(const DevProblem& d, const ChainView& s, int64_t discard_, int64_t thin_, bool want_peak, int cus)
        : dp(d), in(s), discard(discard_), thin(thin_), peak(want_peak), n_cus(cus) {
        nf = 1;
        sample_bytes = want_peak ? sizeof(double) + sizeof(int) : 0;   // the largest L so far and where
        time_bytes = sizeof(unsigned long long);                      // the dark counter
        tile_bytes = (size_t)kept_steps(s, discard, thin).samples * sizeof(unsigned long long);   // the keys
        lds_head = 0;
        coef = false;
    }
    lcf_status prepare(DevBuf& mem, PqArgs& a, double*) override {
        lcf_status st;
        if ((st = mem.alloc(&keys, (size_t)tile * a.n)) || (st = mem.alloc(&kq.n_dark, (size_t)dp.n_points))) return st;
        kq.keys = keys;
        LCF_HIP(hipMemset(kq.n_dark, 0, (size_t)dp.n_points * sizeof(unsigned long long)));
        if (peak) {
            if ((st = mem.alloc(&pk.best, (size_t)a.n)) || (st = mem.alloc(&pk.at, (size_t)a.n))) return st;
            LCF_HIP(hipMemset(pk.best, 0, (size_t)a.n * sizeof(double)));
            LCF_HIP(hipMemset(pk.at, 0xff, (size_t)a.n * sizeof(int)));   // -1
            pk.keys = keys;
            pk.n = a.n;
        }
        return LCF_OK;
    }
    lcf_status pass(const PqArgs& a, int n_ep, size_t lds) override {
        if (a.mode == 0) {   // the tile's first pass: its keys, then the peaks so far (all on the null stream, in order)
            if (lcf_status st = central_keys_launch(dp, in, discard, thin, a.ep0, n_ep, keys, n_cus)) return st;
            if (peak) {
                pk.ep0 = a.ep0;
                pk.n_ep = n_ep;
                hipLaunchKernelGGL(k_lq_peak, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, 0, pk);
                LCF_HIP(hipGetLastError());
            }
        }
        const unsigned chunks = (unsigned)((a.n + a.chunk - 1) / a.chunk);
        hipLaunchKernelGGL(k_kq_pass, dim3((unsigned)n_ep, chunks), dim3(kPqThreads), lds, 0, a, kq);
        LCF_HIP(hipGetLastError());
        return LCF_OK;
    }
};

// Every (sample, time) pair is evaluated once per tile by the custom model's own program, in front of the tile's first
// pass.  What quantile_run and k_kq_pass call a time is here a unit: series u % (n_filters + 3) of time u / (n_filters + 3).
struct CustomForm : PqForm {
    lcf_engine* grid;
    const ChainView& in;
    const int64_t discard, thin;
    const double T_floor;   // < 0: nothing is counted
    unsigned long long *keys = nullptr, *n_cold = nullptr;
    KqArgs kq{};
    CustomForm(lcf_engine* g, const ChainView& s, int64_t discard_, int64_t thin_, double floor)
        : grid(g), in(s), discard(discard_), thin(thin_), T_floor(floor) {
        nf = 1;
        gran = g->dp.n_filters + kThSeries;
        sample_bytes = 0;
        time_bytes = 2 * sizeof(unsigned long long);   // per unit: the dark counter; the cold one (used per time)
        tile_bytes = (size_t)kept_steps(s, discard, thin).samples * sizeof(unsigned long long);   // a unit's keys
        lds_head = 0;
        coef = false;
    }
    lcf_status prepare(DevBuf& mem, PqArgs& a, double*) override {
        const size_t n_units = (size_t)grid->dp.n_epochs * gran;
        lcf_status st;
        if ((st = mem.alloc(&keys, (size_t)tile * a.n)) || (st = mem.alloc(&kq.n_dark, n_units)) ||
            (st = mem.alloc(&n_cold, (size_t)grid->dp.n_epochs)))
            return st;
        kq.keys = keys;
        LCF_HIP(hipMemset(kq.n_dark, 0, n_units * sizeof(unsigned long long)));
        LCF_HIP(hipMemset(n_cold, 0, (size_t)grid->dp.n_epochs * sizeof(unsigned long long)));
        return LCF_OK;
    }
    lcf_status pass(const PqArgs& a, int n_ep, size_t lds) override {
        if (a.mode == 0)   // the tile's first pass: its keys (all on the null stream, in order)
            if (lcf_status st = custom_keys_launch(grid, in, discard, thin, a.ep0 / gran, n_ep / gran, T_floor, keys, n_cold))
                return st;
        const unsigned chunks = (unsigned)((a.n + a.chunk - 1) / a.chunk);
        hipLaunchKernelGGL(k_kq_pass, dim3((unsigned)n_ep, chunks), dim3(kPqThreads), lds, 0, a, kq);
        LCF_HIP(hipGetLastError());
        return LCF_OK;
    }
};

// The colours of a time are its series; the filters they are made from are recomputed in every pass, once per (sample,
// time).  The peaks of every (sample, filter) are taken tile by tile in front of the tile's first pass; their two arrays
// are the caller's results and lie outside the workspace.
struct ColorForm : PqForm {
    const DevProblem& dp;
    const int32_t* pairs_host;
    const double* dzp_host;
    const bool peak;
    CqArgs cq{};
    CqPeak pk{};
    ColorForm(const DevProblem& d, int32_t n_c, const int32_t* pairs, const double* dzp, bool want_peak)
        : dp(d), pairs_host(pairs), dzp_host(dzp), peak(want_peak) {
        nf = n_c;
        sample_bytes = kNCoef * sizeof(double);
        time_bytes = 0;
        call_bytes = (size_t)n_c * (2 * sizeof(int) + sizeof(double));
        lds_head = (kExpTabSize + (size_t)d.n_filters * kPqThreads) * sizeof(double);
        cq.n_c = n_c;
    }
    lcf_status prepare(DevBuf& mem, PqArgs& a, double* d_coef) override {
        int* d_pairs;
        double* d_dzp;
        lcf_status st;
        if ((st = mem.put(&d_pairs, pairs_host, (size_t)2 * cq.n_c)) || (st = mem.put(&d_dzp, dzp_host, (size_t)cq.n_c)))
            return st;
        cq.pairs = d_pairs;
        cq.dzp = d_dzp;
        hipLaunchKernelGGL(k_pq_coef, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, 0, dp, a, d_coef);
        LCF_HIP(hipGetLastError());
        if (peak) {
            const size_t n_pk = (size_t)dp.n_filters * a.n;
            if ((st = mem.alloc(&pk.best, n_pk)) || (st = mem.alloc(&pk.at, n_pk))) return st;
            LCF_HIP(hipMemset(pk.best, 0, n_pk * sizeof(double)));
            LCF_HIP(hipMemset(pk.at, 0xff, n_pk * sizeof(int)));   // -1
        }
        return LCF_OK;
    }
    template <int MODEL>
    lcf_status launch(const PqArgs& a, int n_ep, size_t lds) {
        if (a.mode == 0 && peak) {   // the tile's first pass: the peaks so far (all on the null stream, in order)
            pk.n_ep = n_ep;
            const size_t peak_lds = (size_t)dp.n_filters * kCqPeakThreads * (sizeof(double) + sizeof(int));
            hipLaunchKernelGGL(k_cq_peak<MODEL>, dim3((unsigned)((a.n + kCqPeakThreads - 1) / kCqPeakThreads)),
                               dim3(kCqPeakThreads), peak_lds, 0, dp, a, pk);
            LCF_HIP(hipGetLastError());
        }
        // (at most 2 KiB + 16 x 4 KiB + 512 x 24 bytes + kPqHistBytes = 126 KiB: whatever bits quantile_run chose)
        if (lds > kCqLdsPerCU) return fail(LCF_ERR_UNSUPPORTED, "a colour pass needs more LDS than a compute unit has");
        LCF_HIP(prepare_kernel(k_cq_pass<MODEL>, lds));
        return launch_pass(k_cq_pass<MODEL>, dp, a, n_ep, lds, cq);
    }
    lcf_status pass(const PqArgs& a, int n_ep, size_t lds) override {
        if (dp.model == kShockCooling) return launch<kShockCooling>(a, n_ep, lds);
        return launch<0>(a, n_ep, lds);
    }
};

// Bytes of the knots and of every filter's coefficients of the engine's template: what a kernel stages in LDS.
size_t template_table_bytes(const lcf_engine* e) {
    return ((size_t)e->tpl_nk + (size_t)e->dp.n_filters * (e->tpl_nk - 1) * 4) * sizeof(double);
}

// The series of a time are component x filter; B and Tm of every (sample, time, filter) are recomputed in every pass,
// the thermal state once per (sample, time).
struct TemplateForm : PqForm {
    const DevProblem& dp;
    TqArgs tq{};
    TemplateForm(const lcf_engine* e, int mask) : dp(e->dp) {
        tq.tp = template_dev(e);
        tq.mask = mask;
        tq.n_comp = __builtin_popcount((unsigned)mask);
        nf = tq.n_comp * dp.n_filters;
        sample_bytes = kNCoef * sizeof(double);
        time_bytes = (size_t)dp.n_filters * sizeof(unsigned long long);   // the dark counters
        lds_head = kExpTabSize * sizeof(double) + kTqMaxFilters * sizeof(unsigned int);
        // the table goes to LDS when a pass workgroup with the most search words and counters still fits a compute unit
        const size_t most = lds_head + (size_t)kPqMaxSearch * 24 + kPqHistBytes;
        tq.stage = most + template_table_bytes(e) <= kCqLdsPerCU;
        if (tq.stage) lds_head += template_table_bytes(e);
    }
    lcf_status prepare(DevBuf& mem, PqArgs& a, double* d_coef) override {
        const size_t n_cnt = (size_t)dp.n_epochs * dp.n_filters;
        if (lcf_status st = mem.alloc(&tq.n_dark, n_cnt)) return st;
        LCF_HIP(hipMemset(tq.n_dark, 0, n_cnt * sizeof(unsigned long long)));
        hipLaunchKernelGGL(k_pq_coef, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, 0, dp, a, d_coef);
        LCF_HIP(hipGetLastError());
        return LCF_OK;
    }
    template <int MODEL>
    lcf_status launch(const PqArgs& a, int n_ep, size_t lds) {
        if (lds > kCqLdsPerCU) return fail(LCF_ERR_UNSUPPORTED, "a template pass needs more LDS than a compute unit has");
        LCF_HIP(prepare_kernel(k_tq_pass<MODEL>, lds));
        return launch_pass(k_tq_pass<MODEL>, dp, a, n_ep, lds, tq);
    }
    lcf_status pass(const PqArgs& a, int n_ep, size_t lds) override {
        if (dp.model == kShockCooling) return launch<kShockCooling>(a, n_ep, lds);
        return launch<0>(a, n_ep, lds);
    }
};

// The searches of every point (time x series of `form`), the times in tiles that fit the workspace, over the walkers of
// the kept steps of `chain` (device memory) as samples.  orig_host[n_ep_all][nf]: where the point's results go, -1 = no
// such point.  out[n_q][n_points], n_valid[n_points] (host).
lcf_status quantile_run(int32_t device, PqForm& form, int n_ep_all, long long n_points, const ChainView& chain,
                        int64_t discard, int64_t thin, const int32_t* orig_host, int32_t component, const double* q,
                        int32_t n_q, int64_t workspace_bytes, DevBuf& mem, double* out, int64_t* n_valid) {
    if (lcf_status st = use_device(device)) return st;
    const KeptSteps kept = kept_steps(chain, discard, thin);
    const long long n_samples = kept.samples;
    const int nf = form.nf, ns = nf * n_q;
    const int bits0 = hist_bits(nf, kPqMaxBits), bits1 = hist_bits(ns, kPqMaxBits);
    const size_t lds_head = form.lds_head + (size_t)ns * 24;
    // device memory: per sample the coefficients (and window), per point the results, per time of a tile the rest
    const size_t fixed = (size_t)n_samples * form.sample_bytes + (size_t)n_points * (n_q + 1) * 8 +
                         (size_t)n_ep_all * (nf * 4 + form.time_bytes) + form.call_bytes + 4096;
    const size_t hist_ep = std::max((size_t)nf << bits0, (size_t)ns << bits1) * 4;
    const size_t per_ep = hist_ep + (size_t)ns * (sizeof(PqSearch) + (size_t)kPqCap * 8) + form.tile_bytes;
    const size_t gran = (size_t)form.gran;
    if (workspace_bytes < 0 || (size_t)workspace_bytes < fixed + per_ep * gran)
        return fail(LCF_ERR_INVALID_ARGUMENT, "workspace_bytes too small: this call needs at least " +
                                                  std::to_string(fixed + per_ep * gran) + " bytes");
    const int tile = (int)(std::min<size_t>(((size_t)workspace_bytes - fixed) / per_ep, (size_t)n_ep_all) / gran * gran);

    double *d_coef, *d_q, *d_out;
    long long* d_nv;
    int* d_orig;
    unsigned int *d_hist, *d_active;
    PqSearch* d_search;
    unsigned long long* d_buf;
    lcf_status st;
    form.tile = tile;
    if ((st = mem.alloc(&d_coef, form.coef ? (size_t)n_samples * kNCoef : 0)) || (st = mem.alloc(&d_q, n_q)) ||
        (st = mem.alloc(&d_out, (size_t)n_points * n_q)) || (st = mem.alloc(&d_nv, n_points)) ||
        (st = mem.alloc(&d_orig, (size_t)n_ep_all * nf)) || (st = mem.alloc(&d_hist, (size_t)tile * hist_ep / 4)) ||
        (st = mem.alloc(&d_active, 1)) || (st = mem.alloc(&d_search, (size_t)tile * ns)) ||
        (st = mem.alloc(&d_buf, (size_t)tile * ns * kPqCap)))
        return st;
    std::vector<double> qf(q, q + n_q);
    for (double& v : qf) v = v / 100.;
    LCF_HIP(hipMemcpy(d_q, qf.data(), n_q * sizeof(double), hipMemcpyHostToDevice));
    LCF_HIP(hipMemcpy(d_orig, orig_host, (size_t)n_ep_all * nf * sizeof(int), hipMemcpyHostToDevice));
    LCF_HIP(hipMemset(d_nv, 0, n_points * sizeof(long long)));

    PqArgs a{};
    a.base = kept.base;
    a.n = n_samples;
    a.n_w = chain.n_w;
    a.step_stride = kept.step_stride;
    a.ld = chain.ld;
    a.coef = d_coef;
    a.orig = d_orig;
    a.n_q = n_q;
    a.component = component;
    a.hist = d_hist;
    a.search = d_search;
    a.buf = d_buf;
    if ((st = form.prepare(mem, a, d_coef))) return st;

    for (int ep0 = 0; ep0 < n_ep_all; ep0 += tile) {
        const int n_ep = std::min(tile, n_ep_all - ep0);
        // samples per workgroup: enough workgroups to fill the device, few enough that merging a workgroup's
        // histogram stays small next to its evaluations (whole multiples of the workgroup; at most 65535 chunks)
        long long chunk = (n_samples * n_ep / 4096 + kPqThreads - 1) / kPqThreads * kPqThreads;
        chunk = std::min<long long>(std::max<long long>(chunk, 4 * kPqThreads), 64 * kPqThreads);
        chunk = std::max<long long>(chunk, ((n_samples + 65534) / 65535 + kPqThreads - 1) / kPqThreads * kPqThreads);
        a.ep0 = ep0;
        a.chunk = chunk;
        PqPick pk{d_hist, d_search, d_orig + (size_t)ep0 * nf, d_q, d_nv, d_active, n_q, bits0, 0};
        // pass 0: the keys' top bits, one histogram per point
        a.mode = 0;
        a.bits = bits0;
        a.shift = 64 - bits0;
        LCF_HIP(hipMemsetAsync(d_hist, 0, (size_t)n_ep * ((size_t)nf << bits0) * 4, 0));
        LCF_HIP(hipMemsetAsync(d_active, 0, 4, 0));
        if ((st = form.pass(a, n_ep, lds_head + ((size_t)nf << bits0) * 4))) return st;
        hipLaunchKernelGGL(k_pq_pick, dim3((unsigned)(n_ep * ns)), dim3(256), 0, 0, pk);
        LCF_HIP(hipGetLastError());
        // passes 1, 2, ...: the next bits of the keys under every search's prefix, while a search holds too many keys
        for (int pbits = bits0; pbits < 64;) {
            unsigned int active = 0;
            LCF_HIP(hipMemcpy(&active, d_active, 4, hipMemcpyDeviceToHost));
            if (!active) break;
            const int bits = std::min(bits1, 64 - pbits);
            a.mode = 1;
            a.bits = bits;
            a.shift = 64 - pbits - bits;
            LCF_HIP(hipMemsetAsync(d_hist, 0, (size_t)n_ep * ((size_t)ns << bits) * 4, 0));
            LCF_HIP(hipMemsetAsync(d_active, 0, 4, 0));
            if ((st = form.pass(a, n_ep, lds_head + ((size_t)ns << bits) * 4))) return st;
            pk.bits = bits;
            pk.mode = 1;
            hipLaunchKernelGGL(k_pq_pick, dim3((unsigned)(n_ep * ns)), dim3(256), 0, 0, pk);
            LCF_HIP(hipGetLastError());
            pbits += bits;
        }
        // last pass: collect the keys of every search that is down to kPqCap, and every search's successor key
        a.mode = 2;
        a.bits = 0;
        a.shift = 0;
        if ((st = form.pass(a, n_ep, lds_head))) return st;
        hipLaunchKernelGGL(k_pq_finish, dim3((unsigned)(n_ep * ns)), dim3(256), 0, 0, d_search, d_buf,
                           d_orig + (size_t)ep0 * nf, n_q, n_points, d_out);
        LCF_HIP(hipGetLastError());
    }
    LCF_HIP(hipMemcpy(out, d_out, (size_t)n_points * n_q * sizeof(double), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(n_valid, d_nv, (size_t)n_points * sizeof(long long), hipMemcpyDeviceToHost));
    return LCF_OK;
}

// What both predictive entry points check before the device is touched.
lcf_status predict_check(const lcf_engine* grid, int32_t component, const double* q, int32_t n_q, const double* out,
                         const int64_t* n_valid) {
    if (!grid || !q || !out || !n_valid) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = custom_refuse(grid, "a predictive band (lcf_predict_*, lcf_sampler_predict_*)")) return st;
    if (lcf_status st = central_refuse(grid, "a predictive band (lcf_predict_*, lcf_sampler_predict_*)")) return st;
    if (lcf_status st = check_percentiles(q, n_q, INT32_MAX, "need at least one percentile")) return st;
    const bool companion = grid->dp.model >= kCompanion && grid->dp.model <= kCompanion3;
    if (component != 0 && !(component == 1 && companion))
        return fail(LCF_ERR_INVALID_ARGUMENT, "component: 0 = the model, 1 = the SiFTO term of a companion-shocking model");
    if (grid->dp.n_points < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine has no points");
    return LCF_OK;
}

// The grid engine's points as a (time, filter) table -- orig[n_epochs][n_filters]: the index of the point in the
// caller's order, -1 where the grid has no such point -- and the run itself.  out[n_q][n_points], n_valid[n_points].
lcf_status predict_run(lcf_engine* grid, const ChainView& in, int64_t discard, int64_t thin, int32_t component,
                       const double* q, int32_t n_q, int64_t workspace_bytes, double* out, int64_t* n_valid) {
    const DevProblem& dp = grid->dp;
    const int N = dp.n_points, NF = dp.n_filters;
    std::vector<int> filt(N), orig(N), epoch(N);
    LCF_HIP(hipMemcpy(filt.data(), dp.pt_filt, N * sizeof(int), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(orig.data(), dp.pt_orig, N * sizeof(int), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(epoch.data(), dp.pt_epoch, N * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int32_t> table((size_t)dp.n_epochs * NF, -1);
    for (int i = 0; i < N; ++i) {
        int32_t& slot = table[(size_t)epoch[i] * NF + filt[i]];
        if (slot >= 0) return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine holds a (time, filter) pair twice");
        slot = orig[i];
    }
    if (NF * n_q > kPqMaxSearch)
        return fail(LCF_ERR_UNSUPPORTED, "filters x percentiles of one call must not exceed 512");
    LightCurveForm form(dp);
    DevBuf mem;
    return quantile_run(grid->device, form, dp.n_epochs, N, in, discard, thin, table.data(), component, q, n_q,
                        workspace_bytes, mem, out, n_valid);
}

// What both thermal entry points check before the device is touched.
lcf_status thermal_check(const lcf_engine* grid, const double* q, int32_t n_q, const double* out, const int64_t* n_valid,
                         const int64_t* n_cold, const int64_t* n_inside) {
    if (!n_cold || !n_inside) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = predict_check(grid, 0, q, n_q, out, n_valid)) return st;
    if (grid->dp.model == kBlackbody)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the blackbody model has no thermal evolution or validity window");
    if (grid->dp.n_points != grid->dp.n_epochs)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine must hold one point per distinct time");
    return LCF_OK;
}

// Thermal form: quantiles of T, R_bb, L_bol and the validity counters on the distinct times of the grid engine.
// out[3][n_q][n_times], n_valid[3][n_times], n_cold[n_times], n_inside[n_times] (host, caller's order).
lcf_status thermal_run(lcf_engine* grid, const ChainView& in, int64_t discard, int64_t thin, const double* q, int32_t n_q,
                       double T_floor, int64_t workspace_bytes, double* out, int64_t* n_valid, int64_t* n_cold,
                       int64_t* n_inside) {
    const DevProblem& dp = grid->dp;
    const int nt = dp.n_points;
    std::vector<int> pt_orig(nt), epoch(nt);
    LCF_HIP(hipMemcpy(pt_orig.data(), dp.pt_orig, nt * sizeof(int), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(epoch.data(), dp.pt_epoch, nt * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int32_t> time_orig(nt);   // the time's index in the caller's order
    for (int i = 0; i < nt; ++i) time_orig[epoch[i]] = pt_orig[i];   // (N points on N distinct times: a bijection)
    if (kThSeries * n_q > kPqMaxSearch)
        return fail(LCF_ERR_UNSUPPORTED, "3 x percentiles of one call must not exceed 512");
    // the three quantities take the place of a time's filters: point index = quantity * n_times + time
    std::vector<int32_t> orig((size_t)nt * kThSeries);
    for (int ep = 0; ep < nt; ++ep)
        for (int f = 0; f < kThSeries; ++f) orig[(size_t)ep * kThSeries + f] = f * nt + time_orig[ep];
    std::vector<double> by_q((size_t)n_q * kThSeries * nt);
    ThermalForm form(dp, T_floor);
    DevBuf mem;
    if (lcf_status st = quantile_run(grid->device, form, nt, (long long)kThSeries * nt, in, discard, thin, orig.data(), 0,
                                     q, n_q, workspace_bytes, mem, by_q.data(), n_valid))
        return st;
    for (int f = 0; f < kThSeries; ++f)   // [n_q][3][n_times] -> [3][n_q][n_times]
        for (int j = 0; j < n_q; ++j)
            std::copy_n(&by_q[((size_t)j * kThSeries + f) * nt], nt, out + ((size_t)f * n_q + j) * nt);
    // (the counters are per time of the engine's order: to the caller's)
    std::vector<unsigned long long> cnt((size_t)nt * 2);
    LCF_HIP(hipMemcpy(cnt.data(), form.th.n_cold, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int ep = 0; ep < nt; ++ep) {
        n_cold[time_orig[ep]] = (int64_t)cnt[ep];
        n_inside[time_orig[ep]] = (int64_t)cnt[nt + ep];
    }
    return LCF_OK;
}

// The luminosity form on the epochs of the grid engine (a central-engine problem), in their order.  out[n_q][n_points],
// n_valid / n_dark[n_points], L_peak / i_peak[samples] or both nullptr (host).
lcf_status luminosity_run(lcf_engine* grid, const ChainView& in, int64_t discard, int64_t thin, const double* q,
                          int32_t n_q, int64_t workspace_bytes, double* out, int64_t* n_valid, int64_t* n_dark,
                          double* L_peak, int32_t* i_peak) {
    const DevProblem& dp = grid->dp;
    const int nt = dp.n_points;
    const int64_t n = kept_steps(in, discard, thin).samples;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, grid->device) != hipSuccess || cus <= 0) cus = 64;
    std::vector<int32_t> orig(nt);   // one series per epoch, in the engine's own order
    for (int ep = 0; ep < nt; ++ep) orig[ep] = ep;
    LuminosityForm form(dp, in, discard, thin, L_peak != nullptr, cus);
    DevBuf mem;
    if (lcf_status st = quantile_run(grid->device, form, nt, nt, in, discard, thin, orig.data(), 0, q, n_q,
                                     workspace_bytes, mem, out, n_valid))
        return st;
    std::vector<unsigned long long> dark(nt);
    LCF_HIP(hipMemcpy(dark.data(), form.kq.n_dark, (size_t)nt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int ep = 0; ep < nt; ++ep) n_dark[ep] = (int64_t)dark[ep];
    if (L_peak) {
        LCF_HIP(hipMemcpy(L_peak, form.pk.best, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        LCF_HIP(hipMemcpy(i_peak, form.pk.at, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t s = 0; s < n; ++s)
            if (i_peak[s] < 0) L_peak[s] = std::nan("");
    }
    return LCF_OK;
}

// The custom form on the dense filters x distinct-times grid of the grid engine.  out[n_q][n_filters + 3][n_times],
// n_valid[n_filters + 3][n_times], n_dark[n_filters][n_times], n_cold[n_times] or nullptr (host); times ascending.
lcf_status custom_run(lcf_engine* grid, const ChainView& in, int64_t discard, int64_t thin, const double* q, int32_t n_q,
                      double T_floor, int64_t workspace_bytes, double* out, int64_t* n_valid, int64_t* n_dark,
                      int64_t* n_cold) {
    const DevProblem& dp = grid->dp;
    const int N = dp.n_points, NF = dp.n_filters, nt = dp.n_epochs, gran = NF + kThSeries;
    std::vector<int> filt(N), epoch(N);
    LCF_HIP(hipMemcpy(filt.data(), dp.pt_filt, N * sizeof(int), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(epoch.data(), dp.pt_epoch, N * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<char> seen((size_t)nt * NF, 0);
    for (int i = 0; i < N; ++i) {
        char& slot = seen[(size_t)epoch[i] * NF + filt[i]];
        if (slot) return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine holds a (time, filter) pair twice");
        slot = 1;
    }
    if ((long long)N != (long long)nt * NF)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine must hold every filter at every distinct time");
    if ((long long)nt * gran > INT32_MAX) return fail(LCF_ERR_INVALID_ARGUMENT, "too many (time, series) pairs");
    const int n_units = nt * gran;
    std::vector<int32_t> orig(n_units);   // unit (time, series) -> series * n_times + time
    for (int ep = 0; ep < nt; ++ep)
        for (int f = 0; f < gran; ++f) orig[(size_t)ep * gran + f] = f * nt + ep;
    CustomForm form(grid, in, discard, thin, T_floor >= 0. ? T_floor : -1.);
    DevBuf mem;
    if (lcf_status st = quantile_run(grid->device, form, n_units, n_units, in, discard, thin, orig.data(), 0, q, n_q,
                                     workspace_bytes, mem, out, n_valid))
        return st;
    std::vector<unsigned long long> cnt(n_units);
    LCF_HIP(hipMemcpy(cnt.data(), form.kq.n_dark, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int ep = 0; ep < nt; ++ep)
        for (int f = 0; f < NF; ++f) n_dark[(size_t)f * nt + ep] = (int64_t)cnt[(size_t)ep * gran + f];
    if (n_cold) {
        LCF_HIP(hipMemcpy(cnt.data(), form.n_cold, (size_t)nt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int ep = 0; ep < nt; ++ep) n_cold[ep] = T_floor >= 0. ? (int64_t)cnt[ep] : 0;
    }
    return LCF_OK;
}

// What both colour entry points check before the device is touched.
lcf_status color_check(const lcf_engine* grid, int32_t n_c, const int32_t* pairs, const double* dzp, const double* q,
                       int32_t n_q, const double* out, const int64_t* n_valid, const double* y_peak,
                       const int32_t* peak_index) {
    if (!grid || !pairs || !dzp || !q || !out || !n_valid) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if ((y_peak == nullptr) != (peak_index == nullptr))
        return fail(LCF_ERR_INVALID_ARGUMENT, "y_peak and peak_index are given together or not at all");
    if (lcf_status st = custom_refuse(grid, "a colour band (lcf_predict_colors, lcf_sampler_predict_colors)")) return st;
    if (lcf_status st = central_refuse(grid, "a colour band (lcf_predict_colors, lcf_sampler_predict_colors)")) return st;
    if (lcf_status st = check_percentiles(q, n_q, kPqMaxSearch, "need between 1 and 512 percentiles")) return st;
    if (n_c < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "need at least one colour");
    if ((long long)n_c * n_q > kPqMaxSearch)
        return fail(LCF_ERR_UNSUPPORTED, "colours x percentiles of one call must not exceed 512");
    if (grid->dp.n_points < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine has no points");
    if (grid->dp.n_filters > kCqMaxFilters)
        return fail(LCF_ERR_UNSUPPORTED, "a colour call takes a grid engine of at most 16 filters");
    for (int32_t k = 0; k < 2 * n_c; ++k)
        if (pairs[k] < 0 || pairs[k] >= grid->dp.n_filters)
            return fail(LCF_ERR_INVALID_ARGUMENT, "pairs: an index that is not a filter of the grid engine");
    return LCF_OK;
}

// The colour form on the dense filters x distinct-times grid of the grid engine, given filter-major (caller's point
// f * n_times + t is filter f of the engine at the caller's time t).  out[n_q][n_c][n_times], n_valid[n_c][n_times],
// y_peak / peak_index[n_filters][samples] or both nullptr (host); times in the caller's order, peaks walked in
// ascending time.
lcf_status color_run(lcf_engine* grid, const ChainView& in, int64_t discard, int64_t thin, int32_t n_c,
                     const int32_t* pairs, const double* dzp, const double* q, int32_t n_q, int64_t workspace_bytes,
                     double* out, int64_t* n_valid, double* y_peak, int32_t* peak_index) {
    const DevProblem& dp = grid->dp;
    const int N = dp.n_points, NF = dp.n_filters, nt = dp.n_epochs;
    if ((long long)N != (long long)nt * NF)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine must hold every filter at every distinct time");
    if ((long long)nt * n_c > INT32_MAX) return fail(LCF_ERR_INVALID_ARGUMENT, "too many (time, colour) pairs");
    std::vector<int> filt(N), orig(N), epoch(N);
    LCF_HIP(hipMemcpy(filt.data(), dp.pt_filt, N * sizeof(int), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(orig.data(), dp.pt_orig, N * sizeof(int), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(epoch.data(), dp.pt_epoch, N * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int32_t> time_orig(nt, -1);   // the time's index in the caller's order
    std::vector<char> seen((size_t)nt * NF, 0);
    for (int i = 0; i < N; ++i) {
        char& slot = seen[(size_t)epoch[i] * NF + filt[i]];
        int32_t& t_o = time_orig[epoch[i]];
        if (slot) return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine holds a (time, filter) pair twice");
        slot = 1;
        if (orig[i] / nt != filt[i] || (t_o >= 0 && t_o != orig[i] % nt))
            return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine's points must be the dense grid, filter-major");
        t_o = orig[i] % nt;
    }
    std::vector<int32_t> table((size_t)nt * n_c);   // the colours take the place of a time's filters
    for (int ep = 0; ep < nt; ++ep)
        for (int c = 0; c < n_c; ++c) table[(size_t)ep * n_c + c] = c * nt + time_orig[ep];
    const int64_t n = kept_steps(in, discard, thin).samples;
    ColorForm form(dp, n_c, pairs, dzp, y_peak != nullptr);
    DevBuf mem;
    if (lcf_status st = quantile_run(grid->device, form, nt, (long long)n_c * nt, in, discard, thin, table.data(), 0, q,
                                     n_q, workspace_bytes, mem, out, n_valid))
        return st;
    if (y_peak) {
        LCF_HIP(hipMemcpy(y_peak, form.pk.best, (size_t)NF * n * sizeof(double), hipMemcpyDeviceToHost));
        LCF_HIP(hipMemcpy(peak_index, form.pk.at, (size_t)NF * n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < (int64_t)NF * n; ++k) {
            if (peak_index[k] < 0) y_peak[k] = std::nan("");
            else peak_index[k] = time_orig[peak_index[k]];
        }
    }
    return LCF_OK;
}

// n host samples P[n][ld] as one step of n walkers, on the grid engine's device for as long as `mem` lives.
lcf_status uploaded_samples(const lcf_engine* grid, const double* P, int64_t n, int32_t ld, DevBuf& mem, ChainView* in) {
    if (!P || n < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "need at least one sample");
    if (ld < 1 || ld < grid->dp.n_par) return fail(LCF_ERR_INVALID_ARGUMENT, "ld is smaller than the model's parameter count");
    if (n > (1LL << 40) / ld) return fail(LCF_ERR_INVALID_ARGUMENT, "too many samples");
    return upload_chain(grid->device, ChainView{P, nullptr, 1, n, ld, ld}, mem, in);
}

// The sampler's last stored run, where it lies, if it can be read with the grid engine.
lcf_status stored_samples(const lcf_engine* grid, lcf_sampler* s, int64_t discard, int64_t thin, ChainView* in) {
    std::vector<ChainView> chains;
    int32_t device = 0;
    if (lcf_status st = stored_chains(&s, 1, discard, thin, &chains, &device)) return st;
    if (device != grid->device) return fail(LCF_ERR_UNSUPPORTED, "sampler and grid engine are on different devices");
    if (chains[0].n_dim < grid->dp.n_par)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the chain has fewer columns than the model has parameters");
    *in = chains[0];
    return LCF_OK;
}

// What both template entry points check before the device is touched (`what` names the caller).
lcf_status template_check(const lcf_engine* grid, const double* P, int64_t n, int32_t ld, const char* what) {
    if (!grid || !P) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = custom_refuse(grid, what)) return st;
    if (lcf_status st = central_refuse(grid, what)) return st;
    if (!grid->tpl)
        return fail(LCF_ERR_STATE, std::string(what) + " takes an engine with a second component: call "
                                   "lcf_engine_set_template first (the bands of the model alone are lcf_predict_quantiles)");
    if (grid->dp.n_points < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine has no points");
    if (grid->dp.n_filters > kTqMaxFilters)
        return fail(LCF_ERR_UNSUPPORTED, std::string(what) + " takes a grid engine of at most 16 distinct filters, this "
                                         "one has " + std::to_string(grid->dp.n_filters) + ": split the filters over calls");
    if (n < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "need at least one sample");
    if (ld < grid->dp.n_par + grid->tpl_extra)
        return fail(LCF_ERR_INVALID_ARGUMENT, "ld is smaller than the model's parameter count with the template's columns");
    return LCF_OK;
}

// The engine's points as the dense filters x distinct-times grid, filter-major (color_run's requirement): time_orig[ep]
// is the caller's index of the engine's time ep (the engine's are ascending).
lcf_status template_grid(const lcf_engine* grid, std::vector<int32_t>* time_orig) {
    const DevProblem& dp = grid->dp;
    const int N = dp.n_points, NF = dp.n_filters, nt = dp.n_epochs;
    if ((long long)N != (long long)nt * NF)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine must hold every filter at every distinct time");
    std::vector<int> filt(N), orig(N), epoch(N);
    LCF_HIP(hipMemcpy(filt.data(), dp.pt_filt, N * sizeof(int), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(orig.data(), dp.pt_orig, N * sizeof(int), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(epoch.data(), dp.pt_epoch, N * sizeof(int), hipMemcpyDeviceToHost));
    time_orig->assign(nt, -1);
    std::vector<char> seen((size_t)nt * NF, 0);
    for (int i = 0; i < N; ++i) {
        if (epoch[i] < 0 || epoch[i] >= nt || filt[i] < 0 || filt[i] >= NF || orig[i] < 0 || orig[i] >= N)
            return fail(LCF_ERR_STATE, "the engine's point order is inconsistent");
        char& slot = seen[(size_t)epoch[i] * NF + filt[i]];
        int32_t& t_o = (*time_orig)[epoch[i]];
        if (slot) return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine holds a (time, filter) pair twice");
        slot = 1;
        if (orig[i] / nt != filt[i] || (t_o >= 0 && t_o != orig[i] % nt))
            return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine's points must be the dense grid, filter-major");
        t_o = orig[i] % nt;
    }
    return LCF_OK;
}

// The template form on the dense grid.  out[n_q][n_comp][n_filters][n_times], n_valid[n_comp][n_filters][n_times],
// n_dark[n_filters][n_times] (host); the components in the order total, base, template; times in the caller's order.
lcf_status template_run(lcf_engine* grid, const ChainView& in, int32_t mask, const double* q, int32_t n_q,
                        int64_t workspace_bytes, double* out, int64_t* n_valid, int64_t* n_dark) {
    const DevProblem& dp = grid->dp;
    const int N = dp.n_points, NF = dp.n_filters, nt = dp.n_epochs;
    std::vector<int32_t> time_orig;
    if (lcf_status st = template_grid(grid, &time_orig)) return st;
    TemplateForm form(grid, mask);
    const int nser = form.nf;
    if ((long long)N * form.tq.n_comp > INT32_MAX) return fail(LCF_ERR_INVALID_ARGUMENT, "too many (point, component) pairs");
    std::vector<int32_t> table((size_t)nt * nser);   // component x filter take the place of a time's filters
    for (int ep = 0; ep < nt; ++ep)
        for (int k = 0; k < nser; ++k) table[(size_t)ep * nser + k] = (k / NF) * N + (k % NF) * nt + time_orig[ep];
    DevBuf mem;
    if (lcf_status st = quantile_run(grid->device, form, nt, (long long)form.tq.n_comp * N, in, 0, 1, table.data(), 0, q,
                                     n_q, workspace_bytes, mem, out, n_valid))
        return st;
    std::vector<unsigned long long> cnt((size_t)nt * NF);
    LCF_HIP(hipMemcpy(cnt.data(), form.tq.n_dark, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int ep = 0; ep < nt; ++ep)
        for (int f = 0; f < NF; ++f) n_dark[(size_t)f * nt + time_orig[ep]] = (int64_t)cnt[(size_t)ep * NF + f];
    return LCF_OK;
}

// The features of every (sample, filter) on the dense grid, one launch.  values[3][n_filters][n] (NaN where the index is
// -1), indices[4][n_filters][n] in the caller's order of the times (host).
lcf_status features_run(lcf_engine* grid, const ChainView& in, double* values, int32_t* indices) {
    const DevProblem& dp = grid->dp;
    const int NF = dp.n_filters;
    std::vector<int32_t> time_orig;
    if (lcf_status st = template_grid(grid, &time_orig)) return st;
    const KeptSteps kept = kept_steps(in, 0, 1);
    const long long n = kept.samples;
    const size_t plane = (size_t)NF * n;
    DevBuf mem;
    double* d_coef;
    TqFeatures ft{};
    lcf_status st;
    if ((st = mem.alloc(&d_coef, (size_t)n * kNCoef)) || (st = mem.alloc(&ft.values, kTqValues * plane)) ||
        (st = mem.alloc(&ft.indices, kTqIndices * plane)))
        return st;
    PqArgs a{};
    a.base = kept.base;
    a.n = n;
    a.n_w = in.n_w;
    a.step_stride = kept.step_stride;
    a.ld = in.ld;
    a.coef = d_coef;
    TqArgs tq{};
    tq.tp = template_dev(grid);
    const size_t table = template_table_bytes(grid);
    tq.stage = table <= 60 * 1024;   // (beside the kernel's own exp table, within the 64 KiB every launch may ask for)
    const size_t lds = tq.stage ? table : 0;
    const unsigned blocks = (unsigned)((n + kTqFeatThreads - 1) / kTqFeatThreads);
    hipLaunchKernelGGL(k_pq_coef, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dp, a, d_coef);
    LCF_HIP(hipGetLastError());
    if (dp.model == kShockCooling)
        hipLaunchKernelGGL(k_tq_features<kShockCooling>, dim3(blocks), dim3(kTqFeatThreads), lds, 0, dp, a, tq, ft);
    else
        hipLaunchKernelGGL(k_tq_features<0>, dim3(blocks), dim3(kTqFeatThreads), lds, 0, dp, a, tq, ft);
    LCF_HIP(hipGetLastError());
    LCF_HIP(hipMemcpy(values, ft.values, kTqValues * plane * sizeof(double), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(indices, ft.indices, kTqIndices * plane * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int of_index[kTqValues] = {0, 1, 3};   // y_peak_base, y_peak_template, y_dip belong to i_peak_base, .., i_dip
    for (int v = 0; v < kTqValues; ++v)
        for (size_t k = 0; k < plane; ++k)
            if (indices[of_index[v] * plane + k] < 0) values[v * plane + k] = std::nan("");
    for (size_t k = 0; k < kTqIndices * plane; ++k)
        if (indices[k] >= 0) indices[k] = time_orig[indices[k]];
    return LCF_OK;
}

}  // namespace

extern "C" {

lcf_status lcf_predict_quantiles(lcf_engine* grid, const double* P, int64_t n, int32_t ld, int32_t component,
                                 const double* q, int32_t n_q, int64_t workspace_bytes, double* out, int64_t* n_valid) {
    if (lcf_status st = predict_check(grid, component, q, n_q, out, n_valid)) return st;
    DevBuf mem;
    ChainView in;
    if (lcf_status st = uploaded_samples(grid, P, n, ld, mem, &in)) return st;
    return predict_run(grid, in, 0, 1, component, q, n_q, workspace_bytes, out, n_valid);
}

lcf_status lcf_sampler_predict_quantiles(lcf_engine* grid, lcf_sampler* s, int64_t discard, int64_t thin,
                                         int32_t component, const double* q, int32_t n_q, int64_t workspace_bytes,
                                         double* out, int64_t* n_valid) {
    if (lcf_status st = predict_check(grid, component, q, n_q, out, n_valid)) return st;
    ChainView in;
    if (lcf_status st = stored_samples(grid, s, discard, thin, &in)) return st;
    return predict_run(grid, in, discard, thin, component, q, n_q, workspace_bytes, out, n_valid);
}

lcf_status lcf_predict_thermal(lcf_engine* grid, const double* P, int64_t n, int32_t ld, const double* q, int32_t n_q,
                               double T_floor, int64_t workspace_bytes, double* out, int64_t* n_valid, int64_t* n_cold,
                               int64_t* n_inside) {
    if (lcf_status st = thermal_check(grid, q, n_q, out, n_valid, n_cold, n_inside)) return st;
    DevBuf mem;
    ChainView in;
    if (lcf_status st = uploaded_samples(grid, P, n, ld, mem, &in)) return st;
    return thermal_run(grid, in, 0, 1, q, n_q, T_floor, workspace_bytes, out, n_valid, n_cold, n_inside);
}

lcf_status lcf_sampler_predict_thermal(lcf_engine* grid, lcf_sampler* s, int64_t discard, int64_t thin, const double* q,
                                       int32_t n_q, double T_floor, int64_t workspace_bytes, double* out,
                                       int64_t* n_valid, int64_t* n_cold, int64_t* n_inside) {
    if (lcf_status st = thermal_check(grid, q, n_q, out, n_valid, n_cold, n_inside)) return st;
    ChainView in;
    if (lcf_status st = stored_samples(grid, s, discard, thin, &in)) return st;
    return thermal_run(grid, in, discard, thin, q, n_q, T_floor, workspace_bytes, out, n_valid, n_cold, n_inside);
}

lcf_status lcf_predict_colors(lcf_engine* grid, const double* P, int64_t n, int32_t ld, int32_t n_c, const int32_t* pairs,
                              const double* dzp, const double* q, int32_t n_q, int64_t workspace_bytes, double* out,
                              int64_t* n_valid, double* y_peak, int32_t* peak_index) {
    if (lcf_status st = color_check(grid, n_c, pairs, dzp, q, n_q, out, n_valid, y_peak, peak_index)) return st;
    DevBuf mem;
    ChainView in;
    if (lcf_status st = uploaded_samples(grid, P, n, ld, mem, &in)) return st;
    return color_run(grid, in, 0, 1, n_c, pairs, dzp, q, n_q, workspace_bytes, out, n_valid, y_peak, peak_index);
}

lcf_status lcf_sampler_predict_colors(lcf_engine* grid, lcf_sampler* s, int64_t discard, int64_t thin, int32_t n_c,
                                      const int32_t* pairs, const double* dzp, const double* q, int32_t n_q,
                                      int64_t workspace_bytes, double* out, int64_t* n_valid, double* y_peak,
                                      int32_t* peak_index) {
    if (lcf_status st = color_check(grid, n_c, pairs, dzp, q, n_q, out, n_valid, y_peak, peak_index)) return st;
    ChainView in;
    if (lcf_status st = stored_samples(grid, s, discard, thin, &in)) return st;
    return color_run(grid, in, discard, thin, n_c, pairs, dzp, q, n_q, workspace_bytes, out, n_valid, y_peak, peak_index);
}

lcf_status lcf_predict_template(lcf_engine* grid, const double* P, int64_t n, int32_t ld, int32_t components,
                                const double* q, int32_t n_q, int64_t workspace_bytes, double* out, int64_t* n_valid,
                                int64_t* n_dark) {
    if (!q || !out || !n_valid || !n_dark) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = template_check(grid, P, n, ld, "a band of a template fit (lcf_predict_template)")) return st;
    const int32_t all = LCF_TEMPLATE_MASK_TOTAL | LCF_TEMPLATE_MASK_BASE | LCF_TEMPLATE_MASK_TEMPLATE;
    if (components < 1 || (components & ~all))
        return fail(LCF_ERR_INVALID_ARGUMENT, "components: a non-empty sum of LCF_TEMPLATE_MASK_TOTAL, _BASE and _TEMPLATE");
    if (lcf_status st = check_percentiles(q, n_q, kPqMaxSearch, "need between 1 and 512 percentiles")) return st;
    const long long searches = (long long)__builtin_popcount((unsigned)components) * grid->dp.n_filters * n_q;
    if (searches > kPqMaxSearch)
        return fail(LCF_ERR_UNSUPPORTED, "components x filters x percentiles of one call must not exceed 512, this call has " +
                                         std::to_string(searches) + ": split the percentiles over calls");
    DevBuf mem;
    ChainView in;
    if (lcf_status st = uploaded_samples(grid, P, n, ld, mem, &in)) return st;
    return template_run(grid, in, components, q, n_q, workspace_bytes, out, n_valid, n_dark);
}

lcf_status lcf_template_features(lcf_engine* grid, const double* P, int64_t n, int32_t ld, double* values,
                                 int32_t* indices) {
    if (!values || !indices) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = template_check(grid, P, n, ld, "the features of a template fit (lcf_template_features)")) return st;
    DevBuf mem;
    ChainView in;
    if (lcf_status st = uploaded_samples(grid, P, n, ld, mem, &in)) return st;
    return features_run(grid, in, values, indices);
}

lcf_status lcf_predict_luminosity(lcf_engine* grid, const double* P, int64_t n, int32_t ld, const double* q, int32_t n_q,
                                  int64_t workspace_bytes, double* out, int64_t* n_valid, int64_t* n_dark,
                                  double* L_peak, int32_t* i_peak) {
    if (!grid || !q || !out || !n_valid || !n_dark) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if ((L_peak == nullptr) != (i_peak == nullptr))
        return fail(LCF_ERR_INVALID_ARGUMENT, "L_peak and i_peak are given together or not at all");
    if (!is_central(grid->dp.model))
        return fail(LCF_ERR_UNSUPPORTED, "lcf_predict_luminosity takes a central-engine engine (LCF_MODEL_ARNETT, "
                                         "LCF_MODEL_MAGNETAR); the bands of a photometric model are lcf_predict_quantiles "
                                         "and lcf_predict_thermal");
    if (lcf_status st = check_percentiles(q, n_q, kPqMaxSearch, "need between 1 and 512 percentiles")) return st;
    if (grid->dp.n_points < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine has no epochs");
    DevBuf mem;
    ChainView in;
    if (lcf_status st = uploaded_samples(grid, P, n, ld, mem, &in)) return st;
    return luminosity_run(grid, in, 0, 1, q, n_q, workspace_bytes, out, n_valid, n_dark, L_peak, i_peak);
}

lcf_status lcf_predict_custom(lcf_engine* grid, const double* P, int64_t n, int32_t ld, const double* q, int32_t n_q,
                              double T_floor, int64_t workspace_bytes, double* out, int64_t* n_valid, int64_t* n_dark,
                              int64_t* n_cold) {
    if (!grid || !q || !out || !n_valid || !n_dark) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (grid->dp.model != LCF_MODEL_CUSTOM)
        return fail(LCF_ERR_UNSUPPORTED, "lcf_predict_custom takes an engine of LCF_MODEL_CUSTOM; the bands of a built-in "
                                         "photometric model are lcf_predict_quantiles and lcf_predict_thermal, those of a "
                                         "central-engine model lcf_predict_luminosity");
    if (lcf_status st = custom_ready(grid)) return st;
    if (lcf_status st = check_percentiles(q, n_q, kPqMaxSearch, "need between 1 and 512 percentiles")) return st;
    if (grid->dp.n_points < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "the grid engine has no points");
    DevBuf mem;
    ChainView in;
    if (lcf_status st = uploaded_samples(grid, P, n, ld, mem, &in)) return st;
    return custom_run(grid, in, 0, 1, q, n_q, T_floor, workspace_bytes, out, n_valid, n_dark, n_cold);
}

}  // extern "C"
