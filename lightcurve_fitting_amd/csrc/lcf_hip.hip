// MI355X (gfx950) batched light-curve log-likelihood engine: kernels + C ABI (include/lcf.h).
//
// Data layout in HBM (all float64 unless noted):
//   photometry  t[N], y[N], dy[N], 1/dy[N], int32 pt_filt[N], pt_orig[N], pt_epoch[N]; per filter a FiltDesc
//               -- points ordered by (part, filter), a part being a contiguous range of observation epochs;
//               distinct observation times epoch_t[n_epochs]
//   band tables tab[] = per filter [full | cool | hot] interleaved (a_k, W_k) pairs (the last two Gauss-compressed),
//               each padded to quads
//   walkers     P[n][n_dim] row-major; rows part[n][n_parts + 1] = partial chi^2 sums + log-prior; on the two-kernel
//               paths also derived coefficients coef[n][8] and thermal states therm[n][n_epochs] (1/T, R^2), which
//               the one-launch half-step (k_fused) keeps in LDS
// Work decomposition (k_points / k_fused): workgroup = (walker w, part j) walks the points of part j in chunks of
// 256; lane = one data point.  The exp table and all band tables are staged in LDS once per
// workgroup; lanes of a wave read the same LDS address (broadcast) because neighbouring points share a filter.
// Reductions are wave shuffles + a fixed-order LDS sum: no float atomics anywhere, results are bitwise reproducible
// run to run and independent of the GPU count.  The sampler's kernels (k_fused = a whole half-step in one launch; k_step,
// k_solo, k_solo_run) and what launches them, the multi-transient launches (k_*_multi, k_pop*) and the runs over several
// ranks live further down: this file holds everything that instantiates a kernel template.  The bookkeeping of runs
// (draw records, begin / snapshot / check, lcf_sampler_run) is in lcf_sampler.hip, which shares lcf_internal.h with
// this file; the SED engine is in lcf_sed.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "lcf.h"
#include "lcf_device.h"
#include "lcf_host.h"
#include "lcf_internal.h"
#include "lcf_keys.h"

// Tuning knobs of the likelihood loop (measured on the 1024-walker, 3000-point fit: 2-6 chunks of prefetch and 4-6
// waves per SIMD are within 1 % of each other; 8 waves per SIMD spill and lose 40 %).
#ifndef LCF_KPRE
#define LCF_KPRE 4   // chunks of points whose operands are fetched together
#endif
#ifndef LCF_KPRE_SOLO
#define LCF_KPRE_SOLO 2  // the same in the one-workgroup-per-proposal kernel (4: 3.73e7 walker-steps/s, 3: 3.74e7, 2: 3.78e7)
#endif
#ifndef LCF_WAVES
#define LCF_WAVES 4  // occupancy the register allocator is asked to keep (waves per SIMD)
#endif

using namespace lcf;

// =================================================================================================================
// kernels
// =================================================================================================================
namespace {

// The value lane `lane` (wave-uniform) holds, in every lane: two v_readlane instead of the LDS round trip of a shuffle
// (the serial heads wait for ~20 of them with nothing else to issue).  Used by the one-workgroup-per-proposal heads; in
// k_fused's step_serial the extra scalar registers tip two instantiations into scratch, so it keeps the shuffles.
__device__ __forceinline__ double lane_value(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned int)lo);
}

// v of the lane the DPP control names (a compile-time lane pattern inside a row of 16 lanes), two 32-bit moves
template <int CTRL>
__device__ __forceinline__ double dpp_value(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned int)lo);
}

// Sum over the 64 lanes of a wave, the same number in every lane, in a fixed order: inside quads (lane ^ 1, lane ^ 2), the
// two quads of a row half (mirror of 8), the two halves of a row (mirror of 16) -- data-parallel moves between vector
// registers, no LDS round trip as a shuffle is -- then the four rows (r0 + r1) + (r2 + r3) through scalar registers.
__device__ inline double wave_sum(double v) {
    v += dpp_value<0xB1>(v);    // quad_perm [1, 0, 3, 2]
    v += dpp_value<0x4E>(v);    // quad_perm [2, 3, 0, 1]
    v += dpp_value<0x141>(v);   // row_half_mirror
    v += dpp_value<0x140>(v);   // row_mirror
    return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}

// One thread per walker: derived coefficients, log-prior, skip flag.
__global__ void k_prepare(const DevProblem pb, int n, const double* __restrict__ P, double* __restrict__ coef,
                          double* __restrict__ lprior, int with_prior) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const double* p = P + (size_t)w * pb.n_dim;
    double c[kNCoef];
    walker_coefficients(pb, p, c);
    for (int i = 0; i < kNCoef; ++i) coef[(size_t)w * kNCoef + i] = c[i];
    lprior[w] = with_prior ? walker_log_prior(pb, p) : 0.;
}

// The tables of a point's filter (offsets relative to `base`): the full one and up to two Gauss-compressed
// companions -- the "cool" one valid for 1/T <= inv_tmin, and a shorter "hot" one valid for 1/T <= inv_tmin2
// (inv_tmin2 <= inv_tmin; 0 = none).  The shortest valid table is used.
template <class TabPtr>
struct TabSel {
    TabPtr base;                // LDS copy of the first n_lds samples of the table array (or the array itself)
    long long full, cool, hot;  // offset | count << 32 of each table (count 0: the level does not exist)
    double inv_tmin, inv_tmin2;
    const double2* gbase = nullptr;  // the whole array in global memory, when `base` holds only part of it
    int n_lds = 0x7fffffff;
};

__device__ __forceinline__ long long tab_slice(int off, int cnt) {
    return (long long)(unsigned int)off | ((long long)cnt << 32);
}

template <int VARIANT, class TabPtr>
__device__ __forceinline__ double band_sum_at(const TabSel<TabPtr>& ts, bool use_ctab, double invT, const ExpTab et) {
    long long sel = ts.full;
    sel = (use_ctab && invT <= ts.inv_tmin) ? ts.cool : sel;
    sel = (use_ctab && invT <= ts.inv_tmin2) ? ts.hot : sel;
    const int off = (int)sel, cnt = (int)(sel >> 32);
    // a wave with a point whose table is not staged (colder than every compressed level, long tables) reads global
    // memory for all its points: same values
    if (__builtin_amdgcn_ballot_w64(off >= ts.n_lds) != 0) {
        const double2* tab = ts.gbase + off;
        return VARIANT == 0 ? band_sum_ref(tab, cnt, invT) : band_sum_fast(tab, cnt, invT, et);
    }
    const TabPtr tab = ts.base + off;
    return VARIANT == 0 ? band_sum_ref(tab, cnt, invT) : band_sum_fast(tab, cnt, invT, et);
}

// (interp_log_band_sum, the interpolants' lookup, is in lcf_device.h: the run-time-compiled kernel of custom models takes it too)

// Everything one lane does for its data point after the thermal state (1/T, R_bb^2): band sum(s) -> template term.
// STAGED: the band tables (or their compressed levels) are in LDS; the on-the-fly reddening fall-back exists only in
// the unstaged instantiations, so that it costs the staged kernels no registers.
// ITAB: the instantiation may meet log-space states (engines with shared epochs only: with the thermal state inside the
// point loop the interpolated path's registers do not fit next to it).
// The factors a companion-shocking model applies per filter (models.py:909-917): shock factor x the filter's Kasen
// parameter, its SiFTO parameter, its time shift -- from the fourth entry of the filter's descriptor and the proposal.
__device__ __forceinline__ void companion_factors(const double2 fd3, const double* __restrict__ c, const double* __restrict__ p,
                                                  double& kfac, double& sfac, double& dt) {
    const long long ks = __double_as_longlong(fd3.x);   // {kpar, spar}, dtpar
    const int kp = (int)ks, sp = (int)(ks >> 32), dp = (int)__double_as_longlong(fd3.y);
    kfac = c[5] * (kp >= 0 ? p[kp] : 1.);
    sfac = sp >= 0 ? p[sp] : 1.;
    dt = dp >= 0 ? p[dp] : 0.;
}
// shock component x factor + template x factor: ONE expression, so that every path contracts it the same way
__device__ __forceinline__ double companion_combine(double shock, double kfac, double tmpl, double sfac) {
    return shock * kfac + tmpl * sfac;
}

// MODEL > 0: compile-time model of an engine whose interpolants are all proved from their first interval
// (DevProblem::itab_uniform) and which fits no sigma -- the kernels specialised for the benchmark shapes.
template <int VARIANT, bool STAGED, bool ITAB, int MODEL = 0>
__device__ __forceinline__ double point_model(const DevProblem& pb, const double* __restrict__ c,
                                     const double* __restrict__ p, double t_in, int filt, const double2* tbase,
                                     const FiltDesc* fdesc, const ExpTab et, double invT, double pref, int itab_at) {
    const int model = MODEL ? MODEL : pb.model;
    double S = 0., yfit;
    const double2* fd = reinterpret_cast<const double2*>(fdesc) + kFdD2 * filt;  // the filter's descriptor: 16-byte reads
    // Log-space state (x = ln T > 0, pref = ln R_bb^2; see thermal_state_log): the interpolant if every point of the
    // wave is inside its filter's proved range -- a per-wave choice, like the fast / safe band sums, so that a walker's
    // result never depends on how walkers are batched -- else the sample tables after one exponential each.
    bool by_table = false;
    if (ITAB && VARIANT != 0 && (MODEL || pb.use_itab)) {
        const bool log_form = __double2hiint(invT) >= 0;   // (-0.0 and -1/T have the sign bit set)
        bool inside = log_form;
        if ((!MODEL && !pb.itab_uniform) || model == kShockCooling4) {
            const long long fmeta = __double_as_longlong(fd[1].y);   // {float r_min, int ioff} of the filter's interpolant
            // (ShockCooling4 also needs the band sum at 0.74 T: ln 0.74 / h intervals lower)
            const double r_low = model == kShockCooling4 ? invT - 0.3011050927839216 * pb.itab_inv_h : invT;
            inside = log_form && r_low >= (double)__int_as_float((int)fmeta);
        }
        if (__builtin_amdgcn_ballot_w64(!inside) == 0) {
            by_table = true;
        } else if (log_form) {  // a mixed wave: back to linear space
            invT = exp(-fma(invT, 1. / pb.itab_inv_h, pb.itab_u0));
            pref = exp(pref);
        } else {
            invT = -invT;
        }
    }
    if (by_table) {
        double L = interp_log_band_sum(pb, itab_at, filt, invT);
        if (model == kShockCooling4)  // min(blackbody, suppressed blackbody at 0.74 T), models.py:629-631
            L = fmin(L, interp_log_band_sum(pb, itab_at, filt, invT - 0.3011050927839216 * pb.itab_inv_h) + 1.2044203711356864);
        // (|ln R_bb^2| <= 600 and |ln S| < 100: the exponent can be added as an integer)
        yfit = exp_scaled<false>(fma(L, kInvLn2N, pref * kInvLn2N), et);
    } else if (!STAGED && invT > 0. && pb.redden_slow) {
        // ShockCooling3 through tables too long for LDS: the walker's reddening is applied sample by sample to the
        // full table in global memory (libm; a fall-back, not a fast path)
        const long long full = __double_as_longlong(fd[0].x);
        const int off = (int)full, cnt = (int)(full >> 32);
        for (int k = 0; k < cnt; ++k) {
            const double2 aw = pb.tab[off + k];
            S += aw.y * exp2(-c[6] * pb.tab_ext[off + k]) / expm1(aw.x * invT);
        }
    } else if (invT > 0.) {
        const double2 d0 = fd[0], d1 = fd[1], d2 = fd[2];
        const TabSel<const double2*> ts{tbase, __double_as_longlong(d0.x), __double_as_longlong(d0.y),
                                        __double_as_longlong(d1.x), d2.x, d2.y, pb.tab,
                                        STAGED ? pb.n_lds_tab : 0x7fffffff};
        S = band_sum_at<VARIANT>(ts, pb.use_ctab != 0, invT, et);
        if (model == kShockCooling4) {  // models.py:629-631: min(blackbody, suppressed blackbody)
            const double S2 = band_sum_at<VARIANT>(ts, pb.use_ctab != 0, invT * (1. / 0.74), et);
            S = fmin(S, S2 * (1. / (0.74 * 0.74 * 0.74 * 0.74)));
        }
    }
    // pref may be NaN (propagates) or 0 with 1/T == 0.
    if (!by_table) yfit = (pref != pref) ? pref : pref * S;
    if (model == kShockCooling3) yfit *= c[5];  // models.py:495
    if (model >= kCompanion && model <= kCompanion3) {  // models.py:909-917, 977-980, 1040-1045
        double kfac, sfac, dt;
        companion_factors(fd[3], c, p, kfac, sfac, dt);
        // (the stretch as a reciprocal, taken once per column by the column paths: (t - t_peak - dt) / s within a rounding)
        const double x = (t_in - c[3] - dt) * (1. / c[4]);
        double tmpl;
        if (pb.knot_h > 0.) {   // integer-day knots: interval computed; coefficients from LDS where they are staged
            extern __shared__ __align__(16) unsigned char smem[];
            const int row0 = filt * (pb.n_knots - 1) * 2;   // double2 entries in front of the filter's
            if (STAGED && pb.n_spl_lds > 0) {
                const int spl_at = (int)(kLdsHead * sizeof(double) + (pb.n_lds_tab + kFdD2 * pb.n_filters) * sizeof(double2) +
                                         pb.n_itab_lds * sizeof(double));
                tmpl = spline_eval_uniform(pb, reinterpret_cast<const double2*>(smem + spl_at) + row0, x);
            } else {
                tmpl = spline_eval_uniform(pb, reinterpret_cast<const double2*>(pb.spl) + row0, x);
            }
        } else {
            tmpl = spline_eval(pb.knots, pb.n_knots, pb.spl + (size_t)filt * (pb.n_knots - 1) * 4, x, pb.knot_inv_h);
        }
        yfit = companion_combine(yfit, kfac, tmpl, sfac);
    }
    return yfit;
}

// Diagnostic build only (-DLCF_STAMPS, tools/debug/make_stamp_build.py; never shipped): s_memtime stamps of the first 64
// workgroups of k_solo, written by the first lane of wave `W` into a buffer nothing else reads.
#ifdef LCF_STAMPS
__device__ unsigned long long g_wall[2 * 1024 * 2];   // [launch parity][workgroup][entry, exit] of the 100 MHz wall clock
__device__ unsigned long long g_stamps[64 * 16];
// ... and, for wave 0, the ticks since its previous stamp summed over all half-steps of all launches (g_acc) with the
// number of times the stamp was passed (g_cnt): the mean life of a workgroup, phase by phase (resident launches: the
// last half-step alone says little -- it writes the state and the snapshot).
__device__ unsigned long long g_acc[64 * 16], g_cnt[64 * 16], g_last[64];
__shared__ unsigned long long s_stamp_last;   // (wave 0's previous stamp; garbage at kernel entry: implausible deltas are dropped)
#define LCF_STAMP(W, k)                                                                                        \
    do {                                                                                                       \
        unsigned long long t_;                                                                                 \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                             \
        if (blockIdx.x < 64 && threadIdx.x == 64 * (W)) {                                                      \
            g_stamps[blockIdx.x * 16 + (k)] = t_;                                                              \
            if ((W) == 0) {                                                                                    \
                const unsigned long long d_ = t_ - s_stamp_last;                                               \
                if (d_ < (1ull << 24)) {   /* (fire-and-forget adds: nothing here waits for memory) */         \
                    atomicAdd(&g_acc[blockIdx.x * 16 + (k)], d_);                                              \
                    atomicAdd(&g_cnt[blockIdx.x * 16 + (k)], 1ull);                                            \
                }                                                                                              \
                s_stamp_last = t_;                                                                             \
            }                                                                                                  \
        }                                                                                                      \
    } while (0)
#elif defined(LCF_PROGRESS)
// Diagnostic build (-DLCF_PROGRESS; never shipped): how often each workgroup has passed each stamp -- where the
// workgroups of a launch that cannot finish are.
__device__ unsigned int g_progress[64 * 16];
#define LCF_STAMP(W, k)                                                                                        \
    do {                                                                                                       \
        if (blockIdx.x < 64 && threadIdx.x == 64 * (W)) atomicAdd(&g_progress[blockIdx.x * 16 + (k)], 1u);    \
    } while (0)
#else
#define LCF_STAMP(W, k) do {} while (0)
#endif
// Diagnostic build (-DLCF_POLL_LOOKS; never shipped): how many looks the polls of the resident kernels' heads needed.
// A look is one pass of board_take_pair's loop on wave 0 -- one round trip to memory; a poll's number is that of its
// slowest lane.  Wave 0 counts in LDS (polls of 1, 2, 3 and more looks, and the looks in total) and adds the workgroup's
// counts to g_poll_looks when it leaves the launch (lcf_debug_read_poll_looks; tools/debug/poll_looks.py).
// The same four counts are also kept PER WORKGROUP AND LAUNCH, with the place the workgroup ran at: when it leaves, wave 0
// appends one record of kPollWgWords words to g_poll_wg -- the launch's first half-step (what tells launches apart),
// blockIdx.x, the hardware-id register of wave 0 as read at kernel entry (compute unit, shader array and shader engine in
// bits 8 .. 15), the XCC id, and the counts.  Two workgroups of one launch with the same place shared a compute unit for
// the whole launch (lcf_debug_read_poll_wg; tools/debug/poll_looks_by_cu.py).  Records beyond kPollWgMax are dropped;
// g_poll_wg_n counts them all.
#ifdef LCF_POLL_LOOKS
__device__ unsigned long long g_poll_looks[4];
__shared__ unsigned int s_poll_looks[4], s_poll_now;   // (s_poll_now: the looks of the poll under way, the maximum over its lanes)
constexpr int kPollWgWords = 8, kPollWgMax = 16384;
__device__ unsigned int g_poll_wg[kPollWgMax * kPollWgWords];
__device__ unsigned int g_poll_wg_n;
#endif

// ---- epoch-major likelihood: one lane per COLUMN (an observation time and its points, DevProblem::em_*) ----------------
// The lane computes the column's thermal state in registers and walks the column's points itself: no hand-off of the
// state through LDS, no barrier between states and points, one interval / position of the temperature for all filters
// of the epoch, and as many independent Horner chains per lane as the epoch has filters.
//
// M filters side by side for one column on the interpolated level: filters f0 .. f0 + M - 1 (wave-uniform: the column
// layout is dense), interval j and position s shared by all of them.  Returns y_fit per filter.  `row` = the lane's
// offset 8 j (doubles) inside a filter's interpolant; a filter's interpolant is 8 itab_m doubles long.
// IN_LDS: the interpolants are staged at byte `lds_at` of the dynamic LDS (the address is formed from the LDS symbol
// itself, so that the reads are ds_read_b128 with immediate offsets and not generic-pointer loads); else global memory.
// (A compile-time choice: with both in one function the two sets of loads share registers, and the LDS reads then wait
// for every outstanding global load -- the column's own photometry included.)
// `lnr2k` = ln R_bb^2 x 256 / ln 2: y_fit = 2^((ln S + ln R_bb^2) 256 / ln 2 / 256), the scaling folded into one FMA.
// (PB: DevProblem, or anything else with its `itab_m` and `itab`)
template <int M, bool IN_LDS, class PB>
__device__ __forceinline__ void interp_columns(const PB& pb, int lds_at, int f0, int row, double s, double lnr2k,
                                               const ExpTab et, double (&yfit)[M]) {
    extern __shared__ __align__(16) unsigned char smem[];
    double2 q[M][4];
    const int fstride = pb.itab_m * 8;
    if (IN_LDS) {
        const double2* base = reinterpret_cast<const double2*>(smem + lds_at) + row / 2;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double2* qa = base + ((f0 + m) * fstride) / 2;
            q[m][0] = qa[0], q[m][1] = qa[1], q[m][2] = qa[2], q[m][3] = qa[3];
        }
    } else {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double2* qa = reinterpret_cast<const double2*>(pb.itab + (size_t)(f0 + m) * fstride) + row / 2;
            q[m][0] = qa[0], q[m][1] = qa[1], q[m][2] = qa[2], q[m][3] = qa[3];
        }
    }
    double g[M];
#pragma unroll
    for (int m = 0; m < M; ++m) g[m] = fma(q[m][0].x, s, q[m][0].y);
#pragma unroll
    for (int m = 0; m < M; ++m) g[m] = fma(g[m], s, q[m][1].x);
#pragma unroll
    for (int m = 0; m < M; ++m) g[m] = fma(g[m], s, q[m][1].y);
#pragma unroll
    for (int m = 0; m < M; ++m) g[m] = fma(g[m], s, q[m][2].x);
#pragma unroll
    for (int m = 0; m < M; ++m) g[m] = fma(g[m], s, q[m][2].y);
#pragma unroll
    for (int m = 0; m < M; ++m) g[m] = fma(g[m], s, q[m][3].x);
#pragma unroll
    for (int m = 0; m < M; ++m) g[m] = fma(g[m], s, q[m][3].y);
    // (|ln R_bb^2| <= 600 and |ln S| < 100: the exponent can be added as an integer)
#pragma unroll
    for (int m = 0; m < M; ++m) yfit[m] = exp_scaled<false>(fma(g[m], kInvLn2N, lnr2k), et);
}

// M filters of one dense column of a COMPANION-SHOCKING model side by side: the Kasen blackbody through the interpolants
// (interp_columns) and the SiFTO template from the staged splines (integer-day knots), combined with the filters' factors;
// returns the M squared scaled residuals' sum.  The arithmetic is point_model's, operation for operation.
template <int M>
__device__ __forceinline__ double companion_columns(const DevProblem& pb, int itab_at, int spl_at, const double2* fd2,
                                                    const double* __restrict__ p, const double* __restrict__ c, int f0,
                                                    int row, double s, double lnr2k, double t_in, double inv_s,
                                                    const ExpTab et, const double2* __restrict__ yd, int nc) {
    extern __shared__ __align__(16) unsigned char smem[];
    double2 o[M];
#pragma unroll
    for (int m = 0; m < M; ++m) o[m] = yd[(size_t)(f0 + m) * nc];
    double shock[M];
    interp_columns<M, true>(pb, itab_at, f0, row, s, lnr2k, et, shock);
    double acc = 0.;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double kfac, sfac, dt;
        companion_factors(fd2[kFdD2 * (f0 + m) + 3], c, p, kfac, sfac, dt);
        const double x = (t_in - c[3] - dt) * inv_s;
        const double tmpl = spline_eval_uniform(pb, reinterpret_cast<const double2*>(smem + spl_at) + (f0 + m) * (pb.n_knots - 1) * 2, x);
        const double q = (o[m].x - companion_combine(shock[m], kfac, tmpl, sfac)) * o[m].y;
        acc = fma(q, q, acc);
    }
    return acc;
}

// What a lane needs of its FIRST column before any arithmetic: the observation time and (dense columns of up to kPreK
// filters) the photometry.  None of it depends on the proposal, so the one-launch half-step kernels fetch it ahead of
// the serial head: by the time the coefficients exist the loads have long landed.
constexpr int kPreK = 6;
struct ColumnOperands {
    double t;
    double2 o[kPreK];
    bool have_o;   // (wave-uniform)
};

template <int MODEL = 0>
__device__ __forceinline__ bool columns_fast_kind(const DevProblem& pb, bool by_itab) {
    if (MODEL) return true;   // (what a model-specialised kernel is launched for)
    // dense columns of a power-law model without a fitted sigma and with interpolants proved from their first interval:
    // every point of a wave whose states are all in log space goes through interp_columns
    return by_itab && pb.em_dense && pb.itab_uniform && !pb.use_sigma && (pb.model == kShockCooling || pb.model == kShockCooling2);
}

template <int VARIANT, int MODEL = 0>
__device__ __forceinline__ void fetch_column(const DevProblem& pb, int part, int vtid, ColumnOperands& co) {
    const int c0 = part_entry(pb.part_col0, part), c1 = part_entry(pb.part_col0, part + 1);
    const int cb = c0 + (vtid & ~63), lane = vtid & 63;
    co.have_o = false;
    co.t = 0.;
#pragma unroll
    for (int k = 0; k < kPreK; ++k) co.o[k] = make_double2(0., 0.);
    if (cb >= c1) return;
    const int col = min(cb + lane, c1 - 1);
    co.t = pb.em_t[col];
    if (columns_fast_kind<MODEL>(pb, VARIANT != 0 && pb.use_itab) && pb.em_k == kPreK) {
        co.have_o = true;
#pragma unroll
        for (int k = 0; k < kPreK; ++k) co.o[k] = pb.em_yd[(size_t)k * pb.em_cols + col];
    }
}

// The interpolated points of one dense column (the lane's): sum of squared scaled residuals.
// ... of kPreK filters whose photometry is in registers already (fetch_column): two groups of three, all operands at hand
template <bool IN_LDS, class PB>
__device__ __forceinline__ double fast_column_fetched(const PB& pb, int itab_at, int row, double s, double lnr2k,
                                                      const ExpTab et, const double2 (&o)[kPreK]) {
    static_assert(kPreK == 6, "two groups of three");
    double acc = 0.;
#pragma unroll
    for (int f = 0; f < kPreK; f += 3) {
        double yf[3];
        interp_columns<3, IN_LDS>(pb, itab_at, f, row, s, lnr2k, et, yf);
        const double q0 = (o[f].x - yf[0]) * o[f].y, q1 = (o[f + 1].x - yf[1]) * o[f + 1].y;
        const double q2 = (o[f + 2].x - yf[2]) * o[f + 2].y;
        acc = fma(q0, q0, acc);
        acc = fma(q1, q1, acc);
        acc = fma(q2, q2, acc);
        LCF_STAMP(0, 14 + (f > 0));
    }
    return acc;
}
// ... of any number of filters, photometry fetched group by group
template <bool IN_LDS>
__device__ __forceinline__ double fast_column(const DevProblem& pb, int itab_at, int col, int row, double s, double lnr2k,
                                              const ExpTab et) {
    const int nf = pb.em_k, nc = pb.em_cols;
    const double2* yd = pb.em_yd + col;
    double acc = 0.;
    int f = 0;
#pragma unroll 1
    for (; f + 3 <= nf; f += 3) {
        const double2 o0 = yd[(size_t)f * nc], o1 = yd[(size_t)(f + 1) * nc], o2 = yd[(size_t)(f + 2) * nc];
        double yf[3];
        interp_columns<3, IN_LDS>(pb, itab_at, f, row, s, lnr2k, et, yf);
        const double q0 = (o0.x - yf[0]) * o0.y, q1 = (o1.x - yf[1]) * o1.y, q2 = (o2.x - yf[2]) * o2.y;
        acc = fma(q0, q0, acc);
        acc = fma(q1, q1, acc);
        acc = fma(q2, q2, acc);
    }
    if (f + 2 <= nf) {
        const double2 o0 = yd[(size_t)f * nc], o1 = yd[(size_t)(f + 1) * nc];
        double yf[2];
        interp_columns<2, IN_LDS>(pb, itab_at, f, row, s, lnr2k, et, yf);
        const double q0 = (o0.x - yf[0]) * o0.y, q1 = (o1.x - yf[1]) * o1.y;
        acc = fma(q0, q0, acc);
        acc = fma(q1, q1, acc);
        f += 2;
    }
    if (f < nf) {
        const double2 o0 = yd[(size_t)f * nc];
        double yf[1];
        interp_columns<1, IN_LDS>(pb, itab_at, f, row, s, lnr2k, et, yf);
        const double q0 = (o0.x - yf[0]) * o0.y;
        acc = fma(q0, q0, acc);
    }
    return acc;
}

// One column point by point: any model, fitted sigma, states outside the interpolants, ragged columns.  `dense`: the
// filter index is the loop counter (wave-uniform, scalar table loads).  The ballots inside point_model see the lanes
// that have a point at this position of their column only.
template <int VARIANT, bool LDS_TAB, int MODEL>
__device__ __forceinline__ double general_column(const DevProblem& pb, const double* __restrict__ p,
                                                  const double* __restrict__ c, const double2* tbase, const FiltDesc* fdesc,
                                                  const ExpTab et, int itab_at, double t_in, int col, bool live, double x,
                                                  double pr) {
    const int nc = pb.em_cols;
    double acc = 0.;
    auto one_point = [&](int k, int filt) {
        const double2 o = pb.em_yd[(size_t)k * nc + col];
        const double yfit = point_model<VARIANT, LDS_TAB, true, MODEL>(pb, c, p, t_in, filt, tbase, fdesc, et, x, pr, itab_at);
        const double r = o.x - yfit;   // models.py:121-135
        if (!MODEL && pb.use_sigma) {
            const double dy = o.y;
            const double su = p[pb.n_dim - 1] * (pb.sigma_abs ? pb.sigma_unit_abs : dy);
            const double var = fma(dy, dy, su * su);
            acc += log(kTwoPi * var) + r * r / var;
        } else {
            const double q = r * o.y;
            acc = fma(q, q, acc);
        }
    };
    if (MODEL || pb.em_dense) {
#pragma unroll 1
        for (int k = 0; k < pb.em_k; ++k)
            if (live) one_point(k, k);
    } else {
#pragma unroll 1
        for (int k = 0; k < pb.em_k; ++k) {
            const int filt = pb.em_filt[(size_t)k * nc + col];
            if (live && filt >= 0) one_point(k, filt);
        }
    }
    return acc;
}

// The same for a MODEL-SPECIALISED kernel, out of line: a wave of such a kernel gets here when one of its states is
// outside the interpolants (a phase before the explosion, a temperature outside 2..256 kK) -- rare in a fit, and inlined the
// sample-table code would sit in the kernel's instruction stream and register budget.  Tables, descriptors and the exp
// table are read from global memory (the numbers their staged copies hold), the coefficients through a plain pointer:
// no LDS symbol in here.
template <int VARIANT, int MODEL>
__device__ __attribute__((noinline)) double cold_column(const DevProblem* pbp, const double* c_mem, const double* p, double t_in,
                                                        int col, bool live, double x, double pr) {
    const DevProblem& pb = *pbp;
    double c[kNCoef];
#pragma unroll
    for (int k = 0; k < kNCoef; ++k) c[k] = c_mem[k];
    return general_column<VARIANT, false, MODEL>(pb, p, c, pb.tab, pb.f_desc, ExpTab{pb.exp2tab}, -1, t_in, col, live, x, pr);
}

// ... computing the state of the column itself (for the caller that found the wave outside the fast path before it had one)
template <int VARIANT, int MODEL>
__device__ __attribute__((noinline)) double cold_column_with_state(const DevProblem* pbp, const double* c_mem, const double* p,
                                                                   double t_in, int col, bool live) {
    const DevProblem& pb = *pbp;
    double c[kNCoef], x, pr;
#pragma unroll
    for (int k = 0; k < kNCoef; ++k) c[k] = c_mem[k];
    const ExpTab et{pb.exp2tab};
    thermal_state_log<MODEL>(pb, c, t_in, x, pr, et);
    return general_column<VARIANT, false, MODEL>(pb, p, c, pb.tab, pb.f_desc, et, -1, t_in, col, live, x, pr);
}

// The whole column phase of a lane of a MODEL-specialised kernel in the shape the benchmarks have -- a power-law model,
// kPreK filters, the lane's one column already fetched (fetch_column), interpolants in LDS: straight-line code, the five
// coefficients the state needs as vector registers (no scalar copies, nothing hoisted).  The arithmetic is epochs_loop's
// fast branch, operation for operation.  Returns false (wave-uniform) where a state of the wave is outside the
// interpolants: the caller then takes the general path for the column.
// PB: DevProblem, or what a resident launch holds of it in LDS (ColumnView: consts, itab_u0, itab_inv_h, itab_m, itab).
// HAVE_LT: `lt` = tlog(first.t - sc[0]) was taken in front of the barrier the coefficients arrive behind (the resident
// half-step's early phase logarithm); the phase itself is still formed here, for the test of its sign alone.
template <int MODEL, bool HAVE_LT = false, class PB>
__device__ __forceinline__ bool lean_column(const PB& pb, const double* __restrict__ sc, const ColumnOperands& first,
                                            const ExpTab et, int itab_at, double& acc, double lt = 0.) {
    const double t = first.t - sc[0];
    double u, lp, lL;
    powerlaw_log_state<HAVE_LT>(pb, sc[3], sc[6], sc[7], HAVE_LT ? lt : t, et, u, lp, lL);
    const double r = (u - pb.itab_u0) * pb.itab_inv_h;
    // exactly where thermal_state_log leaves a log-space pair (lL NaN makes lp NaN: every comparison fails)
    const bool ok = t > 0. && r >= 0. && r < (double)pb.itab_m && lp >= -600. && lp <= 600.;
    if (__builtin_amdgcn_ballot_w64(!ok) != 0) return false;
    const int row = 8 * (int)r;
    const double s = fma(__builtin_amdgcn_fract(r), 2., -1.);
    acc = fast_column_fetched<true>(pb, itab_at, row, s, lp * kInvLn2N, et, first.o);
    return true;
}
// The fields lean_column and the head's coefficients read, as a resident launch holds them (copies out of RunUniforms).
struct ColumnView {
    const double* consts;
    double itab_u0, itab_inv_h;
    int itab_m;
    const double* itab;   // (the interpolants in memory: not read by the staged path)
};
struct ConstsView {
    const double* consts;
    int model;
};

// chi^2 share of virtual thread `vtid` (0 .. kBlock-1) of part `part` for one walker: parameters p, coefficients c.
// Virtual wave v = vtid / 64 owns the columns part_col0 + 64 v + lane + 256 m, m = 0, 1, ...: whichever kernel walks a
// part (k_points, k_fused, k_solo, k_pop) and whichever physical wave plays virtual wave v, the lane sums, the wave
// sums (xor butterfly) and the part's sum (w0 + w1) + (w2 + w3) are the same numbers -- chains do not depend on the kernel.
// The band-sum path (interpolant or sample tables; fast or safe exponentials) is chosen per wave, for the filter the wave
// is at: deterministic in the walker and the light curve alone.
// `first` (when FETCHED): the operands of the lane's first column, fetched by the caller (fetch_column, this part and vtid).
// COLD (model-specialised kernels that hold the problem in memory, `pb_mem`, and the coefficients at `c_mem`): the
// general path is the out-of-line cold_column.
template <int VARIANT, bool LDS_TAB, bool FETCHED = false, int MODEL = 0, bool COLD = false>
__device__ inline double epochs_loop(const DevProblem& pb, int part, const double* __restrict__ p,
                                     const double* __restrict__ c, const double2* tbase, const FiltDesc* fdesc,
                                     const ExpTab et, int vtid, int itab_at, const ColumnOperands& first = ColumnOperands{},
                                     bool use_first = true, const DevProblem* pb_mem = nullptr,
                                     const double* c_mem = nullptr) {
    // (`part` and the virtual wave are wave-uniform: scalar registers)
    part = __builtin_amdgcn_readfirstlane(part);
    const int c0 = part_entry(pb.part_col0, part), c1 = part_entry(pb.part_col0, part + 1);
    const int lane = vtid & 63, v64 = __builtin_amdgcn_readfirstlane(vtid & ~63);
    const bool by_itab = MODEL ? true : VARIANT != 0 && pb.use_itab;
    const bool fast_kind = columns_fast_kind<MODEL>(pb, by_itab);
    // companion-shocking models with dense columns, interpolants AND template splines staged (integer-day knots)
    const bool companion_fast = !MODEL && LDS_TAB && by_itab && pb.em_dense && pb.itab_uniform && !pb.use_sigma &&
                                pb.model >= kCompanion && pb.model <= kCompanion3 && itab_at >= 0 && pb.n_spl_lds > 0 &&
                                pb.knot_h > 0.;
    // (generic kernels only: compiled into the model-specialised ones as well it cost them their registers -- 2 to 34
    // spilled -- and photometry without shared epochs ran no faster there, 25.7 against 26.0 us)
    const bool ragged_fast = !MODEL && by_itab && !pb.em_dense && pb.itab_uniform && !pb.use_sigma &&
                             (pb.model == kShockCooling || pb.model == kShockCooling2);
    double term = 0.;
    // (a lane's columns are 256 apart: the time of the next one is requested while this one is computed -- in the generic
    // kernels; the model-specialised ones have no registers to spare for it)
    constexpr bool kAhead = MODEL == 0;
    double t_next = 0.;
    if (kAhead && c0 + v64 < c1 && !(FETCHED && use_first)) t_next = pb.em_t[min(c0 + v64 + lane, c1 - 1)];
#pragma unroll 1
    for (int cb = c0 + v64; cb < c1; cb += kBlock) {
        const bool live = cb + lane < c1;
        const int col = live ? cb + lane : c1 - 1;   // lanes beyond the part repeat its last column; their terms are dropped
        const bool fetched = FETCHED && use_first && cb < c0 + kBlock;
        const double t_in = fetched ? first.t : kAhead ? t_next : pb.em_t[col];
        if (kAhead && cb + kBlock < c1) t_next = pb.em_t[min(cb + kBlock + lane, c1 - 1)];
        // ragged columns: the first point's filter and photometry too, ahead of the state's arithmetic
        int filt0 = 0;
        double2 o0 = make_double2(0., 0.);
        if (ragged_fast) {
            filt0 = pb.em_filt[col];
            o0 = pb.em_yd[col];
        }
        double x, pr;   // the log-space pair of thermal_state_log, or (1/T, R_bb^2)
        if (by_itab) {
            thermal_state_log<MODEL>(pb, c, t_in, x, pr, et);
        } else {
            double T;
            thermal_state<MODEL>(pb, c, t_in, T, x, pr);
        }
        LCF_STAMP(0, 13);
        if (ragged_fast && __builtin_amdgcn_ballot_w64(__double2hiint(x) < 0) == 0) {
            // columns that are NOT one point of every filter (photometry whose observations have their own times: one
            // point per column): the same interpolated arithmetic with the filter read per lane
            const double lnr2k = pr * kInvLn2N;
            const int nc = pb.em_cols;
            double acc = 0.;
#pragma unroll 1
            for (int k = 0; k < pb.em_k; ++k) {
                int filt = filt0;
                double2 o = o0;
                if (k > 0) {   // (not a select between a register and a load: that puts the register in scratch memory)
                    filt = pb.em_filt[(size_t)k * nc + col];
                    o = pb.em_yd[(size_t)k * nc + col];
                }
                const double L = interp_log_band_sum(pb, itab_at, max(filt, 0), x);
                const double q = (o.x - exp_scaled<false>(fma(L, kInvLn2N, lnr2k), et)) * o.y;
                acc = filt >= 0 ? fma(q, q, acc) : acc;
            }
            term += live ? acc : 0.;
            continue;
        }
        if (companion_fast && __builtin_amdgcn_ballot_w64(__double2hiint(x) < 0) == 0) {
            // dense columns of a companion-shocking model, everything staged: groups of three filters side by side
            const int row = 8 * (int)x;
            const double s = fma(__builtin_amdgcn_fract(x), 2., -1.);
            const double lnr2k = pr * kInvLn2N, inv_s = 1. / c[4];
            const int spl_at = itab_at + pb.n_itab_lds * (int)sizeof(double), nf = pb.em_k, ncols = pb.em_cols;
            const double2* fd2 = reinterpret_cast<const double2*>(fdesc);
            const double2* yd = pb.em_yd + col;
            double acc = 0.;
            int f = 0;
#pragma unroll 1
            for (; f + 3 <= nf; f += 3)
                acc += companion_columns<3>(pb, itab_at, spl_at, fd2, p, c, f, row, s, lnr2k, t_in, inv_s, et, yd, ncols);
            if (f + 2 <= nf) {
                acc += companion_columns<2>(pb, itab_at, spl_at, fd2, p, c, f, row, s, lnr2k, t_in, inv_s, et, yd, ncols);
                f += 2;
            }
            if (f < nf) acc += companion_columns<1>(pb, itab_at, spl_at, fd2, p, c, f, row, s, lnr2k, t_in, inv_s, et, yd, ncols);
            term += live ? acc : 0.;
            continue;
        }
        if (fast_kind && __builtin_amdgcn_ballot_w64(__double2hiint(x) < 0) == 0) {
            const int row = 8 * (int)x;
            const double s = fma(__builtin_amdgcn_fract(x), 2., -1.);
            const double lnr2k = pr * kInvLn2N;
            double acc;
            if (fetched && first.have_o)
                acc = itab_at >= 0 ? fast_column_fetched<true>(pb, itab_at, row, s, lnr2k, et, first.o)
                                   : fast_column_fetched<false>(pb, itab_at, row, s, lnr2k, et, first.o);
            else
                acc = itab_at >= 0 ? fast_column<true>(pb, itab_at, col, row, s, lnr2k, et)
                                   : fast_column<false>(pb, itab_at, col, row, s, lnr2k, et);
            term += live ? acc : 0.;   // (a dead lane's sum is dropped as a whole)
            continue;
        }
        if constexpr (COLD && MODEL != 0)
            term += cold_column<VARIANT, MODEL>(pb_mem, c_mem, p, t_in, col, live, x, pr);
        else
            term += general_column<VARIANT, LDS_TAB, MODEL>(pb, p, c, tbase, fdesc, et, itab_at, t_in, col, live, x, pr);
    }
    return term;
}

// Thermal state (T, R_bb^2) of every (walker, distinct observation time): light curves observed in several filters at
// the same epochs share it, so the logarithm and exponentials of the model are paid once per epoch instead of once
// per point.  Used when the light curve has at least two points per distinct time on average.
__global__ __launch_bounds__(kBlock) void k_thermal(const DevProblem pb, int w_lo, int n_w,
                                                    const double* __restrict__ coef,
                                                    const double* __restrict__ lprior, int skip_excluded,
                                                    double2* __restrict__ therm, int log_state) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_w * pb.n_epochs) return;
    const int w = w_lo + idx / pb.n_epochs, ep = idx % pb.n_epochs;
    if (skip_excluded && lprior[w] == -INFINITY) return;
    double T, invT, pref;
    if (log_state)
        thermal_state_log(pb, coef + (size_t)w * kNCoef, pb.epoch_t[ep], invT, pref, ExpTab{pb.exp2tab});
    else
        thermal_state(pb, coef + (size_t)w * kNCoef, pb.epoch_t[ep], T, invT, pref);
    therm[(size_t)w * pb.n_epochs + ep] = make_double2(invT, pref);
}

// Stage the exp table and the staged region (band tables, descriptors, interpolants) in LDS; thread t of nt.  One flat
// copy of the engine's image of that layout, eight 16-byte loads per thread in flight before the first LDS store: a
// loop of load -> store pairs is one memory round trip per iteration, and six of them in a row made staging as long
// as the whole serial head (configs[1]: staged at 5.4 k cycles after kernel entry, now at 4.4 k; half-step 7.82 ->
// 7.51 us).  ShockCooling3: the walker's reddening goes into the staged weights (table by table).
template <int VARIANT, bool LDS_TAB>
__device__ inline void stage_tables(const DevProblem& pb, double* __restrict__ exptab, double2* __restrict__ ltab,
                                    double ebv, int t, int nt) {
    if (LDS_TAB && pb.model == kShockCooling3 && !pb.redden_slow) {
        for (int k = t; k < kExpTabSize; k += nt) exptab[k] = pb.exp2tab[k];
        double2* lfd = ltab + pb.n_lds_tab;   // filter descriptors (48 B = 3 double2 each) behind the tables
        const double2* gfd = reinterpret_cast<const double2*>(pb.f_desc);
        for (int k = t; k < kFdD2 * pb.n_filters; k += nt) lfd[k] = gfd[k];
        for (int k = t; k < pb.n_lds_tab; k += nt) {
            double2 aw = pb.tab[k];
            aw.y *= exp2(-ebv * pb.tab_ext[k]);
            ltab[k] = aw;
        }
        return;
    }
    const int n16 = LDS_TAB ? pb.stage_n16 : kLdsHead / 2;
    const double2* __restrict__ g = pb.stage_image;
    double2* __restrict__ l = reinterpret_cast<double2*>(exptab);
    const int last = n16 - 1;
#pragma unroll 1
    for (int k0 = t; k0 < n16; k0 += 8 * nt) {   // (named values, not an array: that the compiler kept in scratch memory)
        const int k1 = k0 + nt, k2 = k1 + nt, k3 = k2 + nt, k4 = k3 + nt, k5 = k4 + nt, k6 = k5 + nt, k7 = k6 + nt;
        const double2 v0 = g[min(k0, last)], v1 = g[min(k1, last)], v2 = g[min(k2, last)], v3 = g[min(k3, last)];
        const double2 v4 = g[min(k4, last)], v5 = g[min(k5, last)], v6 = g[min(k6, last)], v7 = g[min(k7, last)];
        l[k0] = v0;
        if (k1 < n16) l[k1] = v1;
        if (k2 < n16) l[k2] = v2;
        if (k3 < n16) l[k3] = v3;
        if (k4 < n16) l[k4] = v4;
        if (k5 < n16) l[k5] = v5;
        if (k6 < n16) l[k6] = v6;
        if (k7 < n16) l[k7] = v7;
    }
}

// The points of part `part` for one walker in the filter-sorted order: parameters p, coefficients c (global or LDS),
// thermal states th[pt_epoch - e_off] when THERM.  MODE 0: returns this thread's share of chi^2 (engines without
// thermal states ahead of the points only: with them the likelihood walks the epoch-major copy, epochs_loop);
// MODE 1: y_fit -> out0[row][orig];  MODE 2: T, R_bb -> out0, out1.
template <int VARIANT, int MODE, bool LDS_TAB, bool THERM, int KPRE_POINTWISE = 0>
__device__ inline double points_loop(const DevProblem& pb, int part, size_t row, const double* __restrict__ p,
                                     const double* __restrict__ c, const double2* __restrict__ th_base, int e_off,
                                     const double2* tbase, const FiltDesc* fdesc, const ExpTab et,
                                     double* __restrict__ out0, double* __restrict__ out1, int tid = threadIdx.x,
                                     int itab_at = -1) {
    static_assert(!(THERM && MODE == 0), "the likelihood of an engine with thermal states is epochs_loop's");
    double term = 0.;  // `tid`: this thread's index among the kBlock threads that walk the part
    const int p0 = part_entry(pb.part_start, part), p1 = part_entry(pb.part_start, part + 1);  // this part's points
    // chunks whose operands are fetched together, before any band sum starts (fewer when the thermal state is computed
    // per point: that code needs the registers)
    constexpr int kPre = THERM ? (KPRE_POINTWISE == 1 ? LCF_KPRE_SOLO : LCF_KPRE) : 1;
    for (int k0 = 0; k0 * kBlock < p1 - p0; k0 += kPre) {
        int idx[kPre], filt[kPre];
        double tin[kPre], yv[kPre], idy[kPre];
        double2 th[kPre];
#pragma unroll
        for (int u = 0; u < kPre; ++u) {
            const int i = p0 + (k0 + u) * kBlock + tid;
            idx[u] = i < p1 ? i : -1;
            if (idx[u] < 0) continue;
            // (filter and epoch share a word, and the time is fetched only by who uses it -- per-point thermal states,
            // the SN Ia template, the (T, R) output: 20 instead of 32 bytes per point from L2)
            if (THERM && MODE != 2) {
                int ep;
                if (pb.pt_fe) {
                    const unsigned int fe = (unsigned int)pb.pt_fe[i];
                    filt[u] = (int)(fe & 63u);
                    ep = (int)(fe >> 6);
                } else {
                    filt[u] = pb.pt_filt[i];
                    ep = pb.pt_epoch[i];
                }
                th[u] = th_base[ep - e_off];
                tin[u] = pb.model >= kCompanion && pb.model <= kCompanion3 ? pb.t[i] : 0.;
            } else {
                filt[u] = pb.pt_filt[i];
                tin[u] = pb.t[i];
            }
            if (MODE == 0) {
                const double2 yd = pb.pt_yd[i];   // (y, 1/dy), or (y, dy) when sigma is fitted
                yv[u] = yd.x;
                idy[u] = yd.y;
            }
        }
#pragma unroll
        for (int u = 0; u < kPre; ++u) {
            const int i = idx[u];
            if (i < 0) continue;
            double invT, pref, Tk = 0.;
            if (THERM && MODE != 2) {
                invT = th[u].x;   // (the log-space pair of thermal_state_log when the engine interpolates)
                pref = th[u].y;
            } else {
                thermal_state(pb, c, tin[u], Tk, invT, pref);
            }
            if (MODE == 2) {
                // R_bb = sqrt(pref) keeps the reference's NaN/0 pattern (pref = R_bb^2)
                const size_t j = row * pb.n_points + pb.pt_orig[i];
                out0[j] = Tk;
                out1[j] = sqrt(pref);
                continue;
            }
            const double yfit = point_model<VARIANT, LDS_TAB, THERM>(pb, c, p, tin[u], filt[u], tbase, fdesc, et, invT, pref,
                                                                     itab_at);
            if (MODE == 0) {  // models.py:121-135
                const double r = yv[u] - yfit;
                if (pb.use_sigma) {
                    const double dy = idy[u];
                    const double su = p[pb.n_dim - 1] * (pb.sigma_abs ? pb.sigma_unit_abs : dy);
                    const double var = fma(dy, dy, su * su);
                    term += log(kTwoPi * var) + r * r / var;
                } else {
                    const double q = r * idy[u];
                    term = fma(q, q, term);
                }
            } else {
                out0[row * pb.n_points + pb.pt_orig[i]] = yfit;
            }
        }
    }
    return term;
}

// Workgroup reduction of the chi^2 shares in a fixed order; thread 0 stores the part's partial sum.
__device__ inline double store_part_sum(double term, double* __restrict__ red, double* __restrict__ dst) {
    const int tid = threadIdx.x;
    const double ws = wave_sum(term);
    if ((tid & 63) == 0) red[tid >> 6] = ws;
    __syncthreads();
    if (tid != 0) return 0.;
    const double sum = (red[0] + red[1]) + (red[2] + red[3]);
    *dst = sum;
    return sum;  // (thread 0)
}

// MODE 0: chi^2 partial sums -> part[w][n_parts];  MODE 1: y_fit -> out0[w][orig];  MODE 2: T, R_bb -> out0, out1
// Workgroup = (walker w, part j): it walks the points of part j (a range of epochs, sorted by filter) in chunks of
// 256 with the exp table and ALL band tables staged in LDS once, and reduces once at the end.
template <int VARIANT, int MODE, bool LDS_TAB, bool THERM>
__device__ inline void points_body(const DevProblem& pb, int bid, int w_lo, int n_w, const double* __restrict__ P,
                                   const double* __restrict__ coef, const double* __restrict__ lprior,
                                   const double2* __restrict__ therm, double* __restrict__ out0,
                                   double* __restrict__ out1) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* exptab = reinterpret_cast<double*>(smem);                     // kExpTabSize doubles
    double* red = exptab + kExpTabSize;                                   // 4 doubles
    double2* ltab = reinterpret_cast<double2*>(smem + kLdsHead * sizeof(double));

    const int part = bid / n_w;
    const int w = w_lo + bid % n_w;

    if (MODE == 0 && lprior[w] == -INFINITY) return;  // prior excludes the walker: likelihood skipped (fitting.py:125)

    const double* c = coef + (size_t)w * kNCoef;   // wave-uniform -> scalar loads
    stage_tables<VARIANT, LDS_TAB>(pb, exptab, ltab, pb.model == kShockCooling3 ? c[6] : 0., threadIdx.x, kBlock);
    __syncthreads();

    const double2* tbase = LDS_TAB ? (const double2*)ltab : pb.tab;
    const FiltDesc* fdesc = LDS_TAB ? reinterpret_cast<const FiltDesc*>(ltab + pb.n_lds_tab) : pb.f_desc;
    // byte offset of the staged interpolants in the dynamic LDS (behind the tables and descriptors), or -1
    const int itab_at = (LDS_TAB && pb.n_itab_lds > 0)
                            ? (int)(kLdsHead * sizeof(double) + (pb.n_lds_tab + kFdD2 * pb.n_filters) * sizeof(double2)) : -1;
    if constexpr (MODE == 0 && THERM) {
        // (the thermal states are the lanes' own: k_thermal is not launched for the likelihood)
        const double term = epochs_loop<VARIANT, LDS_TAB>(pb, part, P + (size_t)w * pb.n_dim, c, tbase, fdesc, ExpTab{exptab},
                                                          threadIdx.x, itab_at);
        store_part_sum(term, red, out0 + (size_t)w * part_stride(pb) + part);
    } else {
        const double term = points_loop<VARIANT, MODE, LDS_TAB, THERM>(
            pb, part, (size_t)(w - w_lo), P + (size_t)w * pb.n_dim, c, THERM ? therm + (size_t)w * pb.n_epochs : nullptr, 0,
            tbase, fdesc, ExpTab{exptab}, out0, out1, threadIdx.x, itab_at);
        if (MODE == 0) store_part_sum(term, red, out0 + (size_t)w * part_stride(pb) + part);
    }
}

template <int VARIANT, int MODE, bool LDS_TAB, bool THERM>
__global__ __launch_bounds__(kBlock, LCF_WAVES) void k_points(const DevProblem pb, int w_lo, int n_w, const double* __restrict__ P,
                                                   const double* __restrict__ coef,
                                                   const double* __restrict__ lprior,
                                                   const double2* __restrict__ therm, double* __restrict__ out0,
                                                   double* __restrict__ out1) {
    points_body<VARIANT, MODE, LDS_TAB, THERM>(pb, blockIdx.x, w_lo, n_w, P, coef, lprior, therm, out0, out1);
}

// lnL (and log-posterior) per walker from the partial sums, fixed summation order.  (A separate launch on purpose:
// letting the last workgroup of a walker do this inside k_points needs an agent-scope fence per workgroup, which on
// this part writes back and invalidates the XCD's L2 -- measured 3x slower k_points.)
__global__ void k_finalize(const DevProblem pb, int n, const double* __restrict__ part,
                           const double* __restrict__ lprior, double* __restrict__ out) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const double lp = lprior[w];
    if (lp == -INFINITY) {
        out[w] = -INFINITY;
        return;
    }
    double s = pb.use_sigma ? 0. : pb.log_norm_const;
    for (int k = 0; k < pb.n_parts; ++k) s += part[(size_t)w * part_stride(pb) + k];
    out[w] = lp - 0.5 * s;
}

// blackbody_to_filters, pointwise (models.py:1161-1162): arbitrary (filter, T, R) triples.
template <int VARIANT>
__global__ __launch_bounds__(kBlock) void k_bb_pointwise(const DevProblem pb, int m, const int* __restrict__ filt,
                                                         const int* __restrict__ tab_off,
                                                         const int* __restrict__ ctab_off,
                                                         const double* __restrict__ ctmin,
                                                         const double* __restrict__ T, const double* __restrict__ R,
                                                         double* __restrict__ out) {
    __shared__ double exptab[kExpTabSize];
    if (threadIdx.x < kExpTabSize) exptab[threadIdx.x] = pb.exp2tab[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int f = filt[i];
    const double Tk = T[i], r = R[i];
    double S = 0.;
    if (Tk > 0. && Tk < kTmax) {
        const ExpTab et{exptab};
        // the interpolated level (the engine's default where it has the interpolants): ln S_f(ln T) inside the range the
        // filter's interpolant is proved for -- a per-triple choice, a triple's result depends on nothing else
        bool done = false;
        if (VARIANT != 0 && pb.use_itab) {
            const double x = (log(Tk) - pb.itab_u0) * pb.itab_inv_h;
            if (x >= (double)pb.f_desc[f].r_min && x < (double)pb.itab_m) {
                S = exp_scaled<false>(interp_log_band_sum(pb, -1, f, x) * kInvLn2N, et);
                done = true;
            }
        }
        if (!done) {
            const TabSel<const double2*> ts{pb.tab, tab_slice(tab_off[2 * f], tab_off[2 * f + 1]),
                                            tab_slice(ctab_off[2 * f], ctab_off[2 * f + 1]), 0, 1. / ctmin[f], 0.};
            S = band_sum_at<VARIANT>(ts, pb.use_ctab != 0, 1. / Tk, et);
        }
    }
    out[i] = r * r * S;
}

// One float64 as two 8-byte granules {32 data bits, 32-bit generation tag}: an 8-byte store is the largest that
// arrives whole, so a reader that sees the tag of the generation it waits for in both granules has the value -- no
// flag, no fence, no ordering between stores needed (the "LL" protocol of the collective libraries).  Mailbox
// memory is uncached (fine-grained); stores and polls are system-scope so that they bypass the XCD's L2.
__device__ inline void mbox_post(const DevSampler& sm, long long g, int slot, int col, int stride, double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v), tag = (unsigned long long)(uint32_t)g << 32;
    const size_t at = 2 * ((((size_t)(g & 3) * sm.n_half) + slot) * stride + col);
#pragma unroll
    for (int r = 0; r < kMaxPeers; ++r)
        if (r < sm.n_peers) {
            unsigned long long* p = sm.peer_mbox[r] + at;
            __hip_atomic_store(p, (b & 0xffffffffull) | tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(p + 1, (b >> 32) | tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
}

// The value of generation g, once it has arrived; every lane's wait is bounded (DevSampler::wait_ticks of the 100 MHz wall clock): a
// peer that never delivers ends the run with an error instead of hanging the device.
__device__ inline double mbox_take(const DevSampler& sm, long long g, int slot, int col, int stride) {
    const unsigned long long tag = (unsigned long long)(uint32_t)g;
    const unsigned long long* p = sm.mbox + 2 * ((((size_t)(g & 3) * sm.n_half) + slot) * stride + col);
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        const unsigned long long a = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned long long b = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((a >> 32) == tag && (b >> 32) == tag)
            return __longlong_as_double((long long)((a & 0xffffffffull) | (b << 32)));
        if (wall_clock64() - t0 > sm.wait_ticks) {
            atomicOr(sm.err, 2);
            return qnan();
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// The serial part of a half-step for slot i, executed by ONE wave (lane = 0..63): accept tests of the previous
// half-step (recomputed from the per-slot records, no hand-off between workgroups), the new proposal, and -- for a
// slot this rank evaluates (`mine`) -- its coefficients and log-prior, left in sc[0..kNCoef] (LDS, lane 0 writes).
// `primary`: this wave is the one that commits slot i of the previous half-step and publishes the proposal record
// (exactly one wave per slot and launch is primary; the others only need the proposal for themselves).
template <int ND>
__device__ inline void step_serial(const DevProblem& pb, const DevSampler& sm, int i, bool primary, int lane,
                                   int have_prev, long long prev_row, int have_next,
                                   const DrawRec* __restrict__ draws, const DrawRec* __restrict__ prev_draws,
                                   long long g, bool mine, double* __restrict__ sc, double* __restrict__ sq,
                                   double* __restrict__ coef, double* __restrict__ lprior) {
    const int prev_wid = (have_prev && primary) ? prev_draws[i].wid : 0;
    PriorDev my_prior{0, 0, 0., 0., 0., 1.};
    if (lane < pb.n_dim && pb.has_priors && have_next) my_prior = pb.priors[lane];
    const int pp = (int)((g - 1) & 1), cp = (int)(g & 1);
    constexpr int kD = ND > 0 ? ND : kMaxDim;     // array extent
    const int nd = ND > 0 ? ND : sm.n_dim;         // trip count (constant when ND > 0)
    DrawRec dr{0, 0, -1, -1, 1., 0., 0., 0, 0};
    if (have_next) dr = draws[i];
    const bool active = have_next && dr.wid >= 0;  // (an odd ensemble leaves the last slot of its second half-step empty)
    // --- roles: which accept test (if any) this lane evaluates ---
    int rw = -1, rslot = -1;
    if (lane == 0 && have_prev && primary && prev_wid >= 0) {
        rslot = i;
        rw = prev_wid;  // walker of slot i in the previous half-step (from its draw record)
    } else if ((lane == 1 || lane == 2) && active) {
        rw = lane == 1 ? dr.wid : dr.pid;
        rslot = have_prev ? (lane == 1 ? dr.wprev : dr.pprev) : -1;
    }
    double row[kD], qrow[kD], lp_cur = 0., nlp = 0.;
    bool ok = false;
#pragma unroll
    for (int d = 0; d < kD; ++d) row[d] = qrow[d] = 0.;
    if (rw >= 0) {
        // everything the accept test and both outcomes need, in one wave of loads
        const double* xs = sm.X + (size_t)rw * nd;
#pragma unroll
        for (int d = 0; d < kD; ++d)
            if (d < nd) row[d] = xs[d];
        lp_cur = sm.LP[rw];
        if (rslot >= 0) {
            const SlotRec rc = sm.rec[pp][rslot];
            const double* qs = sm.Q[pp] + (size_t)rslot * nd;
#pragma unroll
            for (int d = 0; d < kD; ++d)
                if (d < nd) qrow[d] = qs[d];
            if (sm.n_peers > 0) {
                // the slot's row from this rank's mailbox, as its owner posted it: the log-prior first (always posted;
                // the partial sums only where the prior allows the proposal)
                const int stride = part_stride(pb);
                const double lpri = mbox_take(sm, g - 1, rslot, pb.n_parts, stride);
                double sum = pb.use_sigma ? 0. : pb.log_norm_const;
                if (lpri != -INFINITY)
                    for (int k = 0; k < pb.n_parts; ++k) sum += mbox_take(sm, g - 1, rslot, k, stride);
                nlp = lpri == -INFINITY ? -INFINITY : lpri - 0.5 * sum;
            } else if (sm.inline_finalize) {
                // the slot's row: partial chi^2 sums, then the log-prior (of this rank's evaluation, or gathered)
                const double* prow = sm.part2[pp] + (size_t)rslot * part_stride(pb);
                double sum = pb.use_sigma ? 0. : pb.log_norm_const;
                for (int k = 0; k < pb.n_parts; ++k) sum += prow[k];
                const double lpri = prow[pb.n_parts];
                nlp = lpri == -INFINITY ? -INFINITY : lpri - 0.5 * sum;
            } else {
                nlp = sm.newlp[pp][rslot];
            }
            ok = (rc.zl + nlp - rc.lp_old) > rc.lnu;  // emcee: (ndim-1) ln z + lp_new - lp_old > ln u
            lp_cur = ok ? nlp : rc.lp_old;
            if (ok) {
#pragma unroll
                for (int d = 0; d < kD; ++d) row[d] = qrow[d];
            }
        }
    }
    if (lane == 0 && rslot >= 0) {  // commit of the previous half-step's slot i
        if (nlp != nlp) atomicOr(sm.err, 1);
        if (ok) {
#pragma unroll
            for (int d = 0; d < kD; ++d)
                if (d < nd) sm.X[(size_t)rw * nd + d] = row[d];
            sm.LP[rw] = nlp;
            atomicAdd((unsigned long long*)&sm.nacc[rw], 1ull);
        }
        if (sm.store_chain) {
            double* crow = sm.chain + ((size_t)prev_row * sm.n_walkers + rw) * nd;
#pragma unroll
            for (int d = 0; d < kD; ++d)
                if (d < nd) crow[d] = row[d];
            sm.chain_lp[(size_t)prev_row * sm.n_walkers + rw] = lp_cur;
        }
    }
    if (have_next && !active) {  // empty slot: nothing to propose; its workgroups skip the likelihood
        if (lane == 0) {
            if (sc) sc[kNCoef] = -INFINITY;
            if (primary && lprior) lprior[i] = -INFINITY;
        }
        return;
    }
    if (active) {
        double q[kMaxDim], lq[kMaxDim];
        double arg = 1.;
#pragma unroll
        for (int d = 0; d < kMaxDim; ++d) q[d] = lq[d] = 0.;
#pragma unroll
        for (int d = 0; d < kD; ++d) {
            const double xi = __shfl(row[d], 1, 64), cj = __shfl(row[d], 2, 64);
            q[d] = d < nd ? cj - (cj - xi) * dr.z : 0.;
            if (lane == d && d < pb.n_par) arg = q[d];
        }
        const double lp_i = __shfl(lp_cur, 1, 64);
        if (!mine) {
            // another rank evaluates this proposal: only what later accept tests need is published here
            // (its log-prior reaches this rank inside the gathered log-posterior)
            if (lane == 0 && primary) {
#pragma unroll
                for (int d = 0; d < kD; ++d)
                    if (d < nd) sm.Q[cp][(size_t)i * nd + d] = q[d];
                sm.rec[cp][i] = SlotRec{dr.zl, dr.lnu, lp_i, 0.};
            }
            return;
        }
        const double lg = flog(arg);  // one logarithm per lane, all at once
#pragma unroll
        for (int d = 0; d < kD; ++d) lq[d] = __shfl(lg, d, 64);
        double c[kNCoef];
        walker_coefficients(pb, q, lq, c, pb.use_itab != 0 && pb.variant != 0);
        // log-prior: lane d evaluates parameter d with its descriptor fetched at kernel entry, then an ordered sum
        double lpr = 0.;
        if (pb.has_priors) {
            double qv = 0.;
#pragma unroll
            for (int d = 0; d < kD; ++d)
                if (lane == d) qv = q[d];
            const double mine = lane < pb.n_dim ? prior_term(my_prior, qv) : 0.;  // one evaluation per lane
#pragma unroll
            for (int d = 0; d < kD; ++d)
                if (d < nd) lpr += __shfl(mine, d, 64);
        }
        if (lane == 0) {
            for (int k = 0; k < kNCoef; ++k) sc[k] = c[k];
            sc[kNCoef] = lpr;
            if (sq) {  // the proposal itself, for a workgroup that goes on to evaluate it
#pragma unroll
                for (int d = 0; d < kD; ++d)
                    if (d < nd) sq[d] = q[d];
            }
            if (primary) {  // publish the per-slot records
#pragma unroll
                for (int d = 0; d < kD; ++d)
                    if (d < nd) sm.Q[cp][(size_t)i * nd + d] = q[d];
                sm.rec[cp][i] = SlotRec{dr.zl, dr.lnu, lp_i, lpr};
                sm.part2[cp][(size_t)i * part_stride(pb) + pb.n_parts] = lpr;  // last column of the slot's row
                if (sm.n_peers > 0) mbox_post(sm, g, i, pb.n_parts, part_stride(pb), lpr);
                if (coef)
                    for (int k = 0; k < kNCoef; ++k) coef[(size_t)i * kNCoef + k] = c[k];
                if (lprior) lprior[i] = lpr;
            }
        }
    }
}

// One 64-thread workgroup per proposal slot i: it commits half-step g - 1 for slot i and draws slot i of half-step g
// COOPERATIVELY -- the latency chain of a single thread (three accept tests with dependent loads, then the logarithms of
// the proposal) is spread over lanes that run the same code on different data:
//   lanes 0..2: accept test of {previous slot i, own walker, partner walker}, with every load that does not depend
//   on the outcome issued up front (both candidate rows included);  lanes 0..n_par-1: ln of the proposal's parameters.
// Every lane ends with the same proposal (bitwise); lane 0 publishes it, with the coefficients and the log-prior of the
// slots in [lo, hi) (this rank's shard) for the likelihood launch behind it (k_points: thermal states are its own).
// ND > 0: the walker dimension is a compile-time constant (loops over parameters unroll with exact trip counts and
// the per-parameter arrays live in registers); ND == 0: any dimension up to kMaxDim.
template <int ND>
__device__ inline void step_body(const DevProblem& pb, const DevSampler& sm, int i, int have_prev, long long prev_row,
                                 int have_next, const DrawRec* __restrict__ draws, const DrawRec* __restrict__ prev_draws,
                                 long long g, int lo, int hi, double* __restrict__ coef, double* __restrict__ lprior) {
    __shared__ double sc[kNCoef + 1];
    const bool mine = i >= lo && i < hi;       // this rank evaluates the likelihood of slot i
    if (threadIdx.x < 64)
        step_serial<ND>(pb, sm, i, true, threadIdx.x, have_prev, prev_row, have_next, draws, prev_draws, g, mine, sc, nullptr,
                        coef, lprior);
}

template <int ND>
__global__ __launch_bounds__(64) void k_step(const DevProblem pb, const DevSampler sm, int have_prev, long long prev_row,
                                             int have_next, const DrawRec* __restrict__ draws,
                                             const DrawRec* __restrict__ prev_draws, long long g, int lo, int hi,
                                             double* __restrict__ coef, double* __restrict__ lprior) {
    step_body<ND>(pb, sm, blockIdx.x, have_prev, prev_row, have_next, draws, prev_draws, g, lo, hi, coef, lprior);
}

// ---- single-GPU fit: the whole half-step in ONE launch ---------------------------------------------------------------
// Workgroup = (proposal slot i, part j).  Wave 0 runs the serial part (every part's workgroup redundantly: a few
// hundred cycles, and no workgroup then waits for another; part 0 is the one that commits and publishes) while waves
// 1-3 stage the tables; then all threads compute the thermal states of the part's own epochs straight into LDS and walk
// the part's points.  Against k_step + k_points this saves a launch, the round trip of the thermal states and the
// coefficients through memory, and the second staging.  The partial sums are double-buffered by half-step parity: this
// launch reads the previous half-step's for its accept tests and writes its own.  Same arithmetic in the same order
// as the two-kernel path: chains are bitwise identical.
constexpr int kFusedScratch = kNCoef + 2 + kMaxDim + (kMaxDim & 1);  // doubles: coefficients + log-prior, proposal

// A value every lane holds identically (read from LDS), moved to scalar registers: the per-walker coefficients are
// used by every band sum, and as vector registers they would cost the kernel its occupancy.
__device__ inline double uniform_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffLL));
    const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

template <int ND, int VARIANT, bool THERM>
__global__ __launch_bounds__(kBlock, LCF_WAVES) void k_fused(const DevProblem pb, const DevSampler sm, int have_prev,
                                                  long long prev_row, const DrawRec* __restrict__ draws,
                                                  const DrawRec* __restrict__ prev_draws, long long g, int lo, int hi,
                                                  double* __restrict__ lprior) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* exptab = reinterpret_cast<double*>(smem);
    double* red = exptab + kExpTabSize;
    double2* ltab = reinterpret_cast<double2*>(smem + kLdsHead * sizeof(double));
    const FiltDesc* fdesc = reinterpret_cast<const FiltDesc*>(ltab + pb.n_lds_tab);
    const int itab_at = pb.n_itab_lds > 0
                            ? (int)(kLdsHead * sizeof(double) + (pb.n_lds_tab + kFdD2 * pb.n_filters) * sizeof(double2)) : -1;
    double* sc = reinterpret_cast<double*>(ltab + pb.stage_d2);
    double* sq = sc + kNCoef + 2;
    const int tid = threadIdx.x;
    // Multi-GPU: this rank evaluates the slots [lo, hi) only.  Every other slot (commit + light proposal, no
    // likelihood) takes one WAVE of the workgroups launched behind the shard's own.
    const int n_own = hi - lo;
    if ((int)blockIdx.x >= n_own * pb.n_parts) {
        const int k = ((int)blockIdx.x - n_own * pb.n_parts) * (kBlock / 64) + (tid >> 6);
        const int slot = k < lo ? k : k + n_own;
        if (slot < sm.n_half)
            step_serial<ND>(pb, sm, slot, true, tid & 63, have_prev, prev_row, 1, draws, prev_draws, g, false, nullptr,
                            nullptr, nullptr, nullptr);
        return;
    }
    const int part = blockIdx.x / n_own, i = lo + blockIdx.x % n_own;
    const bool reddened = pb.model == kShockCooling3;
    if (tid < 64)
        step_serial<ND>(pb, sm, i, part == 0, tid, have_prev, prev_row, 1, draws, prev_draws, g, true, sc, sq, nullptr,
                        lprior);
    else if (!reddened)
        stage_tables<VARIANT, true>(pb, exptab, ltab, 0., tid - 64, kBlock - 64);
    __syncthreads();
    if (sc[kNCoef] == -INFINITY) return;  // prior excludes the proposal: likelihood skipped (fitting.py:125)
    double cs[kNCoef];
#pragma unroll
    for (int k = 0; k < kNCoef; ++k) cs[k] = uniform_f64(sc[k]);
    if (reddened) stage_tables<VARIANT, true>(pb, exptab, ltab, cs[6], tid, kBlock);
    if (reddened) __syncthreads();
    double term;
    if constexpr (THERM)
        term = epochs_loop<VARIANT, true>(pb, part, sq, cs, ltab, fdesc, ExpTab{exptab}, tid, itab_at);
    else
        term = points_loop<VARIANT, 0, true, false>(pb, part, 0, sq, cs, nullptr, 0, ltab, fdesc, ExpTab{exptab}, nullptr,
                                                    nullptr, tid, itab_at);
    const double psum = store_part_sum(term, red, sm.part2[g & 1] + (size_t)i * part_stride(pb) + part);
    if (sm.n_peers > 0 && tid == 0) mbox_post(sm, g, i, part, part_stride(pb), psum);  // straight into every rank's mailbox
}

__device__ inline unsigned long long* board_entry(unsigned long long* board, const DevSampler& sm, unsigned int tag, int wid,
                                                  int col) {
    return board + 2 * ((((size_t)(tag & (unsigned int)(sm.ring - 1)) * sm.n_walkers) + wid) * board_row_entries(sm.n_dim) + col);
}
// A value the loop optimiser must not compute ahead of the loop over the half-steps: what it hoists there lives across
// the whole launch and comes back from scratch memory on the path every other workgroup waits for.
__device__ __forceinline__ int not_hoisted(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
// ---- the resident half-step's record and LDS batches (k_solo_run) -----------------------------------------------------
// The draw records are read through a constant-address-space pointer -- scalar loads, served from the scalar cache that
// the hint of the previous half-step has filled -- and the accept test reloads what it needs of the record behind
// barrier 2 instead of carrying it across the columns.
// The LDS operands of the head and of the commit are requested by ONE statement per phase and waited for once.
// Written as instructions because the compiler orders plain LDS reads by their first use and sinks them below
// branches: the source's "one batch" became two to four dependent round trips on the wave everybody waits for.
// (Measured and dropped: the same for the column entry behind barrier 1 -- nine reads, one wait, then the branch on the
// abort word: 0.01 us per half-step SLOWER in every alternation, DESIGN section 5.  All eight waves pass there at once,
// and each then waits for operands it would otherwise have had in its own time.)
// kCommitWave: the wave that runs what stands behind barrier 2 -- accept test, post, state, snapshot, chain.  Wave 0
// leaves at barrier 2 for the loop top and the poll of the workgroup's next item, whose rows come from the board and
// never from this workgroup's registers or LDS; the commit reloads every operand anyway.
// kShadowWave: the wave that loads the abort word and hints the next draw record in the head's shadow (not the
// committing wave: it would then reach barrier 0 a round trip behind its commit).
constexpr int kCommitWave = 1;
constexpr int kShadowWave = 2;
typedef unsigned int lcf_u32x4 __attribute__((ext_vector_type(4)));
typedef int lcf_i32x4 __attribute__((ext_vector_type(4)));
// A draw record of the resident kernels: every field through a constant-address-space pointer -- scalar loads of
// the 48 bytes, out of the scalar cache where the hint of the previous half-step has put them -- because through the
// ordinary pointer the compiler must assume that the half-step's own stores and statements change the record, and reads
// it with vector loads, field by field where it is used.  What makes the constant view sound: the records of a launch are
// written by k_draws in EARLIER kernels of the same stream and by nothing while the launch runs (the generation of the
// next block goes behind the launch in the stream), and a kernel starts with the scalar cache invalidated.
__device__ __forceinline__ DrawRec draw_record(const DrawRec* p) {
    typedef const DrawRec __attribute__((address_space(4)))* DrawPtr;
    const DrawPtr c = (DrawPtr)p;
    DrawRec r;
    r.wid = c->wid, r.pid = c->pid, r.wprev = c->wprev, r.pprev = c->pprev;
    r.z = c->z, r.zl = c->zl, r.lnu = c->lnu;
    r.wage = c->wage, r.page = c->page;
    // What the head reads is requested HERE, together, and held in scalar registers: left to itself the compiler sinks
    // every one of these loads to its use -- the partner's age into the head, z behind the poll, each a round trip
    // of its own on the path everybody waits for.  ((n_dim - 1) ln z and ln u are not held: the commit reloads them.)
    int z_lo = __double2loint(r.z), z_hi = __double2hiint(r.z);
    asm volatile("" : "+s"(r.wid), "+s"(r.pid), "+s"(z_lo), "+s"(z_hi), "+s"(r.wage), "+s"(r.page));
    r.z = __hiloint2double(z_hi, z_lo);
    return r;
}
// Byte offset of an object of the workgroup's LDS, as the address operand of an LDS instruction.
__device__ __forceinline__ unsigned int lds_offset(const void* p) {
    typedef const __attribute__((address_space(3))) unsigned char* LdsBytes;
    return (unsigned int)(__SIZE_TYPE__)(LdsBytes)p;
}
__device__ __forceinline__ double f64_of(unsigned int lo, unsigned int hi) { return __hiloint2double((int)hi, (int)lo); }
// The half-step's scratch words (sc: coefficients, log-prior | abort word; sq; sx; solo_half_step's layout), in bytes
// from `sc`.  The resident kernels keep TWO copies of them (kScBlock bytes each) in front of the launch's block: wave 1
// commits item n out of one copy while wave 0 writes the head of item n + 1 into the other (solo_half_step, `copy`).
constexpr int kScProposal = (kNCoef + 2) * 8;
constexpr int kScPosition = kScProposal + (kMaxDim + (kMaxDim & 1)) * 8;
constexpr int kScLogPost = kScPosition + kMaxDim * 8;                  // log-posterior | acceptance count
constexpr int kScBlock = (kNCoef + 2 + 2 * (kMaxDim + (kMaxDim & 1)) + 4) * 8;
static_assert(kScLogPost % 16 == 0 && kScBlock % 16 == 0, "16-byte reads");
static_assert(offsetof(RunUniforms, ring_mask) == 8 && offsetof(RunUniforms, row_bytes) == 12 && offsetof(RunUniforms, ver_bytes) == 16 &&
              offsetof(RunUniforms, sum0) == 32 && offsetof(RunUniforms, n_parts) == 40,
              "the groups the batch below reads with one instruction each");
// The commit, behind barrier 2: the eight wave sums (`red_at`), log-posterior | count, this lane's number of the proposal
// and of the position (`mine_at`: sc + 8 mine), the launch block's words (`ru_at`) for the sum and for the row's address --
// and, in the same wait, (n_dim - 1) ln z | ln u and the walker of the draw record `rec`, by scalar loads (they stand
// behind the LDS reads: the record's address may be fresh from a vector instruction).
struct CommitOperands {
    lcf_u32x4 a0, a1, b0, b1, lc, sums, geo;   // sums: sum0 | n_parts, n_walkers; geo: board | ring_mask, row_bytes
    double ver_bytes, q_mine, x_mine;          // (ver_bytes: its bits)
    lcf_u32x4 zl_lnu;
    int wid;
};
__device__ __forceinline__ void commit_batch(unsigned int red_at, unsigned int sc_at, unsigned int mine_at, unsigned int ru_at,
                                             const void* rec, CommitOperands& c) {
    asm volatile("ds_read_b128 %0, %12\n\t"
                 "ds_read_b128 %1, %12 offset:16\n\t"
                 "ds_read_b128 %2, %12 offset:32\n\t"
                 "ds_read_b128 %3, %12 offset:48\n\t"
                 "ds_read_b128 %4, %13 offset:%17\n\t"
                 "ds_read_b128 %5, %15 offset:32\n\t"
                 "ds_read_b128 %6, %15\n\t"
                 "ds_read_b64 %7, %15 offset:16\n\t"
                 "ds_read_b64 %8, %14 offset:%18\n\t"
                 "ds_read_b64 %9, %14 offset:%19\n\t"
                 "s_load_dwordx4 %10, %16, 0x18\n\t"
                 "s_load_dword %11, %16, 0x0\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(c.a0), "=&v"(c.a1), "=&v"(c.b0), "=&v"(c.b1), "=&v"(c.lc), "=&v"(c.sums), "=&v"(c.geo), "=&v"(c.ver_bytes),
                   "=&v"(c.q_mine), "=&v"(c.x_mine), "=&s"(c.zl_lnu), "=&s"(c.wid)
                 : "v"(red_at), "v"(sc_at), "v"(mine_at), "v"(ru_at), "s"(rec), "n"(kScLogPost), "n"(kScProposal), "n"(kScPosition)
                 : "memory");
}
// (n_dim - 1) ln z | ln u and the walker of the record alone (the four-group kernels' commit, which has no batch)
__device__ __forceinline__ void record_reload(const void* rec, lcf_u32x4& zl_lnu, int& wid) {
    asm volatile("s_nop 4\n\ts_load_dwordx4 %0, %2, 0x18\n\ts_load_dword %1, %2, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(zl_lnu), "=&s"(wid) : "s"(rec) : "memory");
}
// ... from a resident launch's block of invariants (RunUniforms): the same address, multiplied out once per launch
__device__ __forceinline__ size_t board_entry_bytes(unsigned int ring_mask, unsigned long long ver_bytes, unsigned int row_bytes,
                                                    unsigned int tag, int wid, int col) {
    return (tag & ring_mask) * ver_bytes + ((size_t)(unsigned int)wid * row_bytes + 16u * (unsigned int)col);
}
__device__ __forceinline__ size_t board_entry_bytes(const RunUniforms& u, unsigned int tag, int wid, int col) {
    return board_entry_bytes(u.ring_mask, u.ver_bytes, u.row_bytes, tag, wid, col);
}
__device__ __forceinline__ unsigned long long* board_entry(unsigned long long* board, const RunUniforms& u, unsigned int tag,
                                                           int wid, int col) {
    return reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(board) + board_entry_bytes(u, tag, wid, col));
}
__device__ inline unsigned int* board_progress(unsigned long long* board, const DevSampler& sm) {
    return reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(board) +
                                           board_rows_bytes(sm.ring, sm.n_walkers, sm.n_dim));
}
// 16-byte accesses past every cache (sc0 sc1 = system scope: they meet in memory, whichever XCD or GPU the other side
// is on).  The store is not waited for; the load is (a poll has nothing else to do).  Written as instructions because
// the language has no 16-byte atomic: the hardware moves an aligned 16-byte lane access as one piece, and the tags make
// even 8-byte pieces safe.
// AGENT: the board of a one-launch run lives in this GPU's ordinary memory and is shared by its own workgroups only.
// Its 16-byte accesses are nevertheless issued at system scope (sc0 sc1), like those of the inter-rank boards: with sc1
// alone (device scope) the same run takes TWICE as long (0.70 against 0.37 ms per launch of 64 half-steps at configs[1]
// -- polls served from a cache for a while before they see memory); only the 4-byte words of the tail keep the scope.
template <bool AGENT>
__device__ __forceinline__ void store16_past_caches(unsigned long long* p, unsigned long long lo, unsigned long long hi) {
    const lcf_u32x4 v = {(unsigned int)lo, (unsigned int)(lo >> 32), (unsigned int)hi, (unsigned int)(hi >> 32)};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}
template <bool AGENT>
__device__ __forceinline__ void load16_past_caches(const unsigned long long* p, unsigned long long& lo, unsigned long long& hi) {
    lcf_u32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
    hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
}
template <bool AGENT = false>
__device__ inline void board_post_at(unsigned long long* entry, unsigned int tag, double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v), t = (unsigned long long)tag << 32;
    store16_past_caches<AGENT>(entry, (b & 0xffffffffull) | t, (b >> 32) | t);
}
template <bool AGENT = false>
__device__ inline void board_post(unsigned long long* board, const DevSampler& sm, unsigned int tag, int wid, int col, double v) {
    board_post_at<AGENT>(board_entry(board, sm, tag, wid, col), tag, v);
}
template <bool AGENT = false>
__device__ inline bool board_aborted_at(const unsigned int* flag) {
    return (AGENT ? __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) != 0u;
}
template <bool AGENT = false>
__device__ inline bool board_aborted(const DevSampler& sm) {
    return board_aborted_at<AGENT>(board_progress(sm.board, sm) + kMaxPeers);
}
__device__ inline unsigned int* board_arrivals(const DevSampler& sm) { return board_progress(sm.board, sm) + kMaxPeers + 5; }
// (what: 1 = a row, a = tag, b = walker, c = column; 2 = the progress words, a = half-step, b = rank that is behind;
// 3 = a row again, but the launch's workgroups were not all resident after DevSampler::resident_ticks: c = how many were)
__device__ inline void board_abort(const DevSampler& sm, unsigned int what, unsigned int a, unsigned int b, unsigned int c) {
    unsigned int* flag = board_progress(sm.board, sm) + kMaxPeers;
    if (atomicCAS_system(flag, 0u, 1u) == 0u) {   // the first one to give up says what it was waiting for
        __hip_atomic_store(flag + 1, what, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(flag + 2, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(flag + 3, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(flag + 4, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    atomicOr(sm.err, 2);
    if (sm.snap_flags) sm.snap_flags[kSnapFlags + (blockIdx.x & (kSnapFlags - 1))] = 2u;
}
// The number with tag `tag` from this rank's board, once it is there (bounded wait: DevSampler::wait_ticks, then the launch is aborted
// and the run ends with an error; NaN after an abort).
// `arrive_goal` != 0 (resident launches): the value of the arrivals word from which all workgroups of this launch have
// started.  Rows of a launch whose workgroups are all resident arrive within microseconds; a wait that has lasted
// DevSampler::resident_ticks (50 ms) looks at the word ONCE: all there -> keep waiting (a stalled peer rank, a busy
// device); not all there -> the launch cannot make progress (another resident kernel holds the CUs): give up now.
// (Measured and dropped, round 4: FOUR loads of the entry kept in flight a quarter of a round trip apart, each looked at
// when it returns -- finer sampling than one look per round trip, but whoever finds its row must still wait for the other
// three loads before their registers may be used again: 5.71 against 5.31 us per half-step at configs[1].  And the upper
// bound of a head computed AHEAD of the partner's commit -- a second wave computes it from stale rows while the first one
// polls, wrong chain, timing only: 5.13 against 5.31 us; with the two candidate heads, the second post and the second
// poll a real version needs, nothing would be left of the 0.19.)
// `p`: the entry (board_entry of this rank's board).
template <bool AGENT = false>
__device__ inline double board_take_at(const DevSampler& sm, const unsigned long long* p, unsigned int tag, int wid, int col,
                                       unsigned int arrive_goal = 0u) {
    const unsigned long long t0 = wall_clock64();
    bool resident = arrive_goal == 0u;
    for (int spin = 0;; ++spin) {
        unsigned long long a, b;
        load16_past_caches<AGENT>(p, a, b);
        if ((unsigned int)(a >> 32) == tag && (unsigned int)(b >> 32) == tag)
            return __longlong_as_double((long long)((a & 0xffffffffull) | (b << 32)));
        if ((spin & 15) == 15) {
            if (board_aborted<AGENT>(sm)) return qnan();
            if (!resident && wall_clock64() - t0 > sm.resident_ticks) {
                const unsigned int there = __hip_atomic_load(board_arrivals(sm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((int)(there - arrive_goal) < 0) {
                    board_abort(sm, 3u, tag, (unsigned int)wid, there);
                    return qnan();
                }
                resident = true;
            }
            if (wall_clock64() - t0 > sm.wait_ticks) {
                const bool was_first = !board_aborted<AGENT>(sm);
                board_abort(sm, 1u, tag, (unsigned int)wid, (unsigned int)col);
                if (was_first) {   // (what the entry holds instead: an older tag = never posted)
                    unsigned int* seen = board_arrivals(sm) + 1;
                    seen[0] = (unsigned int)a;
                    seen[1] = (unsigned int)(a >> 32);
                    seen[2] = (unsigned int)b;
                    seen[3] = (unsigned int)(b >> 32);
                }
                return qnan();
            }
        }
        __builtin_amdgcn_s_sleep(1);
    }
}
template <bool AGENT = false>
__device__ inline double board_take(const DevSampler& sm, unsigned int tag, int wid, int col, unsigned int arrive_goal = 0u) {
    return board_take_at<AGENT>(sm, board_entry(sm.board, sm, tag, wid, col), tag, wid, col, arrive_goal);
}
// ---- the poll of the resident kernels' head (k_solo_run): TWO entries per lane -------------------------------------
// What board_take_at looks at on every 16th look, out of line: the poll loop of the one wave everybody waits for is then
// a load pair, the tag tests and a sleep.  Same order, bounds and error words as board_take_at.
// Returns 0: keep waiting; 2: keep waiting, and every workgroup of the launch is known to have started; 1: the launch
// is aborted.  `seen`: the entry as last loaded (what an abort leaves for diagnosis).
template <bool AGENT>
__device__ __attribute__((noinline)) int board_wait_check(const DevSampler* smp, unsigned long long t0, bool resident,
                                                          unsigned int arrive_goal, unsigned int tag, int wid, int col,
                                                          lcf_u32x4 seen) {
    const DevSampler& sm = *smp;
    if (board_aborted<AGENT>(sm)) return 1;
    int state = 0;
    if (!resident && wall_clock64() - t0 > sm.resident_ticks) {
        const unsigned int there = __hip_atomic_load(board_arrivals(sm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int)(there - arrive_goal) < 0) {
            board_abort(sm, 3u, tag, (unsigned int)wid, there);
            return 1;
        }
        state = 2;
    }
    if (wall_clock64() - t0 > sm.wait_ticks) {
        const bool was_first = !board_aborted<AGENT>(sm);
        board_abort(sm, 1u, tag, (unsigned int)wid, (unsigned int)col);
        if (was_first) {   // (what the entry holds instead: an older tag = never posted)
            unsigned int* out = board_arrivals(sm) + 1;
            out[0] = seen.x;
            out[1] = seen.y;
            out[2] = seen.z;
            out[3] = seen.w;
        }
        return 1;
    }
    return state;
}
// The numbers of the entries `pa` (tag `tag_a`, walker `wid_a`) and `pb_` (`tag_b`, `wid_b`), both column `col`, once BOTH
// are there: each look requests the two 16-byte entries back to back and waits once, so every entry is still sampled
// once per look, on the lane that uses it.  (A lane with one entry to wait for passes it twice.)  NaN after an abort.
// `waited`: this lane needed more than one look (or the launch is aborted).
template <bool AGENT>
__device__ __forceinline__ void board_take_pair(const DevSampler& sm, const unsigned long long* pa, const unsigned long long* pb_,
                                                unsigned int tag_a, unsigned int tag_b, int wid_a, int wid_b, int col,
                                                unsigned int arrive_goal, double& va, double& vb, bool& waited) {
    const unsigned long long t0 = wall_clock64();
    bool resident = arrive_goal == 0u;
    for (int spin = 0;; ++spin) {
        lcf_u32x4 a, b;
        asm volatile("global_load_dwordx4 %0, %2, off sc0 sc1\n\tglobal_load_dwordx4 %1, %3, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(a), "=&v"(b) : "v"(pa), "v"(pb_) : "memory");
        const bool a_ok = a.y == tag_a && a.w == tag_a, b_ok = b.y == tag_b && b.w == tag_b;
        if (a_ok && b_ok) {
            va = __hiloint2double((int)a.z, (int)a.x);
            vb = __hiloint2double((int)b.z, (int)b.x);
            waited = spin != 0;
#ifdef LCF_POLL_LOOKS
            atomicMax(&s_poll_now, (unsigned int)spin + 1u);
#endif
            return;
        }
        if ((spin & 15) == 15) {
            // (the entry this lane still waits for)
            const int state = board_wait_check<AGENT>(&sm, t0, resident, arrive_goal, a_ok ? tag_b : tag_a, a_ok ? wid_b : wid_a,
                                                      col, a_ok ? b : a);
            if (state == 1) {
                va = vb = qnan();
                waited = true;
                return;
            }
            resident = resident || state == 2;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Version of a row a half-step G asks for: the walker's last move was `age` half-steps ago; rows nobody has moved in
// this run carry the run's start tag.
__device__ inline unsigned int board_tag(long long G, int age, long long g_run0) {
    const long long t = G - age + 1;
    return (unsigned int)(t < g_run0 ? g_run0 : t);
}

// Start of a run: this rank's complete state as version `tag` (= the run's first half-step: "the state in front of it")
// on its OWN board; the abort word is cleared.  (Progress words are absolute half-step numbers and are never reset: a
// faster rank may already have posted into this board.)
__global__ void k_board_init(const DevSampler sm, unsigned int tag) {
    const int cols = sm.n_dim + 2;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < kBoardClear) __hip_atomic_store(board_progress(sm.board, sm) + kMaxPeers + idx, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (idx >= (long long)sm.n_walkers * cols) return;
    const int wid = (int)(idx / cols), col = (int)(idx % cols);
    const double v = col < sm.n_dim ? sm.X[(size_t)wid * sm.n_dim + col] : col == sm.n_dim ? sm.LP[wid] : (double)sm.nacc[wid];
    board_post(sm.board, sm, tag, wid, col, v);
}

// The rows of half-step G, as every rank posted them, into this rank's state (end of a run: `n_hs` = 2, the last step)
// and / or into the chain (`to_chain`, every half-step of a run that stores it).  A wave takes as many slots as whole rows
// fit its 64 lanes (8 rows of 8 entries for up to six parameters), lane = (row, column): behind a resident launch of an
// 8-GPU run there are 64 x 4096 rows to collect, and a wave per row left 57 of 64 lanes idle on a kernel that is nothing
// but round trips to uncached memory (33 us per 131 k rows; 0.25 ns per row).
__global__ void k_board_collect(const DevSampler sm, long long G, long long row, const DrawRec* __restrict__ draws, int n_hs,
                                int to_state, int to_chain) {
    const int nd = sm.n_dim, re = board_row_entries(nd), rpw = 64 / re;   // rows per wave (kMaxDim + 2 <= 24 entries: >= 2)
    const int lane = threadIdx.x & 63, sub = lane / re, col = lane - sub * re;
    const long long wave = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const long long item = wave * rpw + sub;
    if (sub >= rpw || item >= (long long)n_hs * sm.n_half) return;
    const int h = (int)(item / sm.n_half);
    const DrawRec dr = draws[item];
    if (dr.wid < 0 || col > nd + 1) return;
    if (board_aborted(sm)) return;
    const double v = board_take(sm, (unsigned int)(G + h + 1), dr.wid, col);
    if (to_state) {
        if (col < nd) sm.X[(size_t)dr.wid * nd + col] = v;
        else if (col == nd) sm.LP[dr.wid] = v;
        else sm.nacc[dr.wid] = (long long)v;
    }
    if (to_chain && sm.store_chain) {
        if (col < nd) sm.chain[((size_t)(row + h / 2) * sm.n_walkers + dr.wid) * nd + col] = v;
        else if (col == nd) sm.chain_lp[(size_t)(row + h / 2) * sm.n_walkers + dr.wid] = v;
    }
}

// The serial head of one proposal, executed by ONE wave (lane = 0..63): rows of the walker and of its partner ->
// proposal -> logarithms (one parameter per lane) -> coefficients, log-prior; lane 0 leaves them in LDS: sc[0 .. kNCoef)
// the coefficients, sc[kNCoef] the log-prior, sq the proposal, sx the walker's position and sx[kMaxDim] its
// log-posterior.
// BOARD: the rows come from this rank's row board instead of X / LP -- lanes 0 .. nd-1 poll the partner's position,
// lanes 16 .. 16+nd+1 the walker's position, log-posterior and acceptance count (left in sx[kMaxDim + 1]), each for the
// version the draw record names -- and are handed round by shuffles; everything after that is the same arithmetic.
// What the head reads from memory, requested first (head_fetch) and used later (proposal_head): the kernels put their
// other early loads between the two, so that nothing of theirs queues in front of these.
template <int ND>
struct HeadRows {
    static constexpr int kD = ND > 0 ? ND : kMaxDim;
    double x[kD], cj[kD];   // the walker's position, the partner's
    double lp_i, got;       // the walker's log-posterior; BOARD: this lane's word of the rows
    PriorDev prior;         // lane d: the prior of parameter d
};

// (The resident k_solo_run has a head of its own: lane_head_fetch / lane_head below.)
template <int ND, int BOARD = 0>
__device__ __forceinline__ void head_fetch(const DevProblem& pb, const DevSampler& sm, const DrawRec& dr, int lane,
                                           HeadRows<ND>& h, long long G = 0, long long g_run0 = 0, unsigned int arrive_goal = 0u) {
    constexpr int kD = ND > 0 ? ND : kMaxDim;
    const int nd = ND > 0 ? ND : sm.n_dim;
    const double* xs = sm.X + (size_t)dr.wid * nd;
    const double* cs_ = sm.X + (size_t)dr.pid * nd;
    h.got = 0.;
    if (BOARD) {
        const bool own = lane >= 16;
        const int col = own ? lane - 16 : lane;
        if (own ? col <= nd + 1 : col < nd) {
            const unsigned int tag = board_tag(G, own ? dr.wage : dr.page, g_run0);
            const int who = own ? dr.wid : dr.pid;
            h.got = board_take<BOARD == 2>(sm, tag, who, col, arrive_goal);
        }
    }
    h.lp_i = BOARD ? lane_value(h.got, 16 + nd) : sm.LP[dr.wid];
#pragma unroll
    for (int d = 0; d < kD; ++d) {
        h.x[d] = d < nd ? (BOARD ? lane_value(h.got, 16 + d) : xs[d]) : 0.;
        h.cj[d] = d < nd ? (BOARD ? lane_value(h.got, d) : cs_[d]) : 0.;
    }
    // (measured: requesting the prior in FRONT of the poll instead changes nothing -- 5.45 against 5.43 us; its way from L2
    // is hidden behind the logarithms either way)
    h.prior = PriorDev{0, 0, 0., 0., 0., 1.};
    if (lane < pb.n_dim && pb.has_priors) h.prior = pb.priors[lane];
}

template <int ND, int BOARD = 0, int MODEL = 0>
__device__ __forceinline__ void proposal_head(const DevProblem& pb, const DevSampler& sm, const DrawRec& dr, int lane,
                                              double* __restrict__ sc, double* __restrict__ sq, double* __restrict__ sx,
                                              const HeadRows<ND>& h) {
    constexpr int kD = ND > 0 ? ND : kMaxDim;
    const int nd = ND > 0 ? ND : sm.n_dim;
    const PriorDev my_prior = h.prior;
    double x[kD], q[kMaxDim], lq[kMaxDim];
#pragma unroll
    for (int d = 0; d < kMaxDim; ++d) q[d] = lq[d] = 0.;
    const double got = h.got;
    const double lp_i = h.lp_i;
    double arg = 1.;
#pragma unroll
    for (int d = 0; d < kD; ++d) {
        x[d] = h.x[d];
        const double cj = h.cj[d];
        q[d] = d < nd ? cj - (cj - x[d]) * dr.z : 0.;   // emcee: c_j - (c_j - x_i) z
        if (lane == d && d < pb.n_par) arg = q[d];
    }
#ifdef LCF_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    LCF_STAMP(0, 2);
    const double lg = flog(arg);
#pragma unroll
    for (int d = 0; d < kD; ++d) lq[d] = lane_value(lg, d);
    LCF_STAMP(0, 3);
    double c[kNCoef];
    walker_coefficients<MODEL>(pb, q, lq, c, MODEL ? true : pb.use_itab != 0);
    LCF_STAMP(0, 4);
    double lpr = 0.;
    if (pb.has_priors) {
        double qv = 0.;
#pragma unroll
        for (int d = 0; d < kD; ++d)
            if (lane == d) qv = q[d];
        const double mine = lane < pb.n_dim ? prior_term(my_prior, qv) : 0.;
#pragma unroll
        for (int d = 0; d < kD; ++d)
            if (d < nd) lpr += lane_value(mine, d);   // the same ordered sum as walker_log_prior
    }
    const double count = BOARD ? lane_value(got, 16 + nd + 1) : 0.;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kNCoef; ++k) sc[k] = c[k];
        sc[kNCoef] = lpr;
#pragma unroll
        for (int d = 0; d < kD; ++d)
            if (d < nd) {
                sq[d] = q[d];
                sx[d] = x[d];
            }
        sx[kMaxDim] = lp_i;
        if (BOARD) sx[kMaxDim + 1] = count;   // the walker's acceptance count so far
    }
    LCF_STAMP(0, 5);
}

// ---- the head of the RESIDENT kernels (k_solo_run), lane-parallel ---------------------------------------------------
// The same numbers as head_fetch + proposal_head, operation for operation, but every value stays on the lane that uses
// it: lane d < nd polls for the partner's coordinate d AND the walker's (lanes nd, nd + 1: the walker's log-posterior and
// acceptance count), computes its own coordinate of the proposal and its logarithm, takes its own prior's term, and
// writes its own words of sq / sx.  Only what the coefficients read and the terms of the log-prior -- summed in order --
// travel through scalar registers; lane 0 writes coefficients and log-prior.  The LDS layout is proposal_head's.
// What does not change within a launch comes from the launch's block in LDS, `ru` (RunUniforms).
struct LaneRows {
    double cj, x;     // lane d < nd: coordinate d of the partner, of the walker; lanes nd, nd + 1: x = log-posterior, count
    PriorDev prior;   // lane d: the prior of parameter d
    int n_par, n_dim, has_priors;   // the block's words for lane_head, requested in front of the poll
};

template <int ND, int BOARD>
__device__ __forceinline__ void lane_head_fetch(const DevSampler& sm, const DrawRec& dr, int lane_in, LaneRows& h, long long G,
                                                long long g_run0, unsigned int arrive_goal, const RunUniforms* ru,
                                                int* late_word) {
    const int nd = ND > 0 ? ND : __builtin_amdgcn_readfirstlane(ru->nd);
    const int lane = not_hoisted(lane_in);   // (lane masks and addresses: computed here, not carried across the launch)
    h.cj = h.x = 0.;
    // (lane_head's share of the block goes out with the board's geometry, in front of the poll: the poll's statements
    // order memory, so behind them the read would be a round trip of its own in front of the store of the proposal)
    unsigned char* board = reinterpret_cast<unsigned char*>(ru->board);
    unsigned int ring_mask = ru->ring_mask, row_bytes = ru->row_bytes;
    unsigned long long ver_bytes = ru->ver_bytes;
    h.n_par = ru->n_par, h.n_dim = ru->n_dim, h.has_priors = ru->has_priors;
    // ONE wait for the board's geometry and lane_head's words, here, on every lane: a value that is still on its
    // way at the poll is waited for behind it, with everything requested since
    asm volatile("" : "+v"(board), "+v"(ring_mask), "+v"(row_bytes), "+v"(ver_bytes), "+v"(h.n_par), "+v"(h.n_dim), "+v"(h.has_priors));
#ifdef LCF_POLL_LOOKS
    if (lane == 0) atomicExch(&s_poll_now, 0u);
#endif
    bool waited = false;   // (lanes that do not poll do not wait)
    if (lane <= nd + 1) {
        const unsigned int wtag = board_tag(G, dr.wage, g_run0), ptag = board_tag(G, dr.page, g_run0);
        // (lanes nd, nd + 1 have no entry of the partner's to wait for: they ask for their own twice)
        const bool both = lane < nd;
        const unsigned int tag_l = both ? ptag : wtag;
        const int wid_l = both ? dr.pid : dr.wid;
        const unsigned long long* const pa =
            reinterpret_cast<const unsigned long long*>(board + board_entry_bytes(ring_mask, ver_bytes, row_bytes, tag_l, wid_l, lane));
        const unsigned long long* const pw =
            reinterpret_cast<const unsigned long long*>(board + board_entry_bytes(ring_mask, ver_bytes, row_bytes, wtag, dr.wid, lane));
        board_take_pair<BOARD == 2>(sm, pa, pw, tag_l, wtag, wid_l, dr.wid, lane, arrive_goal, h.cj, h.x, waited);
    }
    // Is this item LATE?  Every polling lane found its rows at the first look: the producers were through before this
    // workgroup asked, so it is behind them -- a workgroup that had to wait is ahead and has slack.  One wave-uniform bit,
    // stored as the 4-byte word above the abort word (the upper half of the double beside the log-prior, which every
    // wave reads behind barrier 1 anyway; the lower half is wave 2's), here and not at the head's end: the store is
    // then long over at barrier 1.
    {
        const int late = __ballot(waited) == 0ull ? 1 : 0;
        if (lane == 0) *late_word = late;
    }
#ifdef LCF_POLL_LOOKS
    if (lane == 0) {   // (an aborted poll counts nothing)
        const unsigned int looks = atomicAdd(&s_poll_now, 0u);
        if (looks > 0u) {
            atomicAdd(&s_poll_looks[looks < 3u ? looks - 1u : 2u], 1u);
            atomicAdd(&s_poll_looks[3], looks);
        }
    }
#endif
    // (the block holds a flat prior where the problem has none; lanes >= kMaxDim read the entry of lane - 16, 32, 48 and
    // never use it: a prior's term is taken from lanes below n_dim only)
    h.prior = ru->priors[lane & (kMaxDim - 1)];
}

// ShockCooling with a parameter that is not positive: the coefficients through pw / pow / sqrt / log, ~1300 instructions
// that a fit hardly ever executes, out of line as cold_column is.  `p_mem`: the proposal (sq), `c_mem`: where the
// coefficients go (sc), both in LDS; lane 0 (`write`) stores them.
template <int MODEL>
__device__ __attribute__((noinline)) void cold_coefficients(const double* consts, const double* p_mem, double* c_mem, bool write) {
    static_assert(MODEL == kShockCooling, "the model whose coefficients have a branch worth moving out");
    double p[kMaxDim], lq[kMaxDim], c[kNCoef];
#pragma unroll
    for (int d = 0; d < kMaxDim; ++d) p[d] = lq[d] = 0.;
#pragma unroll
    for (int d = 0; d < 5; ++d) p[d] = p_mem[d];
#pragma unroll
    for (int d = 0; d < 4; ++d) lq[d] = flog(p[d]);   // (as the one-thread-per-walker callers take them; this branch reads none)
    walker_coefficients<MODEL>(ConstsView{consts, MODEL}, p, lq, c, true);
    if (write) {
#pragma unroll
        for (int k = 0; k < kNCoef; ++k) c_mem[k] = c[k];
    }
}

// EARLY: the other waves stand at a barrier ("barrier 0") directly behind the store of the proposal, and take the
// logarithm of their columns' phases from its t_0 while this wave computes the rest of the head.
template <int ND, int BOARD, int MODEL, bool EARLY = false>
__device__ __forceinline__ void lane_head(const DevProblem& pb, const DrawRec& dr, int lane_in, double* __restrict__ sc,
                                          double* __restrict__ sq, double* __restrict__ sx, const LaneRows& h,
                                          const RunUniforms* ru) {
    constexpr int kD = ND > 0 ? ND : kMaxDim;
    const int nd = ND > 0 ? ND : __builtin_amdgcn_readfirstlane(ru->nd);
    const int lane = not_hoisted(lane_in);
    // (the head's share of the block, requested together -- by lane_head_fetch, in front of the poll; has_priors as a
    // scalar, for the branch)
    const int n_par = h.n_par, n_dim = h.n_dim;
    const int has_priors = __builtin_amdgcn_readfirstlane(h.has_priors);
    const double cj = h.cj, x = h.x;
    const double q = lane < nd ? cj - (cj - x) * dr.z : 0.;   // emcee: c_j - (c_j - x_i) z
#ifdef LCF_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    LCF_STAMP(0, 2);
    // proposal, position, log-posterior and count: one store each, from the lanes that hold them
    if (lane < nd) sq[lane] = q;
    if constexpr (EARLY) __syncthreads();   // barrier 0: the wait is this store's
    if (lane <= nd + 1) sx[lane < nd ? lane : lane - nd + kMaxDim] = x;
    const double lg = flog(lane < n_par ? q : 1.);
    // what the coefficients read, wave-uniform (a kernel compiled for one model keeps only the broadcasts its model uses)
    double p[kMaxDim], lq[kMaxDim];
#pragma unroll
    for (int d = 0; d < kMaxDim; ++d) p[d] = lq[d] = 0.;
#pragma unroll
    for (int d = 0; d < kD; ++d) {
        p[d] = lane_value(q, d);
        lq[d] = lane_value(lg, d);
    }
    LCF_STAMP(0, 3);
    double c[kNCoef];
    bool c_stored = false;
    if constexpr (MODEL == kShockCooling) {
        // (walker_coefficients' own test, made here so that only its plain-power branch is inlined)
        const double v = p[0], M = p[1], f = p[2], R = p[3];
        if (v > 0. && M > 0. && f > 0. && R > 0. && v < 1e100 && M < 1e100 && f < 1e100 && R < 1e100) {
            walker_coefficients<MODEL, ConstsView, true>(ConstsView{ru->consts, MODEL}, p, lq, c, true);
        } else {
#pragma unroll
            for (int k = 0; k < kNCoef; ++k) c[k] = 0.;
            cold_coefficients<MODEL>(ru->consts, sq, sc, lane == 0);
            c_stored = true;
        }
    } else {
        walker_coefficients<MODEL>(ConstsView{ru->consts, MODEL ? MODEL : ru->model}, p, lq, c, MODEL ? true : pb.use_itab != 0);
    }
    LCF_STAMP(0, 4);
    double lpr = 0.;
    if (has_priors) {
        const double mine = lane < n_dim ? prior_term(h.prior, q) : 0.;
#pragma unroll
        for (int d = 0; d < kD; ++d)
            if (d < nd) lpr += lane_value(mine, d);   // the same ordered sum as walker_log_prior
    }
    if (lane == 0) {
        if (!c_stored) {
#pragma unroll
            for (int k = 0; k < kNCoef; k += 2) *reinterpret_cast<double2*>(sc + k) = make_double2(c[k], c[k + 1]);
        }
        sc[kNCoef] = lpr;
    }
    LCF_STAMP(0, 5);
}

// ---- single-GPU fit, one workgroup per PROPOSAL: a half-step that owns its accept test ------------------------------
// k_fused gives every (proposal, part) its own workgroup, so no workgroup knows the proposal's likelihood: the accept
// test is re-derived by whoever needs the walker in the next launch, from per-slot records (proposal, draw, partial
// sums) that every launch publishes and the next one loads.  Here ONE workgroup of NPARTS x 256 threads evaluates all
// parts of its proposal -- threads [256 j, 256 j + 256) walk part j exactly as a k_fused workgroup would, same chunks,
// same reduction tree, so the chain is bitwise the one k_fused and the two-kernel path produce -- and thread 0 then
// accepts or rejects and commits the walker itself.  What that removes from the serial head of every half-step:
// the second dependent round trip (slot records, proposals and partial sums of three slots), the three redundant
// accept tests, the per-part repetition of the whole serial section, and every global store except the commit.
// Within a launch X[wid] is read and written by the walker's own workgroup only (partners come from the
// complementary colour, which this half-step does not move), so there is nothing to synchronise.
constexpr int kSoloScratch = kNCoef + 2 + 2 * (kMaxDim + (kMaxDim & 1));  // doubles: coefficients, log-prior, q, x
static_assert(kScBlock == (kSoloScratch + 4) * (int)sizeof(double), "one copy of the scratch words");

// The commit of a plain launch (k_solo without BOARD), by thread 0: accept / reject and commit (models.py:121-135 ->
// fitting.py:121-128 -> emcee's stretch move).  `red`: the wave sums, 4 per part; `sq` / `sx`: the proposal and the
// walker's position, log-posterior behind it; `lpr`: the proposal's log-prior (`excluded`: it is -inf, no likelihood).
template <int ND>
__device__ __forceinline__ void plain_commit(const DevProblem& pb, const DevSampler& sm, const DrawRec& dr, long long row,
                                             long long G, const double* red, const double* sq, const double* sx, double lpr,
                                             bool excluded, const int nd) {
    constexpr int kD = ND > 0 ? ND : kMaxDim;
    double nlp = -INFINITY;
    if (!excluded) {
        double sum = pb.use_sigma ? 0. : pb.log_norm_const;   // fixed order: parts, each (w0 + w1) + (w2 + w3)
        for (int k = 0; k < pb.n_parts; ++k) sum += (red[4 * k] + red[4 * k + 1]) + (red[4 * k + 2] + red[4 * k + 3]);
        nlp = lpr - 0.5 * sum;
    }
    const double lp_i = sx[kMaxDim];
    const bool ok = (dr.zl + nlp - lp_i) > dr.lnu;   // emcee: (ndim - 1) ln z + lp_new - lp_old > ln u
    if (nlp != nlp) atomicOr(sm.err, 1);
    if (ok) {
#pragma unroll
        for (int d = 0; d < kD; ++d)
            if (d < nd) sm.X[(size_t)dr.wid * nd + d] = sq[d];
        sm.LP[dr.wid] = nlp;
        atomicAdd(reinterpret_cast<unsigned long long*>(&sm.nacc[dr.wid]), 1ull);  // (no return value: nothing waits)
    }
    if (sm.store_chain) {
        double* crow = sm.chain + ((size_t)row * sm.n_walkers + dr.wid) * nd;
#pragma unroll
        for (int d = 0; d < kD; ++d)
            if (d < nd) crow[d] = ok ? sq[d] : sx[d];
        sm.chain_lp[(size_t)row * sm.n_walkers + dr.wid] = ok ? nlp : lp_i;
    }
    LCF_STAMP(0, 10);
#ifdef LCF_STAMPS
    if (blockIdx.x < 1024) g_wall[((G & 1) * 1024 + blockIdx.x) * 2 + 1] = wall_clock64();
#endif
}

// BOARD (multi-GPU, lcf_sampler_run_rows): the launch covers this rank's slots [slot_lo, slot_lo + gridDim.x) of
// half-step G; rows come from this rank's row board and the commit posts the walker's new row on EVERY rank's board.
// No rank computes anything about another rank's proposals, and nothing but these rows travels.
// NPARTS: 2 = engines with up to two parts, one per 256 threads; 4 = three or four parts, the two groups of 256
// threads take parts j, j + 2 one after the other.  512 threads either way, so that two workgroups share a CU and one's
// serial head overlaps the other's points (1024-thread workgroups for four parts, one per CU: companion fit 1.26e7
// walker-steps/s; this way 1.41e7).
// MODEL > 0: the kernel is compiled for that one model and for what the benchmark shapes have in common -- dense columns,
// interpolants proved from their first interval, no fitted sigma -- so that the other models' arithmetic is not in its
// instruction stream (a launch streams its code from L2 into cold instruction caches: 89 KiB of kernel, ~28 KiB of
// them executed, cost the generic kernel a third of its time).
// NPARTS = 8: three or four parts again, but FOUR groups of 256 threads, one part each at the same time (1024 threads):
// for launches of at most one workgroup per CU -- a rank's share of a strongly scaled ensemble, configs[2] on 8 GPUs:
// 256 proposals -- where a second workgroup to overlap with does not exist and the parts of one proposal can.
// BOARD = 3: the same between ranks (k_solo_run<..., RANKS>): rows from this rank's board, the commit posts on every rank's;
// state and chain are collected from the board behind the launch (k_board_collect), nothing else is written here.
// BOARD = 2: one half-step of a ONE-LAUNCH run (k_solo_run below): rows from / to this GPU's own board, the chain written
// here; `first`: the workgroup's first half-step of the launch (tables staged, first columns fetched: both stay).
// Returns true when the run is aborted (uniform over the workgroup).
template <int ND, int VARIANT, bool THERM, int NPARTS, int BOARD, int MODEL>
__device__ __forceinline__ bool solo_half_step(const DevProblem& pb, const DevProblem* __restrict__ pbp, const DevSampler& sm, long long row,
                                               const DrawRec* __restrict__ draws, const DrawRec* draws_next, long long G,
                                               long long g_run0, int i, unsigned char* smem, ColumnOperands& first_col,
                                               bool first, bool write_state, const int tid, const int run_flags = 0,
                                               const unsigned int arrive_goal = 0u, const RunUniforms* ru = nullptr,
                                               const DrawRec* held = nullptr, const int copy = 0) {
    // RES (k_solo_run): the launch's invariants come from its block in LDS, `ru` (RunUniforms, right behind the words
    // below), wherever the half-step would otherwise load a field of `pb` / `sm`; the cold paths keep `pb`.
    // `copy` (RES; 0 or 1, wave-uniform): which of the two copies of the scratch words this item uses -- the parity of
    // the workgroup's count of items.  Behind barrier 2 wave 1 alone commits the item, out of this copy, while wave 0
    // is already in the head of the workgroup's next item and writes the other one.
    constexpr bool RES = BOARD >= 2;
    double* exptab = reinterpret_cast<double*>(smem);
    double* red = exptab + kExpTabSize;                                     // 4 wave sums per part (32 reserved)
    double2* ltab = reinterpret_cast<double2*>(smem + kLdsHead * sizeof(double));
    const FiltDesc* fdesc = RES ? nullptr : reinterpret_cast<const FiltDesc*>(ltab + pb.n_lds_tab);   // (RES: where needed)
    int itab_at = -1;
    if constexpr (!RES)
        itab_at = pb.n_itab_lds > 0
                      ? (int)(kLdsHead * sizeof(double) + (pb.n_lds_tab + kFdD2 * pb.n_filters) * sizeof(double2)) : -1;
    double* sc = RES ? reinterpret_cast<double*>(const_cast<RunUniforms*>(ru)) - (copy ? kSoloScratch + 4 : 2 * (kSoloScratch + 4))
                     : reinterpret_cast<double*>(ltab + pb.stage_d2);  // coefficients, then log-prior
    double* sq = sc + kNCoef + 2;                                           // the proposal
    double* sx = sq + kMaxDim + (kMaxDim & 1);                              // the walker's current position, lp, draw
    // BOARD: [0] = 1: the launch is aborted (RES: the word beside the log-prior, so that one LDS read brings both);
    // RES: [1] = 1: the item is late -- its poll found every row at the first look (wave 0's word; lane_head_fetch)
    int* sctl = reinterpret_cast<int*>(sc + (RES ? kNCoef + 1 : kSoloScratch + 2));
    constexpr int kGroups = NPARTS == 8 ? 4 : 2;     // groups of 256 threads, each walks one part at a time
    constexpr int kThreads = kBlock * kGroups;
    const int nd = ND > 0 ? ND : RES ? __builtin_amdgcn_readfirstlane(ru->nd) : sm.n_dim;
    const bool reddened = !MODEL && (RES ? __builtin_amdgcn_readfirstlane(ru->model) : pb.model) == kShockCooling3;
    LCF_STAMP(0, 0);
#ifdef LCF_STAMPS
    if (tid == 0 && blockIdx.x < 1024) g_wall[((G & 1) * 1024 + blockIdx.x) * 2] = wall_clock64();
#endif
    const DrawRec dr = held != nullptr ? *held : draws[i];     // wave-uniform (`held`: the caller has read it, draw_record)
    if (BOARD == 1 && blockIdx.x == 0 && tid < sm.n_board_ranks)
        // This launch runs, so every launch in front of it in the stream has finished: tell every rank that this rank
        // is through with all half-steps before G (stream order does the counting; no atomics).
        __hip_atomic_store(board_progress(sm.peer_board[tid], sm) + sm.board_rank, (unsigned int)G, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    if (dr.wid < 0) return false;    // an odd ensemble's smaller colour leaves its last slot empty
    LCF_STAMP(0, 1);
    // the operands of this thread's first column (of the first part its half of the workgroup walks): requested now,
    // needed behind the barrier
    // (the head's own loads go first; the other waves' streams -- tables, photometry: 80 KiB per workgroup through the
    // same path -- start once they are out: rows + proposal 3.8 k cycles with everything requested at once, 2.1 k alone)
    // (model-specialised kernels only: the generic ones need the registers for the point-by-point path)
    constexpr bool kFetch = MODEL != 0;
    // The early phase logarithm (resident kernels that can take lean columns): a column's tlog(t - t_0) needs nothing of
    // the head but the proposal's t_0, which exists one multiply-add behind the poll -- and the seven other waves stand
    // idle until the head is through.  Wave 0 therefore passes a barrier of its own ("barrier 0") right behind the store of
    // the proposal, and the others take the logarithm of their column between that barrier and barrier 1, in the shadow
    // of wave 0's own logarithm, coefficients and priors; behind barrier 1 lean_column starts from it.  Every wave
    // passes barrier 0 on every path that passes barrier 1; an excluded proposal, a shape that is not lean and an
    // aborted launch drop the value.  t_0 is coordinate kT0 of the proposal: c[0] of walker_coefficients, per model.
    constexpr bool kEarly = RES && MODEL != 0 && NPARTS <= 2;
    constexpr int kT0 = MODEL == kShockCooling ? 4 : MODEL == kShockCooling2 ? 3 : -1;
    static_assert(!kEarly || kT0 >= 0, "a model-specialised resident kernel names the coordinate that is t_0");
    // (Wave 0 is the head and takes the logarithm of its own columns behind barrier 1.  Measured and dropped: a wave of
    // another SIMD that takes them too and hands them over in 64 doubles of LDS -- DESIGN section 5.)
    double lt_early = 0.;
    if (tid < 64) {
        // Resident workgroups drift apart, so this head shares its SIMD with column waves of the CU's other workgroup:
        // the one wave that everybody behind it waits for goes first (5.75 against 6.03 us per half-step; with a launch
        // per half-step both workgroups are in their heads at once and the priority only starves the staging waves:
        // 8.06 against 7.71 us)
        if (BOARD >= 2) __builtin_amdgcn_s_setprio(3);
        if constexpr (RES) {
            LaneRows rows;
            lane_head_fetch<ND, BOARD>(sm, dr, tid, rows, G, g_run0, arrive_goal, ru, sctl + 1);
            if (kFetch && first) fetch_column<VARIANT, MODEL>(pb, tid / kBlock, tid % kBlock, first_col);
            lane_head<ND, BOARD, MODEL, kEarly>(pb, dr, tid, sc, sq, sx, rows, ru);
        } else {
            HeadRows<ND> rows;
            head_fetch<ND, BOARD>(pb, sm, dr, tid, rows, G, g_run0, arrive_goal);
            if (kFetch && first) fetch_column<VARIANT, MODEL>(pb, tid / kBlock, tid % kBlock, first_col);
            proposal_head<ND, BOARD, MODEL>(pb, sm, dr, tid, sc, sq, sx, rows);
        }
        if (BOARD >= 2) __builtin_amdgcn_s_setprio(0);
    } else {
        if (kFetch && first) fetch_column<VARIANT, MODEL>(pb, tid / kBlock, tid % kBlock, first_col);
        // Touch the draw record this block index needs in the NEXT launch: block -> XCD placement repeats from launch
        // to launch, so the record is then in this XCD's L2 instead of HBM when the next serial head starts with it
        // (a hint only: nothing depends on the value or on the placement).
        if (BOARD >= 2) {
            // Resident launches: the record is read by scalar loads at the top of the next half-step (k_solo_run reads
            // the records through a constant-address-space pointer; while they went through an ordinary pointer the
            // compiler read them with vector loads, which this hint only served from the XCD's L2), so it is the scalar
            // cache of this CU that should hold it by then -- two scalar loads, of the record's first and last word: a
            // 48-byte record sits at offset 0, 16, 32 or 48 of a 64-byte line and straddles two of them at 32 and 48 --
            // waited for here, by a wave that has nothing else to do in the shadow of the head (5.51 -> 5.42 us per
            // half-step against the vector touch below, which only brings the record into the XCD's L2).
            // (Wave 2's duty, as the abort word below: wave 1 comes here from the commit of the previous item, and a
            // round trip of its own in front of barrier 0 would make wave 0 wait for it.)
            if (tid >= 64 * kShadowWave && tid < 64 * kShadowWave + 64 && draws_next != nullptr) {
                const int* nxt = reinterpret_cast<const int*>(draws_next + i);
                int a_, b_;
                asm volatile("s_load_dword %0, %2, 0x0\n\ts_load_dword %1, %2, 0x2c\n\ts_waitcnt lgkmcnt(0)"
                             : "=&s"(a_), "=&s"(b_) : "s"(nxt) : "memory");
            }
        } else if (tid == 64 && draws_next != nullptr) {
            const volatile int* nxt = reinterpret_cast<const volatile int*>(draws_next + i);
            (void)nxt[0];
            (void)nxt[sizeof(DrawRec) / sizeof(int) - 1];
        }
        // (the abort word: requested while wave 0 still polls, in front of barrier 0 -- these waves reach this place while
        // wave 0 is still in its poll, so the round trip is over before wave 0 arrives; into THIS item's copy of the words)
        if constexpr (RES)
            if (tid == 64 * kShadowWave) sctl[0] = board_aborted_at<BOARD == 2>(ru->abort_word) ? 1 : 0;   // (in the shadow of the head)
        if constexpr (kEarly) {
            const int tid_e = not_hoisted(tid);
            // (only a wave that will take lean columns needs the value: the group's record is a launch invariant, and a
            // wave without columns has no operands -- have_o)
            const bool lean_e = __builtin_amdgcn_readfirstlane(ru->group[__builtin_amdgcn_readfirstlane(tid_e / kBlock)].lean) != 0;
            const bool mine = lean_e && first_col.have_o;
            __syncthreads();   // barrier 0: wave 0 has stored the proposal
            const double t0 = sq[kT0];
            if (mine) lt_early = tlog(first_col.t - t0);
        }
        // (the tables of the launch's first half-step stay behind barrier 0: in front of it wave 0 would wait for them)
        if (!reddened && first) stage_tables<VARIANT, true>(pb, exptab, ltab, 0., tid - 64, kThreads - 64);
        LCF_STAMP(1, 11);
        if (BOARD == 1 && tid < 128) {
            // In the shadow of the head: has every rank finished half-step G - 2 (lane = rank)?  has this rank given up?
            const int lane = tid - 64;
            const unsigned int* progress = board_progress(sm.board, sm);
            const unsigned long long t0 = wall_clock64();
            bool abort = false;
            for (;;) {
                bool ok = true;
                // rank `lane` has posted P when all its half-steps before P were finished: G - 2 is finished from P = G - 1
                if (G - 2 >= g_run0 && lane < sm.n_board_ranks)   // (earlier half-steps ended with an earlier run)
                    ok = (int)(__hip_atomic_load(progress + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) -
                               (unsigned int)(G - 1)) >= 0;
                abort = board_aborted(sm);
                if (__all(ok) || abort) break;
                if (wall_clock64() - t0 > sm.wait_ticks) {
                    board_abort(sm, 2u, (unsigned int)G, (unsigned int)__builtin_ctzll(~__ballot(ok)), 0u);
                    abort = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            if (lane == 0) sctl[0] = abort ? 1 : 0;
        }
    }
    __syncthreads();
    LCF_STAMP(0, 6);
    double lpr;
    // (RES, lean columns: the group's record, the interpolants' grid and the state's constants)
    lcf_i32x4 col_group = {0, 0, 0, 0}, col_itab = {0, 0, 0, 0};
    double2 col_grid = make_double2(0., 0.);
    double col_consts[5] = {0., 0., 0., 0., 0.};
    if constexpr (RES) {
        // log-prior and abort word in one read; and with it everything of the block that the columns read
        const double2 la = *reinterpret_cast<const double2*>(sc + kNCoef);
        if constexpr (MODEL != 0 && NPARTS <= 2) {
            const int group = __builtin_amdgcn_readfirstlane(not_hoisted(tid) / kBlock);
            col_group = *reinterpret_cast<const lcf_i32x4*>(&ru->group[group]);
            col_grid = *reinterpret_cast<const double2*>(&ru->itab_u0);
            col_itab = *reinterpret_cast<const lcf_i32x4*>(&ru->itab_m);
            const double2 k23 = *reinterpret_cast<const double2*>(&ru->consts[2]);
            col_consts[2] = k23.x, col_consts[3] = k23.y, col_consts[4] = ru->consts[4];
        }
        lpr = la.x;
        if (__builtin_amdgcn_readfirstlane(__double2loint(la.y)) != 0) return true;
        // The columns of a LATE item go first on their SIMDs: a CU holds two resident workgroups for a whole launch, and
        // at equal priority the issue slots go to the OLDER wave -- launch-long to the same workgroup, whether it is
        // behind or ahead.  (A scalar condition: s_setprio ignores EXEC.)  Back to 0 in front of barrier 2, on every path.
        if (__builtin_amdgcn_readfirstlane(__double2hiint(la.y)) != 0) __builtin_amdgcn_s_setprio(1);
    } else {
        if (BOARD && sctl[0] != 0) return true;   // (uniform: everybody reads the same word)
        lpr = sc[kNCoef];
    }
    double term = 0.;
    const bool excluded = lpr == -INFINITY;  // prior excludes the proposal: likelihood skipped (fitting.py:125)
    // The benchmark shape in a MODEL-specialised kernel: every lane has ONE column, fetched ahead of the head
    // (lean_column); anything else -- more columns than lanes, another filter count, interpolants outside LDS, a wave with
    // a state outside the interpolants -- goes through epochs_loop / the cold path, same numbers.
    bool lean = false;
    if (MODEL != 0 && NPARTS <= 2 && !excluded) {
        const int tid_c = RES ? not_hoisted(tid) : tid;
        const int part = __builtin_amdgcn_readfirstlane(tid_c / kBlock), ltid = tid_c % kBlock;
        int c0, c1;
        if constexpr (RES) {
            c0 = __builtin_amdgcn_readfirstlane(col_group.x);
            c1 = __builtin_amdgcn_readfirstlane(col_group.y);
            lean = first_col.have_o && __builtin_amdgcn_readfirstlane(col_group.z) != 0;
        } else {
            c0 = part_entry(pb.part_col0, part);
            c1 = part_entry(pb.part_col0, part + 1);
            lean = first_col.have_o && itab_at >= 0 && c1 - c0 <= kBlock && part < pb.n_parts;   // (wave-uniform)
        }
        if (lean) {
            LCF_STAMP(0, 7);
            double acc = 0.;
            if (c0 + (ltid & ~63) < c1) {   // (a virtual wave without columns adds nothing)
                const bool live = c0 + ltid < c1;
                bool in_grid;
                if constexpr (kEarly) {
                    if (__builtin_amdgcn_readfirstlane(tid_c >> 6) == 0)   // (wave 0 was the head)
                        lt_early = tlog(first_col.t - sc[0]);
                    in_grid = lean_column<MODEL, true>(ColumnView{col_consts, col_grid.x, col_grid.y, col_itab.x, nullptr}, sc,
                                                       first_col, ExpTab{exptab}, col_itab.y, acc, lt_early);
                } else if constexpr (RES)
                    in_grid = lean_column<MODEL>(ColumnView{col_consts, col_grid.x, col_grid.y, col_itab.x, nullptr}, sc, first_col,
                                                 ExpTab{exptab}, col_itab.y, acc);
                else
                    in_grid = lean_column<MODEL>(pb, sc, first_col, ExpTab{exptab}, itab_at, acc);
                if (!in_grid)
                    acc = cold_column_with_state<VARIANT, MODEL>(pbp, sc, sq, first_col.t, min(c0 + ltid, c1 - 1), live);
                term = live ? acc : 0.;     // (lanes beyond the part repeated its last column)
            }
            LCF_STAMP(0, 8);
            LCF_STAMP(1, 12);
            const double ws = wave_sum(term);
            if ((tid & 63) == 0) red[tid_c >> 6] = ws;
        }
    }
    if (!excluded && !lean) {
        double cs[kNCoef];
#pragma unroll
        for (int k = 0; k < kNCoef; ++k) cs[k] = uniform_f64(sc[k]);
        if constexpr (RES) {   // (the general path: not where the time goes)
            fdesc = reinterpret_cast<const FiltDesc*>(ltab + pb.n_lds_tab);
            itab_at = __builtin_amdgcn_readfirstlane(ru->itab_at);
        }
        if (reddened) stage_tables<VARIANT, true>(pb, exptab, ltab, cs[6], tid, kThreads);
        // threads [256 j, 256 j + 256) are the virtual threads of part j (NPARTS = 4: then of part j + 2, ...): each lane
        // computes the thermal state of its column and walks the column's points (epochs_loop)
        const int part = tid / kBlock, ltid = tid % kBlock;
        if (reddened) __syncthreads();
        LCF_STAMP(0, 7);
        if (NPARTS > 2) {
#pragma unroll 1
            for (int pp = part; pp < pb.n_parts; pp += kGroups) {
                term = epochs_loop<VARIANT, true, kFetch, MODEL, true>(pb, pp, sq, cs, ltab, fdesc, ExpTab{exptab}, ltid, itab_at,
                                                                       first_col, pp == part, pbp, sc);
                const double ws = wave_sum(term);
                if ((tid & 63) == 0) red[4 * pp + (ltid >> 6)] = ws;
            }
        } else {
            if (part < pb.n_parts)
                term = epochs_loop<VARIANT, true, kFetch, MODEL, true>(pb, part, sq, cs, ltab, fdesc, ExpTab{exptab}, ltid, itab_at,
                                                                       first_col, true, pbp, sc);
            LCF_STAMP(0, 8);
            LCF_STAMP(1, 12);
            const double ws = wave_sum(term);
            if ((tid & 63) == 0) red[tid >> 6] = ws;
        }
    }
    if constexpr (RES) __builtin_amdgcn_s_setprio(0);   // (a late item's columns ran at priority 1)
    __syncthreads();
    LCF_STAMP(0, 9);
    if (BOARD) {
        // ---- accept / reject by ONE wave (wave 0; the resident kernels: wave 1); lanes 0 .. nd+1 post the row (position,
        // log-posterior, acceptance count) on every rank's board; this rank's X / LP / counts follow for its own walkers
        // (the others' come from the board when the run ends, and the chain is written from the board)
        // (RES: by the committing wave, wave 1 -- kCommitWave.  Wave 0 is the head of the workgroup's next item and
        // leaves here for its poll: nothing below needs it, every operand is reloaded from LDS and the draw record, and
        // `lpr` / `excluded` were read behind barrier 1 by every wave.  Every wave still passes the same barriers per item.)
        constexpr int kCommit0 = RES ? 64 * kCommitWave : 0;   // the committing wave's first thread
        if (tid < kCommit0 || tid >= kCommit0 + 64) return false;
        if (BOARD >= 2) __builtin_amdgcn_s_setprio(3);   // (the row's readers wait for this)
        if constexpr (RES) {
            // Every LDS read between here and the post -- the wave sums, the walker's log-posterior and count, this lane's
            // number of the proposal and of the position, the block's words for the sum and for the row's address -- and
            // the record's words for the accept test and the post, which nobody has carried across the columns.
            // The sum keeps its order, (w0 + w1) + (w2 + w3) per part, parts in order.
            const int ctid = tid - kCommit0;   // the lane: column of the row
            const int col = not_hoisted(ctid);
            const int mine = col < nd ? col : 0;
            const unsigned int tag = (unsigned int)(G + 1);
            int wid = dr.wid;
            double zl = dr.zl, lnu = dr.lnu, sum, lp_i, count0, q_mine, x_mine;
            size_t entry;   // (the same on every rank's board)
            unsigned char* own_board;
            if constexpr (NPARTS <= 2) {
                // ONE statement requests all of it, the record's words by scalar loads, and waits once (commit_batch)
                const unsigned int sc_at = lds_offset(sc);
                CommitOperands c;
                commit_batch(lds_offset(red), sc_at, sc_at + 8u * (unsigned int)mine, lds_offset(ru), draws + i, c);
                wid = c.wid, zl = f64_of(c.zl_lnu.x, c.zl_lnu.y), lnu = f64_of(c.zl_lnu.z, c.zl_lnu.w);
                // (board_entry_bytes, from the batch's words)
                entry = (tag & c.geo.z) * (unsigned long long)__double_as_longlong(c.ver_bytes) +
                        ((size_t)(unsigned int)wid * c.geo.w + 16u * (unsigned int)col);
                own_board = reinterpret_cast<unsigned char*>((size_t)c.geo.x | ((size_t)c.geo.y << 32));
                sum = f64_of(c.sums.x, c.sums.y);
                const int n_parts = (int)c.sums.z;
                const double s1 = sum + ((f64_of(c.a0.x, c.a0.y) + f64_of(c.a0.z, c.a0.w)) + (f64_of(c.a1.x, c.a1.y) + f64_of(c.a1.z, c.a1.w)));
                sum = n_parts > 0 ? s1 : sum;
                const double s2 = sum + ((f64_of(c.b0.x, c.b0.y) + f64_of(c.b0.z, c.b0.w)) + (f64_of(c.b1.x, c.b1.y) + f64_of(c.b1.z, c.b1.w)));
                sum = n_parts > 1 ? s2 : sum;
                lp_i = f64_of(c.lc.x, c.lc.y), count0 = f64_of(c.lc.z, c.lc.w);
                q_mine = c.q_mine, x_mine = c.x_mine;
            } else {
                // Plain LDS reads (the four-group kernels)
                lcf_u32x4 r;
                record_reload(draws + i, r, wid);
                zl = f64_of(r.x, r.y), lnu = f64_of(r.z, r.w);
                const double2* red2 = reinterpret_cast<const double2*>(red);
                const double2 lc = *reinterpret_cast<const double2*>(sx + kMaxDim);   // log-posterior | acceptance count
                q_mine = sq[mine], x_mine = sx[mine];
                entry = board_entry_bytes(*ru, tag, wid, col);
                own_board = reinterpret_cast<unsigned char*>(ru->board);
                sum = ru->sum0;
                const int n_parts = __builtin_amdgcn_readfirstlane(ru->n_parts);
                for (int k = 0; k < n_parts; ++k) sum += (red2[2 * k].x + red2[2 * k].y) + (red2[2 * k + 1].x + red2[2 * k + 1].y);
                lp_i = lc.x, count0 = lc.y;
            }
            const double scored = lpr - 0.5 * sum;
            const double nlp = excluded ? -INFINITY : scored;
            const bool ok = (zl + nlp - lp_i) > lnu;
            const double count = count0 + (ok ? 1. : 0.);
            if (ctid <= nd + 1) {
                const double v = ctid < nd ? (ok ? q_mine : x_mine) : ctid == nd ? (ok ? nlp : lp_i) : count;
                // the row first: its readers wait for it; state, snapshot and chain follow
                if (BOARD == 2) {
                    board_post_at<true>(reinterpret_cast<unsigned long long*>(own_board + entry), tag, v);
                } else {
#pragma unroll
                    for (int r = 0; r < kMaxPeers; ++r)
                        if (r < sm.n_board_ranks)
                            board_post_at(reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(sm.peer_board[r]) + entry),
                                          tag, v);
                }
                // (a one-launch run writes the state in its last step only: every walker moves exactly once there, while two
                // moves of a walker in one launch come from different workgroups, and whose store reaches memory last is open)
                if (BOARD == 2 && write_state) {   // (the set of state buffers the run did NOT start from: chosen by the fill)
                    if (ctid < nd)
                        ru->X[(size_t)wid * nd + ctid] = v;
                    else if (ctid == nd)
                        ru->LP[wid] = v;
                    else
                        ru->nacc[wid] = (long long)v;
                    unsigned long long* const snap = ru->snap_out;
                    if (snap) {   // ... and the host's copy of it
                        const size_t nw = ru->n_walkers;
                        if (ctid < nd) snap[1 + (size_t)wid * nd + ctid] = (unsigned long long)__double_as_longlong(v);
                        else if (ctid == nd) snap[1 + nw * nd + wid] = (unsigned long long)__double_as_longlong(v);
                        else snap[1 + nw * nd + nw + wid] = (unsigned long long)(long long)v;
                    }
                }
                if (BOARD == 2 && (run_flags & kRunStoreChain)) {   // (one GPU: every walker's row is decided here)
                    const size_t at = (size_t)row * ru->n_walkers + wid;
                    if (ctid < nd) ru->chain[at * nd + ctid] = v;
                    else if (ctid == nd) ru->chain_lp[at] = v;
                }
            }
            if (ctid == 0 && nlp != nlp) {
                atomicOr(sm.err, 1);
                if (BOARD == 2 && sm.snap_flags) sm.snap_flags[blockIdx.x & (kSnapFlags - 1)] = 1u;
            }
            __builtin_amdgcn_s_setprio(0);
            LCF_STAMP(kCommitWave, 10);
            return false;
        }
        // (from here on BOARD = 1 alone: the resident forms have returned)
        double nlp = -INFINITY;
        if (!excluded) {
            double sum = pb.use_sigma ? 0. : pb.log_norm_const;
            for (int k = 0; k < pb.n_parts; ++k) sum += (red[4 * k] + red[4 * k + 1]) + (red[4 * k + 2] + red[4 * k + 3]);
            nlp = lpr - 0.5 * sum;
        }
        const double lp_i = sx[kMaxDim];
        const bool ok = (dr.zl + nlp - lp_i) > dr.lnu;
        const double count = sx[kMaxDim + 1] + (ok ? 1. : 0.);
        if (tid <= nd + 1) {
            const double v = tid < nd ? (ok ? sq[tid] : sx[tid]) : tid == nd ? (ok ? nlp : lp_i) : count;
#pragma unroll
            for (int r = 0; r < kMaxPeers; ++r)
                if (r < sm.n_board_ranks) board_post(sm.peer_board[r], sm, (unsigned int)(G + 1), dr.wid, tid, v);
            // (the three pointers are read HERE, in front of the branches, on purpose: read where they are used, the
            // same instructions come out in another order in all 25 BOARD = 1 kernels -- tools/isa_diff.py)
            double* X = sm.X;
            double* LP = sm.LP;
            long long* nacc = sm.nacc;
            if (tid < nd)
                X[(size_t)dr.wid * nd + tid] = v;
            else if (tid == nd)
                LP[dr.wid] = v;
            else
                nacc[dr.wid] = (long long)v;
        }
        if (tid == 0 && nlp != nlp) atomicOr(sm.err, 1);
        LCF_STAMP(0, 10);
        return false;
    }
    if (tid != 0) return false;
    plain_commit<ND>(pb, sm, dr, row, G, red, sq, sx, lpr, excluded, nd);
    return false;
}

template <int ND, int VARIANT, bool THERM, int NPARTS, bool BOARD = false, int MODEL = 0>
__global__ __launch_bounds__(kBlock * (NPARTS == 8 ? 4 : 2), LCF_WAVES)
void k_solo(const DevProblem* __restrict__ pbp, const DevSampler sm, long long row, const DrawRec* __restrict__ draws,
            const DrawRec* draws_next, long long G, long long g_run0, int slot_lo) {
    extern __shared__ __align__(16) unsigned char smem[];
    ColumnOperands first_col;
    // The problem is read through a constant-address-space pointer: scalar loads where a field is used, instead of
    // 700 bytes of kernel arguments preloaded into (and spilled from) scalar registers.
    typedef const DevProblem __attribute__((address_space(4)))* ProblemPtr;
    const DevProblem& pb = *(const DevProblem*)(ProblemPtr)pbp;
    solo_half_step<ND, VARIANT, THERM, NPARTS, BOARD ? 1 : 0, MODEL>(pb, pbp, sm, row, draws, draws_next, G, g_run0,
                                                                     blockIdx.x + (BOARD ? slot_lo : 0), smem, first_col, true,
                                                                     true, threadIdx.x);
}

// ---- a whole run (or a block of it) in ONE launch -------------------------------------------------------------------
// The workgroups stay: workgroup b takes slot b (b + gridDim.x, ...) of half-step G0, then of G0 + 1, ... -- no kernel
// boundary between half-steps, tables staged and first columns fetched once per launch, and nothing makes two
// workgroups of a CU run in step, so one's serial head overlaps the other's columns.  What a half-step needs from an
// earlier one -- the rows of its walker and of the partner -- comes from a board of tagged rows in this GPU's memory,
// exactly as between the ranks of a row-board run (BOARD = 2): a head polls for the version its draw record names.
// Every wait is for a row of an EARLIER half-step, so the launch makes progress as long as all its workgroups are
// resident at once: the host launches no more than the device holds.  The ring keeps more versions than a launch has
// half-steps (DevSampler::ring), so no workgroup can overrun a version another one still waits for.
// RANKS: the launch of ONE RANK of a row-board run.  The rank's workgroups take its slots [slot_lo, slot_lo + n_slots) of
// every half-step of the launch; rows come from the rank's own board, every commit goes to the boards of all ranks
// (BOARD = 3).  What bounds the drift between ranks is a word per rank and launch instead of one per half-step: the
// launch's first workgroup posts "this rank has reached half-step G0" on every board -- stream order proves that all the
// rank's earlier launches and their row collections are complete -- and no workgroup starts before every rank has
// reached `need_progress` (the first half-step of the launch before the previous one; 0: nothing to wait for).  With
// at most kRunSpan half-steps per launch, anything a rank still reads is then less than kRing versions behind
// anything another rank writes.
// The launch's block of invariants (RunUniforms), written by ONE wave (lane = 0 .. 63) in front of the loop over the
// half-steps: the first half-step's head reads it like every other one.  `ranks`: no state is written by the launch.
__device__ __forceinline__ void fill_run_uniforms(const DevProblem& pb, const DevSampler& sm, RunUniforms* ru, int run_flags,
                                                  bool ranks, int lane) {
    if (lane == 0) {
        const int entries = board_row_entries(sm.n_dim);
        ru->board = sm.board;
        ru->ring_mask = (unsigned int)(sm.ring - 1);
        ru->row_bytes = 16u * (unsigned int)entries;
        ru->ver_bytes = (unsigned long long)sm.n_walkers * (unsigned long long)entries * 16ull;
        ru->abort_word = board_progress(sm.board, sm) + kMaxPeers;
        ru->sum0 = pb.use_sigma ? 0. : pb.log_norm_const;
        ru->n_parts = pb.n_parts;
        ru->n_walkers = sm.n_walkers;
        ru->n_dim = pb.n_dim;
        ru->n_par = pb.n_par;
        ru->has_priors = pb.has_priors;
        ru->model = pb.model;
        // (one-launch runs write the state into the set of buffers the run did NOT start from -- kRunFlip says which)
        const bool to_out = !(run_flags & kRunFlip);
        ru->X = ranks ? nullptr : to_out ? sm.X_out : sm.X;
        ru->LP = ranks ? nullptr : to_out ? sm.LP_out : sm.LP;
        ru->nacc = ranks ? nullptr : to_out ? sm.nacc_out : sm.nacc;
        ru->snap_out = sm.snap_out;
        ru->chain = sm.chain;
        ru->chain_lp = sm.chain_lp;
        ru->itab_u0 = pb.itab_u0;
        ru->itab_inv_h = pb.itab_inv_h;
        ru->itab_m = pb.itab_m;
        ru->nd = sm.n_dim;
        ru->pad1 = 0;
    }
    // where the interpolants are staged (solo_half_step's layout)
    const int itab_at = pb.n_itab_lds > 0
                            ? (int)(kLdsHead * sizeof(double) + (pb.n_lds_tab + kFdD2 * pb.n_filters) * sizeof(double2)) : -1;
    if (lane == 1) ru->itab_at = itab_at;
    if (lane >= 2 && lane < 4) {   // per group of 256 threads: its first part
        const int g = lane - 2;
        const int c0 = part_entry(pb.part_col0, g), c1 = part_entry(pb.part_col0, g + 1);
        ru->group[g].c0 = c0;
        ru->group[g].c1 = c1;
        ru->group[g].lean = itab_at >= 0 && c1 - c0 <= kBlock && g < pb.n_parts ? 1 : 0;
        ru->group[g].pad = 0;
    }
    if (lane >= 16 && lane < 28) ru->consts[lane - 16] = pb.consts[lane - 16];
    if (lane >= 32 && lane < 32 + kMaxDim) {
        const int d = lane - 32;
        const bool has = d < pb.n_dim && pb.has_priors;   // (field by field: a struct selected as a whole goes through scratch memory)
        const PriorDev* pr = pb.priors + (has ? d : 0);
        ru->priors[d].kind = has ? pr->kind : 0;
        ru->priors[d].pad = 0;
        ru->priors[d].p_min = has ? pr->p_min : 0.;
        ru->priors[d].p_max = has ? pr->p_max : 0.;
        ru->priors[d].mean = has ? pr->mean : 0.;
        ru->priors[d].stddev = has ? pr->stddev : 1.;
    }
}

template <int ND, int VARIANT, bool THERM, int NPARTS, int MODEL, bool RANKS = false>
__global__ __launch_bounds__(kBlock * (NPARTS == 8 ? 4 : 2), LCF_WAVES)
void k_solo_run(const DevProblem* __restrict__ pbp, const DevSampler* __restrict__ smp, long long rel0,
                const DrawRec* __restrict__ draws0, long long g_run0, int n_hs, long long state_from, int n_wg, int run_flags,
                unsigned int arrive_goal, int slot_lo, int n_slots, long long need_progress) {
    // (n_wg = gridDim.x, except in the test of a launch whose workgroups are not all there: LCF_RUN_TEST_MISSING)
    extern __shared__ __align__(16) unsigned char smem[];
    // (a lane's first column: fetched by the launch's first half-step and kept -- 26 registers, a few of them spilled;
    // fetching it again every half-step costs 0.5 us, in front of the head's own loads)
    ColumnOperands first_col;
    // Problem AND sampler are read through constant-address-space pointers: scalar loads where a field is used.  As
    // kernel arguments the sampler's 60 words stayed in scalar registers across the loop over the half-steps -- and
    // most of them in spill lanes.  What varies from run to run travels in `run_flags`, so that the copy in device
    // memory is written once per sampler (lcf_sampler::run_image).
    typedef const DevProblem __attribute__((address_space(4)))* ProblemPtr;
    typedef const DevSampler __attribute__((address_space(4)))* SamplerPtr;
    const DevProblem& pb = *(const DevProblem*)(ProblemPtr)pbp;
    const DevSampler& sm = *(const DevSampler*)(SamplerPtr)smp;
    constexpr int kBoard = RANKS ? 3 : 2;
    bool first = true;
    // What no half-step of the launch changes: into LDS, once (RunUniforms), behind the half-step's scratch words.
    // Filled HERE, not by the launch's first executed half-step (`first` below): that half-step's head reads the block
    // in front of its first barrier like every other one.  So the block does not depend on `first`, nor on whether a
    // workgroup's first slot is an empty one; what `first` still guards is the staging of the tables and the first columns.
    // (in front of it: the two copies of the half-step's scratch words)
    RunUniforms* const ru = reinterpret_cast<RunUniforms*>(smem + kLdsHead * sizeof(double) + (size_t)pb.stage_d2 * sizeof(double2) +
                                                           2 * (kSoloScratch + 4) * sizeof(double));
    if (threadIdx.x >= 64 && threadIdx.x < 128) fill_run_uniforms(pb, sm, ru, run_flags, RANKS, threadIdx.x - 64);
    if (!RANKS) __syncthreads();   // (RANKS: the barrier below)
    // "this workgroup has started": what a workgroup that waits unusually long for a row looks at (board_take)
    if (threadIdx.x == 0) __hip_atomic_fetch_add(board_arrivals(sm), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (RANKS) {
        __shared__ int s_abort;
        if (blockIdx.x == 0 && threadIdx.x < sm.n_board_ranks)
            __hip_atomic_store(board_progress(sm.peer_board[threadIdx.x], sm) + sm.board_rank, (unsigned int)(g_run0 + rel0),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (threadIdx.x < 64) {
            bool abort = false;
            if (need_progress > 0) {
                const int lane = threadIdx.x;
                const unsigned int* progress = board_progress(sm.board, sm);
                const unsigned long long t0 = wall_clock64();
                for (;;) {
                    bool ok = true;
                    if (lane < sm.n_board_ranks)
                        ok = (int)(__hip_atomic_load(progress + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) -
                                   (unsigned int)need_progress) >= 0;
                    abort = board_aborted(sm);
                    if (__all(ok) || abort) break;
                    if (wall_clock64() - t0 > sm.wait_ticks) {
                        board_abort(sm, 2u, (unsigned int)(g_run0 + rel0), (unsigned int)__builtin_ctzll(~__ballot(ok)),
                                    (unsigned int)need_progress);
                        abort = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(8);
                }
            }
            if (threadIdx.x == 0) s_abort = abort ? 1 : 0;
        }
        __syncthreads();
        if (s_abort != 0) return;
    }
    if (!RANKS && rel0 == 0) {
        // The run's first launch: the state in front of it is version g_run0 of every row (what a draw record's age
        // points at until the walker has moved in this run).  Whoever needs a row polls for it: no barrier behind this.
        // (RANKS: every rank holds the whole state and has posted it on its OWN board: k_board_init, in front of the run.)
        const int nd = ND > 0 ? ND : sm.n_dim;
        const int col = threadIdx.x & 31;   // (n_dim + 2 <= kMaxDim + 2 columns)
        const bool flip = (run_flags & kRunFlip) != 0;
        const double* X = flip ? sm.X_out : sm.X;
        const double* LP = flip ? sm.LP_out : sm.LP;
        const long long* nacc = flip ? sm.nacc_out : sm.nacc;
        for (int w = blockIdx.x * (int)(blockDim.x / 32) + (int)(threadIdx.x / 32); w < sm.n_walkers;
             w += n_wg * (int)(blockDim.x / 32))
            if (col <= nd + 1) {
                const double v = col < nd ? X[(size_t)w * nd + col] : col == nd ? LP[w] : (double)nacc[w];
                board_post<true>(sm.board, sm, (unsigned int)g_run0, w, col, v);
            }
    }
    const int slot_end = slot_lo + n_slots;
    const int n_half = sm.n_half;   // (one scalar register across the loop instead of a load per half-step)
    // (Measured and dropped: the draw record of the NEXT half-step requested one half-step ahead -- by a wave beside the head
    // into LDS, or as a scalar load carried in registers across the half-step -- instead of the touch that only brings
    // it into this XCD's L2: 5.80 / 5.94 against 5.51 us per half-step.  The record's two round trips are hidden
    // already; what the extra live registers cost is not.)
    // Which copy of the scratch words an item uses: the parity of the workgroup's count of executed items (an empty slot
    // is no item), so that the committing wave reads item n's words while wave 0 writes item n + 1's.  Counted from 0 in
    // every launch: nothing in LDS outlives one.
    int copy = 0;
#ifdef LCF_POLL_LOOKS
    if (threadIdx.x == 0)   // (wave 0 alone touches the counts)
        for (int k = 0; k < 4; ++k) atomicExch(&s_poll_looks[k], 0u);
    // where this workgroup runs: HW_ID (register 4, all 32 bits) and XCC_ID (register 20, bits 0 .. 3) of wave 0
    const unsigned int poll_hw_id = __builtin_amdgcn_s_getreg(4 | (31 << 11)), poll_xcc_id = __builtin_amdgcn_s_getreg(20 | (3 << 11));
#endif
#pragma unroll 1
    for (int h = 0; h < n_hs; ++h) {
        const DrawRec* draws = draws0 + (size_t)h * n_half;
#pragma unroll 1
        for (int i = slot_lo + blockIdx.x; i < slot_end; i += n_wg) {
            // the record, once for this test and for the half-step
            const DrawRec rec = draw_record(draws + i);
            if (rec.wid < 0) continue;   // (uniform) an odd ensemble's smaller colour leaves its last slot empty
            // the record this workgroup needs next: its next slot of this half-step, else its first of the next one
            const bool more = i + n_wg < slot_end;
            const DrawRec* hint = more ? draws + n_wg : h + 1 < n_hs ? draws + n_half + (slot_lo + (int)blockIdx.x - i) : nullptr;
            const int tid = threadIdx.x;
            if (solo_half_step<ND, VARIANT, THERM, NPARTS, kBoard, MODEL>(pb, pbp, sm, (rel0 + h) >> 1, draws, hint,
                                                                          g_run0 + rel0 + h, g_run0, i, smem, first_col, first,
                                                                          rel0 + h >= state_from, tid, run_flags, arrive_goal, ru,
                                                                          &rec, copy))
                return;
            first = false;
            copy ^= 1;
        }
    }
#ifdef LCF_POLL_LOOKS
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) atomicAdd(&g_poll_looks[k], (unsigned long long)atomicAdd(&s_poll_looks[k], 0u));
    if (threadIdx.x == 0) {
        const unsigned int at = atomicAdd(&g_poll_wg_n, 1u);
        if (at < (unsigned int)kPollWgMax) {
            unsigned int* rec = g_poll_wg + (size_t)at * kPollWgWords;
            rec[0] = (unsigned int)(g_run0 + rel0), rec[1] = blockIdx.x, rec[2] = poll_hw_id, rec[3] = poll_xcc_id;
            for (int k = 0; k < 4; ++k) rec[4 + k] = atomicAdd(&s_poll_looks[k], 0u);
        }
    }
#endif
}

// The images of DevProblem / DevSampler that kernels read through constant-address-space pointers are WRITTEN BY A
// KERNEL on the stream of the launches that read them: ordinary producer -> consumer order between two kernels of one
// queue.  (A host copy into an image whose address an earlier one had -- a sampler destroyed, the next created -- left
// some workgroups of the next launch with the old struct out of an XCD's L2: rows posted for another board layout, a
// launch that waited for them for ever.  Seen once the inter-rank boards grew and allocations started to recycle
// addresses; tools/debug/rows_mismatch.py.)
template <class T>
__global__ void k_put_image(T* __restrict__ dst, const T src) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *dst = src;
}

// ---- population mode: one launch covers the same half-step of MANY independent transients (blockIdx.y) --------------
struct MultiItem {
    DevProblem pb;
    DevSampler sm;
    const DrawRec* draws[2];        // the sampler's two block buffers (block b in buffer b & 1)
    long long blk_first, blk_steps; // steps in block 0 / in every later block
    double* coef;
    double* lprior;
    // resident population launches (k_pop_run): the transient's board is sm.board; `flip`: its start state is in
    // sm.X_out / LP_out / nacc_out; `arrive0`: its board's count of started workgroups before this run; `itab_extra`:
    // doubles of pb.itab the launch stages in LDS itself, behind the image (the engine's image has them only for long
    // light curves -- a launch per half-step cannot afford 24 KiB more per workgroup, a launch per 32 steps can)
    long long g_run0;
    int flip, itab_extra;
    unsigned int arrive0, pad;
};

// Draw records of a transient's half-step `rel` of the run (the host keeps that block resident).
__device__ inline const DrawRec* item_rows(const MultiItem& it, long long rel) {
    const long long k = rel / 2;
    const long long b = k < it.blk_first ? 0 : 1 + (k - it.blk_first) / it.blk_steps;
    const long long k0 = b == 0 ? 0 : it.blk_first + (b - 1) * it.blk_steps;
    return it.draws[b & 1] + (size_t)(rel - 2 * k0) * it.sm.n_half;
}

template <int ND>
__global__ __launch_bounds__(64) void k_step_multi(const MultiItem* __restrict__ items, int have_prev, long long prev_row,
                                                   int have_next, long long rel, long long g) {
    const MultiItem& it = items[blockIdx.y];
    const int nh = it.sm.n_half;
    if ((int)blockIdx.x >= nh) return;
    step_body<ND>(it.pb, it.sm, blockIdx.x, have_prev, prev_row, have_next,
                  have_next ? item_rows(it, rel) : nullptr, have_prev ? item_rows(it, rel - 1) : nullptr,
                  g, 0, nh, it.coef, it.lprior);
}

template <int VARIANT, bool LDS_TAB, bool THERM>
__global__ __launch_bounds__(kBlock) void k_points_multi(const MultiItem* __restrict__ items, int parity) {
    const MultiItem& it = items[blockIdx.y];
    const int nh = it.sm.n_half;
    if ((int)blockIdx.x >= nh * it.pb.n_parts) return;
    points_body<VARIANT, 0, LDS_TAB, THERM>(it.pb, blockIdx.x, 0, nh, it.sm.Q[parity], it.coef, it.lprior, nullptr,
                                            it.sm.part2[parity], nullptr);
}

// ---- population mode, ONE launch per half-step (k_pop): a workgroup takes FOUR proposals of one transient -----------
// The two launches above spend most of a half-step in k_step_multi's latency chain and in global round trips (proposal,
// coefficients, thermal states and partial sums all travel through memory).  Here one workgroup of four waves owns four
// consecutive proposal slots of a transient: it stages the transient's tables once, every wave runs the serial head of
// ONE of the proposals (four latency chains side by side instead of one after the other), all threads then compute the
// thermal states of the four proposals together and walk the points proposal by proposal -- thread t takes the points
// t, t + 256, ... of a part exactly as a k_points workgroup does, same reduction tree, so a transient's chain is bitwise
// the one the two-launch path produces -- and lane 0 of wave w accepts or rejects and commits proposal w.  Nothing
// between launches but the committed state: no slot records, no coefficients, no thermal states in memory.  The
// transient's DevProblem is read through a constant-address-space pointer: scalar loads, as kernel arguments are.
constexpr int kPopScratch = kSoloScratch + 6;   // doubles per proposal: k_solo's + (ln z term, ln u, walker id), padded
constexpr int kPopMaxParts = 4;
#ifndef LCF_POP_RUN_GROUP
#define LCF_POP_RUN_GROUP 4
#endif
constexpr int kPopRunGroup = LCF_POP_RUN_GROUP;   // proposals (= waves) per workgroup of the resident form (k_pop_run)

#ifndef LCF_POP_WAVES
#define LCF_POP_WAVES LCF_WAVES
#endif
// GROUP = proposals (= waves) per workgroup: 4, or 8 with two proposals' points walked side by side (threads
// [0, 256) and [256, 512), each half exactly as a k_points workgroup).
template <int ND, int VARIANT, int GROUP, int MODEL = 0>
__global__ __launch_bounds__(64 * GROUP, LCF_POP_WAVES) void k_pop(const MultiItem* __restrict__ items, long long rel) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef const MultiItem __attribute__((address_space(4)))* ItemPtr;
    const ItemPtr itp = (ItemPtr)(items + blockIdx.y);
    const MultiItem& it = *(const MultiItem*)itp;
    const DevProblem& pb = it.pb;
    const DevSampler& sm = it.sm;
    constexpr int kThreads = 64 * GROUP;
    const int nh = sm.n_half, slot0 = blockIdx.x * GROUP;
    if (slot0 >= nh) return;
    double* exptab = reinterpret_cast<double*>(smem);
    double2* ltab = reinterpret_cast<double2*>(smem + kLdsHead * sizeof(double));
    const FiltDesc* fdesc = reinterpret_cast<const FiltDesc*>(ltab + pb.n_lds_tab);
    const int itab_at = pb.n_itab_lds > 0
                            ? (int)(kLdsHead * sizeof(double) + (pb.n_lds_tab + kFdD2 * pb.n_filters) * sizeof(double2)) : -1;
    double* scratch = reinterpret_cast<double*>(ltab + pb.stage_d2);       // [GROUP][kPopScratch]
    double* red = scratch + GROUP * kPopScratch;                             // [GROUP][4 * kPopMaxParts] wave sums
    constexpr int kD = ND > 0 ? ND : kMaxDim;
    const int nd = ND > 0 ? ND : sm.n_dim;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        // ---- the serial heads, one per wave, side by side
        double* sc = scratch + wave * kPopScratch;
        double* sq = sc + kNCoef + 2;
        double* sx = sq + kMaxDim + (kMaxDim & 1);
        const int slot = slot0 + wave;
        DrawRec dr{-1, -1, -1, -1, 1., 0., 0., 0, 0};
        if (slot < nh) dr = item_rows(it, rel)[slot];     // wave-uniform
        const bool active = dr.wid >= 0;  // (an odd ensemble's smaller colour leaves its last slot empty)
        // (the rows are requested first, the tables staged while they are on their way: a launch per half-step pays the
        // staging every time, and in front of the heads it was a round trip of its own)
        HeadRows<ND> rows;
        if (active) head_fetch<ND>(pb, sm, dr, lane, rows);
        stage_tables<VARIANT, true>(pb, exptab, ltab, 0., tid, kThreads);
        if (active) proposal_head<ND, false, MODEL>(pb, sm, dr, lane, sc, sq, sx, rows);
        if (lane == 0) {
            if (!active) sc[kNCoef] = -INFINITY;
            sx[kMaxDim + 1] = dr.zl;
            sx[kMaxDim + 2] = dr.lnu;
            reinterpret_cast<int*>(sx + kMaxDim + 3)[0] = dr.wid;
        }
    }
    __syncthreads();
    // ---- thermal states + points: the unit of work is a VIRTUAL WAVE (proposal w, part, v) -- the 64 columns
    // part_col0 + 64 v + lane (+ 256 m) of epochs_loop, exactly what wave v of a k_points workgroup for (w, part) walks, so a
    // transient's chain is bitwise the one every other kernel produces.  The physical waves take the units round-robin,
    // proposal fastest: with up to GROUP non-empty units per (part, v) every wave stays with one proposal.
    {
        const int n_units = GROUP * pb.n_parts * 4;
#pragma unroll 1
        for (int u = wave; u < n_units; u += GROUP) {
            const int w = u % GROUP, pv = u / GROUP, part = pv >> 2, v = pv & 3;
            const double* sc = scratch + w * kPopScratch;
            double ws = 0.;
            const bool empty = part_entry(pb.part_col0, part) + 64 * v >= part_entry(pb.part_col0, part + 1);
            if (!empty && sc[kNCoef] != -INFINITY) {   // (wave-uniform)
                double cs[kNCoef];
#pragma unroll
                for (int k = 0; k < kNCoef; ++k) cs[k] = uniform_f64(sc[k]);
                const double term = epochs_loop<VARIANT, true, false, MODEL>(pb, part, sc + kNCoef + 2, cs, ltab, fdesc, ExpTab{exptab},
                                                               64 * v + lane, itab_at);
                ws = wave_sum(term);
            }
            if (lane == 0) red[(w * kPopMaxParts + part) * 4 + v] = ws;
        }
    }
    // (no barrier here: u = wave (mod GROUP), so a wave has walked the units of ITS proposal only -- the sums it reads
    // below are the ones its own lane 0 wrote, and a wave's LDS operations execute in order)
    if (lane != 0) return;
    // ---- accept / reject and commit (models.py:121-135 -> fitting.py:121-128 -> emcee's stretch move), one lane per proposal
    const double* sc = scratch + wave * kPopScratch;
    const double* sq = sc + kNCoef + 2;
    const double* sx = sq + kMaxDim + (kMaxDim & 1);
    const int wid = reinterpret_cast<const int*>(sx + kMaxDim + 3)[0];
    if (wid < 0) return;
    const double lpr = sc[kNCoef];
    double nlp = -INFINITY;
    if (lpr != -INFINITY) {
        double sum = pb.use_sigma ? 0. : pb.log_norm_const;   // fixed order: parts, each (w0 + w1) + (w2 + w3)
        const double* r = red + wave * kPopMaxParts * 4;
        for (int k = 0; k < pb.n_parts; ++k) sum += (r[4 * k] + r[4 * k + 1]) + (r[4 * k + 2] + r[4 * k + 3]);
        nlp = lpr - 0.5 * sum;
    }
    const double lp_i = sx[kMaxDim];
    const bool ok = (sx[kMaxDim + 1] + nlp - lp_i) > sx[kMaxDim + 2];   // emcee: (ndim - 1) ln z + lp_new - lp_old > ln u
    if (nlp != nlp) atomicOr(sm.err, 1);
    if (ok) {
#pragma unroll
        for (int d = 0; d < kD; ++d)
            if (d < nd) sm.X[(size_t)wid * nd + d] = sq[d];
        sm.LP[wid] = nlp;
        atomicAdd(reinterpret_cast<unsigned long long*>(&sm.nacc[wid]), 1ull);  // (no return value: nothing waits)
    }
    if (sm.store_chain) {
        const long long row = rel / 2;
        double* crow = sm.chain + ((size_t)row * sm.n_walkers + wid) * nd;
#pragma unroll
        for (int d = 0; d < kD; ++d)
            if (d < nd) crow[d] = ok ? sq[d] : sx[d];
        sm.chain_lp[(size_t)row * sm.n_walkers + wid] = ok ? nlp : lp_i;
    }
}

// What one lane of a wave wrote to LDS, read by the wave's other lanes WITHOUT a workgroup barrier in between: the hardware
// executes a wave's LDS operations in order, but the compiler sees one thread -- it may move a load of sc[k] in front of
// `if (lane == 0) sc[k] = ...` for the lanes that do not store.  A fence at wavefront scope costs no instruction and keeps
// the order of the program.
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- population mode with RESIDENT workgroups ------------------------------------------------------------------------
// k_pop's half-step in a loop over up to kRunSpanSolo half-steps, as k_solo_run is k_solo's: gridDim.y = transient,
// gridDim.x = the workgroups that stay for it (what the device holds, shared evenly); workgroup b takes the groups
// b, b + gridDim.x, ... of GROUP proposals of every half-step.  What a half-step needs from an earlier one comes from the
// transient's own board of tagged rows (the sampler's k_solo_run board): a wave's head polls the rows its draw record
// names, its commit posts the walker's new row.  No kernel boundary, the tables staged ONCE per launch -- and with them
// the interpolants, which a launch per half-step reads from L2 point by point because staging 24 KiB more per workgroup
// and half-step costs more than it saves.  A wave walks the units of ITS proposal only (u = wave mod GROUP), so beyond the
// staging there is no barrier at all.  Same arithmetic, same reduction tree: the chains are bitwise k_pop's.
constexpr int pop_run_waves(int group) { return group == 12 ? 6 : group == 10 ? 5 : 4; }   // waves per SIMD the build aims at
template <int ND, int VARIANT, int GROUP, int MODEL = 0>
__global__ __launch_bounds__(64 * GROUP, pop_run_waves(GROUP))
void k_pop_run(const MultiItem* __restrict__ items, long long rel0, int n_hs, long long state_from, int store_chain, int launch_no,
               int n_wg) {
    // (n_wg = gridDim.x, except in the test of a launch whose workgroups are not all there: LCF_RUN_TEST_MISSING)
    extern __shared__ __align__(16) unsigned char smem[];
    typedef const MultiItem __attribute__((address_space(4)))* ItemPtr;
    const ItemPtr itp = (ItemPtr)(items + blockIdx.y);
    const MultiItem& it = *(const MultiItem*)itp;
    const DevProblem& pb = it.pb;
    const DevSampler& sm = it.sm;
    constexpr int kThreads = 64 * GROUP;
    const int nh = sm.n_half;
    double* exptab = reinterpret_cast<double*>(smem);
    double2* ltab = reinterpret_cast<double2*>(smem + kLdsHead * sizeof(double));
    const FiltDesc* fdesc = reinterpret_cast<const FiltDesc*>(ltab + pb.n_lds_tab);
    const int itab_at = pb.n_itab_lds > 0
                            ? (int)(kLdsHead * sizeof(double) + (pb.n_lds_tab + kFdD2 * pb.n_filters) * sizeof(double2)) : -1;
    double* scratch = reinterpret_cast<double*>(ltab + pb.stage_d2);       // [GROUP][kPopScratch]
    double* red = scratch + GROUP * kPopScratch;                             // [GROUP][4 * kPopMaxParts] wave sums
    constexpr int kD = ND > 0 ? ND : kMaxDim;
    const int nd = ND > 0 ? ND : sm.n_dim;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long g_run0 = it.g_run0;
    const unsigned int arrive_goal = it.arrive0 + (unsigned int)(launch_no + 1) * (unsigned int)n_wg;
    const bool flip = it.flip != 0;
    if (tid == 0) __hip_atomic_fetch_add(board_arrivals(sm), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (rel0 == 0) {   // the transient's start state as version g_run0 of every row (whoever needs one polls for it)
        const int col = tid & 31;
        const double* X = flip ? sm.X_out : sm.X;
        const double* LP = flip ? sm.LP_out : sm.LP;
        const long long* nacc = flip ? sm.nacc_out : sm.nacc;
        for (int w = blockIdx.x * (kThreads / 32) + tid / 32; w < sm.n_walkers; w += n_wg * (kThreads / 32))
            if (col <= nd + 1) {
                const double v = col < nd ? X[(size_t)w * nd + col] : col == nd ? LP[w] : (double)nacc[w];
                board_post<true>(sm.board, sm, (unsigned int)g_run0, w, col, v);
            }
    }
    stage_tables<VARIANT, true>(pb, exptab, ltab, 0., tid, kThreads);
    if (it.itab_extra > 0) {   // the interpolants behind the image (DevProblem::n_itab_lds of this copy says they are there)
        double2* dst = reinterpret_cast<double2*>(smem + itab_at);
        const double2* src = reinterpret_cast<const double2*>(pb.itab);
        for (int k = tid; k < it.itab_extra / 2; k += kThreads) dst[k] = src[k];
    }
    __syncthreads();
    double* sc = scratch + wave * kPopScratch;
    double* sq = sc + kNCoef + 2;
    double* sx = sq + kMaxDim + (kMaxDim & 1);
    const int n_groups = (nh + GROUP - 1) / GROUP;
#pragma unroll 1
    for (int h = 0; h < n_hs; ++h) {
        const long long rel = rel0 + h, G = g_run0 + rel;
        const DrawRec* draws = item_rows(it, rel);
#pragma unroll 1
        for (int grp = blockIdx.x; grp < n_groups; grp += n_wg) {
            const int slot = grp * GROUP + wave;
            DrawRec dr{-1, -1, -1, -1, 1., 0., 0., 0, 0};
            if (slot < nh) dr = draws[slot];     // wave-uniform
            if (dr.wid < 0) continue;            // (an odd ensemble's smaller colour leaves its last slot empty)
            {
                // (the head is a latency chain that the proposal's points wait for; the waves it shares the SIMD with are
                // mostly in their points: 22.73 -> 21.97 us per half-step at configs[4])
                __builtin_amdgcn_s_setprio(2);
                HeadRows<ND> rows;
                head_fetch<ND, 2>(pb, sm, dr, lane, rows, G, g_run0, arrive_goal);
                proposal_head<ND, 2, MODEL>(pb, sm, dr, lane, sc, sq, sx, rows);
                __builtin_amdgcn_s_setprio(0);
                // (Measured and dropped: the rows of the wave's NEXT proposal requested here and looked at when its head
                // starts -- 23.6 against 21.9 us per half-step: loads return in order, so the first loads of the points
                // wait for that round trip past the caches, and the request costs registers.)
            }
            wave_lds_order();   // (lane 0 wrote coefficients, log-prior, proposal and row; every lane reads them)
            // ---- the units of this wave's proposal: (part, v) = the 64 columns part_col0 + 64 v + lane, as in k_pop
            const double lpr = sc[kNCoef];
            if (lpr != -INFINITY) {
                double cs[kNCoef];
#pragma unroll
                for (int k = 0; k < kNCoef; ++k) cs[k] = uniform_f64(sc[k]);
#pragma unroll 1
                for (int pv = 0; pv < pb.n_parts * 4; ++pv) {
                    const int part = pv >> 2, v = pv & 3;
                    double ws = 0.;
                    const bool empty = part_entry(pb.part_col0, part) + 64 * v >= part_entry(pb.part_col0, part + 1);
                    if (!empty) {
                        const double term = epochs_loop<VARIANT, true, false, MODEL>(pb, part, sq, cs, ltab, fdesc, ExpTab{exptab},
                                                                                     64 * v + lane, itab_at);
                        ws = wave_sum(term);
                    }
                    if (lane == 0) red[(wave * kPopMaxParts + part) * 4 + v] = ws;
                }
            }
            // ---- accept / reject; lanes 0 .. nd+1 post the walker's row (position, log-posterior, acceptance count)
            wave_lds_order();   // (lane 0 wrote the sums)
            __builtin_amdgcn_s_setprio(3);   // (the row's readers wait for this: 23.05 -> 22.70 us per half-step at configs[4])
            double nlp = -INFINITY;
            if (lpr != -INFINITY) {
                double sum = pb.use_sigma ? 0. : pb.log_norm_const;   // fixed order: parts, each (w0 + w1) + (w2 + w3)
                const double* r = red + wave * kPopMaxParts * 4;
                for (int k = 0; k < pb.n_parts; ++k) sum += (r[4 * k] + r[4 * k + 1]) + (r[4 * k + 2] + r[4 * k + 3]);
                nlp = lpr - 0.5 * sum;
            }
            const double lp_i = sx[kMaxDim];
            const bool ok = (dr.zl + nlp - lp_i) > dr.lnu;   // emcee: (ndim - 1) ln z + lp_new - lp_old > ln u
            const double count = sx[kMaxDim + 1] + (ok ? 1. : 0.);
            if (lane <= nd + 1) {
                double qv = 0., xv = 0.;
#pragma unroll
                for (int d = 0; d < kD; ++d)
                    if (lane == d && d < nd) {
                        qv = sq[d];
                        xv = sx[d];
                    }
                const double v = lane < nd ? (ok ? qv : xv) : lane == nd ? (ok ? nlp : lp_i) : count;
                board_post<true>(sm.board, sm, (unsigned int)(G + 1), dr.wid, lane, v);
                if (rel >= state_from) {   // the run's last step: the state, into the set of buffers the run did not start from
                    double* X = flip ? sm.X : sm.X_out;
                    double* LP = flip ? sm.LP : sm.LP_out;
                    long long* nacc = flip ? sm.nacc : sm.nacc_out;
                    if (lane < nd) X[(size_t)dr.wid * nd + lane] = v;
                    else if (lane == nd) LP[dr.wid] = v;
                    else nacc[dr.wid] = (long long)v;
                }
                if (store_chain) {
                    const long long row = rel / 2;
                    if (lane < nd) sm.chain[((size_t)row * sm.n_walkers + dr.wid) * nd + lane] = v;
                    else if (lane == nd) sm.chain_lp[(size_t)row * sm.n_walkers + dr.wid] = v;
                }
            }
            if (lane == 0 && nlp != nlp) atomicOr(sm.err, 1);
            __builtin_amdgcn_s_setprio(0);
            wave_lds_order();   // (the next proposal's head overwrites what the lanes have just read)
        }
    }
}

}  // namespace

// =================================================================================================================
// host side
// =================================================================================================================
namespace lcf {
thread_local std::string g_err;
lcf_status fail(lcf_status st, const std::string& msg) {
    g_err = msg;
    return st;
}
}  // namespace lcf

// `dp` into its image in device memory: by a kernel on the engine's stream (see k_put_image), complete on return.
lcf_status lcf_engine::sync_dp() {
    if (!d_dp) {
        LCF_HIP(hipMalloc((void**)&d_dp, sizeof(DevProblem)));
        owned.push_back(d_dp);
    }
    LCF_HIP(hipDeviceSynchronize());   // (nothing in flight reads the old image)
    hipLaunchKernelGGL(k_put_image<DevProblem>, dim3(1), dim3(64), 0, stream, d_dp, dp);
    LCF_HIP(hipGetLastError());
    LCF_HIP(hipStreamSynchronize(stream));
    return LCF_OK;
}

namespace {

// ---- the instantiation table: which kernels exist ---------------------------------------------------------------------
// A launch site -- for k_solo and k_solo_run the plan of a run, once per run: take_solo(), take_run() -- takes its family's
// instantiation for the fit dimension through dispatch(); a dimension outside the family's list takes the generic
// kernel, ND = 0 (the dimension at run time).  Models with kernels of their own take them through dispatch_model() at
// their own dimension, resident runs with rows of their own through dispatch_row().  Every instantiation costs compile time.
template <int... V> struct Dims {};
template <int M, int ND> struct Model {};              // model M's own kernels, at fit dimension ND
template <class... S> struct Models {};
template <int ND, int NP, int M> struct RunRow {};     // k_solo_run<ND, 1, true, NP, M, ...>
template <class... R> struct RunRows {};
// (k_solo, k_solo_run and k_pop; 0 = none, the generic kernel)
using SpecialisedModels = Models<Model<kShockCooling, 5>, Model<kShockCooling2, 4>>;
#ifndef LCF_DEV_BUILD
using StepDims = Dims<2, 3, 4, 5, 6, 7, 8, 9>;   // k_step: the fit dimensions of the supported models (+ sigma)
using SoloDims = Dims<4, 5, 6, 7, 8, 9>;         // k_fused, k_solo, k_solo_run
using PopDims = Dims<4, 5, 6, 8>;                // k_pop, k_step_multi
using PopRunModels = SpecialisedModels;          // k_pop_run (otherwise generic only)
// k_solo_run between ranks (RANKS), row by row: the benchmark shapes' own kernels and the companion fit's dimension;
// everything else takes the generic kernel
using RanksRuns = RunRows<RunRow<5, 2, kShockCooling>, RunRow<4, 2, kShockCooling2>, RunRow<8, 2, 0>, RunRow<8, 8, 0>,
                          RunRow<8, 4, 0>>;
#else   // the device-only compile of the ISA report: the benchmarks' dimensions, the counted kernels
using StepDims = Dims<5, 8>;
using SoloDims = Dims<5, 8>;
using PopDims = Dims<5, 8>;
using PopRunModels = Models<Model<kShockCooling, 5>>;
using RanksRuns = RunRows<RunRow<5, 2, kShockCooling>>;
#endif
using WideRuns = RunRows<RunRow<8, 8, 0>>;   // k_solo_run of 1024 threads on one GPU: the eight-parameter models

template <int V> using Int = std::integral_constant<int, V>;

// f(Int<V>) for the entry V of the list equal to v; f(Int<OTHER>) when there is none.
template <int OTHER = 0, int... V, class F>
void dispatch(Dims<V...>, int v, F&& f) {
    if (!((v == V && (f(Int<V>{}), true)) || ...)) f(Int<OTHER>{});
}

// f(Int<ND>, Int<M>) for the entry of the list with M = spec and ND = n_dim; false when there is none.
template <int... M, int... ND, class F>
bool dispatch_model(Models<Model<M, ND>...>, int n_dim, int spec, F&& f) {
    return ((n_dim == ND && spec == M && (f(Int<ND>{}, Int<M>{}), true)) || ...);
}

// f(Int<ND>, Int<NP>, Int<M>) for the row (n_dim, np, spec) of the list; false when there is none.
template <int... ND, int... NP, int... M, class F>
bool dispatch_row(RunRows<RunRow<ND, NP, M>...>, int n_dim, int np, int spec, F&& f) {
    return ((n_dim == ND && np == NP && spec == M && (f(Int<ND>{}, Int<NP>{}, Int<M>{}), true)) || ...);
}

template <int... ND, int... NP, int... M>
constexpr bool has_dim(RunRows<RunRow<ND, NP, M>...>, int n_dim) {
    return ((n_dim == ND) || ...);
}

template <int... M, int... ND>
constexpr int table_model(Models<Model<M, ND>...>, int model, int n_dim) {
    return ((model == M && n_dim == ND ? M : 0) + ...);
}

template <int VARIANT, int MODE>
void launch_points_v(const DevProblem& pb, dim3 grid, size_t lds, hipStream_t st, int w_lo, int n, const double* dP,
                     const double* coef, const double* lprior, const double2* therm, double* out0, double* out1) {
    const auto go = [&](auto kernel) {
        prepare_kernel(kernel, lds);
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, st, pb, w_lo, n, dP, coef, lprior, therm, out0, out1);
    };
    if (pb.tab_in_lds)
        pb.use_therm ? go(k_points<VARIANT, MODE, true, true>) : go(k_points<VARIANT, MODE, true, false>);
    else
        pb.use_therm ? go(k_points<VARIANT, MODE, false, true>) : go(k_points<VARIANT, MODE, false, false>);
}

// Launches the per-point kernel for walkers [w_lo, w_lo + n) (absolute indices into P / coef / lprior / therm).
template <int MODE>
void launch_points(const lcf_engine* e, int w_lo, int n, const double* dP, const double* coef, const double* lprior,
                   double2* therm, double* out0, double* out1, hipStream_t st, bool do_thermal = true) {
    const DevProblem& pb = e->dp;
    if (pb.use_therm && do_thermal && MODE == 1) {   // (the likelihood's lanes compute their own: epochs_loop)
        const long long total = (long long)n * pb.n_epochs;
        hipLaunchKernelGGL(k_thermal, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, pb, w_lo, n,
                           coef, lprior, MODE == 0 ? 1 : 0, therm, (MODE != 2 && pb.variant != 0 && pb.use_itab) ? 1 : 0);
    }
    const dim3 grid((unsigned)((size_t)n * pb.n_parts));
    if (pb.variant == 0)
        launch_points_v<0, MODE>(pb, grid, e->lds_bytes, st, w_lo, n, dP, coef, lprior, therm, out0, out1);
    else
        launch_points_v<1, MODE>(pb, grid, e->lds_bytes, st, w_lo, n, dP, coef, lprior, therm, out0, out1);
}

}  // namespace

namespace lcf {
// log-likelihood / log-posterior of n walkers, device pointers, enqueue only.
lcf_status logprob_dev(lcf_engine* e, int64_t n, const double* dP, double* dout, hipStream_t st, int with_prior) {
    if (n == 0) return LCF_OK;
    const bool custom = e->dp.model == LCF_MODEL_CUSTOM;   // the attached program's kernel between the same two launches
    if (custom)
        if (lcf_status s = custom_ready(e)) return s;
    const bool central = is_central(e->dp.model);           // k_central_points (lcf_central.hip), likewise
    const int bs = 128;
    hipLaunchKernelGGL(k_prepare, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, st, e->dp, (int)n, dP, e->wcoef,
                       e->wlprior, with_prior);
    if (e->tpl) return template_loglike(e, n, dP, dout, st);   // (a second component: model values, then k_template)
    if (custom) {
        if (lcf_status s = custom_launch(e, 0, 0, (int)n, dP, e->wlprior, e->wpart, nullptr, st)) return s;
    } else if (central) {
        if (lcf_status s = central_launch(e, 0, 0, (int)n, dP, e->wlprior, e->wpart, st)) return s;
    } else {
        launch_points<0>(e, 0, (int)n, dP, e->wcoef, e->wlprior, e->wtherm, e->wpart, nullptr, st);
    }
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, st, e->dp, (int)n, e->wpart,
                       e->wlprior, dout);
    LCF_HIP(hipGetLastError());
    if (e->lim_at) return limits_add(e, n, dP, dout, st);   // (upper limits: the censored terms, lcf_limits.hip)
    return LCF_OK;
}

lcf_status limits_model(lcf_engine* e, int64_t n, int64_t lo, int64_t m, const double* dP, bool prepare, hipStream_t st) {
    lcf_engine* at = e->lim_at;
    if (at->dp.model == LCF_MODEL_CUSTOM)
        if (lcf_status s = custom_ready(at)) return s;
    // The rows' coefficients are a function of the model, its constants and the row (walker_coefficients), all of which
    // the two engines share: the limit engine's launches read the ones this engine's k_prepare wrote.
    if (prepare) {
        const int bs = 128;
        hipLaunchKernelGGL(k_prepare, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, st, e->dp, (int)n, dP, e->wcoef,
                           e->wlprior, 0);
    }
    if (at->dp.model == LCF_MODEL_CUSTOM) {
        if (lcf_status s = custom_launch(at, 1, (int)lo, (int)m, dP, e->wlprior, e->lim_m, nullptr, st)) return s;
    } else {
        launch_points<1>(at, (int)lo, (int)m, dP, e->wcoef, e->wlprior, at->wtherm, e->lim_m, nullptr, st);
    }
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

lcf_status prepare_rows(lcf_engine* e, int64_t n, const double* dP, hipStream_t st) {
    const int bs = 128;
    hipLaunchKernelGGL(k_prepare, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, st, e->dp, (int)n, dP, e->wcoef,
                       e->wlprior, 0);
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

lcf_status template_model(lcf_engine* e, int64_t lo, int64_t m, const double* dP, double* out, hipStream_t st) {
    if (e->dp.model == LCF_MODEL_CUSTOM) {
        if (lcf_status s = custom_launch(e, 1, (int)lo, (int)m, dP, e->wlprior, out, nullptr, st)) return s;
    } else {
        launch_points<1>(e, (int)lo, (int)m, dP, e->wcoef, e->wlprior, e->wtherm, out, nullptr, st);
    }
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}
}  // namespace lcf

namespace {

lcf_status logprob_host(lcf_engine* e, int64_t n, const double* P, double* out, int with_prior) {
    if (!e || n < 0 || (n > 0 && (!P || !out))) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return LCF_OK;
    if (n > (1 << 22)) return fail(LCF_ERR_INVALID_ARGUMENT, "at most 2^22 walkers per call");
    LCF_HIP(hipSetDevice(e->device));
    if (lcf_status st = e->reserve(n)) return st;
    LCF_HIP(hipMemcpyAsync(e->wP, P, n * e->dp.n_dim * sizeof(double), hipMemcpyHostToDevice, e->stream));
    if (lcf_status st = logprob_dev(e, n, e->wP, e->wout, e->stream, with_prior)) return st;
    LCF_HIP(hipMemcpyAsync(out, e->wout, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    LCF_HIP(hipStreamSynchronize(e->stream));
    return LCF_OK;
}

}  // namespace

extern "C" {

int32_t lcf_abi_version(void) { return LCF_ABI_VERSION; }

const char* lcf_last_error(void) { return lcf::g_err.c_str(); }

int32_t lcf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

lcf_status lcf_log_likelihood(lcf_engine* e, int64_t n, const double* P, double* out) {
    return logprob_host(e, n, P, out, 0);
}
lcf_status lcf_log_posterior(lcf_engine* e, int64_t n, const double* P, double* out) {
    return logprob_host(e, n, P, out, 1);
}
lcf_status lcf_log_likelihood_dev(lcf_engine* e, int64_t n, const double* dP, double* dout, void* stream) {
    if (!e || n < 0 || (n > 0 && (!dP || !dout))) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    LCF_HIP(hipSetDevice(e->device));
    if (lcf_status st = e->reserve(n)) return st;
    return logprob_dev(e, n, dP, dout, stream ? (hipStream_t)stream : e->stream, 0);
}
lcf_status lcf_log_posterior_dev(lcf_engine* e, int64_t n, const double* dP, double* dout, void* stream) {
    if (!e || n < 0 || (n > 0 && (!dP || !dout))) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    LCF_HIP(hipSetDevice(e->device));
    if (lcf_status st = e->reserve(n)) return st;
    return logprob_dev(e, n, dP, dout, stream ? (hipStream_t)stream : e->stream, 1);
}

static lcf_status evaluate_impl(lcf_engine* e, int64_t n, const double* P, double* o0, double* o1, int mode) {
    if (!e || n < 0 || (n > 0 && (!P || !o0 || (mode == 2 && !o1)))) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0 || e->dp.n_points == 0) return LCF_OK;
    const bool custom = e->dp.model == LCF_MODEL_CUSTOM;
    if (custom)
        if (lcf_status st = custom_ready(e)) return st;
    const bool central = is_central(e->dp.model);
    if (central && mode == 2)
        if (lcf_status st = central_refuse(e, "lcf_temperature_radius")) return st;
    LCF_HIP(hipSetDevice(e->device));
    if (lcf_status st = e->reserve(n)) return st;
    const size_t N = e->dp.n_points;
    // bound the device scratch to ~256 MiB per pass
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)((256u << 20) / (N * sizeof(double) * (mode == 2 ? 2 : 1)))));
    if (lcf_status st = e->reserve_big(per * N * sizeof(double) * (mode == 2 ? 2 : 1))) return st;
    LCF_HIP(hipMemcpyAsync(e->wP, P, n * e->dp.n_dim * sizeof(double), hipMemcpyHostToDevice, e->stream));
    const int bs = 128;
    hipLaunchKernelGGL(k_prepare, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, e->stream, e->dp, (int)n, e->wP,
                       e->wcoef, e->wlprior, 0);
    for (int64_t lo = 0; lo < n; lo += per) {
        const int64_t m = std::min(per, n - lo);
        double* b0 = e->wbig;
        double* b1 = e->wbig + per * N;
        if (custom) {
            if (lcf_status st = custom_launch(e, mode, (int)lo, (int)m, e->wP, e->wlprior, b0, mode == 2 ? b1 : nullptr, e->stream))
                return st;
        } else if (central) {
            if (lcf_status st = central_launch(e, 1, (int)lo, (int)m, e->wP, e->wlprior, b0, e->stream)) return st;
        } else if (mode == 1)
            launch_points<1>(e, (int)lo, (int)m, e->wP, e->wcoef, e->wlprior, e->wtherm, b0, nullptr, e->stream);
        else
            launch_points<2>(e, (int)lo, (int)m, e->wP, e->wcoef, e->wlprior, e->wtherm, b0, b1, e->stream);
        LCF_HIP(hipGetLastError());
        LCF_HIP(hipMemcpyAsync(o0 + lo * N, b0, m * N * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        if (mode == 2) LCF_HIP(hipMemcpyAsync(o1 + lo * N, b1, m * N * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        LCF_HIP(hipStreamSynchronize(e->stream));
    }
    return LCF_OK;
}

lcf_status lcf_model_evaluate(lcf_engine* e, int64_t n, const double* P, double* y_fit) {
    if (e && e->tpl) return lcf_template_evaluate(e, n, P, LCF_TEMPLATE_TOTAL, y_fit);   // (both components)
    return evaluate_impl(e, n, P, y_fit, nullptr, 1);
}
lcf_status lcf_temperature_radius(lcf_engine* e, int64_t n, const double* P, double* T_K, double* R_bb) {
    return evaluate_impl(e, n, P, T_K, R_bb, 2);
}

lcf_status lcf_blackbody_to_filters(lcf_engine* e, int64_t m, const int32_t* filt_idx, const double* T, const double* R,
                                    double* out) {
    if (!e || m < 0 || (m > 0 && (!filt_idx || !T || !R || !out))) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (m == 0) return LCF_OK;
    for (int64_t i = 0; i < m; ++i)
        if (filt_idx[i] < 0 || filt_idx[i] >= e->dp.n_filters) return fail(LCF_ERR_INVALID_ARGUMENT, "filt_idx out of range");
    LCF_HIP(hipSetDevice(e->device));
    const size_t bytes = m * (3 * sizeof(double) + sizeof(int));
    if (lcf_status st = e->reserve_big(bytes + 64)) return st;
    double* dT = e->wbig;
    double* dR = dT + m;
    double* dO = dR + m;
    int* dF = reinterpret_cast<int*>(dO + m);
    LCF_HIP(hipMemcpyAsync(dT, T, m * sizeof(double), hipMemcpyHostToDevice, e->stream));
    LCF_HIP(hipMemcpyAsync(dR, R, m * sizeof(double), hipMemcpyHostToDevice, e->stream));
    LCF_HIP(hipMemcpyAsync(dF, filt_idx, m * sizeof(int), hipMemcpyHostToDevice, e->stream));
    const dim3 grid((unsigned)((m + kBlock - 1) / kBlock));
    if (e->dp.variant == 0)
        hipLaunchKernelGGL(k_bb_pointwise<0>, grid, dim3(kBlock), 0, e->stream, e->dp, (int)m, dF, e->d_tab_off, e->d_ctab_off,
                           e->d_ctmin, dT, dR, dO);
    else
        hipLaunchKernelGGL(k_bb_pointwise<1>, grid, dim3(kBlock), 0, e->stream, e->dp, (int)m, dF, e->d_tab_off, e->d_ctab_off,
                           e->d_ctmin, dT, dR, dO);
    LCF_HIP(hipGetLastError());
    LCF_HIP(hipMemcpyAsync(out, dO, m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    LCF_HIP(hipStreamSynchronize(e->stream));
    return LCF_OK;
}

}  // extern "C"

extern "C" lcf_status lcf_profile_loglike_kernel(lcf_engine* e, int64_t n, const double* P, int32_t reps,
                                                 double* avg_ms) {
    if (!e || n <= 0 || !P || reps <= 0 || !avg_ms) return fail(LCF_ERR_INVALID_ARGUMENT, "bad argument");
    if (lcf_status st = custom_refuse(e, "lcf_profile_loglike_kernel")) return st;
    if (lcf_status st = central_refuse(e, "lcf_profile_loglike_kernel")) return st;
    if (lcf_status st = limits_refuse(e, "lcf_profile_loglike_kernel")) return st;
    if (lcf_status st = template_refuse(e, "lcf_profile_loglike_kernel")) return st;
    LCF_HIP(hipSetDevice(e->device));
    if (lcf_status st = e->reserve(n)) return st;
    LCF_HIP(hipMemcpyAsync(e->wP, P, n * e->dp.n_dim * sizeof(double), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_prepare, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, e->stream, e->dp, (int)n, e->wP,
                       e->wcoef, e->wlprior, 0);
    launch_points<0>(e, 0, (int)n, e->wP, e->wcoef, e->wlprior, e->wtherm, e->wpart, nullptr, e->stream);  // warm-up (+ thermal states)
    hipEvent_t a, b;
    LCF_HIP(hipEventCreate(&a));
    LCF_HIP(hipEventCreate(&b));
    LCF_HIP(hipEventRecord(a, e->stream));
    for (int r = 0; r < reps; ++r)
        launch_points<0>(e, 0, (int)n, e->wP, e->wcoef, e->wlprior, e->wtherm, e->wpart, nullptr, e->stream, false);
    LCF_HIP(hipEventRecord(b, e->stream));
    LCF_HIP(hipStreamSynchronize(e->stream));
    float ms = 0.f;
    LCF_HIP(hipEventElapsedTime(&ms, a, b));
    hipEventDestroy(a);
    hipEventDestroy(b);
    LCF_HIP(hipGetLastError());
    *avg_ms = (double)ms / reps;
    return LCF_OK;
}

// (In namespace lcf: the functions lcf_internal.h declares, which lcf_sampler.hip calls; everything `static` stays
// internal to this file.)
namespace lcf {

// Commit half-step g_next - 1 (if pending) and draw half-step g_next (if have_next); coefficients and log-priors of the
// slots [lo, hi) for the likelihood launch behind it.
lcf_status launch_next(lcf_sampler* s, bool have_next, int lo, int hi, hipStream_t st) {
    lcf_engine* e = s->e;
    const DevSampler& ds = s->ds;
    const long long g = s->g_next;
    const int have_prev = s->pending ? 1 : 0;
    if (!have_prev && !have_next) return LCF_OK;
    const long long prev_row = have_prev ? (g - 1 - s->g_run0) / 2 : 0;
    const long long rel = g - s->g_run0;
    if (st != e->stream) s->foreign_stream = true;
    if (have_next)
        if (lcf_status r = enter_half_step(&s, 1, rel, st)) return r;
    const DrawRec* draws = have_next ? s->rows(rel) : nullptr;
    const DrawRec* prev_draws = have_prev ? s->rows(rel - 1) : nullptr;
    dispatch(StepDims{}, ds.n_dim, [&](auto nd) {
        hipLaunchKernelGGL(k_step<decltype(nd)::value>, dim3((unsigned)ds.n_half), dim3(64), 0, st, e->dp, ds, have_prev, prev_row,
                           have_next ? 1 : 0, draws, prev_draws, g, lo, hi, s->coef, s->lprior);
    });
    LCF_HIP(hipGetLastError());
    if (have_next)
        if (lcf_status r = leave_half_step(&s, 1, st)) return r;
    s->pending = have_next;
    if (have_next) s->g_next = g + 1;
    return LCF_OK;
}

// Log-posteriors of the shard's proposals from their partial sums (sharded runs: the all-gather sends these).
static lcf_status launch_finalize(lcf_sampler* s, int lo, int hi, hipStream_t st) {
    if (hi <= lo) return LCF_OK;
    lcf_engine* e = s->e;
    const int par = (int)((s->g_next - 1) & 1), bs = 128;
    hipLaunchKernelGGL(k_finalize, dim3((hi - lo + bs - 1) / bs), dim3(bs), 0, st, e->dp, hi - lo,
                       s->ds.part2[par] + (size_t)lo * (e->dp.n_parts + 1), s->lprior + lo, s->ds.newlp[par] + lo);
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

// Likelihood of the proposals [lo, hi) of the half-step drawn last; `finalize`: and their log-posteriors.
lcf_status launch_eval(lcf_sampler* s, int lo, int hi, bool finalize, hipStream_t st) {
    lcf_engine* e = s->e;
    if (hi <= lo) return LCF_OK;
    double* part = s->ds.part2[(s->g_next - 1) & 1];
    launch_points<0>(e, lo, hi - lo, s->ds.Q[(s->g_next - 1) & 1], s->coef, s->lprior, nullptr, part, nullptr, st);
    LCF_HIP(hipGetLastError());
    return finalize ? launch_finalize(s, lo, hi, st) : LCF_OK;
}

constexpr size_t kLdsPerCU = 160 * 1024;

static size_t fused_lds_bytes(const lcf_engine* e) {
    return e->lds_bytes + kFusedScratch * sizeof(double);
}

// The environment's switches over how a run is executed, as they stand now: read when a run is planned (plan_run,
// population_plan), so a switch holds for the runs planned while it is set.
struct RunSwitches {
    bool no_fused, no_solo, no_specialised, no_wide_solo, no_run_kernel, rows_per_half_step, run_any_size, run_test_missing;
    int run_grid;   // LCF_RUN_GRID (tests): a resident launch has at most so many workgroups
};
static RunSwitches run_switches() {
    const auto set = [](const char* name) { return std::getenv(name) != nullptr; };
    const char* grid = std::getenv("LCF_RUN_GRID");
    return RunSwitches{set("LCF_NO_FUSED"), set("LCF_NO_SOLO"), set("LCF_NO_SPECIALISED"), set("LCF_NO_WIDE_SOLO"),
                       set("LCF_NO_RUN_KERNEL"), set("LCF_ROWS_PER_HALF_STEP"), set("LCF_RUN_ANY_SIZE"),
                       set("LCF_RUN_TEST_MISSING"), grid ? std::atoi(grid) : INT_MAX};
}

static bool fused_eligible(const lcf_sampler* s, const RunSwitches& sw) {
    const lcf_engine* e = s->e;
    return !sw.no_fused && s->half_step_kernel != LCF_HALF_STEP_PHASES && e->dp.tab_in_lds &&
           fused_lds_bytes(e) <= 80 * 1024;  // (two workgroups per CU; measured with 160 KiB allowed: no gain)
}
// (what the sharded, peer-mailbox and per-half-step drivers ask, half-step by half-step)
bool fused_eligible(const lcf_sampler* s) { return fused_eligible(s, run_switches()); }

// One launch for a whole half-step of a single-GPU run: commit half-step g_next - 1 (if pending), draw half-step
// g_next and evaluate its likelihood.
lcf_status launch_fused(lcf_sampler* s, int lo, int hi, hipStream_t st) {
    lcf_engine* e = s->e;
    const DevSampler& ds = s->ds;
    const long long g = s->g_next;
    const int have_prev = s->pending ? 1 : 0;
    const long long prev_row = have_prev ? (g - 1 - s->g_run0) / 2 : 0;
    const long long rel = g - s->g_run0;
    if (st != e->stream) s->foreign_stream = true;
    if (lcf_status r = enter_half_step(&s, 1, rel, st)) return r;
    const DrawRec* draws = s->rows(rel);
    const DrawRec* prev_draws = have_prev ? s->rows(rel - 1) : nullptr;
    const int foreign = ds.n_half - (hi - lo);
    const dim3 grid((unsigned)((size_t)(hi - lo) * e->dp.n_parts + (foreign + kBlock / 64 - 1) / (kBlock / 64)));
    const size_t lds = fused_lds_bytes(e);
    double* lprior = ds.inline_finalize ? nullptr : s->lprior;  // the finalize launch of a sharded run reads it
    const auto go = [&](auto kernel) {
        prepare_kernel(kernel, lds);
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, st, e->dp, ds, have_prev, prev_row, draws, prev_draws, g, lo, hi,
                           lprior);
    };
    const bool v1 = e->dp.variant != 0, therm = e->dp.use_therm;
    dispatch(SoloDims{}, ds.n_dim, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        if (v1) therm ? go(k_fused<ND, 1, true>) : go(k_fused<ND, 1, false>);
        else therm ? go(k_fused<ND, 0, true>) : go(k_fused<ND, 0, false>);
    });
    LCF_HIP(hipGetLastError());
    if (lcf_status r = leave_half_step(&s, 1, st)) return r;
    s->pending = true;
    s->g_next = g + 1;
    return LCF_OK;
}

// ---- one workgroup per proposal (k_solo): single-GPU runs whose parts fit one workgroup -----------------------------
static size_t solo_lds_bytes(const lcf_engine* e) {
    return kLdsHead * sizeof(double) + (size_t)e->dp.stage_d2 * sizeof(double2) +
           (kSoloScratch + 4) * sizeof(double);
}

// ... of a resident launch (k_solo_run): a second copy of the scratch words (the committing wave reads one item's while
// wave 0 writes the next one's), and the block of launch invariants behind them (RunUniforms)
static size_t run_lds_bytes(const lcf_engine* e) {
    return solo_lds_bytes(e) + (kSoloScratch + 4) * sizeof(double) + sizeof(RunUniforms);
}

// The model-specialised kernels (k_solo / k_pop <..., MODEL>) take engines of the shape the benchmarks have: a power-law
// model (ShockCooling, ShockCooling2) without a fitted sigma, dense columns, interpolated band sums proved from their
// first interval.  0: the generic kernel.
static int specialised_model(const DevProblem& dp, const RunSwitches& sw) {
    if (sw.no_specialised || !dp.use_therm || !dp.use_itab || dp.variant == 0 || !dp.em_dense || !dp.itab_uniform || dp.use_sigma)
        return 0;
    return table_model(SpecialisedModels{}, dp.model, dp.n_dim);
}

// ---- the instantiation table, walked: once per run, for its plan (plan_run) ------------------------------------------------
// (Two walks, k_solo's here and k_solo_run's behind the sampler's images below: a kernel's place in the code object is the
// place of its first use in this file, and timings at the 0.3 % level depend on where the resident kernels lie.)
static void took(RunPlan& p, int nd, int np, int m) {
    const int taken[4] = {nd, np, m, p.rows ? 1 : 0};
    std::copy(taken, taken + 4, p.instance);
    p.threads = kBlock * (np == 8 ? 4 : 2);
}

// The plan's instance of k_solo for the fit dimension, NP parts per workgroup and the model's own kernel `spec`.
static void take_solo(RunPlan& p, int n_dim, int np, int spec) {
    const auto go = [&](auto nd, auto np_, auto m) {
        constexpr int ND = decltype(nd)::value, NP = decltype(np_)::value, M = decltype(m)::value;
        p.solo = p.rows ? k_solo<ND, 1, true, NP, true, M> : k_solo<ND, 1, true, NP, false, M>;
        took(p, ND, NP, M);
    };
    dispatch(SoloDims{}, n_dim, [&](auto nd) {
        dispatch<8>(Dims<2, 4>{}, np, [&](auto np_) {
            const auto own = [&](auto snd, auto m) { go(snd, np_, m); };
            if constexpr (decltype(np_)::value == 8) go(nd, np_, Int<0>{});   // (no model has a 1024-thread kernel)
            else if (!dispatch_model(SpecialisedModels{}, nd, spec, own)) go(nd, np_, Int<0>{});
        });
    });
}

// One half-step of a k_solo plan: ONE launch, one workgroup per proposal, accept test and commit included (between
// ranks: of this rank's slots only, rows from / to the row boards).
lcf_status launch_solo(lcf_sampler* s, const RunPlan& plan, long long rel, hipStream_t st) {
    const DevSampler& ds = s->ds;
    if (lcf_status r = enter_half_step(&s, 1, rel, st)) return r;
    const DrawRec* draws = s->rows(rel);
    const bool next_here = rel + 1 < 2 * s->run_steps && s->block_of_step((rel + 1) / 2) == s->blk_current;
    const DrawRec* draws_next = next_here ? draws + ds.n_half : nullptr;
    LCF_HIP(prepare_kernel(plan.solo, plan.lds));
    hipLaunchKernelGGL(plan.solo, dim3((unsigned)(plan.hi - plan.lo)), dim3(plan.threads), plan.lds, st, s->e->d_dp, ds, rel / 2,
                       draws, draws_next, s->g_run0 + rel, s->g_run0, plan.lo);
    LCF_HIP(hipGetLastError());
    return leave_half_step(&s, 1, st);
}

struct RunBusy { hipEvent_t ev = nullptr; hipStream_t stream = nullptr; bool used = false; bool enqueuing = false; };
static RunBusy g_run_busy[64];
static std::mutex g_run_mutex;

// May a one-launch run go on stream `st` of device `dev` now?  Yes unless another stream's is being enqueued (between its
// claim and its release: the device counts as busy from the claim on, not only once the release has recorded the event)
// or still in flight.
bool run_claim(int dev, hipStream_t st) {
    if (dev < 0 || dev >= 64) return false;
    std::lock_guard<std::mutex> lock(g_run_mutex);
    RunBusy& b = g_run_busy[dev];
    if (b.stream != st) {
        if (b.enqueuing) return false;
        if (b.used) {
            // (the event may have been recorded last on a stream that no longer exists -- its engine destroyed: whatever
            // the query then says, nothing is in flight there; and what it says must not stay behind as the "last error")
            const hipError_t q = hipEventQuery(b.ev);
            (void)hipGetLastError();
            if (q == hipErrorNotReady) return false;
        }
    }
    if (!b.ev && hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess) return false;
    b.stream = st;
    b.enqueuing = true;
    return true;
}
void run_release(int dev, hipStream_t st) {   // behind the last launch of the run (or on the way out of a failed enqueue)
    std::lock_guard<std::mutex> lock(g_run_mutex);
    RunBusy& b = g_run_busy[dev];
    b.used = hipEventRecord(b.ev, st) == hipSuccess;
    b.enqueuing = false;
}

// Workgroups of a resident launch, `per_cu` of them per CU: all on the device at once, on the compute units the engine's
// stream may use (a CU mask on the stream -- or on the process -- leaves fewer than the device has), `max_grid` at the most
// (RunSwitches::run_grid).
static int run_capacity(const lcf_engine* e, int per_cu, int max_grid) {
    int cus = e->n_cus;
    uint32_t mask[16] = {0};
    if (hipExtStreamGetCUMask(e->stream, 16, mask) == hipSuccess) {
        int bits = 0;
        for (uint32_t m : mask) bits += __builtin_popcount(m);
        if (bits > 0 && bits < cus) cus = bits;
    }
    (void)hipGetLastError();
    return std::min(per_cu * cus, max_grid);
}

// What a resident plan asks of the device, once per run and ahead of its launches: the kernel's LDS attribute and how many
// of its workgroups the device holds at once.  (What a process pays ONCE per kernel: lcf_sampler_board_connect does it
// ahead of the first run, so that no rank's first launch makes such calls while another rank's resident workgroups
// already wait for it.)
lcf_status prepare_run(const lcf_engine* e, RunPlan& plan) {
    int per_cu = 0;
    if (hipError_t err = prepare_kernel(plan.run, plan.lds, plan.threads, &per_cu))
        return fail(LCF_ERR_HIP, std::string("preparing k_solo_run: ") + hipGetErrorString(err));
    plan.cap = run_capacity(e, per_cu, plan.max_grid);
    if (plan.cap < 1) return fail(LCF_ERR_UNSUPPORTED, "k_solo_run does not fit the device");
    return LCF_OK;
}

// The sampler as k_solo_run reads it, in device memory (a constant-address-space pointer in the kernel): written when a
// sampler's first one-launch run is enqueued and again only when something in it has changed (a longer chain).  The
// two sets of state buffers keep their places in it -- X / LP / nacc = the set the sampler was created with -- and the
// launch's flags say which of them holds the run's start state.
static DevSampler run_struct(const lcf_sampler* s) {
    DevSampler rs = s->ds;
    const bool flip = s->run_flip;
    rs.X = flip ? s->alt_X : s->ds.X;
    rs.LP = flip ? s->alt_LP : s->ds.LP;
    rs.nacc = flip ? s->alt_nacc : s->ds.nacc;
    rs.X_out = flip ? s->ds.X : s->alt_X;
    rs.LP_out = flip ? s->ds.LP : s->alt_LP;
    rs.nacc_out = flip ? s->ds.nacc : s->alt_nacc;
    rs.store_chain = rs.inline_finalize = rs.n_peers = 0;   // (per run: in the flags, or not read by this kernel)
    rs.board = static_cast<unsigned long long*>(s->run_board_mem);
    rs.peer_board[0] = rs.board;
    rs.n_board_ranks = 1;
    rs.board_rank = 0;
    rs.ring = kRunRing;
    rs.snap_out = reinterpret_cast<unsigned long long*>(s->snap);
    rs.snap_flags = s->snap_flags();
    return rs;
}

// The buffers a sampler's resident launches need beside its own: the board of tagged rows and the second set of state.
lcf_status run_buffers(lcf_sampler* s) {
    if (s->run_board_mem) return LCF_OK;
    if (lcf_status r = polled_alloc(s->e->device, false, s->run_board_bytes(), &s->run_board_mem)) return r;
    const size_t nw = s->ds.n_walkers;
    if (lcf_status r = dalloc(&s->alt_X, nw * s->ds.n_dim, s->owned)) return r;
    if (lcf_status r = dalloc(&s->alt_LP, nw, s->owned)) return r;
    return dalloc(&s->alt_nacc, nw, s->owned);
}

// An image of the sampler in device memory (lcf_sampler::Image): allocated when first asked for, and rewritten when `rs`,
// what a launch is about to read there, is not what was written last.  `rs` null: allocated only.
static lcf_status put_image(lcf_sampler* s, lcf_sampler::Image& im, const DevSampler* rs, hipStream_t st) {
    if (!im.dev) {
        LCF_HIP(hipMalloc((void**)&im.dev, sizeof(DevSampler)));
        s->owned.push_back(im.dev);
        im.valid = false;
    }
    if (rs && (!im.valid || std::memcmp(rs, &im.host, sizeof *rs) != 0)) {
        // (by a kernel, in stream order behind the launches that read the old image: k_put_image)
        hipLaunchKernelGGL(k_put_image<DevSampler>, dim3(1), dim3(64), 0, st, im.dev, *rs);
        LCF_HIP(hipGetLastError());
        std::memcpy(&im.host, rs, sizeof *rs);
        im.valid = true;
    }
    return LCF_OK;
}

// The image k_solo_run reads (run_struct), and the launch's flags.
static lcf_status run_image(lcf_sampler* s, hipStream_t st, const DevSampler** out, int* flags) {
    const DevSampler rs = run_struct(s);
    if (lcf_status r = put_image(s, s->run_image, &rs, st)) return r;
    *out = s->run_image.dev;
    *flags = (s->ds.store_chain ? kRunStoreChain : 0) | (s->run_flip ? kRunFlip : 0);
    return LCF_OK;
}

// The same for a rank of a row-board run (k_solo_run<..., RANKS>): the rank's own board and its peers', no second set of
// state buffers (state and chain are collected from the board), no snapshot words.
static lcf_status rows_image(lcf_sampler* s, hipStream_t st, const DevSampler** out) {
    DevSampler rs = s->ds;
    rs.store_chain = rs.inline_finalize = rs.n_peers = 0;
    rs.X_out = nullptr;
    rs.LP_out = nullptr;
    rs.nacc_out = nullptr;
    rs.snap_out = nullptr;
    rs.snap_flags = nullptr;
    if (lcf_status r = put_image(s, s->rows_image, &rs, st)) return r;
    *out = s->rows_image.dev;
    return LCF_OK;
}

// ... and its instance of k_solo_run: row by row where the family is listed so (between ranks; the wide size on one GPU),
// else as k_solo's.  (NP = 8 where the table has a row for it, else the 512-thread form.)
static void take_run(RunPlan& p, int n_dim, int np, int spec) {
    const auto go = [&](auto nd, auto np_, auto m, auto ranks) {
        p.run = k_solo_run<decltype(nd)::value, 1, true, decltype(np_)::value, decltype(m)::value, decltype(ranks)::value>;
        took(p, nd, np_, m);
    };
    if (p.rows) {
        const auto row = [&](auto nd, auto np_, auto m) { go(nd, np_, m, std::true_type{}); };
        if (!dispatch_row(RanksRuns{}, n_dim, np, spec, row))
            dispatch<4>(Dims<2>{}, np, [&](auto np_) { go(Int<0>{}, np_, Int<0>{}, std::true_type{}); });
    } else {
        const auto row = [&](auto nd, auto np_, auto m) { go(nd, np_, m, std::false_type{}); };
        if (!dispatch_row(WideRuns{}, n_dim, np, spec, row))
            dispatch(SoloDims{}, n_dim, [&](auto nd) {
                dispatch<4>(Dims<2>{}, np, [&](auto np_) {
                    const auto own = [&](auto snd, auto m) { go(snd, np_, m, std::false_type{}); };
                    if (!dispatch_model(SpecialisedModels{}, nd, spec, own)) go(nd, np_, Int<0>{}, std::false_type{});
                });
            });
    }
}

// ---- the plan of a run: which kernel, which instance of it ---------------------------------------------------------------
// The forms, first that applies: a block of half-steps in ONE launch of resident workgroups (k_solo_run), ONE launch per
// half-step with a workgroup per proposal (k_solo), ONE launch per half-step with a workgroup per part (k_fused), separate
// launches.  A resident launch's workgroups wait for each other's rows, so they must all be on the device at once: the
// grid is what the device holds (occupancy x CUs; each workgroup then takes several slots of a half-step), and a process
// keeps ONE such launch in flight per device (`g_run_busy`): a second sampler's run enqueued meanwhile on another stream
// takes a launch per half-step.
// (proposals with a resident workgroup of their own: 2 workgroups of 512 threads per CU of an MI355X)
constexpr int kRunSlots = 512;

// The plan of a run of `s`: of one GPU (all slots of a half-step, [lo, hi) = [0, n_half)) or, `rows`, of the rank's slots
// [lo, hi) of a row-board run.  `resident`: resident workgroups may be taken (the run has steps; the device is free).
// Nothing is asked of the device and nothing in `s` changes.
RunPlan plan_run(const lcf_sampler* s, bool rows, int lo, int hi, bool resident) {
    const RunSwitches sw = run_switches();
    const lcf_engine* e = s->e;
    const DevProblem& dp = e->dp;
    const int choice = s->half_step_kernel, n_dim = s->ds.n_dim, width = hi - lo;
    RunPlan p{rows, lo, hi};
    // 1. One workgroup per proposal?  Not the libm band sum (variant 0 exists to mirror the reference instruction for
    // instruction: it keeps k_fused), and not light curves without shared epochs (thermal state per point, inside the
    // point loop: the serial head's registers on top of the point loop's do not fit 128 without spilling).
    // (LCF_NO_FUSED=1 asks for the separate launches: neither one-launch form then, as set_half_step_kernel('phases'))
    const bool one_wg = !sw.no_solo && !sw.no_fused && (choice == LCF_HALF_STEP_AUTO || choice == LCF_HALF_STEP_SOLO) &&
                        dp.variant != 0 && dp.use_therm && dp.tab_in_lds && dp.n_parts <= kMaxParts &&
                        solo_lds_bytes(e) <= kLdsPerCU;
    if (!one_wg) {
        p.form = fused_eligible(s, sw) ? LCF_KERNEL_FUSED : LCF_KERNEL_PHASES;
        return p;
    }
    // 2. The model's own kernel
    const int spec = specialised_model(dp, sw);
    // 3. Resident?  Launches of at most one workgroup per CU of light curves with more than two parts (a rank's share of a
    // strongly scaled ensemble: configs[2] on 8 GPUs, 256 proposals) have a size of their own, the wide size: resident
    // for the eight-parameter models (the instantiation that exists).
    const bool wide_size = dp.n_parts > 2 && width <= e->n_cus && has_dim(WideRuns{}, n_dim);
    // With several proposals per workgroup and half-step the fixed share of each workgroup competes with the hardware's
    // dispatch of one workgroup per proposal, where a proposal that the prior excludes costs nothing.  Light curves of at
    // most two parts share a workgroup with up to three others: measured per half-step, k_solo_run against k_solo,
    // configs[1]'s light curve with 512 / 1024 / 2048 / 4096 walkers 4.9 / 6.0 / 11.8 / 22.7 against 6.1 / 7.8 / 13.5 /
    // 23.6 us; configs[2] (four parts, 2048 proposals) 80.7 against 76.9 us -- the boundary it saves is 2 % of that launch.
    // Light curves of more than two parts gain little (3000 observations at times of their own, 8 parts, 1024 walkers: 21.8
    // against 23.0 us) and lose below a few hundred proposals (100 walkers: 15.2 against 13.0 us -- the rows' way through the
    // board costs more than the boundary of so small a launch; configs[2]'s light curve with 512 walkers: 14.1 against the
    // 12.8 us of the 1024-thread workgroups that k_solo uses for launches of at most one workgroup per CU): they take it
    // above one proposal per CU, up to 512.  Between ranks up to TWO slots per workgroup -- a rank of a 2-GPU run of
    // configs[2] has 1024 proposals: 36.1 us per half-step resident against 39.8 with a launch per half-step, whose row
    // collection comes per half-step as well; on one GPU the two forms are level at that size, 36.6 / 36.5, and the
    // hardware's dispatch of a workgroup per proposal wins beyond it.
    const bool size = dp.n_parts <= 2 ? width <= 4 * kRunSlots
                                      : (width > e->n_cus || wide_size) && width <= (rows ? 2 : 1) * kRunSlots;
    // (LCF_RUN_ANY_SIZE, tests: several slots per workgroup at any size; LCF_ROWS_PER_HALF_STEP=1: never between ranks; a
    // sampler whose resident launch gave up once, run_off, or whose rows travel through peer mailboxes: never on one GPU)
    const bool may_stay = choice == LCF_HALF_STEP_AUTO && !sw.no_run_kernel && run_lds_bytes(e) <= kLdsPerCU &&
                          (size || sw.run_any_size) && (rows ? !sw.rows_per_half_step : !s->run_off && s->ds.n_peers == 0);
    const bool stay = resident && may_stay;
    // (every form but k_solo reads the slots; and so that the records a run leaves for the next one serve it either way,
    // so does k_solo where the sampler's runs are resident whenever they may be)
    p.need_slots = rows || may_stay;
    // 4. Parts per workgroup, NP.  Workgroups of 512 threads: one part per 256 threads (up to two parts) or two (three or
    // four); or all four parts of a proposal side by side, 1024 threads, NP = 8, where the launch has at most one
    // workgroup per CU (resident: at the wide size; LCF_NO_WIDE_SOLO=1: the same launches at 512 threads).
    const bool wide = !sw.no_wide_solo && (stay ? wide_size : dp.n_parts > 2 && width <= e->n_cus);
    const int np = dp.n_parts <= 2 ? 2 : wide ? 8 : 4;
    // 5. The row of the instantiation table
    p.form = stay ? LCF_KERNEL_RUN : LCF_KERNEL_SOLO;
    p.lds = stay ? run_lds_bytes(e) : solo_lds_bytes(e);
    if (!stay) {
        take_solo(p, n_dim, np, spec);
        return p;
    }
    p.span = rows ? kRunSpan : kRunSpanSolo;
    p.max_grid = sw.run_grid;
    p.test_missing = sw.run_test_missing;
    take_run(p, n_dim, np, spec);
    return p;
}

// Half-steps [rel, rel + n_hs) of a resident plan that prepare_run has seen, all inside the current block of draw records.
// `need_progress`: see k_solo_run<..., RANKS> (0 on one GPU).
lcf_status launch_run(lcf_sampler* s, const RunPlan& plan, long long rel, int n_hs, hipStream_t st, long long need_progress) {
    const DevSampler* rs = nullptr;
    int run_flags = 0;
    if (lcf_status r = plan.rows ? rows_image(s, st, &rs) : run_image(s, st, &rs, &run_flags)) return r;
    const long long state_from = 2 * (s->run_steps - 1);   // X / LP / counts: written by the run's last step
    unsigned int& arrivals = plan.rows ? s->rows_arrivals : s->run_arrivals;
    const int n_wg = std::min(plan.hi - plan.lo, plan.cap);
    // (test of the recovery from a launch whose workgroups are not all resident: the last one is not launched at all)
    const dim3 grid((unsigned)(plan.test_missing && n_wg > 1 ? n_wg - 1 : n_wg));
    arrivals += (unsigned int)n_wg;   // (0 = "no check": skipped when the count wraps onto it)
    if (arrivals == 0u) arrivals = 1u;
    hipLaunchKernelGGL(plan.run, grid, dim3(plan.threads), plan.lds, st, s->e->d_dp, rs, rel, s->rows(rel), s->g_run0, n_hs,
                       state_from, n_wg, run_flags, arrivals, plan.lo, plan.hi - plan.lo, need_progress);
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

// One half-step of a sharded run on this rank, up to the log-posteriors of its shard [lo, hi).
lcf_status launch_half_step_sharded(lcf_sampler* s, int lo, int hi, hipStream_t st) {
    if (fused_eligible(s) && hi > lo) {
        if (lcf_status r = launch_fused(s, lo, hi, st)) return r;
        return launch_finalize(s, lo, hi, st);
    }
    if (lcf_status r = launch_next(s, true, lo, hi, st)) return r;
    return launch_eval(s, lo, hi, true, st);
}

// The same without the finalize launch: the shard's rows (partial sums + log-prior) are the result.
lcf_status launch_half_step_rows(lcf_sampler* s, int lo, int hi, hipStream_t st) {
    if (fused_eligible(s) && hi > lo) return launch_fused(s, lo, hi, st);
    if (lcf_status r = launch_next(s, true, lo, hi, st)) return r;
    return launch_eval(s, lo, hi, false, st);
}

}  // namespace lcf

extern "C" {

// ---- RCCL, bound at run time (no link-time dependency; the library PyTorch ships is reused when torch is loaded) ----
namespace {
struct Rccl {
    void* handle = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, lcf_comm_id, int) = nullptr;  // ncclUniqueId is a 128-byte struct by value
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*CommUserRank)(void*, int*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;

lcf_status rccl_load(const char* path) {
    if (g_rccl.handle) return LCF_OK;
    void* h = dlopen(path && path[0] ? path : "librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(LCF_ERR_UNSUPPORTED, std::string("cannot load RCCL: ") + dlerror());
    Rccl r;
    r.handle = h;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    r.CommCount = (decltype(r.CommCount))dlsym(h, "ncclCommCount");
    r.CommUserRank = (decltype(r.CommUserRank))dlsym(h, "ncclCommUserRank");
    if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy)
        return fail(LCF_ERR_UNSUPPORTED, "RCCL library lacks the expected symbols");
    g_rccl = r;
    return LCF_OK;
}

lcf_status rccl_check(int rc, const char* what) {
    if (rc == 0) return LCF_OK;
    return fail(LCF_ERR_HIP, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error"));
}
}  // namespace

struct lcf_comm {
    void* comm = nullptr;
    int n_ranks = 1, rank = 0;
};

lcf_status lcf_comm_probe(const char* rccl_path) { return rccl_load(rccl_path); }

lcf_status lcf_comm_unique_id(const char* rccl_path, lcf_comm_id* out) {
    if (!out) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = rccl_load(rccl_path)) return st;
    return rccl_check(g_rccl.GetUniqueId(out), "ncclGetUniqueId");
}

lcf_status lcf_comm_create(const char* rccl_path, const lcf_comm_id* id, int32_t n_ranks, int32_t rank, int32_t device,
                           lcf_comm** out) {
    if (!id || !out || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(LCF_ERR_INVALID_ARGUMENT, "bad argument");
    *out = nullptr;
    if (lcf_status st = rccl_load(rccl_path)) return st;
    LCF_HIP(hipSetDevice(device));
    auto* c = new lcf_comm();
    c->n_ranks = n_ranks;
    c->rank = rank;
    if (lcf_status st = rccl_check(g_rccl.CommInitRank(&c->comm, n_ranks, *id, rank), "ncclCommInitRank")) {
        delete c;
        return st;
    }
    *out = c;
    return LCF_OK;
}

lcf_status lcf_comm_count(const lcf_comm* c, int32_t* n_ranks, int32_t* rank) {
    if (!c || !c->comm) return fail(LCF_ERR_INVALID_ARGUMENT, "null communicator");
    if (!g_rccl.CommCount || !g_rccl.CommUserRank) return fail(LCF_ERR_UNSUPPORTED, "RCCL lacks ncclCommCount");
    int n = 0, r = 0;
    if (lcf_status st = rccl_check(g_rccl.CommCount(c->comm, &n), "ncclCommCount")) return st;
    if (lcf_status st = rccl_check(g_rccl.CommUserRank(c->comm, &r), "ncclCommUserRank")) return st;
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = r;
    return LCF_OK;
}

lcf_status lcf_comm_time_allgather(lcf_comm* c, lcf_sampler* s, int32_t reps, double* avg_ms) {
    if (!c || !s || reps <= 0 || !avg_ms) return fail(LCF_ERR_INVALID_ARGUMENT, "bad argument");
    const int nh = s->ds.n_half;
    if (nh % c->n_ranks) return fail(LCF_ERR_INVALID_ARGUMENT, "the slots of a half-step must divide evenly over the ranks");
    LCF_HIP(hipSetDevice(s->e->device));
    hipStream_t st = s->e->stream;
    const size_t stride = (size_t)s->e->dp.n_parts + 1, width = (size_t)(nh / c->n_ranks);
    double* scratch = nullptr;  // not the sampler's rows: a measurement must not disturb a chain
    LCF_HIP(hipMalloc((void**)&scratch, (size_t)nh * stride * sizeof(double)));
    LCF_HIP(hipMemsetAsync(scratch, 0, (size_t)nh * stride * sizeof(double), st));
    lcf_status rc = LCF_OK;
    for (int k = -2; k < reps && rc == LCF_OK; ++k) {  // two warm-up rounds, then the timed ones
        if (k == 0 && hipEventRecord(s->ev0, st) != hipSuccess) rc = fail(LCF_ERR_HIP, "hipEventRecord");
        if (rc == LCF_OK)
            rc = rccl_check(g_rccl.AllGather(scratch + c->rank * width * stride, scratch, width * stride, /*ncclDouble*/ 8,
                                             c->comm, st), "ncclAllGather");
    }
    if (rc == LCF_OK && hipEventRecord(s->ev1, st) != hipSuccess) rc = fail(LCF_ERR_HIP, "hipEventRecord");
    const hipError_t serr = hipStreamSynchronize(st);
    float ms = 0.f;
    if (rc == LCF_OK && serr == hipSuccess && hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) *avg_ms = ms / reps;
    hipFree(scratch);
    if (rc != LCF_OK) return rc;
    LCF_HIP(serr);
    return LCF_OK;
}

void lcf_comm_destroy(lcf_comm* c) {
    if (!c) return;
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    delete c;
}

// Whole sharded run enqueued natively: per half-step  k_fused (replicated commit + proposals; thermal states and
// likelihood of the shard) -> in-place ncclAllGather of the shard's rows of partial sums.  No host
// round-trip and no Python between half-steps; every rank must call it with the same arguments.
lcf_status lcf_sampler_run_sharded(lcf_sampler* s, lcf_comm* c, int64_t first_step, int64_t n_steps,
                                   int32_t split_mode, const int32_t* perm, int32_t store_chain) {
    if (!s || !c) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    const int nh = s->ds.n_half;
    if (nh % c->n_ranks)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the slots of a half-step must divide evenly over the ranks");
    if (lcf_status st = lcf_sampler_begin(s, first_step, n_steps, split_mode, perm, store_chain)) return st;
    hipStream_t st = s->e->stream;
    const int width = nh / c->n_ranks, lo = c->rank * width, hi = lo + width;
    // What travels is each slot's ROW (partial chi^2 sums + log-prior, n_parts + 1 doubles): the accept tests of the
    // next launch add them up themselves, exactly as on one GPU, so no finalize launch sits in front of the collective.
    s->ds.inline_finalize = 1;
    const size_t stride = (size_t)s->e->dp.n_parts + 1;
    LCF_HIP(hipEventRecord(s->ev0, st));
    for (int64_t k = 0; k < 2 * n_steps; ++k) {
        if (lcf_status r = launch_half_step_rows(s, lo, hi, st)) return r;
        double* buf = s->ds.part2[(s->g_next - 1) & 1];
        if (lcf_status r = rccl_check(g_rccl.AllGather(buf + lo * stride, buf, (size_t)width * stride, /*ncclDouble*/ 8,
                                                       c->comm, st),
                                      "ncclAllGather"))
            return r;
    }
    if (lcf_status r = flush_pending(s, st)) return r;
    LCF_HIP(hipEventRecord(s->ev1, st));
    if (lcf_status r = enqueue_snapshot(s)) return r;
    return lcf_sampler_wait(s);
}

// ---- peer mailboxes: a sharded run without a collective ---------------------------------------------------------------
namespace {
// What the mailboxes and the row boards have in common.  A rank's block of polled memory for the other ranks: its IPC
// handle (`out`) and, for ranks emulated inside one process, its address (`local_ptr`).
lcf_status export_block(void* block, lcf_ipc_handle* out, void** local_ptr) {
    if (out) {
        static_assert(sizeof(hipIpcMemHandle_t) <= sizeof(lcf_ipc_handle), "IPC handle size");
        hipIpcMemHandle_t h;
        LCF_HIP(hipIpcGetMemHandle(&h, block));
        std::memset(out, 0, sizeof(*out));
        std::memcpy(out, &h, sizeof(h));
    }
    if (local_ptr) *local_ptr = block;
    return LCF_OK;
}
// Every rank's block as this rank addresses it, into peers[0, n_ranks): its own (`mine`), plain device pointers
// (`local_ptrs`), or the handles opened through IPC and remembered in `opened` (closed with the sampler).
lcf_status map_blocks(void* mine, int n_ranks, int rank, const lcf_ipc_handle* handles, void* const* local_ptrs,
                      std::vector<void*>& opened, unsigned long long** peers, const char* what_null) {
    for (int r = 0; r < n_ranks; ++r) {
        void* p = nullptr;
        if (r == rank) {
            p = mine;
        } else if (local_ptrs) {  // ranks emulated inside one process: plain device pointers
            p = local_ptrs[r];
        } else {
            hipIpcMemHandle_t h;
            std::memcpy(&h, &handles[r], sizeof(h));
            LCF_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
            opened.push_back(p);
        }
        if (!p) return fail(LCF_ERR_INVALID_ARGUMENT, what_null);
        peers[r] = static_cast<unsigned long long*>(p);
    }
    return LCF_OK;
}

size_t mailbox_bytes(const lcf_sampler* s) {
    return (size_t)4 * s->ds.n_half * (s->e->dp.n_parts + 1) * 2 * sizeof(unsigned long long);
}
lcf_status mailbox_alloc(lcf_sampler* s) {
    if (s->mailbox) return LCF_OK;
    LCF_HIP(hipSetDevice(s->e->device));
    // uncached (fine-grained) device memory: peers' stores over the fabric and this rank's polls meet in memory
    s->mailbox_cap = mailbox_bytes(s);
    if (lcf_status st = polled_alloc(s->e->device, true, s->mailbox_cap, (void**)&s->mailbox)) return st;
    return LCF_OK;
}
}  // namespace

lcf_status lcf_sampler_mailbox_export(lcf_sampler* s, lcf_ipc_handle* out, void** local_ptr) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = mailbox_alloc(s)) return st;
    return export_block(s->mailbox, out, local_ptr);
}

lcf_status lcf_sampler_mailbox_connect(lcf_sampler* s, int32_t n_ranks, int32_t rank, const lcf_ipc_handle* handles,
                                       void* const* local_ptrs) {
    if (!s || n_ranks < 1 || n_ranks > kMaxPeers || rank < 0 || rank >= n_ranks || (!handles && !local_ptrs))
        return fail(LCF_ERR_INVALID_ARGUMENT, "bad argument (at most 8 ranks)");
    if (s->ds.n_half % n_ranks)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the slots of a half-step must divide evenly over the ranks");
    if (!fused_eligible(s)) return fail(LCF_ERR_UNSUPPORTED, "peer-mailbox runs need the one-launch half-step (k_fused)");
    if (lcf_status st = mailbox_alloc(s)) return st;
    LCF_HIP(hipSetDevice(s->e->device));
    if (lcf_status st = map_blocks(s->mailbox, n_ranks, rank, handles, local_ptrs, s->opened, s->ds.peer_mbox,
                                   "null peer mailbox"))
        return st;
    s->ds.mbox = s->mailbox;
    s->peer_ranks = n_ranks;
    s->peer_rank = rank;
    return LCF_OK;
}

// The run of lcf_sampler_run_sharded without its collective: every launch posts the rows of this rank's shard into
// all ranks' mailboxes and polls its own for the rows it needs.  Collective in effect: every rank must call it with the
// same arguments, after ALL ranks have returned from the previous run (the caller's barrier).
lcf_status lcf_sampler_run_peers_async(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                       const int32_t* perm, int32_t store_chain) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (s->peer_ranks < 1) return fail(LCF_ERR_STATE, "lcf_sampler_mailbox_connect must be called first");
    if (!fused_eligible(s)) return fail(LCF_ERR_UNSUPPORTED, "peer-mailbox runs need the one-launch half-step (k_fused)");
    if (lcf_status st = sampler_begin(s, first_step, n_steps, split_mode, perm, store_chain, true)) return st;
    hipStream_t st = s->e->stream;
    const int width = s->ds.n_half / s->peer_ranks, lo = s->peer_rank * width, hi = lo + width;
    s->ds.inline_finalize = 1;
    s->ds.n_peers = s->peer_ranks;
    LCF_HIP(hipEventRecord(s->ev0, st));
    lcf_status rc = LCF_OK;
    for (int64_t k = 0; k < 2 * n_steps && rc == LCF_OK; ++k) rc = launch_fused(s, lo, hi, st);
    if (rc == LCF_OK) rc = flush_pending(s, st);
    s->ds.n_peers = 0;  // (kernel arguments are captured at launch: later runs of other kinds are unaffected)
    if (rc != LCF_OK) return rc;
    LCF_HIP(hipEventRecord(s->ev1, st));
    return enqueue_snapshot(s);
}

lcf_status lcf_sampler_run_peers(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                 const int32_t* perm, int32_t store_chain) {
    if (lcf_status st = lcf_sampler_run_peers_async(s, first_step, n_steps, split_mode, perm, store_chain)) return st;
    return lcf_sampler_wait(s);
}

// ---- multi-GPU without replicated bookkeeping: rows over the boards (lcf_sampler_run_rows) ---------------------------
}  // extern "C"

namespace {
// The plan of this rank's share of a row-board run (resident workgroups, k_solo_run<..., RANKS>, where a single-GPU run
// of the share would take them: plan_run) -- and only k_solo and k_solo_run read and post rows.
lcf_status plan_rows(const lcf_sampler* s, int n_ranks, int rank, bool resident, RunPlan* plan) {
    const int width = s->ds.n_half / n_ranks;
    *plan = plan_run(s, true, rank * width, rank * width + width, resident);
    if (plan->form != LCF_KERNEL_RUN && plan->form != LCF_KERNEL_SOLO)
        return fail(LCF_ERR_UNSUPPORTED, "row-board runs need the one-workgroup-per-proposal half-step (k_solo)");
    return LCF_OK;
}

lcf_status board_alloc(lcf_sampler* s) {
    if (s->board_mem) return LCF_OK;
    LCF_HIP(hipSetDevice(s->e->device));
    // uncached (fine-grained) device memory: peers' stores over the fabric and this rank's polls meet in memory
    if (lcf_status st = polled_alloc(s->e->device, true, s->board_bytes(), &s->board_mem)) return st;
    s->ds.board = static_cast<unsigned long long*>(s->board_mem);
    return LCF_OK;
}
}  // namespace

extern "C" {

lcf_status lcf_sampler_board_export(lcf_sampler* s, lcf_ipc_handle* out, void** local_ptr) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = board_alloc(s)) return st;
    return export_block(s->board_mem, out, local_ptr);
}

lcf_status lcf_sampler_board_connect(lcf_sampler* s, int32_t n_ranks, int32_t rank, const lcf_ipc_handle* handles,
                                     void* const* local_ptrs) {
    if (!s || n_ranks < 1 || n_ranks > kMaxPeers || rank < 0 || rank >= n_ranks || (!handles && !local_ptrs))
        return fail(LCF_ERR_INVALID_ARGUMENT, "bad argument (at most 8 ranks)");
    if (s->ds.n_half % n_ranks)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the slots of a half-step must divide evenly over the ranks");
    RunPlan plan;
    if (lcf_status st = plan_rows(s, n_ranks, rank, true, &plan)) return st;
    if (lcf_status st = board_alloc(s)) return st;
    LCF_HIP(hipSetDevice(s->e->device));
    if (lcf_status st = map_blocks(s->board_mem, n_ranks, rank, handles, local_ptrs, s->board_opened, s->ds.peer_board,
                                   "null peer board"))
        return st;
    s->ds.n_board_ranks = n_ranks;
    s->ds.board_rank = rank;
    // (the kernel a resident run of this rank will take, prepared now: see prepare_run; and the image of the sampler it
    // reads, allocated now: an allocation made by one rank of a process while another rank's resident workgroups already
    // wait for it can hold its launch back for seconds)
    if (lcf_status st = put_image(s, s->rows_image, nullptr, nullptr)) return st;
    return plan.form == LCF_KERNEL_RUN ? prepare_run(s->e, plan) : LCF_OK;
}

// The sharded run in which nothing is replicated: rank r evaluates, accepts and commits the proposals
// [r w, (r + 1) w) of every half-step with k_solo and posts each walker's new row (position, log-posterior, acceptance
// count) on every rank's board; the serial head of a later half-step polls its own board for the rows it needs.  No
// collective, no launch between half-steps, no work about other ranks' walkers.  When the run ends every rank takes
// the last step's rows of ALL walkers from its board, so state, acceptance counts and (if stored) the chain are
// complete on every rank.  Collective in effect: every rank calls it with the same arguments, after ALL ranks have
// returned from the previous run (the caller's barrier); the ranks' samplers must have seen the same sequence of runs.
lcf_status lcf_sampler_run_rows_async(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                      const int32_t* perm, int32_t store_chain) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (s->ds.n_board_ranks < 1) return fail(LCF_ERR_STATE, "lcf_sampler_board_connect must be called first");
    RunPlan plan;
    if (lcf_status st = plan_rows(s, s->ds.n_board_ranks, s->ds.board_rank, n_steps > 0, &plan)) return st;
    static const bool trace = std::getenv("LCF_TRACE_RUN") != nullptr;   // (diagnostic: host time of the enqueue's parts)
    const auto t_in = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (trace)
            std::fprintf(stderr, "lcf_sampler_run_rows (rank %d): %s at %.1f us\n", s->ds.board_rank, what,
                         std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_in).count());
    };
    if (lcf_status st = sampler_begin(s, first_step, n_steps, split_mode, perm, store_chain, true)) return st;
    mark("draw records enqueued");
    hipStream_t st = s->e->stream;
    DevSampler& ds = s->ds;
    long long launches = plan.form == LCF_KERNEL_RUN ? 0 : 2 * n_steps;   // (resident launches: counted below)
    LCF_HIP(hipEventRecord(s->ev0, st));
    const long long cells = (long long)ds.n_walkers * (ds.n_dim + 2);
    hipLaunchKernelGGL(k_board_init, dim3((unsigned)((std::max<long long>(cells, kBoardClear) + 255) / 256)), dim3(256), 0, st, ds,
                       (unsigned int)s->g_run0);
    LCF_HIP(hipGetLastError());
    s->rows_arrivals = 0;   // (k_board_init has cleared the word)
    // (k_board_collect: workgroups of four waves, each wave 64 / board_row_entries rows)
    const int collect_rpw = 64 / board_row_entries(ds.n_dim);
    auto collect_grid = [&](long long rows) { return dim3((unsigned)((rows + 4 * collect_rpw - 1) / (4 * collect_rpw))); };
    if (plan.form == LCF_KERNEL_RUN) {
        // The rank's workgroups stay for a block of up to kRunSpan half-steps (k_solo_run<..., RANKS>); behind every launch
        // the rows of its half-steps -- as every rank posted them -- go from the board into the chain, behind the last one
        // the rows of the last step into X / LP / counts.  A launch may start once every rank has reached the launch before
        // the previous one (need_progress).
        if (lcf_status r = prepare_run(s->e, plan)) return r;
        long long starts[2] = {-1, -1};   // first half-steps (relative) of the two launches in front
        for (long long rel = 0; rel < 2 * n_steps; ++launches) {
            if (lcf_status r = enter_half_step(&s, 1, rel, st)) return r;
            const int n = s->block_span(rel, plan.span);
            const long long need = starts[0] >= 0 ? s->g_run0 + starts[0] : 0;
            if (lcf_status r = launch_run(s, plan, rel, n, st, need)) return r;
            mark("resident launch enqueued");
            if (store_chain) {
                hipLaunchKernelGGL(k_board_collect, collect_grid((long long)n * ds.n_half), dim3(256), 0, st, ds,
                                   (long long)(s->g_run0 + rel), (long long)(rel / 2), s->rows(rel), n, 0, 1);
                LCF_HIP(hipGetLastError());
            }
            if (lcf_status r = leave_half_step(&s, 1, st)) return r;
            starts[0] = starts[1];
            starts[1] = rel;
            rel += n;
        }
    } else {
        for (int64_t k = 0; k < 2 * n_steps; ++k) {
            if (lcf_status r = launch_solo(s, plan, k, st)) return r;
            if (store_chain && (k & 1)) {  // the rows of this step's two half-steps, from every rank, into the chain
                hipLaunchKernelGGL(k_board_collect, collect_grid(2ll * ds.n_half), dim3(256), 0, st, ds,
                                   (long long)(s->g_run0 + k - 1), (long long)(k / 2), s->rows(k - 1), 2, 0, 1);
                LCF_HIP(hipGetLastError());
            }
        }
    }
    if (n_steps > 0) {  // the last step's rows of all walkers into X / LP / counts
        const long long k = 2 * (n_steps - 1);
        hipLaunchKernelGGL(k_board_collect, collect_grid(2ll * ds.n_half), dim3(256), 0, st, ds, (long long)(s->g_run0 + k),
                           (long long)(k / 2), s->rows(k), 2, 1, 0);
        LCF_HIP(hipGetLastError());
    }
    s->g_next += 2 * n_steps;
    s->record_run(plan.form, true, launches, plan.instance);
    LCF_HIP(hipEventRecord(s->ev1, st));
    const lcf_status rc = enqueue_snapshot(s);
    mark("all enqueued");
    return rc;
}

lcf_status lcf_sampler_run_rows(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                const int32_t* perm, int32_t store_chain) {
    if (lcf_status st = lcf_sampler_run_rows_async(s, first_step, n_steps, split_mode, perm, store_chain)) return st;
    return lcf_sampler_wait(s);
}

}  // extern "C"

// ---- population mode: the same n_steps for `n` samplers (one transient each, same walker count) in lock step ---------
// Every launch covers all transients (blockIdx.y = transient), in the first of three forms the population allows
// (population_plan): resident workgroups for blocks of half-steps (k_pop_run), ONE launch per half-step (k_pop), or two
// (k_step_multi + k_points_multi).  Each form is enqueued by a loop of its own over the run's half-steps.
namespace {

// Proposals per workgroup of k_pop: 4.  (Measured at 32 x 512 walkers x 600 points: 49.0 us per half-step; staging the
// interpolants in LDS as well costs occupancy, 61.7 us; workgroups of 8 proposals that can afford it, 50.4 us;
// five waves per SIMD at the price of 8 spilled registers, 47.0 us.)
constexpr int kPopGroup = 4;

bool g_pop_run_off = false;   // a resident launch of this process found its workgroups not all there

// How a population run goes, decided before any of it is enqueued.
struct PopPlan {
    int form = LCF_KERNEL_POPULATION_PHASES;   // LCF_KERNEL_POPULATION_RUN, _POPULATION or _POPULATION_PHASES
    const RunSwitches sw = run_switches();     // the environment's switches as the run found them
    std::vector<MultiItem> items;              // per transient: its sampler by value, the engine's parts merged
    int same_dim = 0;                          // compile-time walker dimension when every transient has the same
    int pop_spec = 0;                          // the model-specialised kernel when every transient takes the same
    int max_parts = 1;
    size_t lds = 0, pop_lds = 0, run_lds = 0;  // of k_points_multi, k_pop and k_pop_run
    // the resident form: k_pop_run<ND, 1, kPopRunGroup, M> of the population's shape, the workgroups of it the device
    // holds, transients per launch, workgroups per transient, and the device's claim (run_claim)
    decltype(&k_pop_run<0, 1, kPopRunGroup, 0>) run_kernel = nullptr;
    int cap = 0, chunk = 0, run_grid = 0;
    RunClaim claim{0, nullptr, false};
    int instance[4] = {-1, -1, -1, -1};        // <ND, 0, M, 0> of the k_pop / k_pop_run taken (no NP: parts at run time)
    // the run's GenItems (batched generation only) and items in device memory, freed with the plan on every way out
    GenItem* d_gen = nullptr;
    MultiItem* d_items = nullptr;
    ~PopPlan() { hipFree(d_gen); hipFree(d_items); }
};

// LDS of a workgroup of `group` proposals of k_pop / k_pop_run: the staged image, the proposals' scratch and wave sums
size_t pop_lds_bytes(const DevProblem& pb, int group) {
    return kLdsHead * sizeof(double) + (size_t)pb.stage_d2 * sizeof(double2) +
           (size_t)group * (kPopScratch + 4 * kPopMaxParts) * sizeof(double);
}

// The resident form, if it fits: the workgroups stay for a block of half-steps and hand each other rows through the
// transients' boards.  The launch stages the interpolants in LDS as well, where the engine's image leaves them out.
lcf_status plan_resident(lcf_sampler** ss, int n, long long g, PopPlan& p) {
    const lcf_sampler* s0 = ss[0];
    // (a board of tagged rows and a second set of state buffers per transient -- 64 KB per walker: a population of
    // thousands of transients stays with a launch per half-step rather than take more than half of the free memory)
    size_t need = 0, free_b = 0, total_b = 0;
    for (int t = 0; t < n; ++t)
        if (!ss[t]->run_board_mem) need += ss[t]->run_board_bytes() + (size_t)ss[t]->ds.n_walkers * (ss[t]->ds.n_dim + 2) * 8;
    const bool memory = need == 0 || (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need <= free_b / 2);
    (void)hipGetLastError();
    if (!memory) return LCF_OK;
    const bool itab_lds = !(std::getenv("LCF_POP_ITAB_LDS") && std::atoi(std::getenv("LCF_POP_ITAB_LDS")) == 0);
    std::vector<int> itab_extra(n, 0);
    for (int t = 0; t < n; ++t) {
        const DevProblem& ip = p.items[t].pb;
        const size_t n_itab = ip.use_itab ? (size_t)ip.n_filters * ip.itab_m * 8 : 0;
        if (itab_lds && n_itab > 0 && ip.n_itab_lds == 0 && ip.n_spl_lds == 0 && n_itab * sizeof(double) <= 40 * 1024)
            itab_extra[t] = (int)n_itab;
        p.run_lds = std::max(p.run_lds, pop_lds_bytes(ip, kPopRunGroup) + (size_t)(itab_extra[t] / 2) * sizeof(double2));
    }
    // fits: a CU's LDS, and at least one workgroup on the compute units the population's stream may use
    if (p.run_lds > kLdsPerCU) return LCF_OK;
    const auto own = [&](auto nd, auto m) {
        p.run_kernel = k_pop_run<decltype(nd)::value, 1, kPopRunGroup, decltype(m)::value>;
        p.instance[0] = decltype(nd)::value;
        p.instance[2] = decltype(m)::value;
    };
    p.instance[0] = p.instance[1] = p.instance[2] = p.instance[3] = 0;
    if (!dispatch_model(PopRunModels{}, p.same_dim, p.pop_spec, own)) p.run_kernel = k_pop_run<0, 1, kPopRunGroup, 0>;
    int per_cu = 0;
    LCF_HIP(prepare_kernel(p.run_kernel, p.run_lds, 64 * kPopRunGroup, &per_cu));
    p.cap = run_capacity(s0->e, per_cu, p.sw.run_grid);
    if (p.cap < 1) return LCF_OK;
    p.claim.dev = s0->e->device;
    p.claim.st = s0->e->stream;
    if (!(p.claim.held = run_claim(p.claim.dev, p.claim.st))) return LCF_OK;
    for (int t = 0; t < n; ++t) {
        lcf_sampler* s = ss[t];
        if (lcf_status r = run_buffers(s)) return r;
        MultiItem& it = p.items[t];
        it.sm = run_struct(s);
        it.g_run0 = g;
        it.flip = s->run_flip ? 1 : 0;
        it.arrive0 = s->run_arrivals;
        if ((it.itab_extra = itab_extra[t])) {
            it.pb.n_itab_lds = itab_extra[t];
            it.pb.stage_d2 += itab_extra[t] / 2;
        }
    }
    // gridDim.x workgroups per transient, all of them on the device at once: what the device holds, shared evenly -- and
    // no more than give every workgroup the same number of groups of proposals per half-step
    const int n_groups = (s0->ds.n_half + kPopRunGroup - 1) / kPopRunGroup;
    p.chunk = std::min(n, p.cap);
    const int room = std::min(std::max(1, p.cap / p.chunk), n_groups);
    const int per_wg = (n_groups + room - 1) / room;
    p.run_grid = (n_groups + per_wg - 1) / per_wg;
    p.form = LCF_KERNEL_POPULATION_RUN;
    return LCF_OK;
}

// The plan of a run that every transient's sampler has begun: the items, the half-steps numbered in lock step from g,
// and the form (`resident`: the resident form may be taken).
lcf_status population_plan(lcf_sampler** ss, int n, int64_t n_steps, long long g, bool resident, PopPlan& p) {
    const DevProblem& p0 = ss[0]->e->dp;
    p.items.resize(n);
    p.same_dim = ss[0]->ds.n_dim;
    for (int t = 0; t < n; ++t) {
        lcf_sampler* s = ss[t];
        s->g_next = s->g_run0 = g;
        s->ds.inline_finalize = 1;
        if (s->ds.n_dim != p.same_dim) p.same_dim = 0;
        p.items[t] = MultiItem{s->e->dp, s->ds, {s->d_draws[0], s->d_draws[1]}, (long long)s->blk_first,
                               (long long)s->blk_steps, s->coef, s->lprior};
        // With many transients in one launch a single workgroup per proposal already fills the chip, and it stages
        // the tables and reduces once for all of the proposal's chunks: fewer parts than the engine's default.
        DevProblem& ip = p.items[t].pb;
        const long long slots = (long long)n * s->ds.n_half;
        const int want = (int)std::max<long long>(1, (kTargetGroups + slots - 1) / slots);
        const int parts = std::min(ip.n_parts, want);
        const int mg = (ip.n_parts + parts - 1) / parts;  // engine parts merged into one workgroup's share
        const int np = (ip.n_parts + mg - 1) / mg;
        const DevProblem& ep = s->e->dp;
        for (int J = 0; J <= kMaxParts; ++J) {
            ip.part_start[J] = J < np ? ep.part_start[J * mg] : ep.n_points;
            ip.part_col0[J] = J < np ? ep.part_col0[J * mg] : ep.em_cols;
        }
        ip.n_parts = np;
        p.lds = std::max(p.lds, s->e->lds_bytes);
        p.max_parts = std::max(p.max_parts, np);
    }
    p.pop_spec = specialised_model(p.items[0].pb, p.sw);
    for (int t = 1; t < n; ++t)
        if (specialised_model(p.items[t].pb, p.sw) != p.pop_spec) p.pop_spec = 0;
    // k_pop where every transient has shared epochs, staged tables, the fast band sum, at most kPopMaxParts merged parts
    // and tables that do not depend on the proposal (ShockCooling3's reddened tables do)
    bool one_launch = std::getenv("LCF_NO_POP") == nullptr && p0.use_therm && p0.variant != 0 && p0.tab_in_lds &&
                      p.max_parts <= kPopMaxParts;
    for (int t = 0; t < n; ++t) {
        one_launch = one_launch && ss[t]->e->dp.model != kShockCooling3;
        p.pop_lds = std::max(p.pop_lds, pop_lds_bytes(p.items[t].pb, kPopGroup));
    }
    if (!one_launch || p.pop_lds > kLdsPerCU) return LCF_OK;
    p.form = LCF_KERNEL_POPULATION;
    if (!resident || std::getenv("LCF_NO_POP_RUN") || p.sw.no_run_kernel || g_pop_run_off || n_steps == 0) return LCF_OK;
    return plan_resident(ss, n, g, p);
}

// Resident form: per block of draw records, launches of `chunk` transients at a time, run_grid workgroups each.
lcf_status enqueue_pop_run(lcf_sampler** ss, int n, PopPlan& p, int64_t n_steps, int32_t store_chain, hipStream_t st,
                           long long* launches) {
    // (test of the recovery from a launch whose workgroups are not all resident: the last one is not launched at all)
    const unsigned int n_wg = (unsigned int)(p.sw.run_test_missing && p.run_grid > 1 ? p.run_grid - 1 : p.run_grid);
    const long long state_from = 2 * (long long)(n_steps - 1);   // X / LP / counts: written by the run's last step
    int run_launches = 0;
    for (long long rel = 0; rel < 2 * n_steps; ++run_launches) {
        if (lcf_status r = enter_half_step(ss, n, rel, st, p.d_gen)) return r;
        const int n_hs = ss[0]->block_span(rel, kRunSpanSolo);
        for (int c0 = 0; c0 < n; c0 += p.chunk) {
            hipLaunchKernelGGL(p.run_kernel, dim3(n_wg, (unsigned)std::min(p.chunk, n - c0)), dim3(64 * kPopRunGroup), p.run_lds,
                               st, p.d_items + c0, rel, n_hs, state_from, store_chain ? 1 : 0, run_launches, p.run_grid);
            LCF_HIP(hipGetLastError());
        }
        for (int t = 0; t < n; ++t) ss[t]->run_arrivals += (unsigned int)p.run_grid;   // (the board's count of them)
        if (lcf_status r = leave_half_step(ss, n, st, p.d_gen)) return r;
        rel += n_hs;
    }
    for (int t = 0; t < n; ++t) ss[t]->flip_state_sets();   // the state behind this run is in the other set now
    p.claim.release();
    *launches = run_launches;
    return LCF_OK;
}

// One launch per half-step: k_pop, a workgroup per kPopGroup proposals, accept test included.
lcf_status enqueue_pop(lcf_sampler** ss, int n, PopPlan& p, int64_t n_steps, hipStream_t st) {
    const int nh = ss[0]->ds.n_half;
    const dim3 grid((unsigned)((nh + kPopGroup - 1) / kPopGroup), (unsigned)n), block(64 * kPopGroup);
    decltype(&k_pop<0, 1, kPopGroup, 0>) kernel = nullptr;   // k_pop<ND, 1, kPopGroup, M> of the population's shape
    const auto own = [&](auto nd, auto m) {
        kernel = k_pop<decltype(nd)::value, 1, kPopGroup, decltype(m)::value>;
        p.instance[0] = decltype(nd)::value;
        p.instance[2] = decltype(m)::value;
    };
    p.instance[1] = p.instance[3] = 0;
    dispatch(PopDims{}, p.same_dim, [&](auto nd) {
        if (!dispatch_model(SpecialisedModels{}, nd, p.pop_spec, own)) own(nd, Int<0>{});
    });
    LCF_HIP(prepare_kernel(kernel, p.pop_lds));
    for (int64_t k = 0; k < 2 * n_steps; ++k) {
        if (lcf_status r = enter_half_step(ss, n, k, st, p.d_gen)) return r;
        hipLaunchKernelGGL(kernel, grid, block, p.pop_lds, st, p.d_items, (long long)k);
        LCF_HIP(hipGetLastError());
        if (lcf_status r = leave_half_step(ss, n, st, p.d_gen)) return r;
    }
    return LCF_OK;
}

// Two launches per half-step: k_step_multi commits the previous half-step and draws the next one, k_points_multi
// evaluates its proposals; one more k_step_multi commits the last.
lcf_status enqueue_pop_phases(lcf_sampler** ss, int n, const PopPlan& p, int64_t n_steps, long long g, hipStream_t st) {
    const DevProblem& p0 = ss[0]->e->dp;
    const int nh = ss[0]->ds.n_half;
    const dim3 gs((unsigned)nh, (unsigned)n), gp((unsigned)(nh * p.max_parts), (unsigned)n);
    decltype(&k_step_multi<0>) step = nullptr;
    dispatch(PopDims{}, p.same_dim, [&](auto nd) { step = k_step_multi<decltype(nd)::value>; });
    decltype(&k_points_multi<0, false, false>) points = nullptr;   // <VARIANT, LDS_TAB, THERM> of the population
    dispatch<1>(Dims<0>{}, p0.variant, [&](auto v) {
        dispatch<1>(Dims<0>{}, p0.tab_in_lds, [&](auto tab) {
            dispatch<1>(Dims<0>{}, p0.use_therm, [&](auto therm) {
                points = k_points_multi<decltype(v)::value, decltype(tab)::value != 0, decltype(therm)::value != 0>;
            });
        });
    });
    LCF_HIP(prepare_kernel(points, p.lds));
    for (int64_t k = 0; n_steps > 0 && k <= 2 * n_steps; ++k) {
        const bool have_next = k < 2 * n_steps, have_prev = k > 0;
        if (have_next)
            if (lcf_status r = enter_half_step(ss, n, k, st, p.d_gen)) return r;
        hipLaunchKernelGGL(step, gs, dim3(64), 0, st, p.d_items, have_prev ? 1 : 0, (long long)((k - 1) / 2), have_next ? 1 : 0,
                           (long long)k, (long long)(g + k));
        LCF_HIP(hipGetLastError());
        if (!have_next) break;
        if (lcf_status r = leave_half_step(ss, n, st, p.d_gen)) return r;
        hipLaunchKernelGGL(points, gp, dim3(kBlock), p.lds, st, p.d_items, (int)((g + k) & 1));
        LCF_HIP(hipGetLastError());
    }
    return LCF_OK;
}

// One pass of lcf_population_run (`resident`: the resident form may be taken).  *repeat: a resident launch gave up;
// every transient is back on the state the run started from, and the caller repeats the steps without that form.
lcf_status population_run(lcf_sampler** ss, int n, int64_t first_step, int64_t n_steps, int32_t split_mode,
                          int32_t store_chain, double* elapsed_ms, bool resident, bool* repeat) {
    const lcf_sampler* s0 = ss[0];
    hipStream_t st = s0->e->stream;
    // Everything of this run -- every transient's draw records, the half-steps, the snapshots -- goes on ONE stream (the
    // first transient's): stream order is all the synchronisation there is.  What the transients' own streams still hold
    // (set_state, an earlier run of their own) is waited for once, here.
    LCF_HIP(hipSetDevice(s0->e->device));
    LCF_HIP(hipDeviceSynchronize());
    long long g = 0;
    for (int t = 0; t < n; ++t) {
        lcf_sampler* s = ss[t];
        if (lcf_status r = sampler_begin(s, first_step, n_steps, split_mode, nullptr, store_chain, true, st,
                                         /*defer: generated for all transients below*/ true)) return r;
        g = std::max(g, s->g_next);
        if (s->e->stream != st) s->foreign_stream = true;   // (until the stream has been waited for)
    }
    // The draw records of ALL transients come from one launch of each generation kernel per block of steps (random
    // splits of samplers with the same block geometry -- what a population has; else sampler by sampler).
    PopPlan p;
    bool batched_gen = split_mode == LCF_SPLIT_RANDOM;
    for (int t = 1; t < n; ++t)
        batched_gen = batched_gen && ss[t]->blk_first == s0->blk_first && ss[t]->blk_steps == s0->blk_steps;
    if (batched_gen) {
        std::vector<GenItem> gen(n);
        for (int t = 0; t < n; ++t)
            gen[t] = GenItem{ss[t]->ds.key0, ss[t]->ds.key1, ss[t]->ds.n_dim, ss[t]->ds.a,
                             {ss[t]->d_perm[0], ss[t]->d_perm[1]}, {ss[t]->d_slot[0], ss[t]->d_slot[1]},
                             {ss[t]->d_draws[0], ss[t]->d_draws[1]}};
        LCF_HIP(hipMalloc((void**)&p.d_gen, (size_t)n * sizeof(GenItem)));
        LCF_HIP(hipMemcpy(p.d_gen, gen.data(), (size_t)n * sizeof(GenItem), hipMemcpyHostToDevice));
    }
    if (n_steps > 0)
        if (lcf_status r = generate_block(ss, n, 0, st, p.d_gen)) return r;
    if (lcf_status r = population_plan(ss, n, n_steps, g, resident, p)) return r;
    LCF_HIP(hipMalloc((void**)&p.d_items, (size_t)n * sizeof(MultiItem)));
    LCF_HIP(hipMemcpyAsync(p.d_items, p.items.data(), (size_t)n * sizeof(MultiItem), hipMemcpyHostToDevice, st));
    LCF_HIP(hipEventRecord(s0->ev0, st));
    long long launches = 2 * n_steps * (p.form == LCF_KERNEL_POPULATION_PHASES ? 2 : 1);
    const lcf_status rc = p.form == LCF_KERNEL_POPULATION_RUN ? enqueue_pop_run(ss, n, p, n_steps, store_chain, st, &launches)
                          : p.form == LCF_KERNEL_POPULATION   ? enqueue_pop(ss, n, p, n_steps, st)
                                                              : enqueue_pop_phases(ss, n, p, n_steps, g, st);
    if (rc) return rc;
    LCF_HIP(hipEventRecord(s0->ev1, st));
    // every transient's snapshot (error word, state, counts) behind the run, on the same stream: ONE wait below serves
    // the 32 state / count / check calls that follow (each of them used to synchronise and launch on its own)
    for (int t = 0; t < n; ++t)
        if (lcf_status r = launch_snapshot(ss[t], st)) return r;
    LCF_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s0->ev0, s0->ev1) == hipSuccess && elapsed_ms) *elapsed_ms = ms;
    bool gave_up = false;
    for (int t = 0; t < n; ++t) {
        ss[t]->g_next = g + 2 * n_steps;
        ss[t]->pending = false;
        ss[t]->foreign_stream = false;      // (the stream has been waited for)
        ss[t]->snap_enqueued = false;
        ss[t]->snap_valid = true;
        ss[t]->last_ms = ms;
        ss[t]->record_run(p.form, false, launches, p.instance);   // (_POPULATION_PHASES: no instance, the -1 it starts with)
        gave_up = gave_up || (p.form == LCF_KERNEL_POPULATION_RUN && (reported_error(ss[t]) & 2));
    }
    if (gave_up) {   // (rewind_resident_run; the caller repeats the steps with a launch per half-step)
        for (int t = 0; t < n; ++t)
            if (lcf_status r = rewind_resident_run(ss[t])) return r;
        std::fprintf(stderr, "liblcf_hip: a resident population launch gave up waiting for a row: its workgroups were not all "
                     "resident (another resident kernel on this GPU?); the steps are repeated with a launch per half-step, as are "
                     "this process's later population runs (LCF_NO_POP_RUN=1 avoids the wait)\n");
        g_pop_run_off = true;
        *repeat = true;
        return LCF_OK;
    }
    for (int t = 0; t < n; ++t)
        if (lcf_status r = lcf_sampler_check(ss[t])) return r;
    return LCF_OK;
}

}  // namespace

extern "C" {

lcf_status lcf_population_run(lcf_sampler** ss, int32_t n, int64_t first_step, int64_t n_steps, int32_t split_mode,
                              int32_t store_chain, double* elapsed_ms) {
    if (!ss || n <= 0) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (n > 65535) return fail(LCF_ERR_INVALID_ARGUMENT, "at most 65535 transients per call");
    if (split_mode == LCF_SPLIT_HOST) return fail(LCF_ERR_UNSUPPORTED, "population runs use identity or random splits");
    const lcf_sampler* s0 = ss[0];
    for (int t = 0; t < n; ++t) {
        const lcf_sampler* s = ss[t];
        if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null sampler");
        const DevProblem &a = s->e->dp, &b = s0->e->dp;
        if (s->e->device != s0->e->device || s->ds.n_walkers != s0->ds.n_walkers || a.variant != b.variant ||
            a.use_therm != b.use_therm || a.tab_in_lds != b.tab_in_lds)
            return fail(LCF_ERR_UNSUPPORTED, "transients of one batched run must agree on device, walker count, "
                                             "band-sum variant, thermal sharing and table placement");
    }
    bool repeat = false;   // (a resident launch gave up: the same steps again, without the resident form)
    lcf_status r = population_run(ss, n, first_step, n_steps, split_mode, store_chain, elapsed_ms, true, &repeat);
    if (r == LCF_OK && repeat)
        r = population_run(ss, n, first_step, n_steps, split_mode, store_chain, elapsed_ms, false, &repeat);
    return r;
}

}  // extern "C"

#ifdef LCF_PROGRESS
extern "C" int lcf_debug_read_progress(unsigned int* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_progress), sizeof(unsigned int) * 64 * 16);
}
#endif
#ifdef LCF_POLL_LOOKS
// (polls of 1, 2, 3 and more looks, looks in total; `reset` != 0: cleared afterwards)
extern "C" int lcf_debug_read_poll_looks(unsigned long long* out, int reset) {
    int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_poll_looks), sizeof(unsigned long long) * 4);
    if (reset) {
        static unsigned long long zeros[4];
        rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_poll_looks), zeros, sizeof zeros);
    }
    return rc;
}
// (the per-workgroup records: `out` holds `max_records` of 8 words -- launch, blockIdx.x, HW_ID, XCC_ID, polls of 1, 2, 3
// and more looks, looks in total; *n_records: how many workgroups have left a launch since the last reset, which may be
// more than were kept; `reset` != 0: cleared afterwards)
extern "C" int lcf_debug_read_poll_wg(unsigned int* out, int max_records, unsigned int* n_records, int reset) {
    int rc = (int)hipMemcpyFromSymbol(n_records, HIP_SYMBOL(g_poll_wg_n), sizeof(unsigned int));
    size_t keep = *n_records < (unsigned int)kPollWgMax ? *n_records : (size_t)kPollWgMax;
    if (max_records < 0) max_records = 0;
    if (keep > (size_t)max_records) keep = (size_t)max_records;
    if (keep > 0) rc |= (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_poll_wg), sizeof(unsigned int) * kPollWgWords * keep);
    if (reset) {
        const unsigned int zero = 0u;
        rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_poll_wg_n), &zero, sizeof zero);
    }
    return rc;
}
#endif
#ifdef LCF_STAMPS
// (sums and counts, 64 x 16 each; `reset` != 0: cleared afterwards, with the "previous stamp" of every workgroup)
extern "C" int lcf_debug_read_stamp_sums(unsigned long long* acc, unsigned long long* cnt, int reset) {
    int rc = (int)hipMemcpyFromSymbol(acc, HIP_SYMBOL(g_acc), sizeof(unsigned long long) * 64 * 16);
    rc |= (int)hipMemcpyFromSymbol(cnt, HIP_SYMBOL(g_cnt), sizeof(unsigned long long) * 64 * 16);
    if (reset) {
        static unsigned long long zeros[64 * 16];
        rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_acc), zeros, sizeof zeros);
        rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_cnt), zeros, sizeof zeros);
        rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_last), zeros, sizeof(unsigned long long) * 64);
    }
    return rc;
}
extern "C" int lcf_debug_read_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 64 * 16);
}
extern "C" int lcf_debug_read_wall(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wall), sizeof(unsigned long long) * 2 * 1024 * 2);
}
#endif
