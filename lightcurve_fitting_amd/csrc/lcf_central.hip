// Central-engine models (LCF_MODEL_ARNETT, LCF_MODEL_MAGNETAR): a bolometric light curve L(t) [W], one number per
// epoch and no filters, from a power source P(s) at the centre of the ejecta through Arnett's diffusion integral
//     L(t) = leak(t) int_0^t P(s) (2 s / tau_m^2) exp(-(t - s)(t + s) / tau_m^2) ds,     t = (MJD - t_0) / (1 + z).
// (include/lcf.h, "central-engine models", has the parameters, the sources and the units.)
//
// The integral is ONE fixed quadrature of 64 nodes, part of the model's definition (DESIGN.md has its measured error):
// the range is cut to [s_lo, t], s_lo = sqrt(max(0, t^2 - 40 tau_m^2)), split at s_lo + (t - s_lo) / 8, and each piece
// takes 32 Gauss-Legendre nodes.  Nodes and weights depend on (t, tau_m) only.
//
// Work decomposition: workgroup = (row, part of the light curve), wave = one epoch at a time (the part's epochs dealt
// round robin to the four waves), lane = one quadrature node.  A lane costs one exponential for the diffusion kernel and
// one (magnetar: none, a division) or two (nickel, cobalt) for the source; the 64 terms are added by a butterfly of
// exchanges in a fixed order, after which every lane holds L(t) and carries the wave's Gaussian sum on.  Everything a
// row brings -- tau_m^-2, the source's amplitude, t_0, the scatter -- is wave-uniform.  Nothing depends on which rows
// are evaluated together and there are no atomics: a row's value is the same bits alone and among any others.
// The engine's own k_prepare (log-prior, lcf_hip.hip) runs in front of the kernel and k_finalize behind it, as for every
// model; rows the prior excludes are skipped.
//
// k_lq_eval is the same evaluation for the luminosity bands (lcf_predict_luminosity; the selection over its keys is in
// lcf_predict.hip): wave = one sample of a chain at a time, its CentralRow built once and kept across the times of a
// tile, lane = one node; the grid is sized to the device and the waves stride over the samples.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lcf_internal.h"
#include "lcf_keys.h"
#include "lcf_plan.h"

namespace {

constexpr int kCentralNodes = 32;        // Gauss-Legendre nodes per piece: two pieces = the 64 lanes of a wave
constexpr double kCentralCut = 40.;      // the range starts where the diffusion kernel is e^-40 of its value at s = t
constexpr double kCentralSplit = 0.125;  // the first piece is this share of the range
// Parts of a light curve (workgroups per row): a wave walks at most 16 epochs up to 256 epochs
constexpr int kCentralOnePart = 64, kCentralFourParts = 256;

// numpy.polynomial.legendre.leggauss(32): nodes, then weights
__constant__ double kGaussLegendre[2 * kCentralNodes] = {
    -0.9972638618494816, -0.9856115115452684, -0.9647622555875064, -0.9349060759377397,
    -0.8963211557660522, -0.84936761373257, -0.7944837959679424, -0.7321821187402897,
    -0.6630442669302152, -0.5877157572407623, -0.5068999089322294, -0.42135127613063533,
    -0.33186860228212767, -0.23928736225213706, -0.1444719615827965, -0.04830766568773831,
    0.04830766568773831, 0.1444719615827965, 0.23928736225213706, 0.33186860228212767,
    0.42135127613063533, 0.5068999089322294, 0.5877157572407623, 0.6630442669302152,
    0.7321821187402897, 0.7944837959679424, 0.84936761373257, 0.8963211557660522,
    0.9349060759377397, 0.9647622555875064, 0.9856115115452684, 0.9972638618494816,
    0.007018610009469298, 0.016274394730905965, 0.025392065309262427, 0.034273862913021626,
    0.042835898022226426, 0.050998059262376244, 0.058684093478535704, 0.06582222277636175,
    0.07234579410884845, 0.07819389578707031, 0.08331192422694685, 0.08765209300440391,
    0.09117387869576386, 0.09384439908080457, 0.09563872007927483, 0.09654008851472781,
    0.09654008851472781, 0.09563872007927483, 0.09384439908080457, 0.09117387869576386,
    0.08765209300440391, 0.08331192422694685, 0.07819389578707031, 0.07234579410884845,
    0.06582222277636175, 0.058684093478535704, 0.050998059262376244, 0.042835898022226426,
    0.034273862913021626, 0.025392065309262427, 0.016274394730905965, 0.007018610009469298};

constexpr double kMsun = 1.988409870698051e33;           // g
constexpr double kEpsNi = 3.9e10, kEpsCo = 6.78e9;       // erg / s / g
constexpr double kTauNi = 8.8, kTauCo = 111.3;           // d
constexpr double kErgPerSecond = 1e-7;                   // W
constexpr double kDay = 86400.;                          // s

// What a row brings, the same in every lane of its waves.
struct CentralRow {
    double amp;        // Arnett: M_Ni Msun [g]; magnetar: E_p 1e51 / (t_p 86400) [erg / s]
    double t_p;        // magnetar: the spin-down time [d]
    double inv_tau2;   // tau_m^-2
    double tau2_cut;   // 40 tau_m^2
    double t_gamma;    // the leakage time [d] (with leakage)
    double t_0;
    bool bad;          // a non-finite parameter, tau_m <= 0, t_p <= 0 or t_gamma <= 0: NaN at every epoch
};

// The source P(s) [W]: the one function a model of this family differs in.
__device__ __forceinline__ double central_source(int model, const CentralRow& r, double s) {
    if (model == LCF_MODEL_MAGNETAR) {
        const double d = 1. + s / r.t_p;
        return r.amp / (d * d) * kErgPerSecond;
    }
    return r.amp * ((kEpsNi - kEpsCo) * exp(-s / kTauNi) + kEpsCo * exp(-s / kTauCo)) * kErgPerSecond;
}

__device__ __forceinline__ CentralRow central_row(int model, bool leak, const double* __restrict__ p) {
    CentralRow r;
    const int at = model == LCF_MODEL_MAGNETAR ? 2 : 1;   // tau_m; then t_gamma (with leakage), then t_0
    const double tau = p[at];
    r.t_p = model == LCF_MODEL_MAGNETAR ? p[1] : 1.;
    r.amp = model == LCF_MODEL_MAGNETAR ? p[0] * 1e51 / (p[1] * kDay) : p[0] * kMsun;
    r.inv_tau2 = 1. / (tau * tau);
    r.tau2_cut = kCentralCut * (tau * tau);
    r.t_gamma = leak ? p[at + 1] : 1.;
    r.t_0 = p[at + (leak ? 2 : 1)];
    const double all = ((p[0] + tau) + (r.t_p + r.t_gamma)) + r.t_0;   // (non-finite if any of them is)
    r.bad = !(fabs(all) < INFINITY) || !(tau > 0.) || !(r.t_p > 0.) || !(r.t_gamma > 0.);
    return r;
}

// Sum over the 64 lanes of a wave, the same number in every lane, in a fixed order (a butterfly of exchanges).
__device__ __forceinline__ double central_wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// L(t) of the row at rest-frame time t, by the wave: `x`, `wgt` = the lane's node and weight, `first` = the lane is in
// the first piece.  The same number in every lane.
__device__ __forceinline__ double central_luminosity(int model, bool leak, const CentralRow& r, double t, double x,
                                                     double wgt, bool first) {
    if (r.bad || t != t) return qnan();
    if (!(t > 0.)) return 0.;
    const double s_lo = sqrt(fmax(0., t * t - r.tau2_cut));
    const double s_mid = s_lo + (t - s_lo) * kCentralSplit;
    const double a = first ? s_lo : s_mid, b = first ? s_mid : t;
    const double h = 0.5 * (b - a), c = 0.5 * (a + b);
    const double s = c + h * x;
    const double g = central_source(model, r, s) * (2. * s * r.inv_tau2) * exp(-((t - s) * (t + s)) * r.inv_tau2) * (h * wgt);
    double L = central_wave_sum(g);
    if (leak) {
        const double q = r.t_gamma / t;
        L *= -expm1(-(q * q));
    }
    return L;
}

// mode 0: chi^2 partial sums -> out0[w][n_parts + 1] (rows the prior excludes are skipped: lprior[w] == -inf);
// mode 1: L(t) -> out0[w - w_lo][point], the caller's order.
// One workgroup of kBlock threads per (row, part): grid = n_w * n_parts, blockIdx.x = part * n_w + (w - w_lo).
__global__ __launch_bounds__(kBlock) void k_central_points(const DevProblem pb, int mode, int w_lo, int n_w,
                                                           const double* __restrict__ P,
                                                           const double* __restrict__ lprior,
                                                           double* __restrict__ out0) {
    __shared__ double red[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int part = blockIdx.x / n_w;
    const int w = w_lo + blockIdx.x % n_w;
    if (part >= pb.n_parts) return;
    if (mode == 0 && lprior[w] == -INFINITY) return;   // (the whole workgroup: no barrier is left waiting)
    const int model = pb.model;
    const bool leak = pb.consts[1] != 0.;
    const double one_plus_z = 1. + pb.consts[0];
    const double* p = P + (size_t)w * pb.n_dim;
    const CentralRow r = central_row(model, leak, p);
    const double x = kGaussLegendre[lane & (kCentralNodes - 1)];
    const double wgt = kGaussLegendre[kCentralNodes + (lane & (kCentralNodes - 1))];
    const bool first = lane < kCentralNodes;
    const size_t row = (size_t)(w - w_lo);
    const int p0 = part_entry(pb.part_start, part), p1 = part_entry(pb.part_start, part + 1);
    double term = 0.;
    for (int i = p0 + wave; i < p1; i += kBlock / 64) {
        const double t = (pb.t[i] - r.t_0) / one_plus_z;
        const double L = central_luminosity(model, leak, r, t, x, wgt, first);
        if (mode == 1) {
            if (lane == 0) out0[row * pb.n_points + i] = L;
            continue;
        }
        const double2 yd = pb.pt_yd[i];   // (y, 1/dy), or (y, dy) when sigma is fitted
        const double d = yd.x - L;
        if (pb.use_sigma) {
            const double dy = yd.y;
            const double su = p[pb.n_dim - 1] * (pb.sigma_abs ? pb.sigma_unit_abs : dy);
            const double var = fma(dy, dy, su * su);
            term += log(kTwoPi * var) + d * d / var;
        } else {
            const double q = d * yd.y;
            term = fma(q, q, term);
        }
    }
    if (mode != 0) return;
    if (lane == 0) red[wave] = term;
    __syncthreads();
    if (tid == 0) out0[(size_t)w * part_stride(pb) + part] = (red[0] + red[1]) + (red[2] + red[3]);
}

// What k_lq_eval reads: sample s is the row at base + (s / n_w) * step_stride + (s % n_w) * ld.
struct LqEval {
    const double* base;
    long long n, n_w, step_stride;
    int ld, ep0, n_ep;
    unsigned long long* keys;   // [n_ep][n]
};

// keys[i][s] = the key of L(t) of sample s at epoch ep0 + i: central_row / central_luminosity in the arithmetic of
// k_central_points mode 1, so the bits are lcf_model_evaluate's.  The wave index goes through readfirstlane: the row's
// address, and with it everything of CentralRow, is then uniform to the compiler as well.
__global__ __launch_bounds__(kBlock) void k_lq_eval(const DevProblem pb, const LqEval a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long n_waves = (long long)gridDim.x * (kBlock / 64);
    const int model = pb.model;
    const bool leak = pb.consts[1] != 0.;
    const double one_plus_z = 1. + pb.consts[0];
    const double x = kGaussLegendre[lane & (kCentralNodes - 1)];
    const double wgt = kGaussLegendre[kCentralNodes + (lane & (kCentralNodes - 1))];
    const bool first = lane < kCentralNodes;
    for (long long s = (long long)blockIdx.x * (kBlock / 64) + wave; s < a.n; s += n_waves) {
        const CentralRow r = central_row(model, leak, a.base + (s / a.n_w) * a.step_stride + (s % a.n_w) * a.ld);
        for (int i = 0; i < a.n_ep; ++i) {
            const double t = (pb.t[a.ep0 + i] - r.t_0) / one_plus_z;
            const double L = central_luminosity(model, leak, r, t, x, wgt, first);
            if (lane == 0) a.keys[(size_t)i * a.n + s] = pq_key(L);
        }
    }
}

const char kRoute[] = "a central-engine model (LCF_MODEL_ARNETT, LCF_MODEL_MAGNETAR) is evaluated by lcf_log_likelihood / "
                      "lcf_log_posterior (and _dev) and lcf_model_evaluate, and sampled through lcf_tempered_* "
                      "(TemperedSampler; one rung at beta = 1 is the ensemble sampler)";

}  // namespace

namespace lcf {

lcf_status central_refuse(const lcf_engine* e, const char* what) {
    if (!e || !is_central(e->dp.model)) return LCF_OK;
    return fail(LCF_ERR_UNSUPPORTED, std::string(what) + " is compiled per photometric model: " + kRoute);
}

lcf_status central_launch(lcf_engine* e, int mode, int w_lo, int n, const double* dP, const double* lprior, double* out0,
                          hipStream_t st) {
    if (n <= 0 || (mode != 0 && e->dp.n_points == 0)) return LCF_OK;   // (mode 0 without epochs: the parts' zeros)
    hipLaunchKernelGGL(k_central_points, dim3((unsigned)((size_t)n * e->dp.n_parts)), dim3(kBlock), 0, st, e->dp, mode,
                       w_lo, n, dP, lprior, out0);
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

lcf_status central_keys_launch(const DevProblem& dp, const ChainView& in, int64_t discard, int64_t thin, int ep0, int n_ep,
                               unsigned long long* keys, int n_cus) {
    const KeptSteps k = kept_steps(in, discard, thin);
    if (k.samples <= 0 || n_ep <= 0) return LCF_OK;
    // eight workgroups of four waves per CU is what the registers allow resident; never more waves than samples
    const long long blocks =
        std::min<long long>((long long)std::max(n_cus, 1) * 8, (k.samples + kBlock / 64 - 1) / (kBlock / 64));
    const LqEval a{k.base, k.samples, in.n_w, k.step_stride, in.ld, ep0, n_ep, keys};
    hipLaunchKernelGGL(k_lq_eval, dim3((unsigned)blocks), dim3(kBlock), 0, 0, dp, a);
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

// lcf_engine_create for the two ids: the epochs stay in the caller's order, in n_parts contiguous ranges.
lcf_status central_engine_create(const lcf_problem* pr, int32_t device, lcf_engine** out) {
    const bool leak = pr->consts[1] != 0.;
    if (pr->n_par != (pr->model == LCF_MODEL_MAGNETAR ? 4 : 3) + (leak ? 1 : 0))
        return fail(LCF_ERR_INVALID_ARGUMENT, "n_par does not match the model (one more parameter with leakage)");
    if (pr->n_filters != 0) return fail(LCF_ERR_INVALID_ARGUMENT, "a central-engine model has no filters: n_filters must be 0");
    if (pr->n_points < 0 || pr->n_points > (1 << 26)) return fail(LCF_ERR_INVALID_ARGUMENT, "bad n_points");
    if (pr->n_points > 0 && (!pr->t || !pr->y || !pr->dy)) return fail(LCF_ERR_INVALID_ARGUMENT, "null light curve");
    if (pr->sigma_type != LCF_SIGMA_RELATIVE && pr->sigma_type != LCF_SIGMA_ABSOLUTE)
        return fail(LCF_ERR_INVALID_ARGUMENT, "sigma_type must be relative or absolute");
    if (!(1. + pr->consts[0] > 0.) || !std::isfinite(pr->consts[0]))
        return fail(LCF_ERR_INVALID_ARGUMENT, "the redshift (consts[0]) must be finite and above -1");
    const int N = (int)pr->n_points;
    const int n_dim = pr->n_par + (pr->use_sigma ? 1 : 0);
    if (lcf_status st = check_prior_kinds(*pr, n_dim)) return st;

    std::unique_ptr<lcf_engine> e;
    if (lcf_status st = engine_shell(device, &e)) return st;

    DevProblem& dp = e->dp;
    dp.model = pr->model;
    dp.n_points = N;
    dp.n_filters = 0;
    dp.n_dim = n_dim;
    dp.n_par = pr->n_par;
    dp.use_sigma = pr->use_sigma ? 1 : 0;
    dp.sigma_abs = pr->sigma_type == LCF_SIGMA_ABSOLUTE;
    dp.has_priors = pr->priors ? 1 : 0;
    dp.variant = 1;
    dp.n_parts = N <= kCentralOnePart ? 1 : N <= kCentralFourParts ? 4 : kMaxParts;
    dp.n_chunks = dp.n_parts;
    dp.cpb = 1;
    for (int j = 0; j <= kMaxParts; ++j) {
        dp.part_start[j] = j < dp.n_parts ? (int)((long long)N * j / dp.n_parts) : N;
        dp.part_ep0[j] = 0;
        dp.part_col0[j] = 0;
    }
    std::memcpy(dp.consts, pr->consts, sizeof(dp.consts));
    noise_constants(pr->dy, N, &dp.log_norm_const, &dp.sigma_unit_abs);
    e->samples_per_eval = (int64_t)N * 2 * kCentralNodes;   // (quadrature nodes of one evaluation)

    std::vector<double> ht(pr->t, pr->t + N), hy(pr->y, pr->y + N), hdy(pr->dy, pr->dy + N), hinv(N);
    std::vector<double2> hyd(N);
    for (int i = 0; i < N; ++i) {
        hinv[i] = 1. / hdy[i];
        hyd[i] = scaled_pair(hy[i], hdy[i], pr->use_sigma);
    }
    const std::vector<PriorDev> hp = prior_rows(*pr, n_dim);
    UploadArena arena(e->owned, (size_t)4096 + (size_t)N * 64);
    lcf_status st = LCF_OK;
    const auto up = [&](const auto& h, auto** d) {
        if (st == LCF_OK) st = put_array(arena, h, d);
    };
    up(ht, &dp.t); up(hy, &dp.y); up(hdy, &dp.dy); up(hinv, &dp.inv_dy); up(hyd, &dp.pt_yd); up(hp, &dp.priors);
    if (st || (st = arena.flush()) || (st = e->sync_dp())) return st;
    *out = e.release();
    return LCF_OK;
}

}  // namespace lcf
