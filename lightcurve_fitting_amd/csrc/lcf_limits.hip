// Upper limits: non-detections as censored (Tobit) terms of the likelihood (include/lcf.h, "upper limits").
//     ln L(p) = [Gaussian log-likelihood of the detections] + sum_j ln Phi((L_lim,j - m_j(p)) / sigma_j(p))
// The engine holds the detections; a second engine of the caller's, on the limits' (t, filter), gives the model values
// m[row][j] through the points launch of lcf_model_evaluate (limits_model, lcf_hip.hip) behind k_finalize, on the rows'
// coefficients that the likelihood's own k_prepare has just written (the two engines share the model and its constants);
// k_limits, here, turns them into the terms and adds their sum to the row's finished log-likelihood: two launches more
// per likelihood call (three where the limits share epochs: their thermal states).  No existing kernel changes.
//
// k_limits: one wavefront per row, lane l takes the limits l, l + 64, ... in that order, and the 64 partial sums are
// added by a butterfly of exchanges of fixed shape -- the order of the sum depends on n_lim alone, never on the rows in
// the launch: a row's value is the same bits alone and among any others.
//
// ln Phi(z) is evaluated where each form is accurate:
//     z <= 0:  log(erfcx(-z / sqrt 2) / 2) - z^2 / 2     (no underflow: erfcx(u) ~ 1 / (u sqrt pi); -inf once z^2 overflows)
//     z >  0:  log1p(-erfc(z / sqrt 2) / 2)               (no cancellation: the tail itself is the small number)
// The naive log(erfc(-z / sqrt 2) / 2) is -inf from z = -38.5 down and exactly 0 from z = 8.3 up.  At z = 0 both forms
// take the logarithm of a number next to 1/2.  The largest error is the right tail's: erfc(u) changes by the relative
// 2 u^2 eps with the rounding of u = z / sqrt 2, 1.5e-13 at z = 37 (DESIGN.md has the measured figures).
#include <hip/hip_runtime.h>

#include <cmath>

#include "lcf_internal.h"

namespace {

constexpr double kInvSqrt2 = 0.70710678118654752440;
constexpr int64_t kMaxLimits = 1 << 20;
constexpr size_t kLimitScratch = 256u << 20;   // bytes of model values per pass (as lcf_model_evaluate bounds its own)

__device__ inline double log_ndtr(double z) {
    if (z <= 0.) return log(0.5 * erfcx(-z * kInvSqrt2)) - 0.5 * (z * z);
    return log1p(-0.5 * erfc(z * kInvSqrt2));   // (NaN takes this branch and stays NaN)
}

// Rows [row0, row0 + n_rows): m[r][n_lim] are the model values of row row0 + r.  terms (or null): [r][n_lim], likewise;
// dout (or null): the rows' log-likelihoods, to which the sums are added; lprior (or null): rows at -inf are skipped.
__global__ __launch_bounds__(64) void k_limits(int n_rows, int row0, int n_lim, const double* __restrict__ m,
                                               const double* __restrict__ L_lim, const double* __restrict__ dy,
                                               const double* __restrict__ P, int n_dim, int use_sigma, int sigma_abs,
                                               double unit_abs, const double* __restrict__ lprior,
                                               double* __restrict__ terms, double* __restrict__ dout) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= n_rows) return;
    const size_t row = (size_t)row0 + r;
    if (lprior && lprior[row] == -INFINITY) return;   // the prior excludes the row: it stays -inf
    const double s = use_sigma ? P[row * n_dim + (n_dim - 1)] : 0.;
    double sum = 0.;
    for (int j = lane; j < n_lim; j += 64) {
        const double d = dy[j];
        double sigma = d;
        if (use_sigma) {
            const double su = s * (sigma_abs ? unit_abs : d);
            sigma = sqrt(fma(d, d, su * su));
        }
        const double z = (L_lim[j] - m[(size_t)r * n_lim + j]) / sigma;
        const double t = log_ndtr(z);
        if (terms) terms[(size_t)r * n_lim + j] = t;
        sum += t;
    }
    for (int k = 32; k >= 1; k >>= 1) sum += __shfl_xor(sum, k, 64);
    if (dout && lane == 0) dout[row] += sum;
}

const char kRoute[] = "an engine with upper limits attached (lcf_engine_set_limits) is evaluated by lcf_log_likelihood / "
                      "lcf_log_posterior (and _dev) and lcf_limit_terms, and sampled through lcf_tempered_* "
                      "(TemperedSampler; one rung at beta = 1 is the ensemble sampler)";

void launch_limits(lcf_engine* e, int64_t lo, int64_t m, const double* dP, const double* lprior, double* terms,
                   double* dout, hipStream_t st) {
    const DevProblem& pb = e->dp;
    hipLaunchKernelGGL(k_limits, dim3((unsigned)m), dim3(64), 0, st, (int)m, (int)lo, (int)e->n_lim, e->lim_m, e->lim_L,
                       e->lim_dy, dP, pb.n_dim, pb.use_sigma, pb.sigma_abs, pb.sigma_unit_abs, lprior, terms, dout);
}

}  // namespace

// The limit engine's workspace for n rows and the model values of a pass: what the enqueue-only limits_add finds in place.
lcf_status lcf_engine::reserve_limits(int64_t n) {
    if (!lim_at || n <= 0) return LCF_OK;
    if (lcf_status st = lim_at->reserve(n)) return st;
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(n, 64), (int64_t)(kLimitScratch / (n_lim * sizeof(double)))));
    if (per <= lim_rows) return LCF_OK;
    LCF_HIP(hipStreamSynchronize(stream));
    if (lim_m) hipFree(lim_m);
    lim_m = nullptr;
    lim_rows = 0;
    LCF_HIP(hipMalloc((void**)&lim_m, (size_t)per * n_lim * sizeof(double)));
    lim_rows = per;
    return LCF_OK;
}

namespace lcf {

lcf_status limits_refuse(const lcf_engine* e, const char* what) {
    if (!e || !e->lim_at) return LCF_OK;
    return fail(LCF_ERR_UNSUPPORTED, std::string(what) + " computes the likelihood in kernels of its own, which do not know "
                                     "upper limits: " + kRoute);
}

lcf_status limits_add(lcf_engine* e, int64_t n, const double* dP, double* dout, hipStream_t st) {
    if (!e->lim_at || n <= 0) return LCF_OK;
    if (e->lim_rows < 1 || e->lim_at->cap < n)
        return fail(LCF_ERR_STATE, "the workspace of the upper limits was not reserved for this many rows");
    for (int64_t lo = 0; lo < n; lo += e->lim_rows) {
        const int64_t m = std::min(e->lim_rows, n - lo);
        if (lcf_status s = limits_model(e, n, lo, m, dP, false, st)) return s;   // (k_prepare of these rows has run)
        launch_limits(e, lo, m, dP, e->wlprior, nullptr, dout, st);
    }
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

}  // namespace lcf

extern "C" {

lcf_status lcf_engine_set_limits(lcf_engine* e, lcf_engine* at, int64_t n_lim, const double* L_lim, const double* dy) {
    if (!e) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (is_central(e->dp.model))
        return fail(LCF_ERR_UNSUPPORTED, "a central-engine model (Arnett, Magnetar) fits a bolometric table, which has no "
                                         "non-detections: upper limits belong to photometric engines");
    if (lcf_status st = template_refuse(e, "lcf_engine_set_limits")) return st;
    LCF_HIP(hipSetDevice(e->device));
    if (!at || n_lim == 0) {   // detach
        LCF_HIP(hipStreamSynchronize(e->stream));
        e->lim_at = nullptr;
        e->n_lim = 0;
        return LCF_OK;
    }
    if (n_lim < 0 || n_lim > kMaxLimits || !L_lim || !dy)
        return fail(LCF_ERR_INVALID_ARGUMENT, "n_lim must be in [0, 2^20], with L_lim and dy given");
    if (*e->samplers > 0)
        return fail(LCF_ERR_UNSUPPORTED, std::string("a live lcf_sampler uses this engine and computes the likelihood in "
                                                     "kernels of its own, which do not know upper limits: ") + kRoute);
    const DevProblem &a = e->dp, &b = at->dp;
    if (at == e || at->lim_at) return fail(LCF_ERR_INVALID_ARGUMENT, "the limits' engine must be another engine, without limits of its own");
    if (at->device != e->device) return fail(LCF_ERR_INVALID_ARGUMENT, "the limits' engine is on another device");
    if (b.model != a.model || b.n_par != a.n_par || b.use_sigma != a.use_sigma || b.n_dim != a.n_dim)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the limits' engine must have the engine's model, n_par and use_sigma");
    if (std::memcmp(a.consts, b.consts, sizeof(a.consts)) != 0)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the limits' engine must have the engine's constants");
    if ((int64_t)b.n_points != n_lim)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the limits' engine must hold one point per limit");
    for (int64_t j = 0; j < n_lim; ++j)
        if (!std::isfinite(L_lim[j]) || !std::isfinite(dy[j]) || !(dy[j] > 0.))
            return fail(LCF_ERR_INVALID_ARGUMENT, "L_lim and dy must be finite, dy > 0");
    LCF_HIP(hipStreamSynchronize(e->stream));   // (launches in flight read the old limits)
    for (double** p : {&e->lim_L, &e->lim_dy, &e->lim_m}) {
        if (*p) hipFree(*p);
        *p = nullptr;
    }
    e->lim_rows = 0;
    e->lim_at = nullptr;
    e->n_lim = 0;
    LCF_HIP(hipMalloc((void**)&e->lim_L, n_lim * sizeof(double)));
    LCF_HIP(hipMalloc((void**)&e->lim_dy, n_lim * sizeof(double)));
    LCF_HIP(hipMemcpy(e->lim_L, L_lim, n_lim * sizeof(double), hipMemcpyHostToDevice));
    LCF_HIP(hipMemcpy(e->lim_dy, dy, n_lim * sizeof(double), hipMemcpyHostToDevice));
    e->lim_at = at;
    e->n_lim = n_lim;
    // (callers that reserved before the limits came -- a tempered driver -- find the workspace in place)
    return e->reserve_limits(std::max<int64_t>(e->cap, 64));
}

lcf_status lcf_limit_terms(lcf_engine* e, int64_t n, const double* P, double* out) {
    if (!e || n < 0 || (n > 0 && (!P || !out))) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (!e->lim_at) return fail(LCF_ERR_STATE, "the engine has no upper limits: call lcf_engine_set_limits first");
    if (n == 0) return LCF_OK;
    if (n > (1 << 22)) return fail(LCF_ERR_INVALID_ARGUMENT, "at most 2^22 rows per call");
    LCF_HIP(hipSetDevice(e->device));
    if (lcf_status st = e->reserve(n)) return st;
    const size_t nl = (size_t)e->n_lim;
    if (lcf_status st = e->reserve_big((size_t)e->lim_rows * nl * sizeof(double))) return st;
    LCF_HIP(hipMemcpyAsync(e->wP, P, n * e->dp.n_dim * sizeof(double), hipMemcpyHostToDevice, e->stream));
    for (int64_t lo = 0; lo < n; lo += e->lim_rows) {
        const int64_t m = std::min(e->lim_rows, n - lo);
        if (lcf_status st = limits_model(e, n, lo, m, e->wP, lo == 0, e->stream)) return st;
        launch_limits(e, lo, m, e->wP, nullptr, e->wbig, nullptr, e->stream);
        LCF_HIP(hipGetLastError());
        LCF_HIP(hipMemcpyAsync(out + (size_t)lo * nl, e->wbig, (size_t)m * nl * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        LCF_HIP(hipStreamSynchronize(e->stream));
    }
    return LCF_OK;
}

}  // extern "C"
