// Second component: a stretched, per-filter template added to the engine's model (include/lcf.h, "second component").
//     tau_j  = r_f S_f((t_j - t_max - dt_f) / s),   m_j(p) = base_j(p_base) + tau_j,   f = the filter of point j
//     ln L(p) = -1/2 sum_j [ln(2 pi sigma_j^2) + ((y_j - m_j) / sigma_j)^2]
// S_f is a piecewise cubic on the template's knots (lcf::spline_eval: 0 outside them and for a NaN argument), t_max and s
// are two columns of the row behind the base model's, r_f and dt_f further columns for the filters that have them (1 and
// 0 for the others), sigma stays the last column.  What BaseCompanionShocking does with the SiFTO template, for any
// photometric engine and any template.
//
// The likelihood of such an engine is three launches (logprob_dev, lcf_hip.hip): k_prepare as for every engine, the
// engine's own mode-1 points launch -- the launches of lcf_model_evaluate -- into scratch [rows][n_points], and
// k_template, here, which adds the template to the model values and sums.  No existing kernel changes: the engine's
// n_dim grows by the extra columns, which k_prepare, walker_coefficients and walker_log_prior tolerate (they stride by
// n_dim, read p[0 .. n_par) and take the priors of all n_dim columns).
//
// k_template: one wavefront per row, lane l takes the points l, l + 64, ... of the caller's order, and the 64 partial
// sums are added by a butterfly of exchanges of fixed shape -- the order of the sum depends on n_points alone: a row's
// value is the same bits alone and among any others.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lcf_internal.h"
#include "lcf_template.h"

namespace {

constexpr size_t kTemplateScratch = 256u << 20;   // bytes of model values per pass (as lcf_model_evaluate bounds its own)
constexpr int kMaxKnots = 1 << 16;

// (What k_template reads about the engine, by value: TemplateDev / template_dev, lcf_template.h.)

enum { kLogLike = 0, kTotal = LCF_TEMPLATE_TOTAL, kBase = LCF_TEMPLATE_BASE, kTemplate = LCF_TEMPLATE_TEMPLATE };

// Rows [row0, row0 + n_rows): m[r][n_points] holds the base model's values of row row0 + r.
// mode kLogLike: dout[row] = lprior[row] - sum / 2 (lprior is 0 for a likelihood; a row at -inf stays -inf, unread);
// mode kTotal / kBase / kTemplate: the component replaces m[r][.] in place.
__global__ __launch_bounds__(64) void k_template(const TemplateDev a, int n_rows, int row0, int mode,
                                                 const double* __restrict__ P, const double* __restrict__ lprior,
                                                 double* __restrict__ m, double* __restrict__ dout) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= n_rows) return;
    const size_t row = (size_t)row0 + r;
    if (mode == kLogLike && lprior[row] == -INFINITY) {   // the prior excludes the row
        if (lane == 0) dout[row] = -INFINITY;
        return;
    }
    if (mode == kBase) return;
    const double* p = P + row * a.n_dim;
    const double t_max = p[a.i_tmax];
    const double inv_s = 1. / p[a.i_s];   // (the built-in companion kernels: (t - t_max - dt) * (1 / s))
    const double s = a.use_sigma ? p[a.n_dim - 1] : 0.;
    const size_t spl = (size_t)(a.n_knots - 1) * 4;
    double* mr = m + (size_t)r * a.n_points;
    double sum = 0.;
    for (int j = lane; j < a.n_points; j += 64) {
        const int f = a.filt[j];
        const int fp = a.fac[f], op = a.off[f];
        const double fac = fp >= 0 ? p[fp] : 1.;
        const double dt = op >= 0 ? p[op] : 0.;
        const double x = (a.t[j] - t_max - dt) * inv_s;
        const double tau = fac * lcf::spline_eval(a.knots, a.n_knots, a.coef + f * spl, x, a.inv_h);
        if (mode == kTemplate) {
            mr[j] = tau;
            continue;
        }
        const double mj = mr[j] + tau;
        if (mode == kTotal) {
            mr[j] = mj;
            continue;
        }
        const double d = a.dy[j];
        const double res = a.y[j] - mj;
        if (a.use_sigma) {                // models.py:121-135
            const double su = s * (a.sigma_abs ? a.unit_abs : d);
            const double var = fma(d, d, su * su);
            sum += log(kTwoPi * var) + res * res / var;
        } else {
            const double q = res / d;
            sum = fma(q, q, sum);
        }
    }
    if (mode != kLogLike) return;
    for (int k = 32; k >= 1; k >>= 1) sum += __shfl_xor(sum, k, 64);
    if (lane == 0) dout[row] = lprior[row] - 0.5 * (a.use_sigma ? sum : a.log_norm_const + sum);
}

const char kRoute[] = "an engine with a second component attached (lcf_engine_set_template) is evaluated by "
                      "lcf_log_likelihood / lcf_log_posterior (and _dev) and lcf_template_evaluate, and sampled through "
                      "lcf_tempered_* (TemperedSampler; one rung at beta = 1 is the ensemble sampler)";

void launch_template(const lcf_engine* e, int64_t lo, int64_t m, int mode, const double* dP, const double* lprior,
                     double* values, double* dout, hipStream_t st) {
    hipLaunchKernelGGL(k_template, dim3((unsigned)m), dim3(64), 0, st, template_dev(e), (int)m, (int)lo, mode, dP, lprior,
                       values, dout);
}

// rows of model values a pass holds: all n, at most kTemplateScratch bytes
int64_t rows_per_pass(const lcf_engine* e, int64_t n) {
    const size_t row_bytes = std::max<size_t>(1, (size_t)e->dp.n_points) * sizeof(double);
    return std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(n, 64), (int64_t)(kTemplateScratch / row_bytes)));
}

template <class T>
lcf_status upload(T** dst, const T* src, size_t n) {
    LCF_HIP(hipMalloc((void**)dst, std::max<size_t>(n, 1) * sizeof(T)));
    if (n) LCF_HIP(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return LCF_OK;
}

// The engine as it was created: its own n_dim and priors, no template.
lcf_status detach(lcf_engine* e) {
    if (!e->tpl) return LCF_OK;
    LCF_HIP(hipStreamSynchronize(e->stream));
    e->tpl = false;
    e->dp.n_dim = e->base_n_dim;
    e->dp.priors = e->base_priors;
    e->dp.has_priors = e->base_has_priors;
    e->free_template();
    e->free_ws();   // (the workspace holds rows of the other width)
    return e->sync_dp();
}

}  // namespace

// The model values of a pass: what the enqueue-only template_loglike finds in place.
lcf_status lcf_engine::reserve_template(int64_t n) {
    if (!tpl || n <= 0) return LCF_OK;
    const int64_t per = rows_per_pass(this, n);
    if (per <= tpl_rows) return LCF_OK;
    LCF_HIP(hipStreamSynchronize(stream));
    if (tpl_m) hipFree(tpl_m);
    tpl_m = nullptr;
    tpl_rows = 0;
    LCF_HIP(hipMalloc((void**)&tpl_m, (size_t)per * std::max(dp.n_points, 1) * sizeof(double)));
    tpl_rows = per;
    return LCF_OK;
}

namespace lcf {

lcf_status template_refuse(const lcf_engine* e, const char* what) {
    if (!e || !e->tpl) return LCF_OK;
    return fail(LCF_ERR_UNSUPPORTED, std::string(what) + " computes the likelihood in kernels of its own, which do not know "
                                     "a second component: " + kRoute);
}

lcf_status template_loglike(lcf_engine* e, int64_t n, const double* dP, double* dout, hipStream_t st) {
    if (n <= 0) return LCF_OK;
    if (e->dp.model == LCF_MODEL_CUSTOM)
        if (lcf_status s = custom_ready(e)) return s;
    if (e->tpl_rows < 1 || e->cap < n)
        return fail(LCF_ERR_STATE, "the workspace of the second component was not reserved for this many rows");
    for (int64_t lo = 0; lo < n; lo += e->tpl_rows) {
        const int64_t m = std::min(e->tpl_rows, n - lo);
        if (lcf_status s = template_model(e, lo, m, dP, e->tpl_m, st)) return s;   // (k_prepare of these rows has run)
        launch_template(e, lo, m, kLogLike, dP, e->wlprior, e->tpl_m, dout, st);
    }
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

}  // namespace lcf

extern "C" {

lcf_status lcf_engine_set_template(lcf_engine* e, int32_t n_knots, const double* knots, const double* coef,
                                   const int32_t* filt_factor_par, const int32_t* filt_offset_par, int32_t tmax_par,
                                   int32_t s_par, int32_t n_extra, const lcf_prior* priors) {
    if (!e) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (is_central(e->dp.model))
        return fail(LCF_ERR_UNSUPPORTED, "a central-engine model (Arnett, Magnetar) fits a bolometric table, which has no "
                                         "filters: a second component belongs to photometric engines");
    if (e->dp.model >= kCompanion && e->dp.model <= kCompanion3)
        return fail(LCF_ERR_UNSUPPORTED, "a companion-shocking model has a template of its own (SiFTO): a second component "
                                         "belongs to the shock-cooling models and custom models");
    LCF_HIP(hipSetDevice(e->device));
    if (!knots || n_knots == 0) return detach(e);
    if (*e->samplers > 0)
        return fail(LCF_ERR_UNSUPPORTED, std::string("a live lcf_sampler uses this engine and computes the likelihood in "
                                                     "kernels of its own, which do not know a second component: ") + kRoute);
    if (e->lim_at)
        return fail(LCF_ERR_UNSUPPORTED, "upper limits together with a second component are out of scope: detach the limits "
                                         "(lcf_engine_set_limits) first");
    const DevProblem& pb = e->dp;
    const int base_dim = e->tpl ? e->base_n_dim : pb.n_dim;
    const int n_dim = base_dim + n_extra;
    const int first = pb.n_par, last = pb.n_par + n_extra;   // the extra columns: behind the model's, in front of sigma
    if (n_knots < 4 || n_knots > kMaxKnots || !coef || !filt_factor_par || !filt_offset_par)
        return fail(LCF_ERR_INVALID_ARGUMENT, "a template needs 4 to 65536 knots, its coefficients and the filters' columns");
    if (n_extra < 2 || n_dim > kMaxDim)
        return fail(LCF_ERR_INVALID_ARGUMENT, "n_extra must be at least 2 (t_max and s), and the row at most 16 columns");
    if (tmax_par < first || tmax_par >= last || s_par < first || s_par >= last || tmax_par == s_par)
        return fail(LCF_ERR_INVALID_ARGUMENT, "t_max and s must be two of the extra columns");
    for (int k = 0; k < n_knots; ++k)
        if (!std::isfinite(knots[k]) || (k > 0 && !(knots[k] > knots[k - 1])))
            return fail(LCF_ERR_INVALID_ARGUMENT, "the knots must be finite and strictly increasing");
    const size_t n_coef = (size_t)pb.n_filters * (n_knots - 1) * 4;
    for (size_t k = 0; k < n_coef; ++k)
        if (!std::isfinite(coef[k])) return fail(LCF_ERR_INVALID_ARGUMENT, "the template's coefficients must be finite");
    for (int f = 0; f < pb.n_filters; ++f)
        for (int v : {filt_factor_par[f], filt_offset_par[f]})
            if (v != -1 && (v < first || v >= last || v == tmax_par || v == s_par))
                return fail(LCF_ERR_INVALID_ARGUMENT, "a filter's factor or offset must be -1 or one of the extra columns");
    std::vector<PriorDev> rows(priors ? n_dim : 0);
    for (int i = 0; priors && i < n_dim; ++i) {
        if (priors[i].kind < 0 || priors[i].kind > 2) return fail(LCF_ERR_INVALID_ARGUMENT, "bad prior kind");
        rows[i] = PriorDev{priors[i].kind, 0, priors[i].p_min, priors[i].p_max, priors[i].mean, priors[i].stddev};
    }
    // equally spaced knots (to 1e-9 of the spacing): spline_eval computes the interval and corrects it against the knots
    const double h = (knots[n_knots - 1] - knots[0]) / (n_knots - 1);
    bool uniform = true;
    for (int k = 0; k < n_knots; ++k) uniform = uniform && std::fabs(knots[k] - (knots[0] + k * h)) <= 1e-9 * h;

    // the photometry in the caller's order, from the engine's own (ordered by part and filter; pt_orig says where from)
    const size_t N = (size_t)pb.n_points;
    std::vector<double> st(N), sy(N), sdy(N), ct(N), cy(N), cdy(N);
    std::vector<int> sf(N), so(N), cf(N);
    LCF_HIP(hipStreamSynchronize(e->stream));   // (launches in flight read the old template)
    if (N) {
        LCF_HIP(hipMemcpy(st.data(), pb.t, N * sizeof(double), hipMemcpyDeviceToHost));
        LCF_HIP(hipMemcpy(sy.data(), pb.y, N * sizeof(double), hipMemcpyDeviceToHost));
        LCF_HIP(hipMemcpy(sdy.data(), pb.dy, N * sizeof(double), hipMemcpyDeviceToHost));
        LCF_HIP(hipMemcpy(sf.data(), pb.pt_filt, N * sizeof(int), hipMemcpyDeviceToHost));
        LCF_HIP(hipMemcpy(so.data(), pb.pt_orig, N * sizeof(int), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < N; ++i) {
        const int o = so[i];
        if (o < 0 || (size_t)o >= N || sf[i] < 0 || sf[i] >= pb.n_filters)
            return fail(LCF_ERR_STATE, "the engine's point order is inconsistent");
        ct[o] = st[i], cy[o] = sy[i], cdy[o] = sdy[i], cf[o] = sf[i];
    }
    if (!e->tpl) {
        e->base_n_dim = pb.n_dim;
        e->base_priors = pb.priors;
        e->base_has_priors = pb.has_priors;
    }
    e->tpl = false;
    e->free_template();
    lcf_status r = LCF_OK;
    if ((r = upload(&e->tpl_knots, knots, (size_t)n_knots)) || (r = upload(&e->tpl_coef, coef, n_coef)) ||
        (r = upload(&e->tpl_t, ct.data(), N)) || (r = upload(&e->tpl_y, cy.data(), N)) ||
        (r = upload(&e->tpl_dy, cdy.data(), N)) || (r = upload(&e->tpl_filt, cf.data(), N)) ||
        (r = upload(&e->tpl_fac, filt_factor_par, (size_t)pb.n_filters)) ||
        (r = upload(&e->tpl_off, filt_offset_par, (size_t)pb.n_filters)) ||
        (r = upload(&e->tpl_priors, rows.data(), rows.size()))) {
        e->free_template();
        e->dp.n_dim = e->base_n_dim, e->dp.priors = e->base_priors, e->dp.has_priors = e->base_has_priors;
        e->free_ws();
        e->sync_dp();
        return r;
    }
    e->tpl_nk = n_knots;
    e->tpl_extra = n_extra;
    e->tpl_tmax = tmax_par;
    e->tpl_s = s_par;
    e->tpl_inv_h = uniform ? 1. / h : 0.;
    e->dp.n_dim = n_dim;
    e->dp.priors = priors ? e->tpl_priors : nullptr;
    e->dp.has_priors = priors ? 1 : 0;
    e->tpl = true;
    const int64_t had = e->cap;
    e->free_ws();   // (the workspace held rows of the old width)
    if (lcf_status s = e->sync_dp()) return s;
    // (callers that reserved before the template came find the workspace in place)
    return e->reserve(std::max<int64_t>(had, 64));
}

lcf_status lcf_template_evaluate(lcf_engine* e, int64_t n, const double* P, int32_t component, double* out) {
    if (!e || n < 0 || (n > 0 && (!P || !out))) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (!e->tpl) return fail(LCF_ERR_STATE, "the engine has no second component: call lcf_engine_set_template first");
    if (component != LCF_TEMPLATE_TOTAL && component != LCF_TEMPLATE_BASE && component != LCF_TEMPLATE_TEMPLATE)
        return fail(LCF_ERR_INVALID_ARGUMENT, "component must be LCF_TEMPLATE_TOTAL, _BASE or _TEMPLATE");
    if (n == 0 || e->dp.n_points == 0) return LCF_OK;
    if (n > (1 << 22)) return fail(LCF_ERR_INVALID_ARGUMENT, "at most 2^22 rows per call");
    if (e->dp.model == LCF_MODEL_CUSTOM)
        if (lcf_status st = custom_ready(e)) return st;
    LCF_HIP(hipSetDevice(e->device));
    if (lcf_status st = e->reserve(n)) return st;
    const size_t N = (size_t)e->dp.n_points;
    LCF_HIP(hipMemcpyAsync(e->wP, P, n * e->dp.n_dim * sizeof(double), hipMemcpyHostToDevice, e->stream));
    if (lcf_status st = prepare_rows(e, n, e->wP, e->stream)) return st;
    for (int64_t lo = 0; lo < n; lo += e->tpl_rows) {
        const int64_t m = std::min(e->tpl_rows, n - lo);
        if (lcf_status st = template_model(e, lo, m, e->wP, e->tpl_m, e->stream)) return st;
        launch_template(e, lo, m, component, e->wP, e->wlprior, e->tpl_m, nullptr, e->stream);
        LCF_HIP(hipGetLastError());
        LCF_HIP(hipMemcpyAsync(out + (size_t)lo * N, e->tpl_m, (size_t)m * N * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        LCF_HIP(hipStreamSynchronize(e->stream));
    }
    return LCF_OK;
}

}  // extern "C"
