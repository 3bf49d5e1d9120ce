// Bolometric light curves on gfx950: the two per-epoch / per-sample loops of the reference's calculate_bolometric that
// have no device code elsewhere in the library.
//
//   k_bb_lstsq  blackbody_lstsq (bolometric.py:483-534): scipy's curve_fit of the monochromatic planck_fast at each
//               filter's freq_eff * (1+z), unweighted, bounded -- here a projected Levenberg-Marquardt with the
//               analytic Jacobian, one problem per epoch -- and curve_fit's covariance at the optimum.
//   k_bb_lum    pseudo (bolometric.py:32-59) and stefan_boltzmann (:422-453) for every posterior sample.
//
// Work decomposition (DESIGN.md "Bolometric light curves"): both kernels give one lane one independent problem.  An
// epoch holds 3-20 points and its solver is a serial loop of ~10-50 iterations, each one pass over the points; a wave
// of 64 epochs runs as long as its slowest epoch, which on a whole light curve is a few microseconds.  A luminosity
// sample is a 580-point trapezoid whose exponentials come from one expm1 recurrence (below); 1e7 samples are 1.6e5
// waves of arithmetic with one 16-byte load and one 16-byte store per lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "lcf.h"
#include "lcf_host.h"

using namespace lcf;

namespace {

constexpr double kBbC1 = 0.0479924307336622;    // h / k_B in kK / THz                       models.py:1101
constexpr double kBbC2 = 281739904251.4432;     // 8 pi^2 h / c^2 in W/Hz / (1000 Rsun)^2 / THz^3   models.py:1102
constexpr double kSigmaSB = 2.744452656619892e+28;   // W (1000 Rsun)^-2 kK^-4          bolometric.py:419
constexpr double kFourPi = 12.566370614359172;
constexpr int kLstsqBlock = 64;
constexpr int kLumBlock = 256;

struct BbPoint {
    double f, dfdT, dfdR;
};

// planck_fast(nu, T, R, cutoff) (models.py:1127-1128) with its T-, R-derivatives.  The reference's power() conventions
// (lcf::pw): 1/T -> 0 for T <= 0, and 1 / (exp(a) - 1) -> 0 where exp(a) - 1 is 0 or overflows.
__device__ __forceinline__ BbPoint bb_point(double nu, double T, double R, double cut) {
    const double K = kBbC2 * nu * nu * nu * fmin(1., cut / nu);
    const double inv_t = T > 0. ? 1. / T : 0.;
    const double a = kBbC1 * (inv_t * nu);
    const double em = expm1(a);
    BbPoint p{0., 0., 0.};
    if (em > 0. && em < INFINITY) {
        const double g = K / em;
        p.f = R * R * g;
        p.dfdR = 2. * R * g;
        // d/dT [1 / (e^a - 1)] = (a / T) e^a / (e^a - 1)^2 = (1 / (e^a - 1)) (a / T) (1 + 1 / (e^a - 1))
        p.dfdT = p.f * (a * inv_t) * (1. + 1. / em);
    }
    return p;
}

// One pass over an epoch's points at x = (T, R): cost = 1/2 sum r^2 of the residuals scaled by s, and the normal
// equations' A = J^T J, g = J^T r (same scale).
struct Pass {
    double cost, a00, a01, a11, g0, g1;
};

__device__ Pass bb_pass(const double* __restrict__ freq, const double* __restrict__ lum, int i0, int i1, double zp1,
                        double cut, double s, double T, double R) {
    Pass p{0., 0., 0., 0., 0., 0.};
    for (int i = i0; i < i1; ++i) {
        const BbPoint q = bb_point(freq[i] * zp1, T, R, cut);
        const double r = s * (q.f - lum[i]), j0 = s * q.dfdT, j1 = s * q.dfdR;
        p.cost = fma(r, r, p.cost);
        p.a00 = fma(j0, j0, p.a00);
        p.a01 = fma(j0, j1, p.a01);
        p.a11 = fma(j1, j1, p.a11);
        p.g0 = fma(j0, r, p.g0);
        p.g1 = fma(j1, r, p.g1);
    }
    p.cost *= 0.5;
    return p;
}

// Projected Levenberg-Marquardt on the box [lo, hi]: a variable at a bound whose gradient points out of the box is held
// there; the other variable(s) take the damped Gauss-Newton step (Marquardt's scaling D = max diag(J^T J) seen so
// far), and the step is projected onto the box.  Damping by Nielsen's gain-ratio rule.  Converged (status 1) when the
// proposed step moves no variable by more than xtol relative -- whether or not it would lower the cost: at the
// floating-point optimum rejected steps shrink until they do -- or (status 2) when the projected gradient is zero.
// Status 0: the iteration cap; -1: an epoch without points, a non-finite input or a non-finite cost.
// out row: T, R, cost, cov_TT, cov_TR, cov_RR, iterations, 0.
__global__ __launch_bounds__(kLstsqBlock) void k_bb_lstsq(long long n_epochs, const int* __restrict__ ep_off,
                                                          const double* __restrict__ freq, const double* __restrict__ lum,
                                                          const double* __restrict__ box, double zp1, double cut,
                                                          int max_iter, double xtol, double* __restrict__ out,
                                                          int* __restrict__ status) {
    const long long e = (long long)blockIdx.x * kLstsqBlock + threadIdx.x;
    if (e >= n_epochs) return;
    const int i0 = ep_off[e], i1 = ep_off[e + 1], m = i1 - i0;
    const double* b = box + 6 * e;   // p0_T, p0_R, lo_T, lo_R, hi_T, hi_R
    const double lo0 = b[2], lo1 = b[3], hi0 = b[4], hi1 = b[5];
    double* o = out + 8 * e;
    double ymax = 0.;
    bool finite = m > 0;
    for (int i = i0; i < i1; ++i) {
        finite = finite && isfinite(lum[i]) && isfinite(freq[i]);
        ymax = fmax(ymax, fabs(lum[i]));
    }
    // (residuals in units of the largest observed value: L_nu ~ 1e20 W/Hz squares to 1e40; the scale cancels in the
    // optimum and in the covariance, and the cost is scaled back below)
    const double s = ymax > 0. && ymax < INFINITY ? 1. / ymax : 1.;
    double T = fmin(fmax(b[0], lo0), hi0), R = fmin(fmax(b[1], lo1), hi1);
    Pass P = bb_pass(freq, lum, i0, i1, zp1, cut, s, T, R);
    int st = finite && isfinite(P.cost) ? 0 : -1;
    double lambda = 1e-3, nu = 2., d0 = P.a00, d1 = P.a11;
    int it = 0;
    for (; st == 0 && it < max_iter; ++it) {
        const bool free0 = !((T <= lo0 && P.g0 > 0.) || (T >= hi0 && P.g0 < 0.));
        const bool free1 = !((R <= lo1 && P.g1 > 0.) || (R >= hi1 && P.g1 < 0.));
        if ((!free0 || P.g0 == 0.) && (!free1 || P.g1 == 0.)) {
            st = 2;
            break;
        }
        d0 = fmax(d0, P.a00);
        d1 = fmax(d1, P.a11);
        const double m00 = fma(lambda, d0, P.a00), m11 = fma(lambda, d1, P.a11);
        double s0 = 0., s1 = 0.;
        if (free0 && free1) {
            const double det = m00 * m11 - P.a01 * P.a01;
            s0 = (P.a01 * P.g1 - m11 * P.g0) / det;
            s1 = (P.a01 * P.g0 - m00 * P.g1) / det;
        } else if (free0) {
            s0 = -P.g0 / m00;
        } else {
            s1 = -P.g1 / m11;
        }
        bool accepted = false;
        if (isfinite(s0) && isfinite(s1)) {
            const double Tn = fmin(fmax(T + s0, lo0), hi0), Rn = fmin(fmax(R + s1, lo1), hi1);
            const double dT = Tn - T, dR = Rn - R;
            if (fabs(dT) <= xtol * fabs(T) && fabs(dR) <= xtol * fabs(R)) {
                st = 1;
                break;
            }
            const Pass Q = bb_pass(freq, lum, i0, i1, zp1, cut, s, Tn, Rn);
            // reduction the linear model predicts for the projected step
            const double pred =
                -(P.g0 * dT + P.g1 * dR) - 0.5 * (P.a00 * dT * dT + 2. * P.a01 * dT * dR + P.a11 * dR * dR);
            if (isfinite(Q.cost) && Q.cost < P.cost) {
                const double rho = pred > 0. ? (P.cost - Q.cost) / pred : 1.;
                const double t = 2. * rho - 1.;
                lambda *= fmax(1. / 3., 1. - t * t * t);
                nu = 2.;
                T = Tn;
                R = Rn;
                P = Q;
                accepted = true;
            }
        }
        if (!accepted) {   // a rejected step, or a singular free block: damp harder
            lambda *= nu;
            nu *= 2.;
        }
        // no step of any length lowers the cost: the optimum to rounding.  (Also where the free block stays singular
        // whatever the damping: J^T J underflowed to 0 under a gradient that did not, and the model is far below the
        // data's last bit.)
        if (!(lambda < 1e300)) {
            st = 1;
            break;
        }
    }
    // curve_fit's covariance: pinv(J^T J) 2 cost / (m - 2) with J = d(model)/d(T, R) at the optimum, the pseudo-inverse
    // through the singular values of J (those <= eps max(m, 2) s_max dropped, scipy's rule).  J = Q [[r00, r01], [0, r11]]
    // by modified Gram-Schmidt over a second pass: J^T J formed directly would square the condition number.
    double c00 = NAN, c01 = NAN, c11 = NAN;
    if (st > 0 && m <= 2) {
        c00 = c01 = c11 = INFINITY;
    } else if (st > 0) {
        const double r00 = sqrt(P.a00);
        const double q = r00 > 0. ? P.a01 / P.a00 : 0.;
        double ss = 0.;
        for (int i = i0; i < i1; ++i) {
            const BbPoint p = bb_point(freq[i] * zp1, T, R, cut);
            const double v = s * p.dfdR - q * (s * p.dfdT);
            ss = fma(v, v, ss);
        }
        const double r01 = r00 > 0. ? P.a01 / r00 : 0., r11 = r00 > 0. ? sqrt(ss) : sqrt(P.a11);
        // singular values of the triangle: s1 s2 = |r00 r11|, s1^2 + s2^2 = r00^2 + r01^2 + r11^2
        const double fro = r00 * r00 + r01 * r01 + r11 * r11, prod = fabs(r00 * r11);
        const double s1 = sqrt(0.5 * (fro + sqrt(fmax(fro * fro - 4. * prod * prod, 0.))));
        const double s2 = s1 > 0. ? prod / s1 : 0.;
        const double scale = 2. * P.cost / (m - 2);
        if (s1 == 0.) {
            c00 = c01 = c11 = 0.;
        } else if (s2 > 2.220446049250313e-16 * fmax(m, 2) * s1) {
            // (R^T R)^-1 = R^-1 R^-T
            const double i00 = 1. / r00, i11 = 1. / r11, i01 = -r01 / (r00 * r11);
            c00 = (i00 * i00 + i01 * i01) * scale;
            c01 = i01 * i11 * scale;
            c11 = i11 * i11 * scale;
        } else {
            // rank one: v v^T / s1^2 with v the leading eigenvector of J^T J = [[a, b], [b, c]]
            const double a = r00 * r00, bb = r00 * r01, c = r01 * r01 + r11 * r11, l1 = s1 * s1;
            double v0 = bb, v1 = l1 - a;
            if (fabs(l1 - c) + fabs(bb) > fabs(v0) + fabs(v1)) v0 = l1 - c, v1 = bb;
            const double nv = sqrt(v0 * v0 + v1 * v1);
            v0 /= nv;
            v1 /= nv;
            c00 = v0 * v0 / l1 * scale;
            c01 = v0 * v1 / l1 * scale;
            c11 = v1 * v1 / l1 * scale;
        }
    }
    o[0] = T;
    o[1] = R;
    o[2] = P.cost / (s * s);
    o[3] = c00;
    o[4] = c01;
    o[5] = c11;
    o[6] = it;
    o[7] = 0.;
    status[e] = st;
}

// pseudo() and stefan_boltzmann() of every sample (T, R): the trapezoid over nu_k = (freq0 + k)(1+z), k < n_grid, of
// planck_fast with the end weights 1/2, times 1e12 (dx = 1 THz).  exp(c1 nu_k / T) - 1 comes from the recurrence
//   E_{k+1} = E_k D + (E_k + D),   E_0 = expm1(c1 nu_0 / T),  D = expm1(c1 (1+z) / T)
// -- expm1 of a sum, every term positive, so no cancellation where c1 nu / T is small and the relative error grows by
// about an ulp per point (NumPy restatement over T = 0.3-300 kK: 2e-14 from the host's pseudo).  E_k = inf (the host's
// exp overflow) gives a zero term, as does 1/T = 0.
__global__ __launch_bounds__(kLumBlock) void k_bb_lum(long long n, const double2* __restrict__ TR, double zp1, double freq0,
                                                      int n_grid, double cut, double2* __restrict__ L) {
    const long long stride = (long long)gridDim.x * kLumBlock;
    for (long long k = (long long)blockIdx.x * kLumBlock + threadIdx.x; k < n; k += stride) {
        const double2 x = TR[k];
        const double T = x.x, R = x.y;
        const double inv_t = T > 0. ? 1. / T : 0.;
        double E = expm1(kBbC1 * (inv_t * (freq0 * zp1)));
        const double D = expm1(kBbC1 * (inv_t * zp1));
        double sum = 0.;
        for (int j = 0; j < n_grid; ++j) {
            const double nu = (freq0 + j) * zp1;
            const double w = (j == 0 || j == n_grid - 1) ? 0.5 : 1.;
            const double K = w * (nu * nu * nu * fmin(1., cut / nu));
            sum += E > 0. && E < INFINITY ? K / E : 0.;
            E = fma(E, D, E + D);
        }
        const double T2 = T * T;
        L[k] = make_double2(kBbC2 * (R * R) * sum * 1e12, kFourPi * (R * R) * kSigmaSB * (T2 * T2));
    }
}

}  // namespace

extern "C" {

lcf_status lcf_bb_lstsq(int32_t device, int64_t n_epochs, const int32_t* ep_off, const double* freq, const double* lum,
                        const double* p0, const double* lo, const double* hi, double z, double cutoff_freq,
                        int32_t max_iter, double xtol, double* out, int32_t* status) {
    if (n_epochs < 0 || !ep_off) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (n_epochs > 0 && (!p0 || !lo || !hi || !out || !status)) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (ep_off[0] != 0) return fail(LCF_ERR_INVALID_ARGUMENT, "ep_off[0] must be 0");
    for (int64_t e = 0; e < n_epochs; ++e)
        if (ep_off[e + 1] < ep_off[e]) return fail(LCF_ERR_INVALID_ARGUMENT, "ep_off must be non-decreasing");
    const int64_t n_pts = ep_off[n_epochs];
    if (n_pts > 0 && (!freq || !lum)) return fail(LCF_ERR_INVALID_ARGUMENT, "null points");
    if (!(z > -1.) || !std::isfinite(z)) return fail(LCF_ERR_INVALID_ARGUMENT, "z must be finite and > -1");
    if (!(cutoff_freq > 0.)) return fail(LCF_ERR_INVALID_ARGUMENT, "cutoff_freq must be > 0");
    if (max_iter < 1 || !(xtol > 0.)) return fail(LCF_ERR_INVALID_ARGUMENT, "max_iter must be >= 1 and xtol > 0");
    std::vector<double> box(6 * std::max<int64_t>(n_epochs, 1));
    for (int64_t e = 0; e < n_epochs; ++e)
        for (int d = 0; d < 2; ++d) {
            const double x = p0[2 * e + d], l = lo[2 * e + d], h = hi[2 * e + d];
            if (!(l < h) || !std::isfinite(x)) return fail(LCF_ERR_INVALID_ARGUMENT, "each bound box needs lo < hi and a finite p0");
            if (x < l || x > h) return fail(LCF_ERR_INVALID_ARGUMENT, "p0 outside the bounds");
            box[6 * e + d] = x;
            box[6 * e + 2 + d] = l;
            box[6 * e + 4 + d] = h;
        }
    lcf_status st = use_device(device);
    if (st != LCF_OK) return st;
    if (n_epochs == 0) return LCF_OK;
    DevBuf b;
    int *doff, *dst;
    double *dfreq, *dlum, *dbox, *dout;
    if ((st = b.alloc(&doff, n_epochs + 1)) || (st = b.alloc(&dfreq, n_pts)) || (st = b.alloc(&dlum, n_pts)) ||
        (st = b.alloc(&dbox, 6 * n_epochs)) || (st = b.alloc(&dout, 8 * n_epochs)) ||
        (st = b.alloc(&dst, n_epochs)))
        return st;
    LCF_HIP(hipMemcpy(doff, ep_off, (n_epochs + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (n_pts) {
        LCF_HIP(hipMemcpy(dfreq, freq, n_pts * sizeof(double), hipMemcpyHostToDevice));
        LCF_HIP(hipMemcpy(dlum, lum, n_pts * sizeof(double), hipMemcpyHostToDevice));
    }
    LCF_HIP(hipMemcpy(dbox, box.data(), 6 * n_epochs * sizeof(double), hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)((n_epochs + kLstsqBlock - 1) / kLstsqBlock);
    hipLaunchKernelGGL(k_bb_lstsq, dim3(grid), dim3(kLstsqBlock), 0, 0, (long long)n_epochs, doff, dfreq, dlum, dbox,
                       1. + z, cutoff_freq, (int)max_iter, xtol, dout, dst);
    LCF_HIP(hipGetLastError());
    LCF_HIP(hipMemcpy(out, dout, 8 * n_epochs * sizeof(double), hipMemcpyDeviceToHost));
    LCF_HIP(hipMemcpy(status, dst, n_epochs * sizeof(int), hipMemcpyDeviceToHost));
    return LCF_OK;
}

lcf_status lcf_bb_luminosity(int32_t device, int64_t n, const double* T, const double* R, double z, double freq0,
                             int32_t n_grid, double cutoff_freq, double* L_pseudo, double* L_bol) {
    if (n < 0 || (n > 0 && (!T || !R || !L_pseudo || !L_bol))) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (!(z > -1.) || !std::isfinite(z)) return fail(LCF_ERR_INVALID_ARGUMENT, "z must be finite and > -1");
    if (!std::isfinite(freq0) || n_grid < 0) return fail(LCF_ERR_INVALID_ARGUMENT, "need a finite freq0 and n_grid >= 0");
    if (!(cutoff_freq > 0.)) return fail(LCF_ERR_INVALID_ARGUMENT, "cutoff_freq must be > 0");
    lcf_status st = use_device(device);
    if (st != LCF_OK) return st;
    if (n == 0) return LCF_OK;
    std::vector<double2> tr(n);
    for (int64_t k = 0; k < n; ++k) tr[k] = make_double2(T[k], R[k]);
    DevBuf b;
    double2 *din, *dout;
    if ((st = b.alloc(&din, n)) || (st = b.alloc(&dout, n))) return st;
    LCF_HIP(hipMemcpy(din, tr.data(), n * sizeof(double2), hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)std::min<int64_t>((n + kLumBlock - 1) / kLumBlock, 256 * 32);
    hipLaunchKernelGGL(k_bb_lum, dim3(grid), dim3(kLumBlock), 0, 0, (long long)n, din, 1. + z, freq0, (int)n_grid,
                       cutoff_freq, dout);
    LCF_HIP(hipGetLastError());
    LCF_HIP(hipMemcpy(tr.data(), dout, n * sizeof(double2), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < n; ++k) {
        L_pseudo[k] = tr[k].x;
        L_bol[k] = tr[k].y;
    }
    return LCF_OK;
}

}  // extern "C"
