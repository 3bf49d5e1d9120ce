// What the stored-key forms of the predictive quantiles (lcf_predict_luminosity, lcf_predict_custom) share between their
// translation units: lcf_central.hip evaluates L(t) of every (sample, time) pair of a tile ONCE into an order-preserving
// key (k_lq_eval, beside k_central_points and its quadrature), a custom model's program does the same for its light
// curves, T, R and L (lcf_custom_keys, lcf_custom_kernel.h), and lcf_predict.hip runs the radix selection and the peak
// walk over the stored keys (k_kq_pass, k_lq_peak, quantile_run).
//
// The key encoding is compiled at run time too, behind a custom model's source (lcf_custom.hip: this header is part of
// the program text, as lcf_device.h is): the run-time compiler sees the device part alone.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>

#include "lcf_host.h"
#endif

namespace lcf {

// doubles ordered as unsigned integers (-inf < ... < -0 < +0 < ... < +inf); pq_value is the inverse, NaNs included
__device__ __forceinline__ unsigned long long pq_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double pq_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

}  // namespace lcf

#ifndef __HIPCC_RTC__
namespace lcf {

struct DevProblem;

// lcf_central.hip: keys[i * n + s] = pq_key(L of sample s at epoch ep0 + i of `dp`), i < n_ep, on the null stream; the
// n samples are the walkers of the kept steps of `in`.  n_cus sizes the grid.
lcf_status central_keys_launch(const DevProblem& dp, const ChainView& in, int64_t discard, int64_t thin, int ep0, int n_ep,
                               unsigned long long* keys, int n_cus);

// lcf_custom.hip: the program's lcf_custom_keys on the null stream -- for the distinct times ep0 ... ep0 + n_ep - 1 of the
// engine, keys[(i * (n_filters + 3) + series) * n + s] of sample s, series = the filters, then T, R, L; with
// T_floor >= 0 the samples with T < T_floor are added to n_cold[ep0 + i].  Samples as above.
lcf_status custom_keys_launch(lcf_engine* e, const ChainView& in, int64_t discard, int64_t thin, int ep0, int n_ep,
                              double T_floor, unsigned long long* keys, unsigned long long* n_cold);

}  // namespace lcf
#endif
