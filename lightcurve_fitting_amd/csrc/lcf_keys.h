// What the luminosity form of the predictive quantiles (lcf_predict_luminosity) shares between its two translation
// units: lcf_central.hip evaluates L(t) of every (sample, time) pair of a tile ONCE into an order-preserving key
// (k_lq_eval, beside k_central_points and its quadrature), lcf_predict.hip runs the radix selection and the peak walk
// over the stored keys (k_kq_pass, k_lq_peak, quantile_run).
#pragma once
#include <hip/hip_runtime.h>

#include "lcf_host.h"

namespace lcf {

struct DevProblem;

// doubles ordered as unsigned integers (-inf < ... < -0 < +0 < ... < +inf); pq_value is the inverse, NaNs included
__device__ __forceinline__ unsigned long long pq_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double pq_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// lcf_central.hip: keys[i * n + s] = pq_key(L of sample s at epoch ep0 + i of `dp`), i < n_ep, on the null stream; the
// n samples are the walkers of the kept steps of `in`.  n_cus sizes the grid.
lcf_status central_keys_launch(const DevProblem& dp, const ChainView& in, int64_t discard, int64_t thin, int ep0, int n_ep,
                               unsigned long long* keys, int n_cus);

}  // namespace lcf
