// What the kernels that order or bin the values of a chain share (lcf_corner.hip, lcf_history.hip): the
// order-preserving 64-bit key of a double and the bin of a value among ascending edges.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

namespace lcf {

// doubles ordered as unsigned integers (-inf < ... < -0 < +0 < ... < +inf)
__host__ __device__ __forceinline__ unsigned long long corner_key(unsigned long long b) {
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double corner_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

// The bin of v among the ascending edges e[0 .. bins]: the largest i with e[i] <= v, the last edge belonging to the last
// bin -- np.searchsorted(e, v, 'right') - 1 with e[bins] folded in; NONE (a number no bin has) for a NaN and outside
// [e[0], e[bins]].  The guess is np.histogram's (multiply and truncate); the edge table decides.
template <unsigned int NONE>
__device__ __forceinline__ unsigned int corner_bin(const double* __restrict__ e, int bins, double v) {
    const double lo = e[0], hi = e[bins];
    if (!(v >= lo && v <= hi)) return NONE;
    const double g = (v - lo) * ((double)bins / (hi - lo));
    int i = g >= 0. && g < (double)bins ? (int)g : g >= (double)bins ? bins - 1 : 0;
    while (i > 0 && v < e[i]) --i;
    while (i < bins - 1 && v >= e[i + 1]) ++i;
    return (unsigned int)i;
}

}  // namespace lcf
