// Kernels of a custom model (LCF_MODEL_CUSTOM): a photosphere T(t), R(t) the user wrote, then blackbody_to_filters and
// the Gaussian term.  This text is compiled at run time (lcf_custom.hip: hiprtc) behind lcf_device.h and the user's
// source, which defines, at global scope,
//
//   __device__ void lcf_user_state(double t_in, const double* p, const double* consts, double z,
//                                  double& T_kK, double& R_1000Rsun);
//
// and once by the offline build behind a sample state function, so that the build's resource report shows the kernels
// and a change that breaks this text breaks the build.  It includes nothing and uses only what lcf_device.h and the
// device part of lcf_keys.h define.
//
// lcf_custom_points: work decomposition as k_points', workgroup = (row, part), lane = one data point of the part in the
// engine's stored order.  Every wave holds points of ONE row, in an order only the engine fixes, and every choice it
// makes is made per point -- or, inside band_sum_fast, per wave -- so a row's value never depends on which rows are
// evaluated with it.  lcf_custom_keys (at the end): lane = sample, every choice per lane, for the same reason.
#pragma once

namespace lcf {

#ifdef LCF_DEVPROBLEM_BYTES
static_assert(sizeof(DevProblem) == LCF_DEVPROBLEM_BYTES,
              "the run-time compiler and the library's compiler disagree about DevProblem");
#endif

// Sum over the 64 lanes of a wave, the same number in every lane, in a fixed order (a butterfly of exchanges).
__device__ inline double custom_wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Band-averaged L_nu of the filter's blackbody at (T [kK], R [1000 Rsun]); the special values of the oracle's
// blackbody_to_filters_pointwise: T <= 0 or T >= kTmax gives 0 (times R^2: a NaN radius stays NaN).  A NaN temperature
// gives NaN.  The band sum as k_bb_pointwise takes it: the interpolant of ln S_f(ln T) where ln T is inside the range
// the filter's is proved for, else the shortest sample table valid at T.
__device__ inline double custom_band_luminosity(const DevProblem& pb, int f, double T, double R, const ExpTab et) {
    if (T != T) return T;
    double S = 0.;
    if (T > 0. && T < kTmax) {
        bool done = false;
        if (pb.variant != 0 && pb.use_itab) {
            const double x = (log(T) - pb.itab_u0) * pb.itab_inv_h;
            if (x >= (double)pb.f_desc[f].r_min && x < (double)pb.itab_m) {
                S = exp_scaled<false>(interp_log_band_sum(pb, -1, f, x) * kInvLn2N, et);
                done = true;
            }
        }
        if (!done) {
            const FiltDesc fd = pb.f_desc[f];
            const double invT = inv_temperature(T);
            int off = fd.off, cnt = fd.cnt;
            if (pb.use_ctab && fd.ccnt > 0 && invT <= fd.inv_tmin) off = fd.coff, cnt = fd.ccnt;
            if (pb.use_ctab && fd.hcnt > 0 && invT <= fd.inv_tmin2) off = fd.hoff, cnt = fd.hcnt;
            const double2* tab = pb.tab + off;
            S = pb.variant == 0 ? band_sum_ref(tab, cnt, invT) : band_sum_fast(tab, cnt, invT, et);
        }
    }
    return R * R * S;
}

// custom_band_luminosity where the lanes of a wave are SAMPLES (lcf_custom_keys): the same special values, interpolant
// and tables, but between the two forms of the band sum every lane chooses for itself -- band_sum_fast takes the safe
// form for the whole wave as soon as one lane needs it, and a sample's value must not depend on the samples beside it.
__device__ inline double custom_band_luminosity_lane(const DevProblem& pb, int f, double T, double R, const ExpTab et) {
    if (T != T) return T;
    double S = 0.;
    if (T > 0. && T < kTmax) {
        bool done = false;
        if (pb.variant != 0 && pb.use_itab) {
            const double x = (log(T) - pb.itab_u0) * pb.itab_inv_h;
            if (x >= (double)pb.f_desc[f].r_min && x < (double)pb.itab_m) {
                S = exp_scaled<false>(interp_log_band_sum(pb, -1, f, x) * kInvLn2N, et);
                done = true;
            }
        }
        if (!done) {
            const FiltDesc fd = pb.f_desc[f];
            const double invT = inv_temperature(T);
            int off = fd.off, cnt = fd.cnt;
            if (pb.use_ctab && fd.ccnt > 0 && invT <= fd.inv_tmin) off = fd.coff, cnt = fd.ccnt;
            if (pb.use_ctab && fd.hcnt > 0 && invT <= fd.inv_tmin2) off = fd.hoff, cnt = fd.hcnt;
            const double2* tab = pb.tab + off;
            if (pb.variant == 0) {
                S = band_sum_ref(tab, cnt, invT);
            } else if (cnt > 0) {
                const double amax = fmax(tab[0].x, tab[cnt - 1].x), spos = invT * kInvLn2N;
                S = amax * invT < 170. ? band_sum_main(tab, cnt, spos, et) : band_sum_safe(tab, cnt, -spos, et);
            }
        }
    }
    return R * R * S;
}

// W (1000 Rsun)^-2 kK^-4 and 4 pi: L = 4 pi sigma_SB R^2 T^4 as k_th_pass (lcf_predict.hip) writes it
constexpr double kCustomSigmaSB = 2.744452656619892e+28;
constexpr double kCustomFourPi = 12.566370614359172;

}  // namespace lcf

// mode 0: chi^2 partial sums -> out0[w][n_parts + 1] (rows the prior excludes are skipped: lprior[w] == -inf);
// mode 1: y_fit -> out0[w - w_lo][orig];  mode 2: T, R as the state function gave them -> out0, out1, likewise.
// One workgroup of lcf::kBlock threads per (row, part): grid = n_w * n_parts, blockIdx.x = part * n_w + (w - w_lo).
extern "C" __global__ __launch_bounds__(lcf::kBlock) void lcf_custom_points(const lcf::DevProblem pb, int mode, int w_lo,
                                                                            int n_w, double z,
                                                                            const double* __restrict__ P,
                                                                            const double* __restrict__ lprior,
                                                                            double* __restrict__ out0,
                                                                            double* __restrict__ out1) {
    using namespace lcf;
    __shared__ double exptab[kExpTabSize];
    __shared__ double red[kBlock / 64];
    const int tid = threadIdx.x;
    const int part = blockIdx.x / n_w;
    const int w = w_lo + blockIdx.x % n_w;
    if (part >= pb.n_parts) return;
    if (mode == 0 && lprior[w] == -INFINITY) return;   // (the whole workgroup: no barrier is left waiting)
    for (int k = tid; k < kExpTabSize; k += kBlock) exptab[k] = pb.exp2tab[k];
    __syncthreads();
    const ExpTab et{exptab};
    const double* p = P + (size_t)w * pb.n_dim;
    const size_t row = (size_t)(w - w_lo);
    const int p0 = part_entry(pb.part_start, part), p1 = part_entry(pb.part_start, part + 1);
    double term = 0.;
    for (int i = p0 + tid; i < p1; i += kBlock) {
        double T = 0., R = 0.;
        lcf_user_state(pb.t[i], p, pb.consts, z, T, R);
        if (mode == 2) {
            const size_t j = row * pb.n_points + pb.pt_orig[i];
            out0[j] = T;
            out1[j] = R;
            continue;
        }
        const double yfit = custom_band_luminosity(pb, pb.pt_filt[i], T, R, et);
        if (mode == 1) {
            out0[row * pb.n_points + pb.pt_orig[i]] = yfit;
            continue;
        }
        const double2 yd = pb.pt_yd[i];   // (y, 1/dy), or (y, dy) when sigma is fitted
        const double r = yd.x - yfit;
        if (pb.use_sigma) {               // models.py:121-135
            const double dy = yd.y;
            const double su = p[pb.n_dim - 1] * (pb.sigma_abs ? pb.sigma_unit_abs : dy);
            const double var = fma(dy, dy, su * su);
            term += log(kTwoPi * var) + r * r / var;
        } else {
            const double q = r * yd.y;
            term = fma(q, q, term);
        }
    }
    if (mode != 0) return;
    const double ws = custom_wave_sum(term);
    if ((tid & 63) == 0) red[tid >> 6] = ws;
    __syncthreads();
    if (tid == 0) out0[(size_t)w * part_stride(pb) + part] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The series of lcf_predict_custom, every (sample, time) pair evaluated ONCE: for the distinct times ep0 + i, i < n_ep,
// of the engine and the samples s < n -- sample s is the row at base + (s / n_w) * step_stride + (s % n_w) * ld --
//   keys[(i * (n_filters + 3) + series) * n + s] = pq_key(value),  series = the filters, then T, R and
//   L = 4 pi sigma_SB R^2 T^4, all of ONE call of lcf_user_state.
// With T_floor >= 0 the samples with T < T_floor (a NaN is not, an exact 0 is) are counted into n_cold[ep0 + i].
// lane = sample: the sample's parameters are read once and kept in registers (a state function that indexes p with
// constants), the times are walked inside, and the 64 keys a wave stores per (time, series) are consecutive.
// grid = (ceil(n / kBlock), gy): workgroup (x, y) takes the times i = y, y + gy, ...  No workgroup or wave waits for
// another; the counter is a wave ballot and one integer atomic per wave and time.
extern "C" __global__ __launch_bounds__(lcf::kBlock) void lcf_custom_keys(const lcf::DevProblem pb, double z,
                                                                          const double* __restrict__ base, long long n,
                                                                          long long n_w, long long step_stride, int ld,
                                                                          int ep0, int n_ep, double T_floor,
                                                                          unsigned long long* __restrict__ keys,
                                                                          unsigned long long* __restrict__ n_cold) {
    using namespace lcf;
    __shared__ double exptab[kExpTabSize];
    const int tid = threadIdx.x;
    for (int k = tid; k < kExpTabSize; k += kBlock) exptab[k] = pb.exp2tab[k];
    __syncthreads();
    const ExpTab et{exptab};
    const long long s = (long long)blockIdx.x * kBlock + tid;
    const bool live = s < n;
    const long long sr = live ? s : n - 1;   // (a lane past the end repeats the last sample and stores nothing)
    const double* row = base + (sr / n_w) * step_stride + (sr % n_w) * ld;
    double p[kMaxDim];
#pragma unroll
    for (int d = 0; d < kMaxDim; ++d) p[d] = d < pb.n_par ? row[d] : 0.;
    const int nf = pb.n_filters;
    const size_t per_time = (size_t)(nf + 3) * (size_t)n;
    for (int i = blockIdx.y; i < n_ep; i += gridDim.y) {
        double T = 0., R = 0.;
        lcf_user_state(pb.epoch_t[ep0 + i], p, pb.consts, z, T, R);
        unsigned long long* k = keys + (size_t)i * per_time + (size_t)sr;
        for (int f = 0; f < nf; ++f) {
            const double y = custom_band_luminosity_lane(pb, f, T, R, et);
            if (live) k[(size_t)f * n] = pq_key(y);
        }
        const double T2 = T * T;
        if (live) {
            k[(size_t)nf * n] = pq_key(T);
            k[(size_t)(nf + 1) * n] = pq_key(R);
            k[(size_t)(nf + 2) * n] = pq_key(kCustomFourPi * (R * R) * kCustomSigmaSB * (T2 * T2));
        }
        if (T_floor >= 0.) {
            const unsigned long long cold = __builtin_amdgcn_ballot_w64(live && T < T_floor);
            if ((tid & 63) == 0 && cold) atomicAdd(&n_cold[ep0 + i], (unsigned long long)__popcll(cold));
        }
    }
}
