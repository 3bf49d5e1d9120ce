// Kernels of a custom model (LCF_MODEL_CUSTOM): a photosphere T(t), R(t) the user wrote, then blackbody_to_filters and
// the Gaussian term.  This text is compiled at run time (lcf_custom.hip: hiprtc) behind lcf_device.h and the user's
// source, which defines, at global scope,
//
//   __device__ void lcf_user_state(double t_in, const double* p, const double* consts, double z,
//                                  double& T_kK, double& R_1000Rsun);
//
// and once by the offline build behind a sample state function, so that the build's resource report shows the kernel
// and a change that breaks this text breaks the build.  It includes nothing and uses only what lcf_device.h defines.
//
// Work decomposition as k_points': workgroup = (row, part), lane = one data point of the part in the engine's stored
// order.  Every wave holds points of ONE row, in an order only the engine fixes, and every choice below is made per
// point -- or, inside band_sum_fast, per wave -- so a row's value never depends on which rows are evaluated with it.
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
