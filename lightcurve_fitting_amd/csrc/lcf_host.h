// Host-side helpers shared by the translation units of liblcf_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "lcf.h"

namespace lcf {

extern thread_local std::string g_err;
lcf_status fail(lcf_status st, const std::string& msg);

#define LCF_HIP(call)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return lcf::fail(e_ == hipErrorOutOfMemory ? LCF_ERR_OUT_OF_MEMORY : LCF_ERR_HIP,              \
                             std::string(#call) + ": " + hipGetErrorString(e_));                           \
    } while (0)

// Every launch with dynamic LDS is prepared here, on the device it goes to.  More than the default 64 KiB must be granted
// per kernel function and device: it is, once (again only should a later launch of the function ask for more -- what
// the launch asks for, not the CU's whole LDS: the kernel may hold static words of its own).  `per_cu`: the workgroups
// of `threads` threads with that LDS one CU holds, asked once per (device, function, threads, LDS bytes).
inline hipError_t prepare_kernel(const void* kernel, size_t lds, int threads = 0, int* per_cu = nullptr) {
    if (lds <= 64 * 1024 && !per_cu) return hipSuccess;
    static std::mutex mutex;
    static std::map<std::pair<int, const void*>, size_t> granted;
    static std::map<std::tuple<int, const void*, int, size_t>, int> occupancy;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    std::lock_guard<std::mutex> lock(mutex);
    if (lds > 64 * 1024) {
        size_t& g = granted[{dev, kernel}];
        if (lds > g) {
            if (hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
            g = lds;
        }
    }
    if (!per_cu) return hipSuccess;
    const auto key = std::make_tuple(dev, kernel, threads, lds);
    auto it = occupancy.find(key);
    if (it == occupancy.end()) {
        int n = 0;
        if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, lds)) return e;
        it = occupancy.emplace(key, n).first;
    }
    *per_cu = it->second;
    return hipSuccess;
}
template <class... A>
hipError_t prepare_kernel(void (*kernel)(A...), size_t lds, int threads = 0, int* per_cu = nullptr) {
    return prepare_kernel(reinterpret_cast<const void*>(kernel), lds, threads, per_cu);
}

template <class T>
lcf_status upload(const std::vector<T>& h, T** d, std::vector<void*>& owned) {
    *d = nullptr;
    if (h.empty()) return LCF_OK;
    LCF_HIP(hipMalloc((void**)d, h.size() * sizeof(T)));
    owned.push_back(*d);
    LCF_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return LCF_OK;
}

// The immutable arrays of an engine go to the device as ONE block with ONE copy: every array of lcf_engine_create used to
// be an allocation and a host-to-device copy of its own (about forty per engine -- 1475 copy kernels in the profile of a
// population of 32 transients).  put() hands out the array's place in the block at once (callers store the pointer in
// the problem) and keeps the bytes in a host image of the block; flush() sends the image.  A block that is full is
// followed by another one.
struct UploadArena {
    std::vector<void*>& owned;   // the device blocks end up here (freed with the engine)
    struct Block { char* dev; std::vector<char> host; size_t used; };
    std::vector<Block> blocks;
    size_t block_bytes;
    explicit UploadArena(std::vector<void*>& o, size_t first_block = 1 << 20) : owned(o), block_bytes(first_block) {}
    lcf_status put(const void* src, size_t bytes, void** dst) {
        *dst = nullptr;
        if (bytes == 0) return LCF_OK;
        const size_t need = (bytes + 255) & ~size_t(255);
        if (blocks.empty() || blocks.back().used + need > blocks.back().host.size()) {
            const size_t cap = std::max(block_bytes, need);
            char* dev = nullptr;
            LCF_HIP(hipMalloc((void**)&dev, cap));
            owned.push_back(dev);
            blocks.push_back(Block{dev, std::vector<char>(cap), 0});
        }
        Block& b = blocks.back();
        std::memcpy(b.host.data() + b.used, src, bytes);
        *dst = b.dev + b.used;
        b.used += need;
        return LCF_OK;
    }
    lcf_status flush() {   // (complete on return)
        for (Block& b : blocks)
            if (b.used) LCF_HIP(hipMemcpy(b.dev, b.host.data(), b.used, hipMemcpyHostToDevice));
        blocks.clear();
        return LCF_OK;
    }
};

template <class T>
lcf_status upload(const std::vector<T>& h, T** d, UploadArena& arena) {
    return arena.put(h.data(), h.size() * sizeof(T), (void**)d);
}

// Autocorrelation time (lcf_autocorr.hip): one series per walker and parameter; element t of series (w, d) at
// chain[t * row_stride + w * n_d + d] in device memory.  tau / window receive n_d entries per entry of `in`, in order.
struct AutocorrSeries {
    const double* chain;
    int64_t n_t, row_stride;
    int32_t n_w, n_d;
};
lcf_status autocorr_run(int32_t device, const AutocorrSeries* in, int32_t n, double c, double* tau, int64_t* window);

// Posterior-predictive quantiles (lcf_predict.hip): n samples in device memory, sample s being the ld-strided row at
// base + (s / n_w) * step_stride + (s % n_w) * ld (a stored chain read in place: n_w walkers per kept step).
struct DevProblem;
struct PredictSamples {
    const double* base;
    int64_t n, n_w, step_stride;
    int32_t ld;
};
// `dp`: the engine of the grid points; orig[n_epochs][n_filters] (host): the index of the point (time, filter) in the
// caller's order, -1 where the grid has no such point.  out[n_q][n_points], n_valid[n_points] (host).
lcf_status predict_run(int32_t device, const DevProblem& dp, const PredictSamples& in, const int32_t* orig,
                       int32_t component, const double* q, int32_t n_q, int64_t workspace_bytes, double* out,
                       int64_t* n_valid);
// Thermal form: quantiles of T, R_bb, L_bol and the validity counters on the distinct times of `dp`; time_orig
// [n_epochs] (host): the time's index in the caller's order.  out[3][n_q][n_epochs], n_valid[3][n_epochs],
// n_cold[n_epochs], n_inside[n_epochs] (host, caller's order).
lcf_status predict_thermal_run(int32_t device, const DevProblem& dp, const PredictSamples& in, const int32_t* time_orig,
                               const double* q, int32_t n_q, double T_floor, int64_t workspace_bytes, double* out,
                               int64_t* n_valid, int64_t* n_cold, int64_t* n_inside);

// Corner histograms (lcf_corner.hip): per entry of `in`, n samples of n_dim columns in device memory, sample s being
// the ld-strided row at base + (s / n_w) * step_stride + (s % n_w) * ld.  Inputs and outputs (host) hold the entries'
// parts one after another, as lcf_samplers_chain_range / lcf_samplers_chain_hist describe them.
struct CornerSamples {
    const double* base;
    int64_t n, n_w, step_stride;
    int32_t ld, n_dim;
};
lcf_status corner_range_run(int32_t device, const CornerSamples* in, int32_t n, double* lo, double* hi, int64_t* n_nan);
lcf_status corner_hist_run(int32_t device, const CornerSamples* in, int32_t n, const double* shift, const double* edges,
                           int32_t bins, int64_t* hist1d, int64_t* hist2d);

// Chain history (lcf_history.hip): per entry of `in`, a whole stored chain [n_t][n_w][n_dim] and its log-probabilities
// [n_t][n_w] (or nullptr) in device memory; the kept steps are discard, discard + thin, ...  Inputs and outputs (host)
// hold the entries' parts one after another, as lcf_samplers_chain_history / lcf_samplers_chain_raster describe them.
struct HistoryChain {
    const double *chain, *log_prob;
    int64_t n_t;
    int32_t n_w, n_dim;
};
lcf_status history_steps_run(int32_t device, const HistoryChain* in, int32_t n, int64_t discard, int64_t thin,
                             const double* q, int32_t n_q, double* stat_lo, double* stat_hi, int64_t* n_valid,
                             int64_t* n_moved);
lcf_status history_raster_run(int32_t device, const HistoryChain* in, int32_t n, int64_t discard, int64_t thin,
                              int32_t t_bins, const double* edges, int32_t v_bins, int64_t* counts);

}  // namespace lcf
