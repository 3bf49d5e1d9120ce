// Host-side helpers shared by the translation units of liblcf_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
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

// `h` into an arena (put(src, bytes, &place): UploadArena, or one that only looks at the bytes); *d: its place.
template <class Arena, class T, class P>
lcf_status put_array(Arena& arena, const std::vector<T>& h, P** d) {
    static_assert(std::is_same<typename std::remove_const<P>::type, T>::value, "the array's own element type");
    return arena.put(h.data(), h.size() * sizeof(T), (void**)d);
}

// One filter's band-table samples (a_k, W_k), k in [k0, k1), behind `tab`, padded to a multiple of four samples with
// zero weights (exactly 0 contribution); *off, *cnt: where they are and how many with the padding.  False: a sample
// that is not a finite a_k > 0 with a finite W_k.
inline bool append_quads(std::vector<double2>& tab, const double* a, const double* w, int k0, int k1, int* off, int* cnt) {
    *off = (int)tab.size();
    for (int k = k0; k < k1; ++k) {
        if (!(a[k] > 0.) || !std::isfinite(a[k]) || !std::isfinite(w[k])) return false;
        tab.push_back(make_double2(a[k], w[k]));
    }
    const double apad = k1 > k0 ? a[k1 - 1] : 1.;
    while ((tab.size() - *off) % 4) tab.push_back(make_double2(apad, 0.));
    *cnt = (int)tab.size() - *off;
    return true;
}

// ---- what a chain analysis is made of --------------------------------------------------------------------------------
// A chain analysis (autocorrelation time, predictive bands, corner histograms, chain history) is ONE file: its kernels,
// its run over ChainViews and both of its C entry points -- the host-array form, which checks its own limits and then
// calls upload_chain, and the sampler form, which calls stored_chains.  It asks for its device with use_device and takes
// every scratch buffer from a DevBuf.  (Objects that own device memory for their lifetime -- engine, samplers, SED engine
// -- keep their `owned` lists.)

// The device a call runs on: LCF_ERR_NO_DEVICE without one, then the range check, then it is made current.  n_cu: its
// compute units (at least 1).
inline lcf_status use_device(int32_t device, int* n_cu = nullptr) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(LCF_ERR_NO_DEVICE, "no HIP device: the engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(LCF_ERR_INVALID_ARGUMENT, "device index out of range");
    LCF_HIP(hipSetDevice(device));
    if (n_cu) {
        LCF_HIP(hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, device));
        if (*n_cu < 1) *n_cu = 1;
    }
    return LCF_OK;
}

// Device memory for as long as a call takes: freed when the buffer goes out of scope.
struct DevBuf {
    std::vector<void*> p;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        for (void* q : p) hipFree(q);
    }
    template <class T>
    lcf_status alloc(T** d, size_t n) {   // (n = 0: one element, so that the pointer is one)
        *d = nullptr;
        LCF_HIP(hipMalloc((void**)d, std::max<size_t>(n, 1) * sizeof(T)));
        p.push_back(*d);
        return LCF_OK;
    }
    template <class T>
    lcf_status put(T** d, const T* h, size_t n) {
        if (lcf_status st = alloc(d, n)) return st;
        if (n) LCF_HIP(hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice));
        return LCF_OK;
    }
};

// Rows of a chain where they lie: n_t steps of n_w walkers, walker w of step t being the n_dim columns at
// chain + (t * n_w + w) * ld, its log-probability at log_prob[t * n_w + w] (or nullptr).  n host samples P[n][ld] are
// one step of n walkers.
struct ChainView {
    const double *chain, *log_prob;
    int64_t n_t, n_w;
    int32_t ld, n_dim;
};
// The kept steps discard, discard + thin, ... of a view: the first one, how many, the doubles from one to the next.
// Their walkers read as samples: sample s of `samples` is the row at base + (s / n_w) * step_stride + (s % n_w) * ld;
// a chain of one step (n host samples) has nothing to step over, and the kernels are handed 0 for it.
struct KeptSteps {
    const double* base;
    int64_t n, stride;
    int64_t samples, step_stride;
};
inline KeptSteps kept_steps(const ChainView& c, int64_t discard, int64_t thin) {
    const int64_t row = c.n_w * c.ld, n = (c.n_t - discard + thin - 1) / thin;
    return KeptSteps{c.chain + discard * row, n, thin * row, n * c.n_w, c.n_t > 1 ? thin * row : 0};
}

// lcf_sampler.hip: the last stored run of every sampler as a view, checked (null, discard / thin, "no stored chain",
// "discard leaves no chain", one device) and settled, and the device they are on.
lcf_status stored_chains(lcf_sampler* const* s, int32_t n, int64_t discard, int64_t thin, std::vector<ChainView>* out,
                         int32_t* device);

// The host arrays of `host` on `device` (checked here: use_device) for as long as `mem` lives; *dev is the chain there.
// The caller's own limits come first: nothing above is asked of a device.
inline lcf_status upload_chain(int32_t device, const ChainView& host, DevBuf& mem, ChainView* dev) {
    if (lcf_status st = use_device(device)) return st;
    const size_t rows = (size_t)host.n_t * host.n_w;
    double *d_chain, *d_lp = nullptr;
    if (lcf_status st = mem.put(&d_chain, host.chain, rows * host.ld)) return st;
    if (host.log_prob)
        if (lcf_status st = mem.put(&d_lp, host.log_prob, rows)) return st;
    *dev = host;
    dev->chain = d_chain;
    dev->log_prob = d_lp;
    return LCF_OK;
}

// The percentiles q[n_q] of a call that takes 1 ... max of them (`what`: the feature's words for that limit).
inline lcf_status check_percentiles(const double* q, int32_t n_q, int32_t max, const char* what) {
    if (n_q < 1 || n_q > max) return fail(LCF_ERR_INVALID_ARGUMENT, what);
    for (int32_t i = 0; i < n_q; ++i)
        if (!(q[i] >= 0. && q[i] <= 100.)) return fail(LCF_ERR_INVALID_ARGUMENT, "percentiles must be in [0, 100]");
    return LCF_OK;
}

}  // namespace lcf
