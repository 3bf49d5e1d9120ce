// Custom models (LCF_MODEL_CUSTOM): the user's T(t), R(t) in HIP device code, compiled at run time for the engine's GPU.
//
// The program handed to the run-time compiler (hiprtc, bound with dlopen like RCCL: the library loads without it) is
//     lcf_device.h  |  #line 1 "user_model" + the user's source  |  lcf_keys.h  |  lcf_custom_kernel.h
// -- the three headers as they were when this library was built (the Makefile turns them into string literals,
// lcf_custom_text.inc), so the compiler's log names the user's own line numbers, and the kernels are built from the very
// DevProblem, band sums, interpolant lookup and key encoding the precompiled kernels use.  -DLCF_DEVPROBLEM_BYTES carries this
// compiler's sizeof(DevProblem) over to a static_assert in the kernel header.  Code objects are cached per process
// by (source, architecture); a module is loaded once per device.  lcf_custom_points is launched on the engine's stream
// with hipModuleLaunchKernel, between the engine's own k_prepare (prior) and k_finalize; lcf_custom_keys on the null
// stream, in front of the passes of lcf_predict_custom over the keys it stores (lcf_predict.hip).
//
// The offline build compiles the kernel header too, behind a sample state function (ShockCooling2 restated): the
// kernels' registers and scratch are in lcf_custom.resources.txt, and a change that breaks the header text breaks `make`.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>

#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>

#include "lcf_internal.h"
#include "lcf_keys.h"

// ---- the sample: ShockCooling2 (models.py:403-406) as a user would write it; exponents through consts ---------------
// consts: A, a, alpha, epsilon_1, epsilon_2 (as for LCF_MODEL_SHOCK_COOLING2); p = T_1, L_1, t_tr, t_0
__device__ void lcf_user_state(double t_in, const double* p, const double* consts, double z, double& T_kK,
                               double& R_1000Rsun) {
    const double t = t_in - p[3];
    T_kK = p[0] * lcf::pw(t, 2. * consts[3] - 0.5);
    const double L = p[1] * exp(-lcf::pw(consts[1] * t / p[2], consts[2])) * lcf::pw(t, -2. * consts[4]) * 1e42;
    R_1000Rsun = lcf::kC3 * sqrt(L) * lcf::pw(T_kK, -2.);
}
#include "lcf_custom_kernel.h"

namespace {

#include "lcf_custom_text.inc"   // kDeviceText, kKeysText, kKernelText: the three headers as built

// The Makefile's code-generation flags (CXXFLAGS there: a change of one is a change of the other).
const char* const kCodegenFlags[] = {"-O3", "-std=c++17", "-ffp-contract=on", "-mllvm", "-disable-machine-licm"};

struct Hiprtc {
    void* handle = nullptr;
    hiprtcResult (*CreateProgram)(hiprtcProgram*, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
    hiprtcResult (*CompileProgram)(hiprtcProgram, int, const char* const*) = nullptr;
    hiprtcResult (*GetProgramLogSize)(hiprtcProgram, size_t*) = nullptr;
    hiprtcResult (*GetProgramLog)(hiprtcProgram, char*) = nullptr;
    hiprtcResult (*GetCodeSize)(hiprtcProgram, size_t*) = nullptr;
    hiprtcResult (*GetCode)(hiprtcProgram, char*) = nullptr;
    hiprtcResult (*DestroyProgram)(hiprtcProgram*) = nullptr;
    const char* (*GetErrorString)(hiprtcResult) = nullptr;
};
Hiprtc g_rtc;
std::mutex g_mutex;   // the binding, the cache and the programs' module tables

std::string dir_of_symbol(const void* sym) {
    Dl_info info;
    if (!dladdr(sym, &info) || !info.dli_fname) return "";
    const std::string path = info.dli_fname;
    const size_t slash = path.rfind('/');
    return slash == std::string::npos ? "" : path.substr(0, slash);
}

// LCF_HIPRTC_LIB, the ROCm tree (ROCM_PATH, HIP_PATH, /opt/rocm), the directory the HIP runtime of this process was
// loaded from (with PyTorch in the process: torch/lib, which ships a libhiprtc.so), the loader's own search path.
lcf_status hiprtc_load() {
    if (g_rtc.handle) return LCF_OK;
    std::vector<std::string> paths;
    if (const char* env = std::getenv("LCF_HIPRTC_LIB")) paths.push_back(env);
    for (const char* var : {"ROCM_PATH", "HIP_PATH"})
        if (const char* env = std::getenv(var))
            if (env[0]) paths.push_back(std::string(env) + "/lib/libhiprtc.so");
    paths.push_back("/opt/rocm/lib/libhiprtc.so");
    const std::string rt = dir_of_symbol(reinterpret_cast<const void*>(&hipGetDeviceCount));
    if (!rt.empty()) paths.push_back(rt + "/libhiprtc.so");
    paths.push_back("libhiprtc.so");
    std::string tried;
    void* h = nullptr;
    for (const std::string& p : paths) {
        h = dlopen(p.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (h) break;
        tried += (tried.empty() ? "" : ", ") + p;
    }
    if (!h)
        return fail(LCF_ERR_UNSUPPORTED, "custom models need the run-time compiler libhiprtc.so, which could not be loaded; tried " +
                                             tried + " (LCF_HIPRTC_LIB names another)");
    Hiprtc r;
    r.handle = h;
#define SYM(f) r.f = (decltype(r.f))dlsym(h, "hiprtc" #f)
    SYM(CreateProgram); SYM(CompileProgram); SYM(GetProgramLogSize); SYM(GetProgramLog); SYM(GetCodeSize); SYM(GetCode);
    SYM(DestroyProgram); SYM(GetErrorString);
#undef SYM
    if (!r.CreateProgram || !r.CompileProgram || !r.GetProgramLogSize || !r.GetProgramLog || !r.GetCodeSize || !r.GetCode ||
        !r.DestroyProgram)
        return fail(LCF_ERR_UNSUPPORTED, "the hiprtc library lacks the expected symbols");
    g_rtc = r;
    return LCF_OK;
}

std::string rtc_error(hiprtcResult rc) {
    return g_rtc.GetErrorString ? g_rtc.GetErrorString(rc) : "hiprtc error " + std::to_string((int)rc);
}

}  // namespace

struct lcf_custom {
    std::string source, arch, log;
    std::vector<char> code;
    struct Loaded { hipModule_t module; hipFunction_t points, keys; };
    std::map<int, Loaded> loaded;   // per device
};

namespace {

std::map<std::pair<std::string, std::string>, std::unique_ptr<lcf_custom>> g_cache;

// `arch` as given, or the base name of the device's architecture ("gfx950" of "gfx950:sramecc+:xnack-")
lcf_status resolve_arch(const char* arch, int device, std::string* out) {
    if (arch && arch[0]) {
        *out = arch;
        return LCF_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(LCF_ERR_NO_DEVICE, "no HIP device to take the architecture from: name one (e.g. \"gfx950\")");
    if (device < 0 || device >= ndev) return fail(LCF_ERR_INVALID_ARGUMENT, "device index out of range");
    hipDeviceProp_t prop;
    LCF_HIP(hipGetDeviceProperties(&prop, device));
    const std::string name = prop.gcnArchName;
    *out = name.substr(0, name.find(':'));
    return LCF_OK;
}

lcf_status compile(lcf_custom* c) {
    const std::string program = std::string("#line 1 \"lcf_device.h\"\n") + kDeviceText + "\n#line 1 \"user_model\"\n" +
                                c->source + "\n#line 1 \"lcf_keys.h\"\n" + kKeysText +
                                "\n#line 1 \"lcf_custom_kernel.h\"\n" + kKernelText;
    hiprtcProgram prog = nullptr;
    hiprtcResult rc = g_rtc.CreateProgram(&prog, program.c_str(), "lcf_custom_model.hip", 0, nullptr, nullptr);
    if (rc != HIPRTC_SUCCESS) return fail(LCF_ERR_HIP, "hiprtcCreateProgram: " + rtc_error(rc));
    const std::string arch_flag = "--offload-arch=" + c->arch;
    const std::string size_flag = "-DLCF_DEVPROBLEM_BYTES=" + std::to_string(sizeof(DevProblem));
    std::vector<const char*> opts(std::begin(kCodegenFlags), std::end(kCodegenFlags));
    opts.push_back(arch_flag.c_str());
    opts.push_back(size_flag.c_str());
    rc = g_rtc.CompileProgram(prog, (int)opts.size(), opts.data());
    size_t n_log = 0;
    if (g_rtc.GetProgramLogSize(prog, &n_log) == HIPRTC_SUCCESS && n_log > 1) {
        c->log.resize(n_log);
        g_rtc.GetProgramLog(prog, &c->log[0]);
        while (!c->log.empty() && c->log.back() == '\0') c->log.pop_back();
    }
    if (rc != HIPRTC_SUCCESS) {
        g_rtc.DestroyProgram(&prog);
        std::string msg = "the custom model does not compile (" + rtc_error(rc) + ")";
        if (c->source.find("lcf_user_state") == std::string::npos)
            msg += ": the source does not define lcf_user_state";
        return fail(LCF_ERR_INVALID_ARGUMENT, msg + "\n" + c->log);
    }
    size_t n_code = 0;
    rc = g_rtc.GetCodeSize(prog, &n_code);
    if (rc == HIPRTC_SUCCESS && n_code > 0) {
        c->code.resize(n_code);
        rc = g_rtc.GetCode(prog, c->code.data());
    }
    g_rtc.DestroyProgram(&prog);
    if (rc != HIPRTC_SUCCESS || c->code.empty()) return fail(LCF_ERR_HIP, "hiprtc returned no code object: " + rtc_error(rc));
    return LCF_OK;
}

const char kRoute[] = "a custom model (LCF_MODEL_CUSTOM) is evaluated by lcf_log_likelihood / lcf_log_posterior (and _dev), "
                      "lcf_model_evaluate and lcf_temperature_radius, sampled through lcf_tempered_* (TemperedSampler; one "
                      "rung at beta = 1 is the ensemble sampler), and its bands over a chain are lcf_predict_custom";

}  // namespace

namespace lcf {

lcf_status custom_refuse(const lcf_engine* e, const char* what) {
    if (!e || e->dp.model != LCF_MODEL_CUSTOM) return LCF_OK;
    return fail(LCF_ERR_UNSUPPORTED, std::string(what) + " is compiled per model: " + kRoute);
}

lcf_status custom_ready(const lcf_engine* e) {
    if (e->custom_points) return LCF_OK;
    return fail(LCF_ERR_STATE, "an engine of LCF_MODEL_CUSTOM has no program: call lcf_engine_set_custom first");
}

// Rows [w_lo, w_lo + n) of P through the program's kernel, enqueued on st.  mode 0: chi^2 partial sums -> out0 (the
// engine's part buffer; rows with lprior == -inf skipped), 1: y_fit -> out0, 2: T, R -> out0, out1.
lcf_status custom_launch(lcf_engine* e, int mode, int w_lo, int n, const double* dP, const double* lprior, double* out0,
                         double* out1, hipStream_t st) {
    if (lcf_status s = custom_ready(e)) return s;
    if (n <= 0 || e->dp.n_points == 0) return LCF_OK;
    DevProblem pb = e->dp;
    double z = e->custom_z;
    void* args[] = {&pb, &mode, &w_lo, &n, &z, &dP, &lprior, &out0, &out1};
    LCF_HIP(hipModuleLaunchKernel(e->custom_points, (unsigned)((size_t)n * pb.n_parts), 1, 1, kBlock, 1, 1, 0, st,
                                  args, nullptr));
    return LCF_OK;
}

// n_cus sizes the grid: the tile's times are spread over blockIdx.y while the samples alone leave the device short of
// eight workgroups per CU.
lcf_status custom_keys_launch(lcf_engine* e, const ChainView& in, int64_t discard, int64_t thin, int ep0, int n_ep,
                              double T_floor, unsigned long long* keys, unsigned long long* n_cold) {
    if (lcf_status s = custom_ready(e)) return s;
    const KeptSteps k = kept_steps(in, discard, thin);
    if (k.samples <= 0 || n_ep <= 0) return LCF_OK;
    DevProblem pb = e->dp;
    double z = e->custom_z;
    const double* base = k.base;
    long long n = k.samples, n_w = in.n_w, step_stride = k.step_stride;
    int ld = in.ld;
    const long long gx = (n + kBlock - 1) / kBlock;
    const long long gy = std::min<long long>(n_ep, std::max<long long>(1, (long long)std::max(e->n_cus, 1) * 8 / gx));
    void* args[] = {&pb, &z, &base, &n, &n_w, &step_stride, &ld, &ep0, &n_ep, &T_floor, &keys, &n_cold};
    LCF_HIP(hipModuleLaunchKernel(e->custom_keys, (unsigned)gx, (unsigned)gy, 1, kBlock, 1, 1, 0, nullptr, args, nullptr));
    return LCF_OK;
}

}  // namespace lcf

extern "C" {

lcf_status lcf_custom_compile(const char* source, const char* arch, int32_t device, lcf_custom** out) {
    if (!source || !out) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::string a;
    if (lcf_status st = resolve_arch(arch, device, &a)) return st;
    std::lock_guard<std::mutex> lock(g_mutex);
    const auto key = std::make_pair(std::string(source), a);
    auto it = g_cache.find(key);
    if (it == g_cache.end()) {
        if (lcf_status st = hiprtc_load()) return st;
        auto c = std::make_unique<lcf_custom>();
        c->source = source;
        c->arch = a;
        if (lcf_status st = compile(c.get())) return st;
        it = g_cache.emplace(key, std::move(c)).first;
    }
    *out = it->second.get();
    return LCF_OK;
}

const char* lcf_custom_log(const lcf_custom* c) { return c ? c->log.c_str() : ""; }

const void* lcf_custom_code(const lcf_custom* c, int64_t* n_bytes) {
    if (n_bytes) *n_bytes = c ? (int64_t)c->code.size() : 0;
    return c && !c->code.empty() ? c->code.data() : nullptr;
}

void lcf_custom_destroy(lcf_custom*) {}   // (programs belong to the per-process cache: see lcf.h)

lcf_status lcf_engine_set_custom(lcf_engine* e, lcf_custom* c) {
    if (!e || !c) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (e->dp.model != LCF_MODEL_CUSTOM) return fail(LCF_ERR_INVALID_ARGUMENT, "the engine was not created with LCF_MODEL_CUSTOM");
    LCF_HIP(hipSetDevice(e->device));
    std::string a;
    if (lcf_status st = resolve_arch(nullptr, e->device, &a)) return st;
    if (a != c->arch)
        return fail(LCF_ERR_INVALID_ARGUMENT, "the program was compiled for " + c->arch + ", the engine's device is " + a);
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = c->loaded.find(e->device);
    if (it == c->loaded.end()) {
        lcf_custom::Loaded l{};
        LCF_HIP(hipModuleLoadData(&l.module, c->code.data()));
        LCF_HIP(hipModuleGetFunction(&l.points, l.module, "lcf_custom_points"));
        LCF_HIP(hipModuleGetFunction(&l.keys, l.module, "lcf_custom_keys"));
        it = c->loaded.emplace(e->device, l).first;
    }
    LCF_HIP(hipStreamSynchronize(e->stream));   // (launches in flight keep the program they were enqueued with)
    e->custom_points = it->second.points;
    e->custom_keys = it->second.keys;
    return LCF_OK;
}

lcf_status lcf_engine_set_custom_redshift(lcf_engine* e, double z) {
    if (!e) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (e->dp.model != LCF_MODEL_CUSTOM) return fail(LCF_ERR_INVALID_ARGUMENT, "the engine was not created with LCF_MODEL_CUSTOM");
    e->custom_z = z;
    return LCF_OK;
}

}  // extern "C"
