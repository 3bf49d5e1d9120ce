// Engine creation: the layout is planned on the host (lcf_plan.h: every argument check, no device), then the engine's
// shell is made on the device and the plan uploaded.  No kernel is compiled here: this file builds in seconds.
#include "lcf_internal.h"
#include "lcf_plan.h"

namespace lcf {

// The shell of an engine on `device`: made current, its compute units counted, a stream of its own.  After it only HIP
// can fail.
lcf_status engine_shell(int32_t device, std::unique_ptr<lcf_engine>* out) {
    if (lcf_status st = use_device(device)) return st;
    auto e = std::make_unique<lcf_engine>();
    e->device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) e->n_cus = cus;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return fail(LCF_ERR_HIP, "hipStreamCreate failed");
    *out = std::move(e);
    return LCF_OK;
}

}  // namespace lcf

extern "C" {

lcf_status lcf_engine_create(const lcf_problem* pr, int32_t device, lcf_engine** out) {
    if (!pr || !out) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    // (no filters: an engine of its own making; a problem of another ABI is read by neither: plan_engine refuses it)
    if (pr->abi_version == LCF_ABI_VERSION && is_central(pr->model)) return central_engine_create(pr, device, out);
    EnginePlan plan;
    if (lcf_status st = plan_engine(*pr, plan_knobs_from_env(), &plan)) return st;
    std::unique_ptr<lcf_engine> e;
    if (lcf_status st = engine_shell(device, &e)) return st;
    e->dp = plan.dp;
    e->have_ctab = plan.have_ctab;
    e->have_itab = plan.have_itab;
    e->samples_per_eval = plan.samples_per_eval;
    e->lds_bytes = plan.lds_bytes;
    // (one block, one copy: the photometry in its layouts, the tables and the staging image; sized for the light curve)
    UploadArena arena(e->owned, (size_t)256 * 1024 + (size_t)plan.dp.n_points * 256);
    if (lcf_status st = upload_plan(plan, arena, &e->dp, &e->d_tab_off, &e->d_ctab_off, &e->d_ctmin)) return st;
    if (lcf_status st = arena.flush()) return st;
    if (lcf_status st = e->sync_dp()) return st;
    *out = e.release();
    return LCF_OK;
}

void lcf_engine_destroy(lcf_engine* e) { delete e; }
int32_t lcf_engine_ndim(const lcf_engine* e) { return e ? e->dp.n_dim : 0; }
int64_t lcf_engine_npoints(const lcf_engine* e) { return e ? e->dp.n_points : 0; }
int64_t lcf_engine_samples_per_eval(const lcf_engine* e) { return e ? e->samples_per_eval : 0; }

lcf_status lcf_engine_set_variant(lcf_engine* e, int32_t variant) {
    if (!e || variant < 0 || variant > 3) return fail(LCF_ERR_INVALID_ARGUMENT, "variant must be 0, 1, 2 or 3");
    if (variant >= 2 && !e->have_ctab) return fail(LCF_ERR_INVALID_ARGUMENT, "no compressed tables were given");
    if (variant == 3 && !e->have_itab) return fail(LCF_ERR_INVALID_ARGUMENT, "no interpolants were given");
    e->dp.variant = variant == 0 ? 0 : 1;
    e->dp.use_ctab = variant >= 2 ? 1 : 0;
    e->dp.use_itab = variant == 3 ? 1 : 0;
    LCF_HIP(hipSetDevice(e->device));
    LCF_HIP(hipStreamSynchronize(e->stream));   // (launches in flight read the old copy)
    return e->sync_dp();
}

// The layout lcf_engine_create would give this problem, without a device (not in lcf.h: tests/sampler_cases.py binds it).
// out[0 .. n_out), n_out >= 47: n_points, n_epochs, use_therm, em_k, em_cols, em_dense; n_parts, n_chunks, cpb; n_tab,
// n_lds_tab, tab_in_lds, redden_slow, use_ctab, use_itab, itab_uniform; n_itab_lds, n_spl_lds, stage_d2, stage_n16; then
// part_start[9], part_col0[9], part_ep0[9] (layout_ints).  *hash: FNV-1a over the bytes of every array, in upload order.
int32_t lcf_debug_engine_layout(const lcf_problem* pr, int32_t* out, int32_t n_out, uint64_t* hash) {
    if (!pr || !out || !hash || n_out < kLayoutInts) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument, or fewer than 47 integers");
    EnginePlan plan;
    if (lcf_status st = plan_engine(*pr, plan_knobs_from_env(), &plan)) return st;
    layout_ints(plan.dp, out);
    HashArena arena;
    DevProblem dp = plan.dp;
    int *tab_off, *ctab_off;
    double* ctmin;
    upload_plan(plan, arena, &dp, &tab_off, &ctab_off, &ctmin);
    *hash = arena.hash;
    return LCF_OK;
}

}  // extern "C"
