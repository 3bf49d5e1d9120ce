// The layout of a light-curve engine, planned on the host: what lcf_engine_create (lcf_engine.hip) uploads.  Nothing here
// calls HIP or reads the environment -- plan_engine is a function of the problem and three knobs, so it runs (and is
// checked: tools/native/plan_check.cpp, tests/test_engine_layout_host.py) on a machine without a device.  Every argument
// check of engine creation is here too: a problem that is refused is refused before a device is asked for.
#pragma once
#include <cmath>
#include <cstdlib>
#include <numeric>

#include "lcf_device.h"
#include "lcf_host.h"

namespace lcf {

// The three environment switches of engine creation (read at every creation: the tests set them per engine).
struct PlanKnobs {
    int parts = 0;                     // LCF_PARTS: workgroups per walker (0: the rule of split_parts)
    bool shared_epochs_only = false;   // LCF_SHARED_EPOCHS_ONLY: thermal states ahead of the points only where points share epochs
    int lds_tab_max = kLdsTabMax;      // LCF_LDS_TAB_MAX: table samples a workgroup stages at most
};
inline PlanKnobs plan_knobs_from_env() {
    PlanKnobs k;
    if (const char* env = std::getenv("LCF_PARTS")) k.parts = std::max(1, std::atoi(env));
    k.shared_epochs_only = std::getenv("LCF_SHARED_EPOCHS_ONLY") != nullptr;
    if (const char* env = std::getenv("LCF_LDS_TAB_MAX")) k.lds_tab_max = std::max(0, std::min(9500, std::atoi(env)));
    return k;
}

// Everything the engine keeps of a problem: the scalar part of DevProblem (its pointers stay null until upload_plan) and
// the host arrays behind them, declared in the order they are uploaded.  An array the problem has no use for is empty.
struct EnginePlan {
    DevProblem dp{};
    bool have_ctab = false, have_itab = false;
    int64_t samples_per_eval = 0;
    size_t lds_bytes = 0;
    std::vector<double> t, y, dy;          // points, ordered by (part, filter)
    std::vector<int> filt, orig;
    std::vector<double2> tab;              // per filter [compressed | hot] of every filter, then the full tables
    std::vector<int> tab_off;              // per filter: (offset, count) of the full table in `tab`
    std::vector<double> ext, itab, exp2;
    std::vector<int> epoch;
    std::vector<double> epoch_t;
    std::vector<double2> image, yd;
    std::vector<double> em_t;              // the epoch-major copy: [em_k][n_cols], a column's points in filter order
    std::vector<double2> em_yd;
    std::vector<int> em_filt, fe;
    std::vector<FiltDesc> f_desc;
    std::vector<double> inv_dy;
    std::vector<int> ctab_off;             // per filter: (offset, count) of the compressed table
    std::vector<double> ctmin, knots, spl;
    std::vector<PriorDev> priors;
};

// The arrays into `arena` (put(src, bytes, &dst)), in this order -- the uploaded block is laid out by it -- and their
// places into dp and the engine's three table pointers.  (The arena decides what a place is: UploadArena's are device
// addresses; lcf_debug_engine_layout's hashes the bytes.)
template <class Arena>
lcf_status upload_plan(const EnginePlan& p, Arena& arena, DevProblem* dp, int** d_tab_off, int** d_ctab_off, double** d_ctmin) {
    lcf_status st = LCF_OK;
    const auto up = [&](const auto& h, auto** d) {
        if (st == LCF_OK) st = put_array(arena, h, d);
    };
    up(p.t, &dp->t); up(p.y, &dp->y); up(p.dy, &dp->dy); up(p.filt, &dp->pt_filt); up(p.orig, &dp->pt_orig);
    up(p.tab, &dp->tab); up(p.tab_off, d_tab_off);
    up(p.ext, &dp->tab_ext); up(p.itab, &dp->itab);
    up(p.exp2, &dp->exp2tab); up(p.epoch, &dp->pt_epoch); up(p.epoch_t, &dp->epoch_t);
    up(p.image, &dp->stage_image); up(p.yd, &dp->pt_yd);
    up(p.em_t, &dp->em_t); up(p.em_yd, &dp->em_yd); up(p.em_filt, &dp->em_filt);
    up(p.fe, &dp->pt_fe);
    up(p.f_desc, &dp->f_desc); up(p.inv_dy, &dp->inv_dy); up(p.ctab_off, d_ctab_off); up(p.ctmin, d_ctmin);
    up(p.knots, &dp->knots); up(p.spl, &dp->spl); up(p.priors, &dp->priors);
    return st;
}

struct HashArena {   // no place, 64-bit FNV-1a over the bytes of every array
    uint64_t hash = 14695981039346656037ull;
    lcf_status put(const void* src, size_t bytes, void** dst) {
        for (size_t i = 0; i < bytes; ++i) hash = (hash ^ static_cast<const unsigned char*>(src)[i]) * 1099511628211ull;
        *dst = nullptr;
        return LCF_OK;
    }
};

// The integers of a layout as lcf_debug_engine_layout writes them: twenty scalars, then the parts' three arrays.
constexpr int kLayoutInts = 20 + 3 * (kMaxParts + 1);
inline void layout_ints(const DevProblem& dp, int32_t* out) {
    const int32_t head[20] = {dp.n_points, dp.n_epochs, dp.use_therm, dp.em_k, dp.em_cols, dp.em_dense,
                              dp.n_parts, dp.n_chunks, dp.cpb,
                              dp.n_tab, dp.n_lds_tab, dp.tab_in_lds, dp.redden_slow, dp.use_ctab, dp.use_itab, dp.itab_uniform,
                              dp.n_itab_lds, dp.n_spl_lds, dp.stage_d2, dp.stage_n16};
    out = std::copy(head, head + 20, out);
    out = std::copy(dp.part_start, dp.part_start + kMaxParts + 1, out);
    out = std::copy(dp.part_col0, dp.part_col0 + kMaxParts + 1, out);
    std::copy(dp.part_ep0, dp.part_ep0 + kMaxParts + 1, out);
}

// ---- helpers the central-engine models' creation (lcf_central.hip) shares -------------------------------------------
// sum_i ln(2 pi dy_i^2) in the caller's order, like np.sum, and np.median(dy) (0 without points)
inline void noise_constants(const double* dy, int N, double* log_norm, double* median) {
    *log_norm = 0.;
    for (int i = 0; i < N; ++i) *log_norm += std::log(2. * M_PI * dy[i] * dy[i]);
    std::vector<double> sorted(dy, dy + N);
    std::sort(sorted.begin(), sorted.end());
    *median = N == 0 ? 0. : (N & 1) ? sorted[N / 2] : 0.5 * (sorted[N / 2 - 1] + sorted[N / 2]);
}
inline lcf_status check_prior_kinds(const lcf_problem& pr, int n_dim) {
    for (int i = 0; pr.priors && i < n_dim; ++i)
        if (pr.priors[i].kind < 0 || pr.priors[i].kind > 2) return fail(LCF_ERR_INVALID_ARGUMENT, "bad prior kind");
    return LCF_OK;
}
inline std::vector<PriorDev> prior_rows(const lcf_problem& pr, int n_dim) {
    std::vector<PriorDev> rows(pr.priors ? n_dim : 0);
    for (size_t i = 0; i < rows.size(); ++i)
        rows[i] = PriorDev{pr.priors[i].kind, 0, pr.priors[i].p_min, pr.priors[i].p_max, pr.priors[i].mean, pr.priors[i].stddev};
    return rows;
}
// observation and the factor its residual is scaled with, side by side: 1 / dy, or dy when sigma is fitted
inline double2 scaled_pair(double y, double dy, bool use_sigma) { return make_double2(y, use_sigma ? dy : 1. / dy); }

// ---- 1. validation ---------------------------------------------------------------------------------------------------
struct Given {   // what kind of problem it is and which optional tables it brings
    bool reddened, companion, ctab, htab, itab;
};
inline Given what_is_given(const lcf_problem& pr) {
    Given g;
    g.reddened = pr.model == LCF_MODEL_SHOCK_COOLING3;
    g.companion = pr.model >= LCF_MODEL_COMPANION_SHOCKING && pr.model <= LCF_MODEL_COMPANION_SHOCKING3;
    // (a reddened model reweights the samples per walker: the compressed tables do not apply)
    g.ctab = pr.ctab_off && pr.ctab_a && pr.ctab_w && pr.ctab_tmin && !g.reddened;
    g.htab = g.ctab && pr.htab_off && pr.htab_a && pr.htab_w && pr.htab_tmin;
    g.itab = !g.reddened && pr.itab_coef && pr.itab_tmin && pr.itab_m > 0 && pr.itab_h > 0.;
    return g;
}

inline lcf_status validate_photometry(const lcf_problem& pr, const Given& g) {
    if (pr.abi_version != LCF_ABI_VERSION) return fail(LCF_ERR_INVALID_ARGUMENT, "abi_version mismatch");
    switch (pr.model) {
        case LCF_MODEL_SHOCK_COOLING: case LCF_MODEL_SHOCK_COOLING2: case LCF_MODEL_SHOCK_COOLING3:
        case LCF_MODEL_SHOCK_COOLING4:
        case LCF_MODEL_COMPANION_SHOCKING: case LCF_MODEL_COMPANION_SHOCKING2: case LCF_MODEL_COMPANION_SHOCKING3:
        case LCF_MODEL_BLACKBODY:
        case LCF_MODEL_CUSTOM:
            break;
        default:
            return fail(LCF_ERR_UNSUPPORTED, "unknown or unsupported model id");
    }
    static const int kNPar[9] = {0, 5, 4, 7, 5, 8, 7, 7, 2};
    // (a custom model has as many parameters as its state function reads: the caller says how many)
    if (pr.model == LCF_MODEL_CUSTOM ? pr.n_par < 0 : pr.n_par != kNPar[pr.model])
        return fail(LCF_ERR_INVALID_ARGUMENT, "n_par does not match the model");
    const int n_dim = pr.n_par + (pr.use_sigma ? 1 : 0);
    if (n_dim > kMaxDim) return fail(LCF_ERR_INVALID_ARGUMENT, "too many parameters");
    if (pr.n_points < 0 || pr.n_points > (1 << 26) || pr.n_filters <= 0)
        return fail(LCF_ERR_INVALID_ARGUMENT, "bad n_points / n_filters");
    if (pr.n_points > 0 && (!pr.t || !pr.y || !pr.dy || !pr.filt_idx))
        return fail(LCF_ERR_INVALID_ARGUMENT, "null photometry");
    if (!pr.tab_off || !pr.tab_a || !pr.tab_w) return fail(LCF_ERR_INVALID_ARGUMENT, "null band tables");
    if (g.reddened && !pr.tab_ext) return fail(LCF_ERR_INVALID_ARGUMENT, "ShockCooling3 needs tab_ext");
    if (pr.sigma_type != LCF_SIGMA_RELATIVE && pr.sigma_type != LCF_SIGMA_ABSOLUTE)
        return fail(LCF_ERR_INVALID_ARGUMENT, "sigma_type must be relative or absolute");
    const int N = (int)pr.n_points, NF = pr.n_filters;
    if (pr.tab_off[0] != 0) return fail(LCF_ERR_INVALID_ARGUMENT, "tab_off[0] must be 0");
    for (int f = 0; f < NF; ++f)
        if (pr.tab_off[f + 1] < pr.tab_off[f]) return fail(LCF_ERR_INVALID_ARGUMENT, "tab_off must be non-decreasing");
    for (int i = 0; i < N; ++i)
        if (pr.filt_idx[i] < 0 || pr.filt_idx[i] >= NF) return fail(LCF_ERR_INVALID_ARGUMENT, "filt_idx out of range");
    if (g.companion) {
        if (!pr.filt_kasen_par || !pr.filt_sifto_par || !pr.filt_dt_par || !pr.spline_knots || !pr.spline_coef || pr.n_knots < 2)
            return fail(LCF_ERR_INVALID_ARGUMENT, "companion-shocking model needs spline and factor tables");
        for (int f = 0; f < NF; ++f)
            for (const int32_t* a : {pr.filt_kasen_par, pr.filt_sifto_par, pr.filt_dt_par})
                if (a[f] < -1 || a[f] >= n_dim) return fail(LCF_ERR_INVALID_ARGUMENT, "factor parameter index out of range");
    }
    return LCF_OK;
}

inline lcf_status validate_tables(const lcf_problem& pr, const Given& g) {
    const int NF = pr.n_filters;
    if (g.itab) {
        if (pr.itab_m > 4096 || !(pr.itab_u0 > 0.) || !std::isfinite(pr.itab_h))
            return fail(LCF_ERR_INVALID_ARGUMENT, "interpolants: 0 < itab_m <= 4096, itab_u0 > 0 (T >= 1 kK), finite itab_h");
        for (int f = 0; f < NF; ++f) {
            if (!(pr.itab_tmin[f] > 0.)) return fail(LCF_ERR_INVALID_ARGUMENT, "itab_tmin must be > 0 (+inf: none)");
            if (std::isfinite(pr.itab_tmin[f]))
                for (int k = 0; k < pr.itab_m * 8; ++k)
                    if (!std::isfinite(pr.itab_coef[(size_t)f * pr.itab_m * 8 + k]))
                        return fail(LCF_ERR_INVALID_ARGUMENT, "non-finite interpolant coefficient");
        }
    }
    if (g.htab) {
        if (pr.htab_off[0] != 0) return fail(LCF_ERR_INVALID_ARGUMENT, "htab_off[0] must be 0");
        for (int f = 0; f < NF; ++f)
            if (pr.htab_off[f + 1] < pr.htab_off[f] || pr.htab_off[f + 1] - pr.htab_off[f] > 252)
                return fail(LCF_ERR_INVALID_ARGUMENT, "htab_off must be non-decreasing, <= 252 samples a filter");
    }
    if (g.ctab) {
        if (pr.ctab_off[0] != 0) return fail(LCF_ERR_INVALID_ARGUMENT, "ctab_off[0] must be 0");
        for (int f = 0; f < NF; ++f)
            if (pr.ctab_off[f + 1] < pr.ctab_off[f]) return fail(LCF_ERR_INVALID_ARGUMENT, "ctab_off must be non-decreasing");
    }
    return LCF_OK;
}

// ---- 2. epochs, columns and parts ------------------------------------------------------------------------------------
// The points are ordered in n_parts contiguous ranges of observation epochs ("parts", one workgroup per walker each),
// sorted by filter inside a part (waves then share a band table).  A part owning whole epochs means its workgroup needs
// the thermal states of those epochs only.
struct PointLayout {
    int N = 0;
    bool all_finite_t = true;
    bool epochs_ahead = false;             // thermal states per (walker, observation time) ahead of the points
    std::vector<double> epochs;            // distinct observation times (exact equality), ascending
    std::vector<int> ep_of;                // the epoch of the caller's point i
    std::vector<int> order;                // the engine's points: the caller's indices by epoch, then by (part, filter)
    // the epoch-major copy (epochs_ahead): per column its epoch and its first point in em_order
    std::vector<int> em_order, col_epoch, col_first;   // em_order: points by (epoch, filter, caller's index)
    int em_k = 1, em_dense = 0, n_cols = 0;
    int n_parts = 1;
    std::vector<int> part_start, part_col0;
};

inline void find_epochs(const lcf_problem& pr, const PlanKnobs& knobs, PointLayout* L) {
    const int N = L->N = (int)pr.n_points;
    // distinct observation times (exact equality): the thermal state depends on (walker, time) only
    L->all_finite_t = std::all_of(pr.t, pr.t + N, [](double v) { return std::isfinite(v); });
    // (with a non-finite time there is no strict weak order to sort by: every point is then its own epoch, in the
    // caller's order, and nothing below compares times)
    L->epochs.assign(pr.t, pr.t + N);
    if (L->all_finite_t) {
        std::sort(L->epochs.begin(), L->epochs.end());
        L->epochs.erase(std::unique(L->epochs.begin(), L->epochs.end()), L->epochs.end());
    }
    L->ep_of.resize(N);
    for (int i = 0; i < N; ++i)
        L->ep_of[i] = L->all_finite_t ? (int)(std::lower_bound(L->epochs.begin(), L->epochs.end(), pr.t[i]) - L->epochs.begin()) : i;
    L->order.resize(N);
    std::iota(L->order.begin(), L->order.end(), 0);
    std::stable_sort(L->order.begin(), L->order.end(), [&](int a, int b) { return L->ep_of[a] < L->ep_of[b]; });
    // Thermal states per (walker, observation time) ahead of the points.  With >= 2 points per distinct time that is
    // sharing; without any (real multi-band photometry: every observation has its own time) it still is what puts a
    // light curve on the fast path -- log-space states, interpolated band sums, k_solo.  shared_epochs_only
    // restores the round-1 rule, sharing or nothing (the tests of the state-inside-the-point-loop kernels set it).
    const bool sharing = 2 * (long long)L->epochs.size() <= N;
    L->epochs_ahead = L->all_finite_t && N > 0 && (sharing || !knobs.shared_epochs_only);
}

// The epoch-major copy the likelihood walks (DevProblem::em_*): COLUMNS = an observation time with up to em_k of its
// points in filter order; an epoch with more points than that takes several columns (em_k = the most points of an epoch,
// but at most twice the mean, so that ragged photometry does not pad the arrays beyond ~3 N entries).
inline void make_columns(const lcf_problem& pr, PointLayout* L) {
    if (!L->epochs_ahead) return;
    const int N = L->N, NF = pr.n_filters, n_ep = (int)L->epochs.size();
    L->em_order = L->order;
    std::stable_sort(L->em_order.begin(), L->em_order.end(), [&](int a, int b) {
        return L->ep_of[a] != L->ep_of[b] ? L->ep_of[a] < L->ep_of[b] : pr.filt_idx[a] < pr.filt_idx[b];
    });
    std::vector<int> cnt(n_ep, 0);
    for (int i = 0; i < N; ++i) ++cnt[L->ep_of[i]];
    const int kmax = *std::max_element(cnt.begin(), cnt.end());
    L->em_k = std::min(kmax, std::max(2, (int)((2LL * N + n_ep - 1) / n_ep)));
    for (int e = 0, at = 0; e < n_ep; ++e) {
        for (int k = 0; k < cnt[e]; k += L->em_k) {
            L->col_epoch.push_back(e);
            L->col_first.push_back(at + k);
        }
        at += cnt[e];
    }
    L->n_cols = (int)L->col_epoch.size();
    L->em_dense = L->em_k == NF && (long long)n_ep * NF == N;
    for (int i = 0; L->em_dense && i < N; ++i)   // every epoch holds filters 0 .. NF-1, one point each
        if (pr.filt_idx[L->em_order[i]] != i % NF) L->em_dense = 0;
}

inline void split_parts(const lcf_problem& pr, const PlanKnobs& knobs, PointLayout* L) {
    const int N = L->N, n_cols = L->n_cols;
    const int n_chunks_all = std::max(1, (N + kBlock - 1) / kBlock);
    // workgroups per walker ("parts"): every one repeats the prologue (table staging; in the fused sampler kernel also
    // the serial part of the half-step), so few of them.  Epoch-major engines: a part is what 256 lanes walk, one
    // column each and round -- one part per 256 columns; else two parts up to 16 chunks of points, then one per 8
    // (measured on the 1024-walker, 3000-point fit in round 1: 2 parts 52 us/step, 4 parts 61, 8 parts 83)
    int n_parts = std::min(n_chunks_all, std::min(kMaxParts, std::max(2, (n_chunks_all + 7) / 8)));
    if (L->epochs_ahead) {
        // ... or, beyond kMaxParts x 256 columns, one part per 256 r columns with the smallest r that fits: a part's
        // 256 lanes then make r full rounds (3000 single-point columns: 6 parts of 500, not 8 of 375 whose second round
        // is half empty)
        int rounds = 1;
        while ((n_cols + kBlock * rounds - 1) / (kBlock * rounds) > kMaxParts) ++rounds;
        n_parts = std::max(n_cols > 64 ? 2 : 1, (n_cols + kBlock * rounds - 1) / (kBlock * rounds));
    }
    if (knobs.parts > 0) n_parts = std::min(std::min(L->epochs_ahead ? n_cols : n_chunks_all, kMaxParts), knobs.parts);
    L->part_start.assign(kMaxParts + 1, N);
    L->part_col0.assign(kMaxParts + 1, n_cols);
    L->part_start[0] = L->part_col0[0] = 0;
    int made = 0;
    for (int j = 1; j < n_parts; ++j) {
        int b;  // boundary j: the first epoch change at or after the equal split (of the columns / of the points)
        if (L->epochs_ahead) {
            int cb = (int)((long long)n_cols * j / n_parts);
            while (cb < n_cols && cb > 0 && L->col_epoch[cb] == L->col_epoch[cb - 1]) ++cb;
            b = cb < n_cols ? L->col_first[cb] : N;   // (`order` and em_order agree on where an epoch starts)
            if (b > L->part_start[made] && b < N) L->part_col0[made + 1] = cb;
        } else {
            b = (int)((long long)N * j / n_parts);
            while (b < N && b > 0 && L->ep_of[L->order[b]] == L->ep_of[L->order[b - 1]]) ++b;
        }
        if (b > L->part_start[made] && b < N) L->part_start[++made] = b;
    }
    L->n_parts = made + 1;
    for (int j = L->n_parts; j <= kMaxParts; ++j) {   // (a boundary that made no part may have left its column behind)
        L->part_start[j] = N;
        L->part_col0[j] = n_cols;
    }
    for (int j = 0; j < L->n_parts; ++j)
        std::stable_sort(L->order.begin() + L->part_start[j], L->order.begin() + L->part_start[j + 1],
                         [&](int a, int b) { return pr.filt_idx[a] < pr.filt_idx[b]; });
}

// The point arrays in the engine's order, the epoch-major copy, and what DevProblem says about both.
inline void fill_points(const lcf_problem& pr, const PointLayout& L, EnginePlan* p) {
    const int N = L.N, NF = pr.n_filters, n_ep = (int)L.epochs.size();
    DevProblem& dp = p->dp;
    p->t.resize(N); p->y.resize(N); p->dy.resize(N); p->inv_dy.resize(N); p->yd.resize(N);
    p->filt.resize(N); p->orig.resize(N); p->epoch.resize(N);
    int64_t samples = 0;
    for (int i = 0; i < N; ++i) {
        const int o = L.order[i], f = pr.filt_idx[o];
        p->t[i] = pr.t[o];
        p->y[i] = pr.y[o];
        p->dy[i] = pr.dy[o];
        p->inv_dy[i] = 1. / pr.dy[o];
        p->yd[i] = scaled_pair(pr.y[o], pr.dy[o], pr.use_sigma);
        p->filt[i] = f;
        p->orig[i] = o;
        p->epoch[i] = L.ep_of[o];
        samples += pr.tab_off[f + 1] - pr.tab_off[f];
    }
    p->samples_per_eval = samples * (pr.model == LCF_MODEL_SHOCK_COOLING4 ? 2 : 1);
    if (NF <= 64) {  // filter and epoch of a point in one word (epochs < 2^26 = the most points an engine takes)
        p->fe.resize(N);
        for (int i = 0; i < N; ++i) p->fe[i] = (int)((unsigned int)p->filt[i] | ((unsigned int)p->epoch[i] << 6));
    }
    p->epoch_t = L.epochs;
    dp.n_points = N;
    dp.n_epochs = n_ep;
    dp.use_therm = L.epochs_ahead;
    dp.n_parts = L.n_parts;
    dp.n_chunks = 0;  // chunks of kBlock points: total over the parts, and (cpb) the most in one part
    dp.cpb = 1;
    for (int j = 0; j <= kMaxParts; ++j) {
        dp.part_start[j] = L.part_start[j];
        dp.part_col0[j] = L.part_col0[j];
        dp.part_ep0[j] = n_ep;
    }
    for (int j = 0; j < L.n_parts; ++j) {
        const int c = (L.part_start[j + 1] - L.part_start[j] + kBlock - 1) / kBlock;
        dp.n_chunks += c;
        dp.cpb = std::max(dp.cpb, c);
        // `order` is filter-sorted inside a part: the part's first epoch is the minimum over its points
        for (int i = L.part_start[j]; L.all_finite_t && i < L.part_start[j + 1]; ++i)
            dp.part_ep0[j] = std::min(dp.part_ep0[j], p->epoch[i]);
    }
    dp.em_k = L.em_k;
    dp.em_cols = L.n_cols;
    dp.em_dense = L.em_dense;
    if (!L.epochs_ahead) return;
    const int n_cols = L.n_cols;
    p->em_t.resize(n_cols);
    p->em_yd.assign((size_t)L.em_k * n_cols, make_double2(0., 0.));
    p->em_filt.assign((size_t)L.em_k * n_cols, -1);
    for (int c = 0; c < n_cols; ++c) {
        const int ep = L.col_epoch[c];
        p->em_t[c] = L.epochs[ep];
        for (int k = 0; k < L.em_k; ++k) {
            const int at = L.col_first[c] + k;
            if (at >= N || L.ep_of[L.em_order[at]] != ep) break;
            const int o = L.em_order[at];
            p->em_yd[(size_t)k * n_cols + c] = scaled_pair(pr.y[o], pr.dy[o], pr.use_sigma);
            p->em_filt[(size_t)k * n_cols + c] = pr.filt_idx[o];
        }
    }
}

// ---- 3. band tables and filter descriptors ---------------------------------------------------------------------------
// The device table: per filter its compressed levels, each padded to a multiple of four samples with zero weights
// (exactly 0 contribution), then the full tables of every filter: when everything does not fit in LDS the (short)
// compressed part still does, and only points colder than its validity read global memory.  *n_compressed: the samples
// in front of the full tables.
inline lcf_status pack_tables(const lcf_problem& pr, const Given& g, EnginePlan* p, int* n_compressed) {
    const int NF = pr.n_filters;
    std::vector<int> phot(2 * NF, 0);  // (offset, count) pairs, like tab_off and ctab_off
    std::vector<double> ptmin2(NF, INFINITY);
    p->tab_off.assign(2 * NF, 0);
    p->ctab_off.assign(2 * NF, 0);
    p->ctmin.assign(NF, INFINITY);
    for (int f = 0; f < NF; ++f) {
        bool ok = true;
        int* c = &p->ctab_off[2 * f];
        if (g.ctab && pr.ctab_off[f + 1] > pr.ctab_off[f]) {
            ok = append_quads(p->tab, pr.ctab_a, pr.ctab_w, pr.ctab_off[f], pr.ctab_off[f + 1], &c[0], &c[1]);
            p->ctmin[f] = pr.ctab_tmin[f];
            if (!(p->ctmin[f] >= 0.)) ok = false;
        }
        if (ok && g.htab && pr.htab_off[f + 1] > pr.htab_off[f]) {
            ok = append_quads(p->tab, pr.htab_a, pr.htab_w, pr.htab_off[f], pr.htab_off[f + 1], &phot[2 * f], &phot[2 * f + 1]);
            ptmin2[f] = pr.htab_tmin[f];
            // the hot level must not claim a wider range than the cool one (selection tests it first)
            if (!(ptmin2[f] >= 0.) || (c[1] > 0 && ptmin2[f] < p->ctmin[f])) ok = false;
        }
        if (!ok)
            return fail(LCF_ERR_INVALID_ARGUMENT,
                        "band tables need finite a_k > 0, finite W_k, t_min >= 0 (hot level: t_min >= the cool one's)");
    }
    *n_compressed = (int)p->tab.size();
    for (int f = 0; f < NF; ++f) {
        int* full = &p->tab_off[2 * f];
        bool ok = append_quads(p->tab, pr.tab_a, pr.tab_w, pr.tab_off[f], pr.tab_off[f + 1], &full[0], &full[1]);
        if (ok && g.reddened) {  // 0.4 log2(10) A_k / E(B-V), aligned with the table (no compressed levels in front)
            for (int k = pr.tab_off[f]; ok && k < pr.tab_off[f + 1]; ++k) {
                ok = std::isfinite(pr.tab_ext[k]);
                p->ext.push_back(0.4 * 3.321928094887362 * pr.tab_ext[k]);
            }
            p->ext.resize(p->tab.size(), 0.);
        }
        if (!ok) return fail(LCF_ERR_INVALID_ARGUMENT, "band tables need finite a_k > 0 and finite W_k");
    }
    if (p->tab.empty()) p->tab.push_back(make_double2(1., 0.));
    p->f_desc.resize(NF);  // per filter: where its tables are and from which temperature each is valid
    for (int f = 0; f < NF; ++f)
        p->f_desc[f] = FiltDesc{p->tab_off[2 * f], p->tab_off[2 * f + 1], p->ctab_off[2 * f], p->ctab_off[2 * f + 1],
                                phot[2 * f], phot[2 * f + 1],
                                // the interpolant holds from max(its proved t_min, the table's first interval)
                                (g.itab && std::isfinite(pr.itab_tmin[f]))
                                    ? std::nextafter((float)std::max((std::log(pr.itab_tmin[f]) - pr.itab_u0) / pr.itab_h, 0.), INFINITY)
                                    : INFINITY,
                                g.itab ? f * pr.itab_m * 8 : 0,
                                p->ctab_off[2 * f + 1] > 0 ? 1. / p->ctmin[f] : 0.,  // t_min = 0 -> inf: always valid
                                phot[2 * f + 1] > 0 ? 1. / ptmin2[f] : 0.,
                                g.companion ? pr.filt_kasen_par[f] : -1, g.companion ? pr.filt_sifto_par[f] : -1,
                                g.companion ? pr.filt_dt_par[f] : -1, 0};
    return LCF_OK;
}

// ---- 5. spline flags (ahead of the LDS plan, which asks whether the knots are exact) -----------------------------------
inline lcf_status spline_flags(const lcf_problem& pr, const Given& g, EnginePlan* p) {
    DevProblem& dp = p->dp;
    dp.n_knots = g.companion ? pr.n_knots : 0;
    if (!g.companion) return LCF_OK;
    const int NF = pr.n_filters, nk = pr.n_knots;
    p->knots.assign(pr.spline_knots, pr.spline_knots + nk);
    p->spl.assign(pr.spline_coef, pr.spline_coef + (size_t)NF * (nk - 1) * 4);
    const std::vector<double>& kn = p->knots;
    for (int k = 1; k < nk; ++k)
        if (!(kn[k] > kn[k - 1])) return fail(LCF_ERR_INVALID_ARGUMENT, "spline knots must ascend");
    const double h = (kn.back() - kn.front()) / (nk - 1);
    bool uniform = true;
    for (int k = 0; k < nk; ++k) uniform = uniform && std::fabs(kn[k] - (kn.front() + k * h)) <= 1e-9 * h;
    // knots that ARE k0 + i h in float64 (SiFTO: integer days): interval by arithmetic, no knot read on the device
    const double h1 = kn[1] - kn[0];
    bool exact = true;
    for (int k = 0; exact && k < nk; ++k) exact = kn[k] == kn[0] + k * h1;
    dp.knot0 = kn.front();
    dp.knot_last = kn.back();
    dp.knot_h = exact ? h1 : 0.;
    dp.knot_inv_h = exact ? 1. / h1 : uniform ? 1. / h : 0.;
    return LCF_OK;
}

// ---- 4. the LDS plan and the staging image ---------------------------------------------------------------------------
inline void plan_lds(const lcf_problem& pr, const Given& g, const PlanKnobs& knobs, int n_compressed, EnginePlan* p) {
    DevProblem& dp = p->dp;
    const int NF = pr.n_filters, N = dp.n_points, n_tab = dp.n_tab = (int)p->tab.size();
    // LDS holds the first n_lds_tab samples of the table array: all of it, or the compressed levels only
    dp.n_lds_tab = NF > kLdsFiltMax ? 0
                   : n_tab <= knobs.lds_tab_max ? n_tab
                   : (n_compressed > 0 && n_compressed <= knobs.lds_tab_max) ? n_compressed : 0;
    // reddened weights are made while staging the FULL tables; when those do not fit nothing is staged and the
    // reddening is applied on the fly (slow path)
    dp.redden_slow = g.reddened && dp.n_lds_tab != n_tab;
    if (dp.redden_slow) dp.n_lds_tab = 0;
    dp.tab_in_lds = dp.n_lds_tab > 0;
    // third level: interpolants of ln S(ln T), staged in LDS behind the descriptors when they take <= 40 KiB
    // (six to ten filters), else read from global memory (L2)
    // (engines whose points share no epochs keep the thermal state inside the point loop, in linear space)
    p->have_itab = g.itab && dp.use_therm;
    dp.use_itab = p->have_itab ? 1 : 0;
    dp.itab_m = g.itab ? pr.itab_m : 0;
    dp.itab_u0 = g.itab ? pr.itab_u0 : 0.;
    dp.itab_inv_h = g.itab ? 1. / pr.itab_h : 0.;
    dp.itab_umax = g.itab ? pr.itab_u0 + pr.itab_h * pr.itab_m : 0.;
    const size_t n_itab = p->have_itab ? (size_t)NF * pr.itab_m * 8 : 0;
    // ... and only where a workgroup walks enough points to pay for staging them (a part of >= 1024 points; the
    // population launches of 600-point transients read the 64 bytes a point needs from L2 instead: staging 24 KiB per
    // workgroup cost them 20 %)
    dp.n_itab_lds = (dp.tab_in_lds && n_itab * sizeof(double) <= 40 * 1024 && N >= 1024 * dp.n_parts) ? (int)n_itab : 0;
    dp.itab_uniform = g.itab ? 1 : 0;
    for (int f = 0; g.itab && f < NF; ++f)
        if (!(pr.itab_tmin[f] <= std::exp(pr.itab_u0) * (1. + 1e-12))) dp.itab_uniform = 0;
    // ... and a companion-shocking model's template splines behind those, when their knots are exactly k0 + i h (the
    // device then needs no knot) and everything still leaves room for two workgroups per CU (80 KiB each): 26 KiB for
    // the eight SiFTO filters -- a point's template costs two LDS reads instead of a chain of dependent loads from L2
    dp.n_spl_lds = 0;
    if (g.companion && dp.tab_in_lds && dp.knot_h > 0.) {
        const size_t n_spl = (size_t)NF * (pr.n_knots - 1) * 4;
        const size_t before = kLdsHead * sizeof(double) + ((size_t)dp.n_lds_tab + kFdD2 * NF) * sizeof(double2) +
                              (size_t)dp.n_itab_lds * sizeof(double);
        if (before + n_spl * sizeof(double) + 2048 <= 80 * 1024) dp.n_spl_lds = (int)n_spl;
    }
    dp.stage_d2 = dp.n_lds_tab + kFdD2 * NF + dp.n_itab_lds / 2 + dp.n_spl_lds / 2;
    p->lds_bytes = kLdsHead * sizeof(double) + (dp.tab_in_lds ? (size_t)dp.stage_d2 * sizeof(double2) : 0);
}

// The exp table, the interpolants as the device reads them, and the image of the kernels' staged LDS (see kLdsHead /
// stage_tables): [exp table | 32 doubles | first n_lds_tab samples of tab | f_desc | staged itab | splines].
inline void stage_image(const lcf_problem& pr, const Given& g, EnginePlan* p) {
    DevProblem& dp = p->dp;
    const int NF = pr.n_filters;
    p->exp2.resize(kExpTabSize);
    for (int j = 0; j < kExpTabSize; ++j) p->exp2[j] = std::exp2(j / (double)kExpTabSize);
    const auto finite_or_0 = [](double v) { return std::isfinite(v) ? v : 0.; };
    if (g.itab) {   // (filters without an interpolant: never read, u_min = +inf)
        p->itab.resize((size_t)NF * pr.itab_m * 8);
        std::transform(pr.itab_coef, pr.itab_coef + p->itab.size(), p->itab.begin(), finite_or_0);
    }
    std::vector<double2>& img = p->image;
    img.assign(kLdsHead / 2, make_double2(0., 0.));
    std::memcpy(img.data(), p->exp2.data(), kExpTabSize * sizeof(double));
    if (dp.tab_in_lds) {
        img.insert(img.end(), p->tab.begin(), p->tab.begin() + dp.n_lds_tab);
        const double2* fd2 = reinterpret_cast<const double2*>(p->f_desc.data());
        img.insert(img.end(), fd2, fd2 + kFdD2 * NF);
        for (int k = 0; k < dp.n_itab_lds; k += 2) img.push_back(make_double2(p->itab[k], p->itab[k + 1]));
        for (int k = 0; k < dp.n_spl_lds; k += 2) img.push_back(make_double2(pr.spline_coef[k], pr.spline_coef[k + 1]));
    }
    dp.stage_n16 = (int)img.size();
}

// ---- 6. noise constants and the model's constants ---------------------------------------------------------------------
inline void plan_constants(const lcf_problem& pr, EnginePlan* p) {
    DevProblem& dp = p->dp;
    std::memcpy(dp.consts, pr.consts, sizeof(dp.consts));
    if (pr.model == LCF_MODEL_SHOCK_COOLING || pr.model == LCF_MODEL_SHOCK_COOLING3)
        dp.consts[11] = pr.consts[1] > 0. ? std::log(pr.consts[1] / 19.5) : 0.;  // hoisted out of the half-step
    if (pr.model == LCF_MODEL_SHOCK_COOLING) {  // logarithms of the two amplitudes' constant factors (log-space state)
        dp.consts[9] = std::log(pr.consts[6] * pr.consts[7] / kKB);
        dp.consts[10] = std::log(kC3sq * pr.consts[5] * pr.consts[0]);
    }
    noise_constants(pr.dy, dp.n_points, &dp.log_norm_const, &dp.sigma_unit_abs);
}

inline lcf_status plan_engine(const lcf_problem& pr, const PlanKnobs& knobs, EnginePlan* out) {
    const Given g = what_is_given(pr);
    if (lcf_status st = validate_photometry(pr, g)) return st;
    if (lcf_status st = validate_tables(pr, g)) return st;
    EnginePlan& p = *out = EnginePlan();
    DevProblem& dp = p.dp;
    dp.model = pr.model;
    dp.n_filters = pr.n_filters;
    dp.n_par = pr.n_par;
    dp.use_sigma = pr.use_sigma ? 1 : 0;
    dp.n_dim = dp.n_par + dp.use_sigma;
    dp.sigma_abs = pr.sigma_type == LCF_SIGMA_ABSOLUTE;
    dp.has_priors = pr.priors ? 1 : 0;
    dp.variant = 1;
    dp.use_ctab = p.have_ctab = g.ctab;

    PointLayout L;
    find_epochs(pr, knobs, &L);
    make_columns(pr, &L);
    split_parts(pr, knobs, &L);
    int n_compressed = 0;
    if (lcf_status st = pack_tables(pr, g, &p, &n_compressed)) return st;
    fill_points(pr, L, &p);
    if (lcf_status st = spline_flags(pr, g, &p)) return st;
    plan_lds(pr, g, knobs, n_compressed, &p);
    stage_image(pr, g, &p);
    plan_constants(pr, &p);
    if (lcf_status st = check_prior_kinds(pr, dp.n_dim)) return st;
    p.priors = prior_rows(pr, dp.n_dim);
    return LCF_OK;
}

}  // namespace lcf
