// The engine's layout rules, checked without a device: a few hundred generated problems through plan_engine
// (csrc/lcf_plan.h), the layout's invariants asserted for every plan.  Built and run by `make -C
// lightcurve_fitting_amd/csrc plan_check`, under the address and undefined-behaviour sanitizers; host code only.
//   plan_check          checks, prints a summary, exits 1 on the first violated invariant
//   plan_check --dump   also prints one line per problem: index, status, hash of the arrays in upload order, the
//                       integers of lcf_debug_engine_layout (to compare two versions of the planner)
#include <cinttypes>
#include <cstdio>
#include <map>
#include <set>

#include "lcf_plan.h"

namespace lcf {   // (the library defines these two in lcf_hip.hip)
thread_local std::string g_err;
lcf_status fail(lcf_status st, const std::string& msg) {
    g_err = msg;
    return st;
}
}  // namespace lcf
using namespace lcf;

namespace {

struct Rng {   // splitmix64: the same problems on every machine
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    double unit() { return (double)(next() >> 11) / 9007199254740992.; }
};

enum Shape { kDense, kRagged, kUnshared, kAllEqual, kOneNaN, kShapes };
const char* const kShapeName[] = {"dense", "ragged", "unshared", "all-equal", "one-NaN"};
enum Kind { kPlain, kReddened, kCompanionExact, kCompanionInexact, kKinds };

struct Spec {
    int N, NF, shape, kind;
    bool ctab, htab, itab, big_tables, priors, sigma, shuffle;
    PlanKnobs knobs;
};

// A problem and the arrays its pointers point into.
struct Problem {
    lcf_problem pr{};
    std::vector<double> t, y, dy, a, w, ext, ca, cw, ctmin, ha, hw, htmin, icoef, itmin, knots, spl;
    std::vector<int32_t> filt, off, coff, hoff, kpar, spar, dtpar;
    std::vector<lcf_prior> priors;
};

void level(Rng& r, int NF, int lo, int span, std::vector<int32_t>* off, std::vector<double>* a, std::vector<double>* w) {
    off->assign(1, 0);
    a->reserve(64);   // (no sample at all is still a table: its pointers are not null)
    w->reserve(64);
    for (int f = 0; f < NF; ++f) {
        const int n = lo + r.below(span);
        for (int k = 0; k < n; ++k) {
            a->push_back(5. + 40. * r.unit());
            w->push_back(r.unit() + 0.01);
        }
        off->push_back((int32_t)a->size());
    }
}

void times(Rng& r, const Spec& s, Problem* p) {
    const int N = s.N, NF = s.NF;
    p->t.resize(N);
    p->filt.resize(N);
    for (int i = 0; i < N; ++i) {
        p->t[i] = 57000.25 + 0.5 * (i / NF);   // dense: epoch i / NF holds the filters 0 .. NF-1 (the last maybe fewer)
        p->filt[i] = i % NF;
    }
    if (s.shape == kRagged) {   // 1 .. NF points per epoch, any filters; one epoch with 40 points
        for (int i = 0, ep = 0; i < N; ++ep) {
            const int n = std::min(N - i, ep == 2 ? 40 : 1 + r.below(NF));
            for (int k = 0; k < n; ++k, ++i) {
                p->t[i] = 57000.25 + 0.5 * ep;
                p->filt[i] = r.below(NF);
            }
        }
    } else if (s.shape == kUnshared) {
        for (int i = 0; i < N; ++i) {
            p->t[i] = 57000.25 + 0.37 * i;
            p->filt[i] = r.below(NF);
        }
    } else if (s.shape == kAllEqual) {
        std::fill(p->t.begin(), p->t.end(), 57003.);
    } else if (s.shape == kOneNaN && N > 0) {
        p->t[N / 2] = NAN;
    }
    if (s.shuffle)   // the caller's order is any order
        for (int i = N - 1; i > 0; --i) {
            const int j = r.below(i + 1);
            std::swap(p->t[i], p->t[j]);
            std::swap(p->filt[i], p->filt[j]);
        }
}

void make_problem(const Spec& s, uint64_t seed, Problem* p) {
    Rng r{seed};
    const int N = s.N, NF = s.NF;
    lcf_problem& pr = p->pr;
    pr.abi_version = LCF_ABI_VERSION;
    pr.model = s.kind == kPlain ? LCF_MODEL_SHOCK_COOLING : s.kind == kReddened ? LCF_MODEL_SHOCK_COOLING3 : LCF_MODEL_COMPANION_SHOCKING;
    pr.n_par = s.kind == kPlain ? 5 : s.kind == kReddened ? 7 : 8;
    pr.use_sigma = s.sigma;
    pr.sigma_type = s.sigma ? LCF_SIGMA_ABSOLUTE : LCF_SIGMA_RELATIVE;
    pr.n_filters = NF;
    pr.n_points = N;
    for (double& c : pr.consts) c = 0.5 + r.unit();
    times(r, s, p);
    p->y.resize(N);
    p->dy.resize(N);
    for (int i = 0; i < N; ++i) {
        p->y[i] = 1e20 * (0.5 + r.unit());
        p->dy[i] = 1e18 * (0.5 + r.unit());
    }
    pr.t = p->t.data(); pr.y = p->y.data(); pr.dy = p->dy.data(); pr.filt_idx = p->filt.data();
    level(r, NF, s.big_tables ? 500 : 0, s.big_tables ? 100 : 70, &p->off, &p->a, &p->w);   // (a filter may have no sample)
    pr.tab_off = p->off.data(); pr.tab_a = p->a.data(); pr.tab_w = p->w.data();
    if (s.kind == kReddened) {
        for (size_t k = 0; k < p->a.size(); ++k) p->ext.push_back(1. + 3. * r.unit());
        pr.tab_ext = p->ext.data();
    }
    if (s.ctab) {
        level(r, NF, 0, 24, &p->coff, &p->ca, &p->cw);
        for (int f = 0; f < NF; ++f) p->ctmin.push_back(f % 5 == 4 ? 0. : 2. + r.unit());
        pr.ctab_off = p->coff.data(); pr.ctab_a = p->ca.data(); pr.ctab_w = p->cw.data(); pr.ctab_tmin = p->ctmin.data();
    }
    if (s.htab) {
        level(r, NF, 0, 10, &p->hoff, &p->ha, &p->hw);
        for (int f = 0; f < NF; ++f) p->htmin.push_back(8. + r.unit());
        pr.htab_off = p->hoff.data(); pr.htab_a = p->ha.data(); pr.htab_w = p->hw.data(); pr.htab_tmin = p->htmin.data();
    }
    if (s.itab) {
        pr.itab_m = 16 + 48 * r.below(2);
        pr.itab_u0 = 0.25;
        pr.itab_h = 0.125;
        for (int f = 0; f < NF; ++f) p->itmin.push_back(f % 7 == 3 ? INFINITY : f % 3 == 1 ? 2. : 1.);
        p->icoef.resize((size_t)NF * pr.itab_m * 8);
        for (int f = 0; f < NF; ++f)
            for (int k = 0; k < pr.itab_m * 8; ++k)   // (a filter without an interpolant may hold anything)
                p->icoef[(size_t)f * pr.itab_m * 8 + k] = std::isfinite(p->itmin[f]) ? r.unit() - 0.5 : NAN;
        pr.itab_coef = p->icoef.data(); pr.itab_tmin = p->itmin.data();
    }
    if (s.kind >= kCompanionExact) {
        pr.n_knots = 40 + r.below(80);
        for (int k = 0; k < pr.n_knots; ++k) p->knots.push_back(s.kind == kCompanionExact ? -20. + k : -20. + 1.1 * k + 0.01 * r.unit());
        p->spl.resize((size_t)NF * (pr.n_knots - 1) * 4);
        for (double& v : p->spl) v = r.unit();
        for (int f = 0; f < NF; ++f) {
            p->kpar.push_back(f % 3 == 0 ? 5 : -1);
            p->spar.push_back(f % 3 == 1 ? 6 : -1);
            p->dtpar.push_back(f % 3 == 2 ? 7 : -1);
        }
        pr.spline_knots = p->knots.data(); pr.spline_coef = p->spl.data();
        pr.filt_kasen_par = p->kpar.data(); pr.filt_sifto_par = p->spar.data(); pr.filt_dt_par = p->dtpar.data();
    }
    if (s.priors) {
        for (int i = 0; i < pr.n_par + pr.use_sigma; ++i) p->priors.push_back(lcf_prior{i % 3, 0, 0.1, 10. + i, 5., 1.});
        pr.priors = p->priors.data();
    }
}

// ---- the invariants ---------------------------------------------------------------------------------------------------
int g_index = 0;
const Spec* g_spec = nullptr;
#define CHECK(cond)                                                                                                     \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            std::fprintf(stderr, "plan_check: problem %d (N %d, %d filters, %s, kind %d, parts %d): %s\n", g_index,     \
                         g_spec->N, g_spec->NF, kShapeName[g_spec->shape], g_spec->kind, g_spec->knobs.parts, #cond);   \
            return false;                                                                                               \
        }                                                                                                               \
    } while (0)

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// (epoch, filter, y, scale) of a point, to tell points apart with
using PointKey = std::tuple<int, int, double, double>;

bool check_points(const Problem& pb, const EnginePlan& p) {
    const lcf_problem& pr = pb.pr;
    const DevProblem& dp = p.dp;
    const int N = (int)pr.n_points;
    CHECK(dp.n_points == N && (int)p.orig.size() == N && (int)p.epoch_t.size() == dp.n_epochs);
    std::vector<char> seen(N, 0);
    for (int i = 0; i < N; ++i) {   // pt_orig is a permutation and the point arrays follow it
        const int o = p.orig[i];
        CHECK(o >= 0 && o < N && !seen[o]);
        seen[o] = 1;
        CHECK(same(p.t[i], pr.t[o]) && same(p.y[i], pr.y[o]) && same(p.dy[i], pr.dy[o]) && p.filt[i] == pr.filt_idx[o]);
        CHECK(same(p.inv_dy[i], 1. / pr.dy[o]) && same(p.yd[i].x, pr.y[o]) && same(p.yd[i].y, pr.use_sigma ? pr.dy[o] : 1. / pr.dy[o]));
        CHECK(p.epoch[i] >= 0 && p.epoch[i] < dp.n_epochs && same(p.epoch_t[p.epoch[i]], pr.t[o]));
        if (pr.n_filters <= 64) CHECK(p.fe[i] == (p.filt[i] | (p.epoch[i] << 6)));
    }
    CHECK(pr.n_filters <= 64 || p.fe.empty());
    // parts: contiguous, not empty, whole epochs, filter-sorted inside
    CHECK(dp.n_parts >= 1 && dp.n_parts <= kMaxParts && dp.part_start[0] == 0);
    std::vector<int> part_of_epoch(dp.n_epochs, -1);
    int n_chunks = 0, cpb = 1;
    for (int j = 0; j <= kMaxParts; ++j) {
        if (j >= dp.n_parts) {
            CHECK(dp.part_start[j] == N && dp.part_ep0[j] == dp.n_epochs && dp.part_col0[j] == dp.em_cols);
            continue;
        }
        const int lo = dp.part_start[j], hi = dp.part_start[j + 1];
        CHECK(lo <= hi && (lo < hi || N == 0));
        const int c = (hi - lo + kBlock - 1) / kBlock;
        n_chunks += c;
        cpb = std::max(cpb, c);
        int first = dp.n_epochs;
        for (int i = lo; i < hi; ++i) {
            CHECK(i == lo || p.filt[i - 1] <= p.filt[i]);
            int& owner = part_of_epoch[p.epoch[i]];
            CHECK(owner == -1 || owner == j);   // no epoch is split across parts
            owner = j;
            first = std::min(first, p.epoch[i]);
        }
        const bool finite = std::all_of(pr.t, pr.t + N, [](double v) { return std::isfinite(v); });
        CHECK(dp.part_ep0[j] == (finite ? first : dp.n_epochs));
    }
    CHECK(dp.n_chunks == n_chunks && dp.cpb == cpb);
    for (int e = 1; e < dp.n_epochs; ++e) CHECK(part_of_epoch[e - 1] <= part_of_epoch[e]);   // parts own ranges of epochs
    // the epoch-major copy
    if (!dp.use_therm) {
        CHECK(p.em_t.empty() && p.em_yd.empty() && p.em_filt.empty() && dp.em_cols == 0 && !dp.em_dense);
        return true;
    }
    const int n_cols = dp.em_cols, K = dp.em_k;
    CHECK(N > 0 && (int)p.em_t.size() == n_cols && p.em_filt.size() == (size_t)K * n_cols && p.em_yd.size() == p.em_filt.size());
    std::map<PointKey, int> points;
    for (int i = 0; i < N; ++i) ++points[PointKey(p.epoch[i], p.filt[i], p.yd[i].x, p.yd[i].y)];
    bool dense = K == pr.n_filters && n_cols == dp.n_epochs;
    std::vector<int> in_part(dp.n_parts, 0);
    for (int c = 0, part = 0; c < n_cols; ++c) {
        CHECK(c == 0 || p.em_t[c - 1] <= p.em_t[c]);
        const int ep = (int)(std::lower_bound(p.epoch_t.begin(), p.epoch_t.end(), p.em_t[c]) - p.epoch_t.begin());
        CHECK(ep < dp.n_epochs && same(p.epoch_t[ep], p.em_t[c]));   // a column holds points of ONE epoch ...
        while (c >= dp.part_col0[part + 1]) ++part;
        CHECK(part < dp.n_parts && part_of_epoch[ep] == part);         // ... of its part's
        int filled = 0;
        for (int k = 0; k < K; ++k) {
            const int f = p.em_filt[(size_t)k * n_cols + c];
            const double2 yd = p.em_yd[(size_t)k * n_cols + c];
            if (f < 0) {
                CHECK(same(yd.x, 0.) && same(yd.y, 0.));
                continue;
            }
            CHECK(filled == k);                                         // ... from k = 0, without a gap
            CHECK(k == 0 || p.em_filt[(size_t)(k - 1) * n_cols + c] <= f);   // ... in filter order
            ++filled;
            auto it = points.find(PointKey(ep, f, yd.x, yd.y));
            CHECK(it != points.end() && it->second > 0);               // every point sits in exactly one slot
            --it->second;
            dense = dense && f == k;
        }
        CHECK(filled > 0);
        dense = dense && filled == K;
        in_part[part] += filled;
    }
    for (const auto& kv : points) CHECK(kv.second == 0);
    for (int j = 0; j < dp.n_parts; ++j) CHECK(in_part[j] == dp.part_start[j + 1] - dp.part_start[j]);   // part_col0 agrees with part_start
    CHECK(dp.part_col0[0] == 0 && (dp.em_dense != 0) == dense);
    return true;
}

bool check_tables(const Problem& pb, const PlanKnobs& knobs, const EnginePlan& p) {
    const lcf_problem& pr = pb.pr;
    const DevProblem& dp = p.dp;
    const int NF = pr.n_filters;
    const bool reddened = pr.model == LCF_MODEL_SHOCK_COOLING3;
    CHECK(dp.n_tab == (int)p.tab.size() && dp.n_tab > 0 && (int)p.f_desc.size() == NF);
    CHECK(reddened ? p.ext.size() == p.tab.size() || (p.ext.empty() && pb.a.empty()) : p.ext.empty());
    int n_compressed = 0;
    std::set<int> taken;
    const auto one = [&](int off, int cnt, const int32_t* src_off, int f, bool full) {   // a level of a filter
        const int n_src = src_off ? src_off[f + 1] - src_off[f] : 0;
        CHECK(cnt % 4 == 0 && cnt >= n_src && cnt < n_src + 4 && off >= 0 && off + cnt <= dp.n_tab);
        for (int k = 0; k < cnt; ++k) {
            CHECK(taken.insert(off + k).second);   // (no two levels overlap)
            if (k >= n_src) CHECK(same(p.tab[off + k].y, 0.) && p.tab[off + k].x > 0.);   // padding weighs nothing
            if (full && reddened) CHECK(k < n_src ? std::isfinite(p.ext[off + k]) : same(p.ext[off + k], 0.));
        }
        return true;
    };
    for (int f = 0; f < NF; ++f) {
        const FiltDesc& d = p.f_desc[f];
        CHECK(one(d.off, d.cnt, pr.tab_off, f, true));
        CHECK(one(d.coff, d.ccnt, p.have_ctab ? pr.ctab_off : nullptr, f, false));
        CHECK(one(d.hoff, d.hcnt, p.have_ctab && pr.htab_off ? pr.htab_off : nullptr, f, false));
        CHECK(p.tab_off[2 * f] == d.off && p.tab_off[2 * f + 1] == d.cnt && p.ctab_off[2 * f] == d.coff && p.ctab_off[2 * f + 1] == d.ccnt);
        CHECK(d.ccnt + d.hcnt == 0 || d.off >= d.coff + d.ccnt);   // the compressed levels come first
        n_compressed += d.ccnt + d.hcnt;
    }
    CHECK(dp.n_lds_tab == 0 || dp.n_lds_tab == n_compressed || dp.n_lds_tab == dp.n_tab);
    CHECK(dp.n_lds_tab <= knobs.lds_tab_max && dp.tab_in_lds == (dp.n_lds_tab > 0) && (NF <= kLdsFiltMax || !dp.tab_in_lds));
    CHECK(!dp.redden_slow || (reddened && !dp.tab_in_lds));
    CHECK((dp.n_itab_lds == 0 || (dp.use_itab && dp.tab_in_lds && dp.n_itab_lds == NF * dp.itab_m * 8)) && dp.n_itab_lds % 2 == 0);
    CHECK((dp.n_spl_lds == 0 || (dp.knot_h > 0. && dp.tab_in_lds && dp.n_spl_lds == NF * (dp.n_knots - 1) * 4)) && dp.n_spl_lds % 2 == 0);
    CHECK(dp.stage_d2 == dp.n_lds_tab + kFdD2 * NF + dp.n_itab_lds / 2 + dp.n_spl_lds / 2);
    CHECK(dp.stage_n16 == (int)p.image.size() && dp.stage_n16 == kLdsHead / 2 + (dp.tab_in_lds ? dp.stage_d2 : 0));
    CHECK(p.lds_bytes == (size_t)dp.stage_n16 * 16 && p.lds_bytes <= 160 * 1024);   // (a CU's LDS)
    CHECK(p.knots.size() == (size_t)dp.n_knots && (dp.knot_h == 0. || same(dp.knot_inv_h, 1. / dp.knot_h)));
    CHECK(g_spec->kind != kCompanionExact || dp.knot_h == 1.);
    CHECK(g_spec->kind != kCompanionInexact || dp.knot_h == 0.);
    return true;
}

std::vector<Spec> specs() {
    const int Ns[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 700, 2049, 5000}, NFs[] = {1, 3, 8, 65};
    std::vector<Spec> out;
    int i = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int N : Ns)
            for (int NF : NFs)
                for (int shape = 0; shape < kShapes; ++shape, ++i) {
                    // the other choices cycle with periods that share no factor with each other or the loops above
                    Spec s{N, NF, shape, (i / 3 + pass) % kKinds, i % 2 == 0, i % 4 == 0, i % 3 != 1, i % 7 == 5, i % 5 < 2,
                           i % 11 == 3, i % 2 == 1 || pass == 1, PlanKnobs{}};
                    s.knobs.parts = (i + 4 * pass) % 9;
                    s.knobs.shared_epochs_only = i % 13 < 4;
                    s.knobs.lds_tab_max = i % 17 == 6 ? 0 : kLdsTabMax;
                    out.push_back(s);
                }
    return out;
}

}  // namespace

int main(int argc, char** argv) {
    const bool dump = argc > 1 && std::string(argv[1]) == "--dump";
    const std::vector<Spec> all = specs();
    int planned = 0, therm = 0, in_lds = 0, dense = 0;
    for (g_index = 0; g_index < (int)all.size(); ++g_index) {
        const Spec& s = all[g_index];
        g_spec = &s;
        Problem pb;
        make_problem(s, 1000 + g_index, &pb);
        EnginePlan plan;
        const lcf_status st = plan_engine(pb.pr, s.knobs, &plan);
        if (st != LCF_OK) {
            std::fprintf(stderr, "plan_check: problem %d refused: %s\n", g_index, g_err.c_str());
            return 1;
        }
        if (!check_points(pb, plan) || !check_tables(pb, s.knobs, plan)) return 1;
        ++planned;
        therm += plan.dp.use_therm;
        in_lds += plan.dp.tab_in_lds;
        dense += plan.dp.em_dense;
        if (dump) {
            HashArena arena;
            DevProblem dp = plan.dp;
            int *tab_off, *ctab_off;
            double* ctmin;
            upload_plan(plan, arena, &dp, &tab_off, &ctab_off, &ctmin);
            int32_t v[kLayoutInts];
            layout_ints(plan.dp, v);
            std::printf("%d %d %016" PRIx64, g_index, (int)st, arena.hash);
            for (int x : v) std::printf(" %d", x);
            HashArena scalars;   // (the problem's scalars; its pointers are null in a plan)
            void* none;
            scalars.put(&plan.dp, sizeof plan.dp, &none);
            std::printf(" %016" PRIx64 " %" PRId64 " %zu %d %d\n", scalars.hash, plan.samples_per_eval, plan.lds_bytes,
                        (int)plan.have_ctab, (int)plan.have_itab);
        }
    }
    std::fprintf(stderr, "plan_check: %d problems planned, every invariant holds (%d epoch-major, %d dense, %d with tables in LDS)\n",
                 planned, therm, dense, in_lds);
    return 0;
}
