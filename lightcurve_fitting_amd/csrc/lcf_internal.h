// What lcf_hip.hip (kernels, launches, runs over ranks and populations), lcf_engine.hip (engine creation), lcf_sampler.hip
// (the bookkeeping of runs) and lcf_tempered.hip (the tempered driver beside the sampler) share: what the sampler's
// kernels and the host exchange, the engine and the sampler behind the C ABI's opaque pointers, and the host functions
// that cross the files.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lcf.h"
#include "lcf_device.h"
#include "lcf_host.h"

using namespace lcf;

namespace {

// ---- ensemble sampler ---------------------------------------------------------------------------------------------
// Half-steps are numbered globally (g = 0, 1, 2, ...).  Everything a proposal needs later for its accept/reject is
// kept per proposal slot in buffers double-buffered by the parity of g, so that ONE kernel (k_next) can, fully in
// parallel and without any inter-workgroup hand-off, (i) commit the previous half-step and (ii) draw the next
// proposals: a thread that needs the position of a walker whose previous move is not committed yet simply evaluates
// that walker's accept test itself (a pure function of immutable per-slot data).
// Per proposal slot: what its accept test needs besides the new log-posterior (one 32-byte load).
struct SlotRec {
    double zl;      // (n_dim - 1) ln z
    double lnu;     // ln u of the accept test
    double lp_old;  // log-posterior of the walker when the proposal was drawn
    double lpri;    // log-prior of the proposal
};
// Per (step, half, slot): the state-independent part of the stretch move, drawn for the whole run in advance.
struct DrawRec {
    int wid, pid;      // active walker and its partner from the complementary colour
    int wprev, pprev;  // their proposal slots in the previous half-step of the run (-1: not active there)
    double z;          // stretch factor
    double zl;         // (n_dim - 1) ln z
    double lnu;        // ln u
    int wage, page;    // half-steps since the walker / the partner last moved (1..3; 0 without slot bookkeeping)
};

struct DevSampler {
    int n_walkers, n_half, n_dim, store_chain;
    uint32_t key0, key1;
    int inline_finalize;  // 1: accept tests sum the chi^2 partials themselves; 0: they read the gathered newlp
    int n_peers;          // > 0: the rows travel through peer mailboxes (below) instead of part2 + a collective
    double a;
    double* X;          // [n_walkers][n_dim]  committed positions
    double* LP;         // [n_walkers]         committed log-posteriors
    double* Q[2];       // [n_half][n_dim]     proposals
    SlotRec* rec[2];    // [n_half]
    double* newlp[2];   // [n_half]            log-posterior of the proposal (finalize kernel / all-gather)
    double* part2[2];   // [n_half][n_parts + 1] per slot: chi^2 partial sums, then the log-prior; half-step parity 0 / 1
    double* chain;      // [n_steps][n_walkers][n_dim]
    double* chain_lp;   // [n_steps][n_walkers]
    long long* nacc;    // [n_walkers]
    int* err;
    // Peer mailboxes (multi-GPU without a collective): every rank owns a mailbox [4 generations][n_half][row] of
    // 16-byte entries; a rank that has evaluated a proposal writes the entry of each of the row's numbers straight into
    // EVERY rank's mailbox (peer memory mapped through IPC; over xGMI on a node), and whoever needs the row polls its
    // own copy.  mbox = this rank's, peer_mbox[r] = rank r's as mapped here (own included).
    unsigned long long* mbox;
    unsigned long long* peer_mbox[kMaxPeers];
    // Row boards (multi-GPU, one workgroup per proposal: lcf_sampler_run_rows).  Every rank owns a board
    // [kRing versions][n_walkers][n_dim + 2] of 16-byte entries in uncached memory -- a walker's position, its
    // log-posterior and its acceptance count after each of its moves, tagged with the half-step -- followed by one
    // progress word per rank, an abort word and four words that say what an aborted launch was waiting for.  The rank
    // that moves a walker posts the row on EVERY rank's board; nobody else computes anything about that walker.
    unsigned long long* board;
    unsigned long long* peer_board[kMaxPeers];
    int n_board_ranks, board_rank;
    int ring, pad_ring;   // versions a board keeps (a power of two): kRing between ranks, kRunRing for one-launch runs
    // One-launch runs write the snapshot the host reads after a run -- [error word | X | LP | n_accepted] in pinned host
    // memory -- themselves, with the state, in their last step; a workgroup that meets a NaN or gives up a wait says so in
    // a word of its own behind it (snap_flags[blockIdx.x & (kSnapFlags - 1)] = 1 / snap_flags[kSnapFlags + ...] = 2;
    // plain stores, cleared with the state only: errors stay until set_state).  Null: the snapshot kernel does it.
    unsigned long long* snap_out;
    unsigned int* snap_flags;
    // ... and write the state into a second set of buffers (the host then swaps the two sets): a launch that gives up
    // leaves the state it started from untouched, and the host runs the same steps again, a launch per half-step.
    double* X_out;
    double* LP_out;
    long long* nacc_out;
    // Bound of every wait for another rank (mailbox entries, board rows, progress words), in ticks of the 100 MHz wall
    // clock: peer_wait_ticks().  A rank's stream holds only a few ms of launches, so a host that stalls longer than
    // this on ONE rank ends the run on ALL of them -- the default is therefore seconds, not the 0.5 s of round 2.
    unsigned long long wait_ticks;
    // ... and of the wait of a resident launch (k_solo_run) for the REST OF ITSELF: LCF_RESIDENT_WAIT_S, default 0.05 s.
    unsigned long long resident_ticks;
};

// Population mode: the draw records of MANY samplers come from one launch of each generation kernel (k_make_perm_multi,
// k_draws_multi in lcf_sampler.hip: blockIdx.y = sampler; equal walker counts and blocks).  What differs from sampler to
// sampler -- the key of its RNG, its walker dimension (the accept test's (n_dim - 1) ln z), its stretch scale, its
// buffers -- comes from an array in device memory.
struct GenItem {
    uint32_t key0, key1;
    int n_dim;
    double a;
    int* perm[2];
    int* slot[2];
    DrawRec* draws[2];
};

// ---- row boards: tagged words in device memory ---------------------------------------------------------------------
// One float64 = ONE 16-byte entry of two 8-byte granules {32 data bits, 32-bit tag}, tag = half-step after which the row
// holds + 1 (the LL protocol of the mailboxes above, the entry posted with one 16-byte store and polled with one 16-byte
// load: each granule carries its own tag, so an entry that arrives in two halves is still never mistaken for complete).
// A row = the walker's n_dim + 2 numbers in consecutive entries, padded to whole 128-byte lines (board_row_entries):
// the lanes of ONE store instruction post a row, into one line (n_dim <= 6) of each board it goes to.
// Between ranks (k_solo<BOARD> per half-step, k_solo_run<..., RANKS> per block of half-steps): a ring of kRing versions.
// Safe because (a) a reader asks for exactly the version the draw record names (DrawRec::wage / page) and waits,
// bounded, until both granules carry its tag; (b) progress words bound how far ranks drift apart: with a launch per
// half-step no rank starts half-step G before every rank has finished G - 2; with a launch per block of up to kRunSpan
// half-steps no rank starts a launch before every rank has STARTED the launch before the previous one (a rank's
// progress word = the first half-step of the launch it has reached, posted by that launch itself: stream order proves
// that everything in front of it, its row collection included, is complete).  Everything a rank still reads is then at
// most 3 kRunSpan + 2 versions behind anything another rank writes: kRing = 256 versions are never overrun.
constexpr int kRing = 256;
constexpr int kSnapFlags = 1024;
// One-launch runs of ONE GPU (k_solo_run, k_pop_run): a launch covers at most kRunSpanSolo half-steps, reads versions >= G - 3 and
// writes G + 1: kRunRing versions are never overrun however far the workgroups of a launch drift apart.
// (Between ranks a launch covers at most kRunSpan half-steps -- the ring of the inter-rank boards bounds it, below; on one
// GPU up to kRunSpanSolo: a launch's start-up -- staging, first fetch, every workgroup arriving, ~18 us at configs[1] --
// is then paid once per 256 half-steps instead of once per 64: 5.41 -> 5.31 us per half-step over a 1000-step run.)
#ifndef LCF_RUN_SPAN_SOLO
#define LCF_RUN_SPAN_SOLO 256
#endif
constexpr int kRunSpanSolo = LCF_RUN_SPAN_SOLO;
constexpr int kRunRing = 2 * kRunSpanSolo;
constexpr int kRunSpan = 64;
static_assert((kRunRing & (kRunRing - 1)) == 0 && kRunRing >= kRunSpanSolo + 8, "the ring of a one-launch run covers a launch");
constexpr int kRunStoreChain = 1, kRunFlip = 2;   // k_solo_run's run_flags: the run stores its chain; its start state is in X_out / LP_out / nacc_out
// 32-bit words behind the rows: progress per rank, abort, 4 x diagnosis, arrivals (workgroups of resident launches that
// have started, counted up from launch to launch: a launch knows the count that says "all of mine are there")
constexpr int kBoardTail = kMaxPeers + 1 + 4 + 1 + 4;
constexpr int kBoardClear = 10;                 // the last words of the tail that set_state clears: abort ... arrivals, and
                                                // the four words of the entry a given-up wait last saw (diagnosis)
static_assert(kRing >= 3 * kRunSpan + 8, "the ring of the inter-rank boards must cover three launches");

__host__ __device__ inline int board_row_entries(int n_dim) { return (n_dim + 2 + 7) & ~7; }   // 16-byte entries per row
__host__ __device__ inline size_t board_rows_bytes(int ring, int n_walkers, int n_dim) {
    return (size_t)ring * n_walkers * board_row_entries(n_dim) * 16;
}

// ---- what a resident launch reads in EVERY half-step and no half-step changes -----------------------------------------
// k_solo_run reads problem and sampler through constant-address-space pointers: a scalar load, and a wait for the scalar
// cache, wherever a field is used -- 26 loads and 18 serialised waits per half-step on the one wave everybody else waits
// for, plus the 64-bit multiplications of a row's address and the select chains of part_col0[part], all for values that
// are the same in every half-step of a launch.  The launch therefore writes them ONCE, already multiplied out, into
// this block of its dynamic LDS (behind the half-step's scratch words; k_solo_run fills it in front of its loop), and
// the half-step reads a phase's share of it with 16-byte LDS reads issued together with the phase's other LDS reads.
// Every group below is 16 bytes or a multiple, at a 16-byte offset.  Resident kernels only (BOARD >= 2 in
// solo_half_step): a launch of one half-step would pay the fill for nothing.
struct alignas(16) RunUniforms {
    // rows: entry (tag, wid, col) = board + (tag & ring_mask) * ver_bytes + wid * row_bytes + 16 col
    unsigned long long* board;
    unsigned int ring_mask, row_bytes;
    unsigned long long ver_bytes;       // one version of every walker's row
    unsigned int* abort_word;           // the board's abort word (board_aborted)
    // accept
    double sum0;                        // what the chi^2 sum starts from: 0 with a fitted sigma, else log_norm_const
    int n_parts, n_walkers;
    // head
    int n_dim, n_par, has_priors, model;
    // the state, the host's snapshot and the chain as this launch writes them (the set of state buffers chosen)
    double* X;
    double* LP;
    long long* nacc;
    unsigned long long* snap_out;
    double* chain;
    double* chain_lp;
    // columns: the interpolants' grid, where they are staged (byte offset in the dynamic LDS, -1: not staged), and per
    // group of 256 threads (of the 512-thread kernels) the columns [c0, c1) of its first part and whether lean_column may
    // take them
    double itab_u0, itab_inv_h;
    int itab_m, itab_at, nd, pad1;      // (nd: the sampler's n_dim, what a row holds)
    struct Group { int c0, c1, lean, pad; } group[2];
    double consts[12];                  // DevProblem::consts
    PriorDev priors[kMaxDim];           // the parameters' priors (flat where the problem has none)
};
static_assert(sizeof(RunUniforms) % 16 == 0 && sizeof(RunUniforms) <= 1024, "a small block of 16-byte groups");

// What every k_solo<...> and every k_solo_run<...> is to the host: one signature per family.
using SoloKernel = void (*)(const DevProblem*, const DevSampler, long long, const DrawRec*, const DrawRec*, long long, long long, int);
using SoloRunKernel = void (*)(const DevProblem*, const DevSampler*, long long, const DrawRec*, long long, int, long long, int, int,
                               unsigned int, int, int, long long);

}  // namespace

// How the half-steps of ONE sampler's run are executed (a run of one GPU, or a rank's share of a row-board run): decided
// by plan_run (lcf_hip.hip) before anything of the run is enqueued; the launchers take it and choose nothing.
struct RunPlan {
    // what is planned: a row-board run, of this rank's slots [lo, hi) (one GPU: all of a half-step's)
    bool rows = false;
    int lo = 0, hi = 0;
    // what the plan is
    int form = LCF_KERNEL_PHASES;         // LCF_KERNEL_RUN (k_solo_run), _SOLO (k_solo), _FUSED or _PHASES
    int instance[4] = {-1, -1, -1, -1};   // <ND, NP, M, ranks> of the k_solo / k_solo_run taken (-1: k_fused / phases)
    SoloKernel solo = nullptr;            // the kernel of that instance: form _SOLO ...
    SoloRunKernel run = nullptr;          // ... form _RUN
    int threads = 0;
    size_t lds = 0;
    bool need_slots = true;               // the draw records carry each walker's slot in the previous half-step
    // resident plans: half-steps a launch covers at most; LCF_RUN_GRID and LCF_RUN_TEST_MISSING as the run found them;
    // and the workgroups the device holds at once (prepare_run)
    int span = 0, max_grid = 0, cap = 0;
    bool test_missing = false;
};

struct lcf_engine {
    int device = 0;
    DevProblem dp{};
    std::vector<void*> owned;
    hipStream_t stream = nullptr;
    int64_t samples_per_eval = 0;
    size_t lds_bytes = 0;
    int* d_tab_off = nullptr;   // per filter: (offset, count) of the full table in the device table
    int* d_ctab_off = nullptr;  // per filter: (offset, count) of the compressed table
    double* d_ctmin = nullptr;
    bool have_ctab = false, have_itab = false;
    int n_cus = 256;             // compute units of the device (launch shapes depend on it)
    DevProblem* d_dp = nullptr;  // `dp` in device memory, for the kernels that read it through a pointer
    // LCF_MODEL_CUSTOM: the likelihood / evaluation kernel and the key kernel (lcf_predict_custom) of the attached program
    // on this device (lcf_engine_set_custom; null: none yet) and the redshift its state function is handed
    hipFunction_t custom_points = nullptr, custom_keys = nullptr;
    double custom_z = 0.;
    lcf_status sync_dp();        // after every change of `dp`
    // workspace for n walkers
    int64_t cap = 0;
    double *wP = nullptr, *wcoef = nullptr, *wlprior = nullptr, *wpart = nullptr, *wout = nullptr;
    double2* wtherm = nullptr;
    // scratch for evaluate-type calls
    size_t big_bytes = 0;
    double* wbig = nullptr;
    // upper limits (lcf_engine_set_limits, lcf_limits.hip): the caller's engine on the limits' points, L_lim and dy of the
    // n_lim limits on the device, and the model values of lim_rows rows at a time, [lim_rows][n_lim] (reserve)
    lcf_engine* lim_at = nullptr;
    int64_t n_lim = 0, lim_rows = 0;
    double *lim_L = nullptr, *lim_dy = nullptr, *lim_m = nullptr;
    // live lcf_samplers on this engine (their kernels compute the likelihood themselves: limits and a template are
    // refused while there are any).  Shared with them: a sampler may be destroyed after its engine.
    std::shared_ptr<int> samplers = std::make_shared<int>(0);
    // second component (lcf_engine_set_template, lcf_template.hip): a stretched template added to the model.  The rows
    // then have tpl_extra columns more than the engine was created with (dp.n_dim has grown; sigma stays last, dp.priors
    // points at tpl_priors); base_* are what creation set, for detaching.  On the device: the knots, the per-filter cubic
    // coefficients [n_filters][tpl_nk - 1][4], per filter the row columns of its factor and offset (-1: none), the
    // photometry in the CALLER'S order (the order of the points launch's output) and the model values of tpl_rows rows
    // at a time, [tpl_rows][n_points] (reserve).
    bool tpl = false;
    int tpl_nk = 0, tpl_extra = 0, tpl_tmax = -1, tpl_s = -1;
    int base_n_dim = 0, base_has_priors = 0;
    const PriorDev* base_priors = nullptr;
    double tpl_inv_h = 0.;
    int64_t tpl_rows = 0;
    double *tpl_knots = nullptr, *tpl_coef = nullptr, *tpl_t = nullptr, *tpl_y = nullptr, *tpl_dy = nullptr, *tpl_m = nullptr;
    int *tpl_filt = nullptr, *tpl_fac = nullptr, *tpl_off = nullptr;
    PriorDev* tpl_priors = nullptr;

    ~lcf_engine() {
        hipSetDevice(device);
        for (void* p : owned) hipFree(p);
        free_ws();
        if (wbig) hipFree(wbig);
        for (double* p : {lim_L, lim_dy, lim_m})
            if (p) hipFree(p);
        free_template();
        if (stream) hipStreamDestroy(stream);
    }
    void free_ws() {
        for (double** p : {&wP, &wcoef, &wlprior, &wpart, &wout}) {
            if (*p) hipFree(*p);
            *p = nullptr;
        }
        if (wtherm) hipFree(wtherm);
        wtherm = nullptr;
        cap = 0;
    }
    void free_template() {
        for (void* p : {(void*)tpl_knots, (void*)tpl_coef, (void*)tpl_t, (void*)tpl_y, (void*)tpl_dy, (void*)tpl_m,
                        (void*)tpl_filt, (void*)tpl_fac, (void*)tpl_off, (void*)tpl_priors})
            if (p) hipFree(p);
        tpl_knots = tpl_coef = tpl_t = tpl_y = tpl_dy = tpl_m = nullptr;
        tpl_filt = tpl_fac = tpl_off = nullptr;
        tpl_priors = nullptr;
        tpl_rows = 0;
    }
    lcf_status reserve_limits(int64_t n);   // lcf_limits.hip: the limit engine's workspace and lim_m for n rows
    lcf_status reserve_template(int64_t n); // lcf_template.hip: tpl_m for n rows
    lcf_status reserve(int64_t n) {
        if (lim_at)
            if (lcf_status st = reserve_limits(n)) return st;
        if (tpl)
            if (lcf_status st = reserve_template(n)) return st;
        if (n <= cap) return LCF_OK;
        LCF_HIP(hipStreamSynchronize(stream));
        free_ws();
        const int64_t c = std::max<int64_t>(n, 64);
        LCF_HIP(hipMalloc((void**)&wP, c * dp.n_dim * sizeof(double)));
        LCF_HIP(hipMalloc((void**)&wcoef, c * kNCoef * sizeof(double)));
        LCF_HIP(hipMalloc((void**)&wlprior, c * sizeof(double)));
        LCF_HIP(hipMalloc((void**)&wpart, c * (dp.n_parts + 1) * sizeof(double)));
        LCF_HIP(hipMalloc((void**)&wout, c * sizeof(double)));
        if (dp.use_therm) LCF_HIP(hipMalloc((void**)&wtherm, c * dp.n_epochs * sizeof(double2)));
        cap = c;
        return LCF_OK;
    }
    lcf_status reserve_big(size_t bytes) {
        if (bytes <= big_bytes) return LCF_OK;
        LCF_HIP(hipStreamSynchronize(stream));
        if (wbig) hipFree(wbig);
        wbig = nullptr;
        big_bytes = 0;
        LCF_HIP(hipMalloc((void**)&wbig, bytes));
        big_bytes = bytes;
        return LCF_OK;
    }
};

namespace lcf {
// Memory that kernels poll comes from, and goes back to, a pool of this process (lcf_sampler.hip).
// polled_alloc: `bytes` of it on the current device, cleared (complete on return).
void polled_give(int dev, bool uncached, size_t bytes, void* p);
lcf_status polled_alloc(int dev, bool uncached, size_t bytes, void** out);
// lcf_engine.hip: an engine on `device` with nothing in it yet -- the device current, its compute units, its stream.
lcf_status engine_shell(int32_t device, std::unique_ptr<lcf_engine>* out);
// lcf_custom.hip: engines of LCF_MODEL_CUSTOM.  custom_refuse: LCF_ERR_UNSUPPORTED, naming the supported route, for what is
// compiled per model (`what` names the caller); LCF_OK for every other engine.
lcf_status custom_refuse(const lcf_engine* e, const char* what);
lcf_status custom_launch(lcf_engine* e, int mode, int w_lo, int n, const double* dP, const double* lprior, double* out0,
                         double* out1, hipStream_t st);
lcf_status custom_ready(const lcf_engine* e);
// lcf_central.hip: engines of LCF_MODEL_ARNETT / LCF_MODEL_MAGNETAR (a bolometric light curve, no filters).
// central_engine_create: what lcf_engine_create does for these two ids; central_refuse: as custom_refuse;
// central_launch: rows [w_lo, w_lo + n) of P through k_central_points on st -- mode 0: chi^2 partial sums -> out0 (the
// engine's part buffer; rows with lprior == -inf skipped), 1: L(t) -> out0[row][point], the caller's order.
inline bool is_central(int model) { return model == LCF_MODEL_ARNETT || model == LCF_MODEL_MAGNETAR; }
lcf_status central_engine_create(const lcf_problem* pr, int32_t device, lcf_engine** out);
lcf_status central_refuse(const lcf_engine* e, const char* what);
lcf_status central_launch(lcf_engine* e, int mode, int w_lo, int n, const double* dP, const double* lprior, double* out0,
                          hipStream_t st);
// lcf_limits.hip: engines with upper limits attached (lcf_engine_set_limits).  limits_refuse: as custom_refuse, for what
// computes the likelihood in kernels of its own; limits_add: the censored terms of rows [0, n) added to dout, enqueued
// on st behind the launches that wrote dout (rows whose e->wlprior is -inf are left alone).
lcf_status limits_refuse(const lcf_engine* e, const char* what);
lcf_status limits_add(lcf_engine* e, int64_t n, const double* dP, double* dout, hipStream_t st);
// lcf_hip.hip: the model at the limits' points -- rows [lo, lo + m) of dP through e->lim_at, the launches of
// lcf_model_evaluate, enqueued on st -> e->lim_m[m][n_lim]; `prepare`: the coefficients of all n rows first (k_prepare into
// e's workspace, no prior), for callers that have not just evaluated the rows' likelihood.
lcf_status limits_model(lcf_engine* e, int64_t n, int64_t lo, int64_t m, const double* dP, bool prepare, hipStream_t st);
// lcf_template.hip: engines with a second component attached (lcf_engine_set_template).  template_refuse: as
// limits_refuse; template_loglike: what logprob_dev enqueues behind its k_prepare for such an engine -- per chunk of
// e->tpl_rows rows the model values (template_model) and k_template, which writes dout.
lcf_status template_refuse(const lcf_engine* e, const char* what);
lcf_status template_loglike(lcf_engine* e, int64_t n, const double* dP, double* dout, hipStream_t st);
// lcf_hip.hip: the engine's own model at its own points -- rows [lo, lo + m) of dP through the launches of
// lcf_model_evaluate (k_thermal first where epochs are shared), enqueued on st -> out[m][n_points], the caller's order
// of the points; the rows' coefficients are in e->wcoef (k_prepare has run).  prepare_rows: k_prepare of rows [0, n)
// into e's workspace, no prior, for callers that have not just evaluated the rows' likelihood.
lcf_status prepare_rows(lcf_engine* e, int64_t n, const double* dP, hipStream_t st);
lcf_status template_model(lcf_engine* e, int64_t lo, int64_t m, const double* dP, double* out, hipStream_t st);
}  // namespace lcf

struct lcf_sampler {
    lcf_engine* e = nullptr;
    int device = 0;           // e->device, kept for the destructor
    std::shared_ptr<int> engine_samplers;   // e->samplers, counted down when this sampler goes
    DevSampler ds{};
    std::vector<void*> owned;
    double *coef = nullptr, *lprior = nullptr;
    // The state-independent draws of a run are produced in BLOCKS of steps, two buffers (block b lives in buffer b & 1):
    // device memory does not grow with the run, the first half-step starts after a short first block, and nothing on
    // the host waits for the generation.  The generation kernels go on the SAME stream as the half-steps, between two
    // of them: block b + 1 right behind the first launch of block b (the last reader of the buffer it overwrites), so
    // stream order is all the synchronisation there is.  (Measured at 1024 walkers x 2000 steps: a low- or
    // normal-priority side stream with events cost 3-4 % of the whole run however rarely it was used; the inline
    // kernels cost 40 us per 256 steps.)
    int64_t blk_first = 0, blk_steps = 0;          // steps in block 0 and in every later block
    int64_t blk_cap = 0;                           // steps a buffer holds
    int* d_perm[2] = {nullptr, nullptr};           // [blk_cap][n_walkers]
    DrawRec* d_draws[2] = {nullptr, nullptr};      // [blk_cap][2][n_half]
    int* d_slot[2] = {nullptr, nullptr};           // [1 + 2 blk_cap][n_walkers] (row 0: the half-step in front)
    int* d_perm_host = nullptr;                    // LCF_SPLIT_HOST: the caller's permutations of the whole run
    int64_t perm_host_rows = 0;
    int split_mode = LCF_SPLIT_IDENTITY;
    bool need_slots = true;                        // draw records carry the slots of the previous half-step
    int64_t blk_generated = -1;                    // last block whose generation is enqueued
    int64_t blk_current = -1;                      // block the half-steps are in
    int64_t run_first = 0, run_steps = 0;
    int64_t spec_first = -1;   // >= 0: buffer 0 holds the first block of a run starting at this step (speculated)
    int spec_mode = 0;
    bool spec_slots = false;
    int64_t chain_cap = 0;
    bool has_state = false;
    long long g_next = 2;     // global half-step counter (never reused: see lcf_sampler_begin)
    long long g_run0 = 2;     // first half-step of the current run
    bool pending = false;     // the last proposed half-step is not committed yet
    bool foreign_stream = false;  // half-steps of the current run were enqueued on a caller's stream
    int half_step_kernel = LCF_HALF_STEP_AUTO;
    int last_kernel = -1;     // what the last run's half-steps were (lcf_sampler_last_run_kernel)
    bool last_rows = false;   // ... and whether it was a row-board run (between ranks)
    long long last_launches = 0;   // launches of that kernel in the last run (lcf_sampler_last_run_launches)
    // <ND, NP, M, ranks> of the half-step kernel launched last (lcf_sampler_last_run_instance; -1: k_fused / phases)
    int last_instance[4] = {-1, -1, -1, -1};
    // ... all four written where a run is enqueued, from its plan
    void record_run(int kernel, bool rows, long long launches, const int instance[4]) {
        last_kernel = kernel;
        last_rows = rows;
        last_launches = launches;
        std::copy(instance, instance + 4, last_instance);
    }
    unsigned long long* mailbox = nullptr;   // this rank's peer mailbox (uncached device memory), see DevSampler
    size_t mailbox_cap = 0;
    void* board_mem = nullptr;               // this rank's row board (uncached device memory), see DevSampler
    std::vector<void*> board_opened;         // peers' boards mapped through IPC
    // One-launch runs write their final state into the other of two sets of state buffers (DevSampler::X_out ...):
    // ds.X / LP / nacc name the set that holds the state behind everything enqueued so far.
    double* alt_X = nullptr;
    double* alt_LP = nullptr;
    long long* alt_nacc = nullptr;
    bool run_off = false;                    // a one-launch run of this sampler gave up once: launches per half-step from then on
    int replay_split = 0, replay_store = 0;  // the last one-launch run, should it have to be repeated
    int64_t replay_first = 0, replay_steps = -1;
    void* run_board_mem = nullptr;           // the board of one-launch runs (k_solo_run): kRunRing versions, this GPU only
    // The sampler as a resident kernel reads it, in device memory, and the host's copy of what was written there last.
    struct Image {
        DevSampler* dev = nullptr;
        DevSampler host{};
        bool valid = false;
    };
    Image run_image;                         // as k_solo_run reads it (run_image)
    bool run_flip = false;                   // ds.X / LP / nacc name the SECOND set of state buffers
    unsigned int run_arrivals = 0;           // workgroups of resident launches enqueued so far (the board's arrivals word)
    Image rows_image;                        // as k_solo_run<..., RANKS> reads it (rows_image)
    unsigned int rows_arrivals = 0;          // the same count for the resident launches of row-board runs (cleared per run)
    size_t run_board_bytes() const {
        return board_rows_bytes(kRunRing, ds.n_walkers, ds.n_dim) + (size_t)kBoardTail * sizeof(unsigned int);
    }
    size_t board_bytes() const {
        return board_rows_bytes(kRing, ds.n_walkers, ds.n_dim) + (size_t)kBoardTail * sizeof(unsigned int);
    }
    // the last kBoardClear words of a board's tail (abort ... arrivals, and the diagnosis of a given-up wait)
    static unsigned char* tail_words(void* board, size_t bytes) {
        return static_cast<unsigned char*>(board) + bytes - kBoardClear * sizeof(unsigned int);
    }
    unsigned char* run_board_tail() const { return tail_words(run_board_mem, run_board_bytes()); }
    unsigned char* board_tail() const { return tail_words(board_mem, board_bytes()); }
    std::vector<void*> opened;               // peers' mailboxes mapped through IPC
    int peer_ranks = 0, peer_rank = 0;
    // Snapshot of (error flag, positions, log-posteriors, acceptance counts) in pinned host memory, copied behind the
    // last launch of a run: the calls that read them back after the run wait for nothing more.
    unsigned char* snap = nullptr;
    bool snap_enqueued = false, snap_valid = false;
    size_t snap_x() const { return 8; }
    size_t snap_lp() const { return snap_x() + (size_t)ds.n_walkers * ds.n_dim * sizeof(double); }
    size_t snap_acc() const { return snap_lp() + (size_t)ds.n_walkers * sizeof(double); }
    size_t snap_bytes() const { return snap_acc() + (size_t)ds.n_walkers * sizeof(long long); }
    size_t snap_alloc() const { return snap_bytes() + 2 * kSnapFlags * sizeof(unsigned int); }   // + the workgroups' error words
    unsigned int* snap_flags() const { return reinterpret_cast<unsigned int*>(snap + snap_bytes()); }
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_snap = nullptr;   // behind the snapshot kernel: what a caller of a finished run waits for
    double last_ms = 0.;

    ~lcf_sampler() {
        // (the device is remembered here: a garbage collector may destroy the engine first, and nothing below needs it)
        hipSetDevice(device);
        if (engine_samplers) --*engine_samplers;
        for (void* p : owned) hipFree(p);
        if (ds.chain) hipFree(ds.chain);
        if (ds.chain_lp) hipFree(ds.chain_lp);
        free_blocks();
        for (void* p : opened) hipIpcCloseMemHandle(p);
        if (mailbox) polled_give(device, true, mailbox_cap, mailbox);
        for (void* p : board_opened) hipIpcCloseMemHandle(p);
        if (board_mem) polled_give(device, true, board_bytes(), board_mem);
        if (run_board_mem) polled_give(device, false, run_board_bytes(), run_board_mem);
        if (snap) hipHostFree(snap);
        if (d_perm_host) hipFree(d_perm_host);
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
        if (ev_snap) hipEventDestroy(ev_snap);
    }
    void free_blocks() {
        for (int b = 0; b < 2; ++b) {
            if (d_perm[b]) hipFree(d_perm[b]);
            if (d_draws[b]) hipFree(d_draws[b]);
            if (d_slot[b]) hipFree(d_slot[b]);
            d_perm[b] = nullptr;
            d_draws[b] = nullptr;
            d_slot[b] = nullptr;
        }
        blk_cap = 0;
    }
    // block of the run's step k (relative), and the block's first step / length
    int64_t block_of_step(int64_t k) const { return k < blk_first ? 0 : 1 + (k - blk_first) / blk_steps; }
    int64_t block_start(int64_t b) const { return b == 0 ? 0 : blk_first + (b - 1) * blk_steps; }
    int64_t block_len(int64_t b) const {
        return std::min(run_steps, block_start(b) + (b == 0 ? blk_first : blk_steps)) - block_start(b);
    }
    // draw records of the run's half-step `rel` (its block must be resident)
    const DrawRec* rows(long long rel) const {
        const int64_t b = block_of_step(rel / 2);
        return d_draws[b & 1] + (size_t)(rel - 2 * block_start(b)) * ds.n_half;
    }
    // half-steps of a resident launch from the run's half-step `rel` on: up to `max_span`, never past the end of the
    // current block of draw records
    int block_span(long long rel, int max_span) const {
        return (int)std::min<long long>(max_span, 2 * (block_start(blk_current) + block_len(blk_current)) - rel);
    }
    // the other set of state buffers holds the state now (see alt_X)
    void flip_state_sets() {
        std::swap(ds.X, alt_X);
        std::swap(ds.LP, alt_LP);
        std::swap(ds.nacc, alt_nacc);
        run_flip = !run_flip;
    }
};

// ---- host functions that cross the two files ------------------------------------------------------------------------
// What the kernels take as arguments -- DevSampler, DrawRec, GenItem -- stays in the anonymous namespace, because the
// kernels' mangled names (which tools/isa_count.py, tools/isa_diff.py and tests/test_host.py match) contain it.  Two
// consequences, accepted knowingly: (1) each of the two files that include this header has types of its own of these
// names, and `struct lcf_sampler`, which holds a DevSampler, is formally a different type in each -- it works because
// both see this one text, and nothing but this header may define them; (2) a function whose signature names such a type
// has internal linkage and cannot cross files, so the functions below take `const void* gen` where they mean an array
// of GenItem in device memory (the callee casts it back; only lcf_population_run passes one).
namespace lcf {

template <class T>
lcf_status dalloc(T** p, size_t n, std::vector<void*>& owned) {
    LCF_HIP(hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T)));
    owned.push_back(*p);
    return LCF_OK;
}

// lcf_sampler.hip
lcf_status generate_multi(const void* gen, int n_items, int n_walkers, int n_half, long long first_step, long long n_steps,
                          int buf, long long front_row, hipStream_t st);
lcf_status generate_block(lcf_sampler* const* ss, int n, int64_t b, hipStream_t consumer, const void* gen = nullptr);
lcf_status enter_half_step(lcf_sampler* const* ss, int n, long long rel, hipStream_t st, const void* gen = nullptr);
lcf_status leave_half_step(lcf_sampler* const* ss, int n, hipStream_t st, const void* gen = nullptr);
lcf_status flush_pending(lcf_sampler* s, hipStream_t st);
lcf_status launch_snapshot(lcf_sampler* s, hipStream_t st);
lcf_status enqueue_snapshot(lcf_sampler* s);
lcf_status settle(lcf_sampler* s);
int reported_error(const lcf_sampler* s);
lcf_status rewind_resident_run(lcf_sampler* s);
lcf_status sampler_begin(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode, const int32_t* perm,
                         int32_t store_chain, bool need_slots, hipStream_t gen = nullptr, bool defer = false);

// lcf_hip.hip
lcf_status logprob_dev(lcf_engine* e, int64_t n, const double* dP, double* dout, hipStream_t st, int with_prior);
lcf_status launch_next(lcf_sampler* s, bool have_next, int lo, int hi, hipStream_t st);
lcf_status launch_eval(lcf_sampler* s, int lo, int hi, bool finalize, hipStream_t st);
lcf_status launch_fused(lcf_sampler* s, int lo, int hi, hipStream_t st);
RunPlan plan_run(const lcf_sampler* s, bool rows, int lo, int hi, bool resident);
lcf_status prepare_run(const lcf_engine* e, RunPlan& plan);
lcf_status launch_solo(lcf_sampler* s, const RunPlan& plan, long long rel, hipStream_t st);
lcf_status launch_run(lcf_sampler* s, const RunPlan& plan, long long rel, int n_hs, hipStream_t st, long long need_progress);
lcf_status launch_half_step_sharded(lcf_sampler* s, int lo, int hi, hipStream_t st);
lcf_status launch_half_step_rows(lcf_sampler* s, int lo, int hi, hipStream_t st);
bool fused_eligible(const lcf_sampler* s);
bool run_claim(int dev, hipStream_t st);
void run_release(int dev, hipStream_t st);
lcf_status run_buffers(lcf_sampler* s);
struct RunClaim {   // releases on every path out of the enqueue
    int dev;
    hipStream_t st;
    bool held;
    void release() { if (held) run_release(dev, st); held = false; }
    ~RunClaim() { release(); }
};

}  // namespace lcf
