// The bookkeeping of runs: the pool of polled memory, the generation of draw records (k_make_perm*, k_slots,
// k_draws*), sampler_begin and the speculated continuation, snapshot / settle / check, lcf_sampler_run[_async], the
// phase API and the state / chain getters.  Instantiates no kernel template: what a half-step launches is in lcf_hip.hip.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "lcf_internal.h"

#ifndef LCF_FIRST_BLOCK
#define LCF_FIRST_BLOCK 32  // steps in the first block of draw records of a run (the later ones: up to 256)
#endif

namespace {

// LCF_RESIDENT_WAIT_S (seconds, default 0.05): how long a workgroup of a resident launch waits for a row before it asks
// whether the launch's other workgroups have started at all (board_take)
unsigned long long resident_wait_ticks() {
    double sec = 0.05;
    if (const char* env = std::getenv("LCF_RESIDENT_WAIT_S")) sec = std::atof(env);
    if (!(sec > 0.)) sec = 0.05;
    return (unsigned long long)(std::min(sec, 600.) * 1e8);
}

// LCF_PEER_WAIT_S (seconds, default 5; the tests of the bounded waits set 0.5)
unsigned long long peer_wait_ticks() {
    double sec = 5.;
    if (const char* env = std::getenv("LCF_PEER_WAIT_S")) sec = std::atof(env);
    if (!(sec > 0.)) sec = 5.;
    return (unsigned long long)(std::min(sec, 600.) * 1e8);
}

// Random red/blue colouring of each step (emcee's randomize_split): one workgroup per step ranks the walkers by a
// 50-bit Philox key (ties impossible: the walker id fills the low 14 bits) with a bitonic sort in LDS.
// perm[step][0 .. n/2) is colour 0.  Deterministic in (seed, step): every rank of a multi-GPU run derives the same
// split without communicating.
// `slot_of` (or null): the slot table of k_slots, written here as well -- the step's two rows, and by the block's first
// workgroup the row in front of the block (`front`, or all -1) -- so that the records need no launch in between.
__device__ __forceinline__ void make_perm_body(int n_walkers, int n_pad, uint32_t key0, uint32_t key1,
                                               long long first_step, int* __restrict__ perm, int n_half,
                                               int* __restrict__ slot_of, const int* __restrict__ front) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
    const long long step = first_step + blockIdx.x;
    for (int w = threadIdx.x; w < n_pad; w += blockDim.x) {
        unsigned long long k = ~0ull;
        if (w < n_walkers) {
            uint32_t r[4];
            philox4x32((uint32_t)w, (uint32_t)step, 2u, 7u, key0, key1, r);
            const unsigned long long h = ((unsigned long long)r[0] << 32) | r[1];
            k = (h & ~0x3fffull) | (unsigned long long)w;
        }
        keys[w] = k;
    }
    __syncthreads();
    // Pairs [64 m, 64 m + 64) -- one wave's share of a stage (blockDim.x is a multiple of 64) -- touch keys
    // [128 m, 128 m + 128) only while the stride is at most 64: such stages follow each other without a workgroup
    // barrier (a wave's LDS operations execute in order); 6 of the 55 stages of 1024 keys need one on either side.
    for (int size = 2; size <= n_pad; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (n_pad >> 1); i += blockDim.x) {
                const int lo = 2 * i - (i & (stride - 1));  // index with bit `stride` clear
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == up) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            const int next = stride > 1 ? stride >> 1 : size;   // the stride of the stage that follows
            if (stride > 64 || next > 64)
                __syncthreads();
            else
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < n_walkers; w += blockDim.x) {
        const int wid = (int)(keys[w] & 0x3fffull);
        perm[(size_t)blockIdx.x * n_walkers + w] = wid;
        if (slot_of) {   // (position w of the permutation: colour 0 = the first n_half entries -- as k_slots)
            const int half = w < n_half ? 0 : 1, slot = w < n_half ? w : w - n_half;
            slot_of[((size_t)blockIdx.x * 2 + 1 + half) * n_walkers + wid] = slot;
            slot_of[((size_t)blockIdx.x * 2 + 1 + (1 - half)) * n_walkers + wid] = -1;
            if (blockIdx.x == 0) slot_of[w] = front ? front[w] : -1;
        }
    }
}

__global__ __launch_bounds__(1024) void k_make_perm(int n_walkers, int n_pad, uint32_t key0, uint32_t key1,
                                                    long long first_step, int* __restrict__ perm, int n_half,
                                                    int* __restrict__ slot_of, const int* __restrict__ front) {
    make_perm_body(n_walkers, n_pad, key0, key1, first_step, perm, n_half, slot_of, front);
}

// Population mode: the same for MANY samplers in one launch (blockIdx.y = sampler; equal walker counts and blocks); what
// differs from sampler to sampler comes from their GenItems.
// `front_row` >= 0: the half-step in front of the block is row `front_row` of the OTHER buffer's slot table (-1: none)
__global__ __launch_bounds__(1024) void k_make_perm_multi(const GenItem* __restrict__ items, int n_walkers, int n_pad,
                                                          long long first_step, int buf, int n_half, long long front_row) {
    const GenItem it = items[blockIdx.y];
    make_perm_body(n_walkers, n_pad, it.key0, it.key1, first_step, it.perm[buf], n_half, it.slot[buf],
                   front_row >= 0 ? it.slot[buf ^ 1] + (size_t)front_row * n_walkers : nullptr);
}

// Slot of every walker in each half-step of a block of steps (-1 where it is not active).  Rows of `slot_of`
// ([1 + 2 n_steps][n_walkers]): row 0 = the half-step in front of the block (copied from the previous block, or all
// -1 at the start of a run), row 1 + 2 k + half = half-step (k, half) of the block.
__global__ void k_slots(int n_walkers, int n_half, const int* __restrict__ perm, long long n_steps,
                        int* __restrict__ slot_of, const int* __restrict__ front) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n_walkers) slot_of[idx] = front ? front[idx] : -1;   // row 0 (nobody in this launch reads it)
    if (idx >= n_steps * n_walkers) return;
    const long long row = idx / n_walkers;
    const int pos = (int)(idx % n_walkers);  // position in the permutation: colour 0 = first n_half entries
    const int wid = perm ? perm[idx] : pos;
    const int half = pos < n_half ? 0 : 1, slot = pos < n_half ? pos : pos - n_half;
    slot_of[((size_t)row * 2 + 1 + half) * n_walkers + wid] = slot;
    slot_of[((size_t)row * 2 + 1 + (1 - half)) * n_walkers + wid] = -1;
}

// The state-independent half of every stretch move of a block of steps, one thread per (step, half, slot).
// n_half = ceil(n_walkers / 2) slots per half-step: colour 0 (the first n_half entries of the step's permutation)
// moves in half 0 against the n_walkers - n_half walkers of colour 1, then colour 1 against colour 0 -- the larger
// colour first, as emcee's red-blue split does for an odd ensemble; the slot an odd ensemble leaves empty in half 1
// gets wid = -1.  `slot_of` null: no slot bookkeeping (the one-workgroup-per-proposal half-step does not need it).
__device__ __forceinline__ void draws_body(const DevSampler& sm, const int* __restrict__ perm, const int* __restrict__ slot_of,
                                           long long first_step, long long n_steps, DrawRec* __restrict__ draws) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_steps * 2 * sm.n_half) return;
    const int i = (int)(idx % sm.n_half), half = (int)((idx / sm.n_half) & 1);
    const long long row = idx / (2 * sm.n_half);
    const int* pr = perm ? perm + (size_t)row * sm.n_walkers : nullptr;
    const int n_act = half == 0 ? sm.n_half : sm.n_walkers - sm.n_half, n_other = sm.n_walkers - n_act;
    DrawRec d;
    if (i >= n_act) {
        d.wid = d.pid = d.wprev = d.pprev = -1;
        d.z = 1.;
        d.zl = d.lnu = 0.;
        d.wage = d.page = 0;
        draws[idx] = d;
        return;
    }
    const int my_slot = half == 0 ? i : sm.n_half + i;  // colour 0 = first n_half entries of the permutation
    const int wid = pr ? pr[my_slot] : my_slot;
    uint32_t r[4], s2[4];
    philox4x32((uint32_t)wid, (uint32_t)(first_step + row), (uint32_t)half, 0u, sm.key0, sm.key1, r);
    philox4x32((uint32_t)wid, (uint32_t)(first_step + row), (uint32_t)half, 1u, sm.key0, sm.key1, s2);
    const double zr = (sm.a - 1.) * u01(r[0], r[1]) + 1.;
    const double z = zr * zr / sm.a;
    int j = (int)(u01(r[2], r[3]) * (double)n_other);
    j = min(j, n_other - 1);
    const int other_slot = half == 0 ? sm.n_half + j : j;
    d.wid = wid;
    d.pid = pr ? pr[other_slot] : other_slot;
    const int* before = slot_of ? slot_of + (size_t)(row * 2 + half) * sm.n_walkers : nullptr;  // the half-step in front
    d.wprev = before ? before[d.wid] : -1;
    d.pprev = before ? before[d.pid] : -1;
    d.z = z;
    d.zl = (double)(sm.n_dim - 1) * log(z);
    d.lnu = log(u01(s2[0], s2[1]));
    // Every walker moves once per step, in one of its two half-steps: a walker that was not active in the half-step in
    // front (half-step G - 1) moved in the one before it, or -- the walker of a step's SECOND half-step only -- three
    // half-steps ago (first half of the previous step).  The sharded one-workgroup-per-proposal run waits for exactly
    // that version of each row.  (Before the first step of a run every age points in front of the run: its start state.)
    d.wage = d.page = 0;
    if (slot_of) {
        if (half == 0) {
            d.wage = before[d.wid] >= 0 ? 1 : 2;
            d.page = before[d.pid] >= 0 ? 1 : 2;
        } else {
            const int* two_back = slot_of + (size_t)(row * 2) * sm.n_walkers;  // second half of the previous step
            d.wage = two_back[d.wid] >= 0 ? 2 : 3;
            d.page = 1;
        }
    }
    draws[idx] = d;
}

__global__ void k_draws(DevSampler sm, const int* __restrict__ perm, const int* __restrict__ slot_of,
                        long long first_step, long long n_steps, DrawRec* __restrict__ draws) {
    draws_body(sm, perm, slot_of, first_step, n_steps, draws);
}
// (population mode, blockIdx.y = sampler: `sm` = the samplers' common walker count; key, dimension and stretch scale
// from the item)
__global__ void k_draws_multi(const GenItem* __restrict__ items, DevSampler sm, int buf, long long first_step,
                              long long n_steps) {
    const GenItem it = items[blockIdx.y];
    sm.key0 = it.key0;
    sm.key1 = it.key1;
    sm.n_dim = it.n_dim;
    sm.a = it.a;
    draws_body(sm, it.perm[buf], it.slot[buf], first_step, n_steps, it.draws[buf]);
}

// State of the sampler as 8-byte words into (mapped, pinned) host memory: [error flag | X | LP | n_accepted].
__global__ void k_snapshot(const DevSampler sm, unsigned long long* __restrict__ out) {
    const long long nx = (long long)sm.n_walkers * sm.n_dim, nw = sm.n_walkers;
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w == 0) out[0] = (unsigned long long)(unsigned int)*sm.err;
    else if (w <= nx) out[w] = reinterpret_cast<const unsigned long long*>(sm.X)[w - 1];
    else if (w <= nx + nw) out[w] = reinterpret_cast<const unsigned long long*>(sm.LP)[w - 1 - nx];
    else if (w <= nx + 2 * nw) out[w] = (unsigned long long)sm.nacc[w - 1 - nx - nw];
}

// ---- memory that kernels POLL (row boards, mailboxes) is never handed back to the driver ---------------------------------
// A board that was freed (hipFree) and whose address range the driver then gave to the next sampler's board left single
// workgroups of the next launches reading the OLD contents of those addresses for as long as they polled -- rows that
// every other workgroup (and the host) could see never arrived for them, 5 s waits, once also a stale row with a valid
// tag (a wrong chain).  Reproduced deterministically by tools/debug/rows_mismatch.py once the inter-rank boards were
// megabytes (freed uncached memory recycled into the next board); gone when such memory is not freed.  So: polled
// memory goes back to a list of this process and is taken from there by the next sampler that needs the same size;
// whoever takes it clears it (stale tags of an earlier life would be valid tags of the next) before anything reads it.
struct PolledBlock { int dev; bool uncached; size_t bytes; void* p; };
std::mutex g_polled_mutex;
std::vector<PolledBlock> g_polled;

void* polled_take(int dev, bool uncached, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_polled_mutex);
    for (size_t k = 0; k < g_polled.size(); ++k)
        if (g_polled[k].dev == dev && g_polled[k].uncached == uncached && g_polled[k].bytes == bytes) {
            void* p = g_polled[k].p;
            g_polled.erase(g_polled.begin() + (long)k);
            return p;
        }
    return nullptr;
}

}  // namespace

namespace lcf {

void polled_give(int dev, bool uncached, size_t bytes, void* p) {
    std::lock_guard<std::mutex> lock(g_polled_mutex);
    g_polled.push_back(PolledBlock{dev, uncached, bytes, p});
}
// `bytes` of polled memory on the current device, cleared (complete on return).
lcf_status polled_alloc(int dev, bool uncached, size_t bytes, void** out) {
    void* p = polled_take(dev, uncached, bytes);
    if (!p) {
        if (uncached)   // fine-grained device memory: peers' stores over the fabric and this rank's polls meet in memory
            LCF_HIP(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached));
        else
            LCF_HIP(hipMalloc(&p, bytes));
    }
    *out = p;
    LCF_HIP(hipMemset(p, 0, bytes));        // tag 0: no version / generation (half-steps are numbered from 2)
    LCF_HIP(hipDeviceSynchronize());
    return LCF_OK;
}

// The launch of the permutation kernels: the walkers padded to a power of two of keys (8 bytes of LDS each), a thread
// per pair of keys.
struct PermShape { int n_pad, threads; };
static PermShape perm_shape(int n_walkers) {
    int n_pad = 2;
    while (n_pad < n_walkers) n_pad <<= 1;
    return {n_pad, std::min(1024, std::max(64, n_pad / 2))};
}

// Enqueue, on stream `gs` (the one the half-steps run on: behind the last reader of the buffer), the generation of
// `len` steps of draw records starting at absolute step `step0` into buffer `buf`.  `front`: where the slots of the
// half-step in front of the block come from (null: nothing in front, the start of a run).
static lcf_status generate_steps(lcf_sampler* s, int buf, int64_t step0, int64_t len, int split_mode, const int* host_perm,
                                 bool need_slots, const int* front, hipStream_t gs) {
    const DevSampler& ds = s->ds;
    const int* perm = nullptr;
    if (split_mode == LCF_SPLIT_RANDOM) {
        const auto [n_pad, threads] = perm_shape(ds.n_walkers);
        LCF_HIP(prepare_kernel(k_make_perm, (size_t)n_pad * 8));
        hipLaunchKernelGGL(k_make_perm, dim3((unsigned)len), dim3(threads), (size_t)n_pad * 8, gs, ds.n_walkers, n_pad,
                           ds.key0, ds.key1, (long long)step0, s->d_perm[buf], ds.n_half,
                           need_slots ? s->d_slot[buf] : nullptr, front);
        perm = s->d_perm[buf];
    } else if (split_mode == LCF_SPLIT_HOST) {
        perm = host_perm;
    }
    const long long total = (long long)len * ds.n_walkers;
    int* slots = nullptr;
    if (need_slots) {
        slots = s->d_slot[buf];
        if (split_mode != LCF_SPLIT_RANDOM)   // (a random split's table comes with its permutations, from k_make_perm)
            hipLaunchKernelGGL(k_slots, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, gs, ds.n_walkers, ds.n_half, perm,
                               (long long)len, slots, front);
    }
    const long long recs = (long long)len * 2 * ds.n_half;
    hipLaunchKernelGGL(k_draws, dim3((unsigned)((recs + 255) / 256)), dim3(256), 0, gs, ds, perm, slots,
                       (long long)step0, (long long)len, s->d_draws[buf]);
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

// The launcher of the batched generation kernels: `n_steps` steps from absolute step `first_step` for the `n_items`
// GenItems at `gen_items` (device memory; equal walker counts), permutations and draw records into their buffers `buf`,
// one launch of each kernel.  An item without a slot table gets records without slot bookkeeping.  `front_row`: as
// k_make_perm_multi takes it.  (A population's samplers, and the rungs of a tempered ensemble: lcf_tempered.hip.)
lcf_status generate_multi(const void* gen_items, int n_items, int n_walkers, int n_half, long long first_step,
                          long long n_steps, int buf, long long front_row, hipStream_t st) {
    const GenItem* gen = static_cast<const GenItem*>(gen_items);
    const auto [n_pad, threads] = perm_shape(n_walkers);
    LCF_HIP(prepare_kernel(k_make_perm_multi, (size_t)n_pad * 8));
    hipLaunchKernelGGL(k_make_perm_multi, dim3((unsigned)n_steps, (unsigned)n_items), dim3(threads), (size_t)n_pad * 8, st, gen,
                       n_walkers, n_pad, first_step, buf, n_half, front_row);
    DevSampler sm{};   // (the kernel reads the common shape from it; key, dimension and stretch scale come from the item)
    sm.n_walkers = n_walkers;
    sm.n_half = n_half;
    const long long recs = n_steps * 2 * n_half;
    hipLaunchKernelGGL(k_draws_multi, dim3((unsigned)((recs + 255) / 256), (unsigned)n_items), dim3(256), 0, st, gen, sm, buf,
                       first_step, n_steps);
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

// Block b of the current run (block b lives in buffer b & 1) for a GROUP of samplers ss[0, n) that share their block
// geometry -- a population's transients, or one sampler on its own; so do enter_half_step and leave_half_step.  `gen`:
// the group's GenItems in device memory, the block of all of them from one launch of each batched generation kernel;
// null: sampler by sampler.
lcf_status generate_block(lcf_sampler* const* ss, int n, int64_t b, hipStream_t consumer, const void* gen_items) {
    const GenItem* gen = static_cast<const GenItem*>(gen_items);
    const int buf = (int)(b & 1);
    if (gen) {
        const lcf_sampler* s0 = ss[0];
        const DevSampler& d0 = s0->ds;
        const int64_t k0 = s0->block_start(b), len = s0->block_len(b);
        const long long front_row = b > 0 ? 2 * (long long)s0->block_len(b - 1) : -1;
        if (lcf_status r = generate_multi(gen, n, d0.n_walkers, d0.n_half, s0->run_first + k0, len, buf, front_row, consumer))
            return r;
    }
    for (int t = 0; t < n; ++t) {
        lcf_sampler* s = ss[t];
        if (!gen) {
            const int64_t k0 = s->block_start(b);
            const int* host_perm = s->split_mode == LCF_SPLIT_HOST ? s->d_perm_host + (size_t)k0 * s->ds.n_walkers : nullptr;
            // the half-step in front of a later block: the last row of the previous block (the other buffer)
            const int* front = (b > 0 && s->need_slots)
                                   ? s->d_slot[buf ^ 1] + (size_t)2 * s->block_len(b - 1) * s->ds.n_walkers : nullptr;
            if (lcf_status r = generate_steps(s, buf, s->run_first + k0, s->block_len(b), s->split_mode, host_perm,
                                              s->need_slots, front, consumer))
                return r;
        }
        s->blk_generated = b;
    }
    return LCF_OK;
}

// A run usually continues where the last one stopped (burn-in -> sampling; run_mcmc(None, ...) in a loop).  Behind the
// last launch of a run, generate the first block of such a continuation, so that its first half-step finds its draw
// records ready: sampler_begin adopts them when the new run matches (first step, split mode, slot bookkeeping).
// (Measured and dropped: the same BESIDE a one-block run instead of behind it -- into the other buffer, on a stream of the
// sampler's own, of the lowest priority, enqueued before or after the run's launch -- so that the caller's
// synchronisation does not wait for it.  The 20 us it takes behind the run disappear, but the resident launch beside it
// takes 16-36 us longer -- its workgroups arrive later: 14.4-15.0 against 14.2 us per step of a 20-step run.)
static lcf_status speculate_continuation(lcf_sampler* s, hipStream_t st) {
    s->spec_first = -1;
    if (s->pending || s->split_mode == LCF_SPLIT_HOST || s->run_steps == 0) return LCF_OK;
    const int64_t first = s->run_first + s->run_steps;
    if (lcf_status r = generate_steps(s, 0, first, s->blk_first, s->split_mode, nullptr, s->need_slots, nullptr, st))
        return r;
    s->spec_first = first;
    s->spec_mode = s->split_mode;
    s->spec_slots = s->need_slots;
    return LCF_OK;
}

// Before launching the run's half-step `rel` on stream `st`: its block of draw records must be generated (it is,
// unless the caller jumped ahead).
lcf_status enter_half_step(lcf_sampler* const* ss, int n, long long rel, hipStream_t st, const void* gen) {
    const lcf_sampler* s0 = ss[0];
    const int64_t b = s0->block_of_step(rel / 2);
    if (b == s0->blk_current) return LCF_OK;
    while (s0->blk_generated < b)
        if (lcf_status r = generate_block(ss, n, s0->blk_generated + 1, st, gen)) return r;
    for (int t = 0; t < n; ++t) ss[t]->blk_current = b;
    return LCF_OK;
}

// After that launch (the last reader of the block left behind, through the previous half-step's records): generate
// the next block into the buffer that is now free.
lcf_status leave_half_step(lcf_sampler* const* ss, int n, hipStream_t st, const void* gen) {
    const lcf_sampler* s0 = ss[0];
    const int64_t last = s0->block_of_step(s0->run_steps - 1);
    if (s0->blk_generated == s0->blk_current && s0->blk_current < last)
        return generate_block(ss, n, s0->blk_current + 1, st, gen);
    return LCF_OK;
}

lcf_status flush_pending(lcf_sampler* s, hipStream_t st) {
    if (!s->pending) return LCF_OK;
    return launch_next(s, false, 0, 0, st);
}

// The snapshot of the sampler's state as it is on stream `st`: one small kernel writes it straight into the pinned host
// buffer (four separate copies cost 4x the fixed price of a device-to-host transfer).
lcf_status launch_snapshot(lcf_sampler* s, hipStream_t st) {
    const long long words = (long long)(s->snap_bytes() / 8);
    hipLaunchKernelGGL(k_snapshot, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, s->ds,
                       reinterpret_cast<unsigned long long*>(s->snap));
    LCF_HIP(hipGetLastError());
    return LCF_OK;
}

// Commit what is pending and copy the snapshot behind it, all on the engine's stream; enqueue only.
lcf_status enqueue_snapshot(lcf_sampler* s) {
    lcf_engine* e = s->e;
    hipStream_t st = e->stream;
    if (s->foreign_stream) {  // half-steps were driven on a caller's stream: order this stream behind them
        LCF_HIP(hipDeviceSynchronize());
        s->foreign_stream = false;
    }
    if (lcf_status r = flush_pending(s, st)) return r;
    if (lcf_status r = launch_snapshot(s, st)) return r;
    LCF_HIP(hipEventRecord(s->ev_snap, st));
    s->snap_enqueued = true;
    s->snap_valid = false;
    return LCF_OK;
}

// The snapshot of the sampler's present state, complete in host memory on return.
lcf_status settle(lcf_sampler* s) {
    LCF_HIP(hipSetDevice(s->e->device));
    if (s->snap_valid && !s->pending && !s->foreign_stream) return LCF_OK;
    if (!s->snap_enqueued || s->pending || s->foreign_stream)
        if (lcf_status r = enqueue_snapshot(s)) return r;
    // Wait for the snapshot, not for the stream: what a run enqueues behind it (the draw records of a possible
    // continuation, 30-40 us of kernels) is nobody's business here -- everything later on the stream is ordered behind
    // it anyway.  A short run ends within a millisecond of this call: poll for that long before handing the wait to
    // the driver.
    {
        const auto t0 = std::chrono::steady_clock::now();
        while (hipEventQuery(s->ev_snap) == hipErrorNotReady &&
               std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(2)) {
        }
    }
    LCF_HIP(hipEventSynchronize(s->ev_snap));
    s->snap_enqueued = false;
    s->snap_valid = true;
    return LCF_OK;
}

// The last stored run of every sampler where it lies, for the chain analyses (lcf_host.h).
lcf_status stored_chains(lcf_sampler* const* s, int32_t n, int64_t discard, int64_t thin, std::vector<ChainView>* out,
                         int32_t* device) {
    if (!s || n < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (discard < 0 || thin < 1) return fail(LCF_ERR_INVALID_ARGUMENT, "need discard >= 0 and thin >= 1");
    for (int32_t i = 0; i < n; ++i) {
        if (!s[i]) return fail(LCF_ERR_INVALID_ARGUMENT, "null sampler");
        if (!s[i]->ds.store_chain || s[i]->run_steps == 0) return fail(LCF_ERR_STATE, "no stored chain");
        if (discard >= s[i]->run_steps) return fail(LCF_ERR_INVALID_ARGUMENT, "discard leaves no chain");
        if (s[i]->e->device != s[0]->e->device) return fail(LCF_ERR_UNSUPPORTED, "the samplers are on different devices");
    }
    out->resize(n);
    for (int32_t i = 0; i < n; ++i) {
        if (lcf_status st = settle(s[i])) return st;  // (the trailing commit writes the last chain row)
        const DevSampler& ds = s[i]->ds;
        (*out)[i] = ChainView{ds.chain, ds.chain_lp, s[i]->run_steps, ds.n_walkers, ds.n_dim, ds.n_dim};
    }
    *device = s[0]->e->device;
    return LCF_OK;
}

// Whatever changes the state on the device makes the host's copy stale.
static void invalidate_snapshot(lcf_sampler* s) { s->snap_enqueued = s->snap_valid = false; }

// What the settled snapshot of a run reports: its error word and the words of the workgroups of one-launch runs.
int reported_error(const lcf_sampler* s) {
    int err = 0;
    std::memcpy(&err, s->snap, sizeof(int));
    const unsigned int* flags = s->snap_flags();
    for (int k = 0; k < 2 * kSnapFlags; ++k) err |= (int)flags[k];
    return err;
}

// A resident launch whose workgroups were not all on the device (somebody else's resident kernel holds CUs) has given
// up within the bound of its waits and written no state -- that goes into the other set of buffers, in the run's last
// step.  Put the sampler back on the state its resident run started from and drop what the run reported; the board's
// tail words and count of started workgroups start again from zero.  (The run's stream must have been waited for.)
lcf_status rewind_resident_run(lcf_sampler* s) {
    s->flip_state_sets();
    int sticky = 0;
    std::memcpy(&sticky, s->snap, sizeof(int));
    sticky &= 1;                                   // (a NaN of an earlier run stays reported)
    LCF_HIP(hipMemcpy(s->ds.err, &sticky, sizeof(int), hipMemcpyHostToDevice));
    std::memcpy(s->snap, &sticky, sizeof(int));
    std::memset(s->snap_flags(), 0, 2 * kSnapFlags * sizeof(unsigned int));
    LCF_HIP(hipMemset(s->run_board_tail(), 0, kBoardClear * sizeof(unsigned int)));
    s->run_arrivals = 0;
    invalidate_snapshot(s);
    return LCF_OK;
}

// Device memory for the chain of a run of n_steps steps (kept until a longer run needs more).
static lcf_status reserve_chain(lcf_sampler* s, int64_t n_steps) {
    DevSampler& ds = s->ds;
    if (n_steps <= s->chain_cap) return LCF_OK;
    LCF_HIP(hipStreamSynchronize(s->e->stream));
    if (ds.chain) hipFree(ds.chain);
    if (ds.chain_lp) hipFree(ds.chain_lp);
    ds.chain = nullptr;
    ds.chain_lp = nullptr;
    s->chain_cap = 0;
    LCF_HIP(hipMalloc((void**)&ds.chain, (size_t)n_steps * ds.n_walkers * ds.n_dim * sizeof(double)));
    LCF_HIP(hipMalloc((void**)&ds.chain_lp, (size_t)n_steps * ds.n_walkers * sizeof(double)));
    s->chain_cap = n_steps;
    return LCF_OK;
}

// Start a run of n_steps steps: settle what the previous run left pending, size the chain and the draw blocks, and
// enqueue the generation of the first block.  Nothing here waits for the device unless a buffer has to grow.
// `need_slots`: the draw records carry each walker's slot in the previous half-step (every path except k_solo).
// `gen`: the stream the first block of draw records is generated on (default: the engine's own -- where a single
// sampler's half-steps follow; a population's half-steps all run on ONE stream, and so do its samplers' records).
// `defer`: the first block is NOT generated here (a population generates the blocks of all its samplers in one launch).
lcf_status sampler_begin(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode, const int32_t* perm,
                         int32_t store_chain, bool need_slots, hipStream_t gen, bool defer) {
    if (!s || n_steps < 0 || first_step < 0) return fail(LCF_ERR_INVALID_ARGUMENT, "bad argument");
    if (split_mode < LCF_SPLIT_IDENTITY || split_mode > LCF_SPLIT_HOST)
        return fail(LCF_ERR_INVALID_ARGUMENT, "bad split_mode");
    if (split_mode == LCF_SPLIT_HOST && !perm && n_steps > 0)
        return fail(LCF_ERR_INVALID_ARGUMENT, "LCF_SPLIT_HOST needs perm");
    if (split_mode == LCF_SPLIT_RANDOM && s->ds.n_walkers > 16384)
        return fail(LCF_ERR_UNSUPPORTED, "device-generated splits support at most 16384 walkers; pass perm");
    if (split_mode != LCF_SPLIT_HOST) perm = nullptr;
    if (!s->has_state) return fail(LCF_ERR_STATE, "lcf_sampler_set_state must be called first");
    lcf_engine* e = s->e;
    LCF_HIP(hipSetDevice(e->device));
    if (s->foreign_stream) {  // the previous run was driven on a caller's stream: order everything behind it
        LCF_HIP(hipDeviceSynchronize());
        s->foreign_stream = false;
    }
    if (lcf_status st = flush_pending(s, e->stream)) return st;  // with the previous run's chain and draw records
    DevSampler& ds = s->ds;
    // leave a gap in the half-step numbering: no stale (last_g == g - 1) match across runs or set_state calls
    s->g_next += 2;
    s->g_run0 = s->g_next;
    ds.store_chain = store_chain ? 1 : 0;
    if (store_chain)
        if (lcf_status st = reserve_chain(s, n_steps)) return st;
    if (perm && n_steps > 0) {
        // validate: every row must be a permutation of 0..n_walkers-1 (out-of-range ids would fault the GPU)
        std::vector<char> seen(ds.n_walkers);
        for (int64_t r = 0; r < n_steps; ++r) {
            std::fill(seen.begin(), seen.end(), 0);
            const int32_t* row = perm + (size_t)r * ds.n_walkers;
            for (int i = 0; i < ds.n_walkers; ++i) {
                if (row[i] < 0 || row[i] >= ds.n_walkers || seen[row[i]])
                    return fail(LCF_ERR_INVALID_ARGUMENT, "perm rows must be permutations of the walker ids");
                seen[row[i]] = 1;
            }
        }
        LCF_HIP(hipStreamSynchronize(e->stream));
        if (n_steps > s->perm_host_rows) {
            if (s->d_perm_host) hipFree(s->d_perm_host);
            s->d_perm_host = nullptr;
            s->perm_host_rows = 0;
            LCF_HIP(hipMalloc((void**)&s->d_perm_host, (size_t)n_steps * ds.n_walkers * sizeof(int)));
            s->perm_host_rows = n_steps;
        }
        LCF_HIP(hipMemcpy(s->d_perm_host, perm, (size_t)n_steps * ds.n_walkers * sizeof(int), hipMemcpyHostToDevice));
    }
    invalidate_snapshot(s);
    s->run_first = first_step;
    s->run_steps = n_steps;
    s->split_mode = split_mode;
    s->need_slots = need_slots;
    s->blk_generated = s->blk_current = -1;
    if (n_steps == 0) return LCF_OK;
    // Block geometry: about 2^18 draw records (12 MiB) per buffer however long the run; a short first block, so that
    // the first half-step waits for a few steps' worth of records only.
    int64_t cap = std::max<int64_t>(4, std::min<int64_t>(256, (int64_t)(1 << 18) / ds.n_walkers));
    if (const char* env = std::getenv("LCF_DRAW_BLOCK")) cap = std::max<int64_t>(1, std::atoll(env));  // (tests: tiny blocks)
    bool grown = false;
    if (cap > s->blk_cap) {
        grown = true;
        LCF_HIP(hipStreamSynchronize(e->stream));
        s->free_blocks();
        for (int b = 0; b < 2; ++b) {
            LCF_HIP(hipMalloc((void**)&s->d_perm[b], (size_t)cap * ds.n_walkers * sizeof(int)));
            LCF_HIP(hipMalloc((void**)&s->d_draws[b], (size_t)cap * 2 * ds.n_half * sizeof(DrawRec)));
            LCF_HIP(hipMalloc((void**)&s->d_slot[b], (size_t)(1 + 2 * cap) * ds.n_walkers * sizeof(int)));
        }
        s->blk_cap = cap;
    }
    s->blk_steps = s->blk_cap;
    s->blk_first = std::min<int64_t>(s->blk_cap, LCF_FIRST_BLOCK);
    if (s->spec_first == first_step && s->spec_mode == split_mode && s->spec_slots == need_slots && !grown && !defer &&
        (gen == nullptr || gen == e->stream)) {   // (a block speculated on the engine's stream is not ordered with another)
        s->spec_first = -1;  // the previous run left this run's first block behind (speculate_continuation)
        s->blk_generated = 0;
        return LCF_OK;
    }
    s->spec_first = -1;
    if (defer) return LCF_OK;
    return generate_block(&s, 1, 0, gen ? gen : e->stream);
}

// What every call of the phase API checks of its half-step (step, half) and shard [lo, hi) of the slots; `in_order`: the
// half-step must be the next one to propose.
static lcf_status check_half_step(const lcf_sampler* s, int64_t step, int32_t half, int32_t lo, int32_t hi, bool in_order) {
    if (!s || half < 0 || half > 1 || step < s->run_first || step >= s->run_first + s->run_steps)
        return fail(LCF_ERR_INVALID_ARGUMENT, "bad step/half");
    if (lo < 0 || hi < lo || hi > s->ds.n_half) return fail(LCF_ERR_INVALID_ARGUMENT, "bad shard range");
    const long long g = s->g_run0 + 2 * (step - s->run_first) + half;
    if (in_order && g != s->g_next) return fail(LCF_ERR_STATE, "half-steps must be proposed in order, each exactly once");
    return LCF_OK;
}

}  // namespace lcf

extern "C" {

lcf_status lcf_sampler_create(lcf_engine* e, int32_t n_walkers, uint64_t seed, double a, lcf_sampler** out) {
    if (!e || !out) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (lcf_status st = custom_refuse(e, "the resident ensemble sampler (lcf_sampler_*, population runs)")) return st;
    if (lcf_status st = central_refuse(e, "the resident ensemble sampler (lcf_sampler_*, population runs)")) return st;
    if (lcf_status st = limits_refuse(e, "the resident ensemble sampler (lcf_sampler_*, population runs)")) return st;
    if (lcf_status st = template_refuse(e, "the resident ensemble sampler (lcf_sampler_*, population runs)")) return st;
    if (n_walkers < 2) return fail(LCF_ERR_INVALID_ARGUMENT, "n_walkers must be >= 2");
    if (!(a > 1.)) return fail(LCF_ERR_INVALID_ARGUMENT, "stretch scale a must be > 1");
    LCF_HIP(hipSetDevice(e->device));
    auto* s = new lcf_sampler();
    s->e = e;
    s->device = e->device;
    s->engine_samplers = e->samplers;
    ++*e->samplers;
    DevSampler& ds = s->ds;
    ds.n_walkers = n_walkers;
    ds.n_half = (n_walkers + 1) / 2;  // slots per half-step: the larger colour of an odd ensemble
    ds.n_dim = e->dp.n_dim;
    ds.key0 = (uint32_t)(seed & 0xffffffffu);
    ds.key1 = (uint32_t)(seed >> 32);
    ds.a = a;
    ds.wait_ticks = peer_wait_ticks();
    ds.resident_ticks = resident_wait_ticks();
    ds.ring = kRing;
    const size_t nw = n_walkers, nh = ds.n_half, nd = ds.n_dim;
    lcf_status st;
#define AL(p, n) if ((st = dalloc(&p, n, s->owned)) != LCF_OK) { delete s; return st; }
    AL(ds.X, nw * nd); AL(ds.LP, nw); AL(ds.nacc, nw); AL(ds.err, 1);
    for (int b = 0; b < 2; ++b) {
        AL(ds.Q[b], nh * nd); AL(ds.rec[b], nh); AL(ds.newlp[b], nh);
    }
    AL(s->coef, nh * kNCoef); AL(s->lprior, nh);
    for (int b = 0; b < 2; ++b) AL(ds.part2[b], nh * (e->dp.n_parts + 1));
#undef AL
    LCF_HIP(hipMemset(ds.nacc, 0, nw * sizeof(long long)));
    LCF_HIP(hipMemset(ds.err, 0, sizeof(int)));
    LCF_HIP(hipEventCreate(&s->ev0));
    LCF_HIP(hipEventCreate(&s->ev1));
    LCF_HIP(hipEventCreateWithFlags(&s->ev_snap, hipEventDisableTiming));
    LCF_HIP(hipHostMalloc((void**)&s->snap, s->snap_alloc(), hipHostMallocDefault));
    std::memset(s->snap, 0, s->snap_alloc());
    *out = s;
    return LCF_OK;
}

void lcf_sampler_destroy(lcf_sampler* s) { delete s; }

lcf_status lcf_sampler_reserve_chain(lcf_sampler* s, int64_t n_steps) {
    if (!s || n_steps < 0) return fail(LCF_ERR_INVALID_ARGUMENT, "bad argument");
    LCF_HIP(hipSetDevice(s->e->device));
    if (s->ds.store_chain && s->run_steps > 0 && n_steps > s->chain_cap)
        return fail(LCF_ERR_STATE, "the stored chain of the last run must be read (lcf_sampler_get_chain) before its buffer grows");
    return reserve_chain(s, n_steps);
}

lcf_status lcf_sampler_set_state(lcf_sampler* s, const double* coords) {
    if (!s || !coords) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    lcf_engine* e = s->e;
    LCF_HIP(hipSetDevice(e->device));
    LCF_HIP(hipDeviceSynchronize());
    s->pending = false;  // an uncommitted move of the old state is dropped with it
    s->foreign_stream = false;
    invalidate_snapshot(s);
    const DevSampler& ds = s->ds;
    if (lcf_status st = e->reserve(ds.n_walkers)) return st;
    LCF_HIP(hipMemcpyAsync(ds.X, coords, (size_t)ds.n_walkers * ds.n_dim * sizeof(double), hipMemcpyHostToDevice, e->stream));
    if (lcf_status st = logprob_dev(e, ds.n_walkers, ds.X, ds.LP, e->stream, 1)) return st;
    LCF_HIP(hipMemsetAsync(ds.nacc, 0, (size_t)ds.n_walkers * sizeof(long long), e->stream));
    LCF_HIP(hipMemsetAsync(ds.err, 0, sizeof(int), e->stream));
    std::memset(s->snap_flags(), 0, 2 * kSnapFlags * sizeof(unsigned int));   // (after the device synchronisation above)
    if (s->run_board_mem)   // (the abort word and its diagnosis behind the rows of the one-launch runs' board)
    {
        LCF_HIP(hipMemsetAsync(s->run_board_tail(), 0, kBoardClear * sizeof(unsigned int), e->stream));
        s->run_arrivals = 0;
    }
    LCF_HIP(hipStreamSynchronize(e->stream));
    s->has_state = true;
    return LCF_OK;
}

lcf_status lcf_sampler_get_state(lcf_sampler* s, double* coords, double* log_prob) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = settle(s)) return st;
    if (coords) std::memcpy(coords, s->snap + s->snap_x(), s->snap_lp() - s->snap_x());
    if (log_prob) std::memcpy(log_prob, s->snap + s->snap_lp(), s->snap_acc() - s->snap_lp());
    return LCF_OK;
}

lcf_status lcf_sampler_begin(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                             const int32_t* perm, int32_t store_chain) {
    if (lcf_status st = sampler_begin(s, first_step, n_steps, split_mode, perm, store_chain, true)) return st;
    // the half-steps of the phase API may be enqueued on a caller's stream, which is not ordered with the engine's own:
    // the first block of draw records (generated on the engine's stream) must be complete before this returns
    LCF_HIP(hipStreamSynchronize(s->e->stream));
    return LCF_OK;
}

// ---- phase-by-phase API (multi-GPU): propose -> evaluate(shard) -> [all-gather newlp] -> accept -------------------
lcf_status lcf_sampler_propose(lcf_sampler* s, int64_t step, int32_t half, void* stream) {
    if (lcf_status st = check_half_step(s, step, half, 0, 0, true)) return st;
    s->ds.inline_finalize = 0;  // accept tests read the gathered newlp
    // the shard is not known yet: every slot gets its coefficients (lcf_sampler_half_step knows it and is cheaper)
    return launch_next(s, true, 0, s->ds.n_half, stream ? (hipStream_t)stream : s->e->stream);
}
// propose + evaluate in one call: the shard is known, so the thermal states of [lo, hi) are computed by the same
// launch that draws the proposals (3 launches per half-step and rank: k_step, k_points, k_finalize).
lcf_status lcf_sampler_half_step(lcf_sampler* s, int64_t step, int32_t half, int32_t lo, int32_t hi, void* stream) {
    if (lcf_status st = check_half_step(s, step, half, lo, hi, true)) return st;
    hipStream_t st = stream ? (hipStream_t)stream : s->e->stream;
    s->ds.inline_finalize = 0;
    return launch_half_step_sharded(s, lo, hi, st);
}

lcf_status lcf_sampler_evaluate(lcf_sampler* s, int32_t lo, int32_t hi, void* stream) {
    if (!s || lo < 0 || hi < lo || hi > s->ds.n_half) return fail(LCF_ERR_INVALID_ARGUMENT, "bad shard range");
    if (!s->pending) return fail(LCF_ERR_STATE, "lcf_sampler_propose must precede lcf_sampler_evaluate");
    return launch_eval(s, lo, hi, true, stream ? (hipStream_t)stream : s->e->stream);
}
lcf_status lcf_sampler_accept(lcf_sampler* s, int64_t step, int32_t half, void* stream) {
    if (lcf_status st = check_half_step(s, step, half, 0, 0, false)) return st;
    // The accept/reject of a half-step is applied by the kernel that draws the next one (it needs the gathered
    // newlp, which is complete once this call is reached); only the run's last half-step is committed here.
    if (step == s->run_first + s->run_steps - 1 && half == 1)
        return flush_pending(s, stream ? (hipStream_t)stream : s->e->stream);
    return LCF_OK;
}
void* lcf_sampler_newlp_ptr(lcf_sampler* s) { return s ? s->ds.newlp[(s->g_next - 1) & 1] : nullptr; }
lcf_status lcf_sampler_set_half_step_kernel(lcf_sampler* s, int32_t choice, int32_t* used) {
    if (!s || choice < LCF_HALF_STEP_AUTO || choice > LCF_HALF_STEP_SOLO)
        return fail(LCF_ERR_INVALID_ARGUMENT, "bad half-step kernel choice");
    s->half_step_kernel = choice;
    static_assert(LCF_KERNEL_SOLO == 2 && LCF_KERNEL_FUSED == 1 && LCF_KERNEL_PHASES == 0, "what *used says of these");
    const int form = plan_run(s, false, 0, s->ds.n_half, true).form;
    if (used) *used = form == LCF_KERNEL_RUN ? 3 : form;
    return LCF_OK;
}

int32_t lcf_sampler_last_run_kernel(const lcf_sampler* s) { return s ? s->last_kernel : -1; }

int64_t lcf_sampler_last_run_launches(const lcf_sampler* s) { return s ? s->last_launches : 0; }

void lcf_sampler_last_run_instance(const lcf_sampler* s, int32_t out[4]) {
    for (int k = 0; out && k < 4; ++k) out[k] = s ? s->last_instance[k] : -1;
}

int32_t lcf_sampler_one_launch(const lcf_sampler* s) {
    return s && plan_run(s, false, 0, s->ds.n_half, false).form != LCF_KERNEL_PHASES ? 1 : 0;
}

lcf_status lcf_sampler_half_step_rows(lcf_sampler* s, int64_t step, int32_t half, int32_t lo, int32_t hi,
                                      void* stream) {
    if (lcf_status st = check_half_step(s, step, half, lo, hi, true)) return st;
    hipStream_t st = stream ? (hipStream_t)stream : s->e->stream;
    s->ds.inline_finalize = 1;  // accept tests add up the gathered rows
    return launch_half_step_rows(s, lo, hi, st);
}

void* lcf_sampler_rows_ptr(lcf_sampler* s, int32_t* row_doubles) {
    if (!s) return nullptr;
    if (row_doubles) *row_doubles = s->e->dp.n_parts + 1;
    return s->ds.part2[(s->g_next - 1) & 1];
}

lcf_status lcf_sampler_check(lcf_sampler* s) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = settle(s)) return st;
    const int err = reported_error(s);
    if (err & 2) {
        // (an aborted multi-rank run leaves the ranks with different states -- a rank has committed its own walkers of
        // the half-step the others gave up on: the ensemble must be set again, on every rank, before the next run)
        const double sec = (double)s->ds.wait_ticks / 1e8;
        unsigned int w[kBoardClear] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const bool run = s->last_kernel == LCF_KERNEL_RUN && s->run_board_mem && !s->last_rows;
        if (run)
            hipMemcpy(w, s->run_board_tail(), sizeof w, hipMemcpyDeviceToHost);
        else if (s->board_mem)
            hipMemcpy(w, s->board_tail(), sizeof w, hipMemcpyDeviceToHost);
        if (run && s->replay_steps >= 0 && s->replay_split != LCF_SPLIT_HOST) {
            // The launch gave up (rewind_resident_run): the same steps with a launch per half-step, as later runs.
            LCF_HIP(hipStreamSynchronize(s->e->stream));
            if (lcf_status r = rewind_resident_run(s)) return r;
            static bool told = false;
            if (!told)
                std::fprintf(stderr, "liblcf_hip: a one-launch run waited %.2f s for version %u of walker %u: its workgroups were "
                             "not all resident (another resident kernel on this GPU?); the steps are repeated with a launch per "
                             "half-step, as are this sampler's later runs (LCF_NO_RUN_KERNEL=1 avoids the wait)\n",
                             w[1] == 3 ? (double)s->ds.resident_ticks / 1e8 : sec, w[2], w[3]);
            if (!told && std::getenv("LCF_TRACE_RUN"))
                std::fprintf(stderr, "liblcf_hip: (what %u, column %u, workgroups started %u; the entry held {%08x tag %u | %08x tag %u}; host: "
                             "%d walkers, board %08x)\n", w[1], w[4], w[5], w[6], w[7], w[8], w[9], s->ds.n_walkers,
                             (unsigned int)(unsigned long long)s->run_board_mem);
            told = true;
            s->run_off = true;
            s->spec_first = -1;
            const int64_t n = s->replay_steps;
            s->replay_steps = -1;
            if (lcf_status st = lcf_sampler_run_async(s, s->replay_first, n, s->replay_split, nullptr, s->replay_store)) return st;
            return lcf_sampler_check(s);
        }
        if (run) {
            char msg[260];
            std::snprintf(msg, sizeof msg, "one-launch run: version %u of walker %u (column %u) was not posted within %.1f s: "
                          "the launch's workgroups were not all resident (another process's persistent kernel on this "
                          "GPU?); set the state again and run with LCF_NO_RUN_KERNEL=1", w[2], w[3], w[4], sec);
            return fail(LCF_ERR_STATE, msg);
        }
        if (w[0]) {
            char msg[300];
            if (w[1] == 1)
                std::snprintf(msg, sizeof msg, "row-board run: version %u of walker %u (column %u) was not posted within "
                              "%.1f s: a rank is missing or behind (set_state is required on all ranks before the next run)",
                              w[2], w[3], w[4], sec);
            else if (w[1] == 3)
                std::snprintf(msg, sizeof msg, "row-board run: version %u of walker %u did not arrive within %.2f s and only "
                              "%u workgroups of this rank's resident launch had started: another resident kernel holds this "
                              "GPU (set_state is required on all ranks before the next run)", w[2], w[3],
                              (double)s->ds.resident_ticks / 1e8, w[4]);
            else if (s->last_kernel == LCF_KERNEL_RUN)
                std::snprintf(msg, sizeof msg, "row-board run: the launch from half-step %u waited %.1f s for rank %u to "
                              "reach half-step %u (set_state is required on all ranks before the next run)", w[2], sec, w[3], w[4]);
            else
                std::snprintf(msg, sizeof msg, "row-board run: half-step %u waited %.1f s for rank %u to finish half-step "
                              "%u (set_state is required on all ranks before the next run)", w[2], sec, w[3], w[2] - 2);
            return fail(LCF_ERR_STATE, msg);
        }
        char msg[200];
        std::snprintf(msg, sizeof msg, "a peer's rows did not arrive within %.1f s (peer-mailbox run; set_state is required "
                      "on all ranks before the next run)", sec);
        return fail(LCF_ERR_STATE, msg);
    }
    if (err) return fail(LCF_ERR_NAN_LOGPROB, "Probability function returned NaN");
    return LCF_OK;
}

// Enqueue a whole run on the engine's stream and return: several samplers (one engine each = one transient of a
// population) then execute concurrently on the device.  lcf_sampler_wait() completes it.
lcf_status lcf_sampler_run_async(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                 const int32_t* perm, int32_t store_chain) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    // (resident workgroups where the plan takes them and no other stream's hold the device: else the plan without them)
    RunPlan plan = plan_run(s, false, 0, s->ds.n_half, n_steps > 0);
    RunClaim claim{s->e->device, s->e->stream, plan.form == LCF_KERNEL_RUN && run_claim(s->e->device, s->e->stream)};
    if (plan.form == LCF_KERNEL_RUN && !claim.held) plan = plan_run(s, false, 0, s->ds.n_half, false);
    if (lcf_status st = sampler_begin(s, first_step, n_steps, split_mode, perm, store_chain, plan.need_slots)) return st;
    hipStream_t st = s->e->stream;
    s->ds.inline_finalize = 1;  // single GPU: no separate finalize / accept launches
    LCF_HIP(hipEventRecord(s->ev0, st));
    if (plan.form == LCF_KERNEL_RUN) {   // the workgroups stay for a block of half-steps and hand each other rows (k_solo_run)
        if (lcf_status r = run_buffers(s)) return r;
        if (lcf_status r = prepare_run(s->e, plan)) return r;
        s->replay_first = first_step;
        s->replay_steps = n_steps;
        s->replay_split = split_mode;
        s->replay_store = store_chain;
        long long launches = 0;
        for (long long rel = 0; rel < 2 * n_steps; ++launches) {   // (the first launch posts the start state on the board itself)
            if (lcf_status r = enter_half_step(&s, 1, rel, st)) return r;
            const int n = s->block_span(rel, plan.span);
            if (lcf_status r = launch_run(s, plan, rel, n, st, 0)) return r;
            if (lcf_status r = leave_half_step(&s, 1, st)) return r;
            rel += n;
        }
        s->record_run(plan.form, false, launches, plan.instance);
        s->g_next += 2 * n_steps;
        s->flip_state_sets();                  // the state behind this run is in the other set now
        LCF_HIP(hipEventRecord(s->ev1, st));
        claim.release();
        // (the last step wrote the snapshot with the state: no snapshot kernel; the caller waits for this event)
        LCF_HIP(hipEventRecord(s->ev_snap, st));
        s->snap_enqueued = true;
        s->snap_valid = false;
        return speculate_continuation(s, st);
    }
    // per half-step: ONE launch (k_fused) when everything a workgroup needs fits in LDS, else
    // [commit previous + draw + thermal states] -> [per-point likelihood]; one trailing commit
    if (plan.form == LCF_KERNEL_SOLO) {  // one workgroup per proposal, nothing pending between launches
        for (int64_t k = 0; k < 2 * n_steps; ++k)
            if (lcf_status r = launch_solo(s, plan, k, st)) return r;
        s->g_next += 2 * n_steps;
    } else if (plan.form == LCF_KERNEL_FUSED) {
        for (int64_t k = 0; k < 2 * n_steps; ++k)
            if (lcf_status r = launch_fused(s, 0, s->ds.n_half, st)) return r;
        if (lcf_status r = flush_pending(s, st)) return r;
    } else {
        for (int64_t k = 0; k < 2 * n_steps; ++k) {
            if (lcf_status r = launch_next(s, true, 0, s->ds.n_half, st)) return r;
            if (lcf_status r = launch_eval(s, 0, s->ds.n_half, false, st)) return r;
        }
        if (lcf_status r = flush_pending(s, st)) return r;
    }
    s->record_run(plan.form, false, 2 * n_steps, plan.instance);
    LCF_HIP(hipEventRecord(s->ev1, st));
    if (lcf_status r = enqueue_snapshot(s)) return r;
    return speculate_continuation(s, st);
}

lcf_status lcf_sampler_wait(lcf_sampler* s) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = lcf_sampler_check(s)) return st;  // (waits for the run and its snapshot)
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) s->last_ms = ms;
    return LCF_OK;
}

lcf_status lcf_sampler_run(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                           const int32_t* perm, int32_t store_chain) {
    static const bool trace = std::getenv("LCF_TRACE_RUN") != nullptr;   // (diagnostic: host time of the two halves)
    const auto t0 = std::chrono::steady_clock::now();
    if (lcf_status st = lcf_sampler_run_async(s, first_step, n_steps, split_mode, perm, store_chain)) return st;
    const auto t1 = std::chrono::steady_clock::now();
    const lcf_status r = lcf_sampler_wait(s);
    if (trace) {
        const auto t2 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "lcf_sampler_run: %lld steps enqueued in %.1f us, waited %.1f us, device %.1f us\n",
                     (long long)n_steps, std::chrono::duration<double, std::micro>(t1 - t0).count(),
                     std::chrono::duration<double, std::micro>(t2 - t1).count(), 1e3 * s->last_ms);
    }
    return r;
}

lcf_status lcf_sampler_get_chain(lcf_sampler* s, double* chain, double* log_prob) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (!s->ds.store_chain || s->run_steps == 0) return fail(LCF_ERR_STATE, "no stored chain");
    if (lcf_status st = settle(s)) return st;  // (the trailing commit writes the last chain row)
    const DevSampler& ds = s->ds;
    if (chain)
        LCF_HIP(hipMemcpy(chain, ds.chain, (size_t)s->run_steps * ds.n_walkers * ds.n_dim * sizeof(double), hipMemcpyDeviceToHost));
    if (log_prob)
        LCF_HIP(hipMemcpy(log_prob, ds.chain_lp, (size_t)s->run_steps * ds.n_walkers * sizeof(double), hipMemcpyDeviceToHost));
    return LCF_OK;
}

lcf_status lcf_sampler_get_naccepted(lcf_sampler* s, int64_t* n_accepted) {
    if (!s || !n_accepted) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = settle(s)) return st;
    std::memcpy(n_accepted, s->snap + s->snap_acc(), s->snap_bytes() - s->snap_acc());
    return LCF_OK;
}

lcf_status lcf_sampler_get_snapshot(lcf_sampler* s, double* coords, double* log_prob, int64_t* n_accepted) {
    if (!s) return fail(LCF_ERR_INVALID_ARGUMENT, "null argument");
    if (lcf_status st = settle(s)) return st;
    if (coords) std::memcpy(coords, s->snap + s->snap_x(), s->snap_lp() - s->snap_x());
    if (log_prob) std::memcpy(log_prob, s->snap + s->snap_lp(), s->snap_acc() - s->snap_lp());
    if (n_accepted) std::memcpy(n_accepted, s->snap + s->snap_acc(), s->snap_bytes() - s->snap_acc());
    return LCF_OK;
}

double lcf_sampler_last_run_ms(const lcf_sampler* s) { return s ? s->last_ms : 0.; }

}  // extern "C"

// (diagnostic, not in lcf.h) a copy of the board of the sampler's one-launch runs: rows, then the tail words
extern "C" long long lcf_debug_read_run_board(lcf_sampler* s, void* out, long long max_bytes) {
    if (!s || !s->run_board_mem) return -1;
    const long long n = std::min<long long>(max_bytes, (long long)s->run_board_bytes());
    if (hipMemcpy(out, s->run_board_mem, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    return n;
}
