/*
 * lcf.h -- C ABI of the MI355X (gfx950) batched light-curve log-likelihood engine.
 *
 * This is the drop-in boundary for the emcee-driven hot path of griffin-h/lightcurve_fitting.  The reference has no
 * native code: the seam is the Python callable that `fitting.lightcurve_mcmc` hands to `emcee.EnsembleSampler`
 * (reference fitting.py:121-130).  Each entry point below names the reference interface it replaces.  All arrays are
 * caller-owned; the engine copies photometry and tables to the device at create time and never writes to caller
 * memory except the documented outputs.  No exceptions cross this boundary: every call returns an lcf_status.
 *
 * Shapes: a "walker block" P is row-major (n x n_dim) float64, exactly what emcee passes to a `vectorize=True`
 * log-probability function.  Units follow the reference (days, kK, 1000 Rsun, THz, W/Hz).
 *
 * Thread-safety: calls on one engine (or one sampler) must be serialised by the caller; distinct engines are
 * independent.  One engine is bound to one HIP device.
 */
#ifndef LCF_H
#define LCF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCF_ABI_VERSION 8

typedef enum lcf_status {
    LCF_OK = 0,
    LCF_ERR_INVALID_ARGUMENT = 1, /* NULL pointer, bad size, unknown model, inconsistent tables */
    LCF_ERR_HIP = 2,              /* a HIP runtime call failed; see lcf_last_error() */
    LCF_ERR_NO_DEVICE = 3,        /* no usable GPU: this library has no CPU fallback */
    LCF_ERR_OUT_OF_MEMORY = 4,
    LCF_ERR_UNSUPPORTED = 5,      /* e.g. an unknown model id, or a host-supplied split in a population run */
    LCF_ERR_NAN_LOGPROB = 6,      /* sampler: a log-probability evaluated to NaN (emcee raises ValueError here) */
    LCF_ERR_STATE = 7             /* call sequence error (e.g. run before set_state) */
} lcf_status;

/* Model families (reference models.py).  Values are stable ABI. */
typedef enum lcf_model {
    LCF_MODEL_SHOCK_COOLING = 1,      /* ShockCooling          models.py:301-353  p = v_s, M_env, f_rho_M, R, t_0     */
    LCF_MODEL_SHOCK_COOLING2 = 2,     /* ShockCooling2         models.py:356-411  p = T_1, L_1, t_tr, t_0             */
    LCF_MODEL_SHOCK_COOLING3 = 3,     /* ShockCooling3         models.py:433-496  p = v_s,M_env,f_rho_M,R,d_L,E(B-V),t_0 */
    LCF_MODEL_SHOCK_COOLING4 = 4,     /* ShockCooling4         models.py:507-632  p = v_s, M_env, f_rho_M, R, t_0     */
    LCF_MODEL_COMPANION_SHOCKING = 5, /* CompanionShocking     models.py:848-918  p = t_0,a,Mv7,t_max,s,r_r,r_i,r_U   */
    LCF_MODEL_COMPANION_SHOCKING2 = 6,/* CompanionShocking2    models.py:921-980  p = t_0,a,Mv7,t_max,s,dt_U,dt_i     */
    LCF_MODEL_COMPANION_SHOCKING3 = 7,/* CompanionShocking3    models.py:983-1045 p = t_0,a,theta,t_max,s,dt_U,dt_i   */
    LCF_MODEL_BLACKBODY = 8,          /* direct (T, R) blackbody, bolometric.py:154-164                              */
    LCF_MODEL_CUSTOM = 9,             /* T(t), R(t) from a program compiled at run time: "custom models" below       */
    LCF_MODEL_ARNETT = 10,            /* bolometric: 56Ni/56Co heating, Arnett diffusion   p = M_Ni, tau_m, [t_gamma,] t_0    */
    LCF_MODEL_MAGNETAR = 11           /* bolometric: magnetar spin-down, Arnett diffusion  p = E_p, t_p, tau_m, [t_gamma,] t_0 */
} lcf_model;

/* Priors (reference models.py:1048-1098).  Bounds are strict: p_min < p < p_max, else log-prior = -inf. */
typedef enum lcf_prior_kind { LCF_PRIOR_UNIFORM = 0, LCF_PRIOR_LOG_UNIFORM = 1, LCF_PRIOR_GAUSSIAN = 2 } lcf_prior_kind;

typedef struct lcf_prior {
    int32_t kind; /* lcf_prior_kind */
    int32_t reserved;
    double p_min, p_max;
    double mean, stddev; /* Gaussian only */
} lcf_prior;

enum { LCF_SIGMA_RELATIVE = 0, LCF_SIGMA_ABSOLUTE = 1 };
enum { LCF_N_CONSTS = 12 };

/*
 * One fitting problem = one light curve + one model instance (with its construction-time constants baked in).
 *
 * consts[] by model:
 *   SHOCK_COOLING, SHOCK_COOLING2: A, a, alpha, epsilon_1, epsilon_2, L_0, T_0, Tph_to_Tcol  (models.py:192-226)
 *   SHOCK_COOLING4:                A, a, alpha, L_br_0, T_col_br_0, t_br_0, t_tr_0           (models.py:567-577)
 *   CUSTOM:                        all 12 are the caller's: what the state function receives as `consts`
 *   ARNETT, MAGNETAR:              redshift z, gamma-ray leakage (0: none; non-zero: t_gamma is a parameter, in front of
 *                                  t_0, and n_par is one more): "central-engine models" below
 *   others:                        unused
 *   (consts[8..11] are scratch for the engine: whatever the caller puts there is overwritten -- not for CUSTOM)
 *
 * Band tables: filter i owns samples tab_off[i] .. tab_off[i+1]-1 of (tab_a, tab_w) with
 *   a_k = c1 nu_k (1+z)  [kK],   W_k = c2 nu'_k^3 min(1, nu_cut/nu'_k) tw_k Tnorm_k,
 * so that L_nu(filter; T, R) = R^2 sum_k W_k / (exp(a_k/T) - 1)   (filters.py:308-310 + models.py:1127-1128).
 *
 * Companion-shocking extras (NULL / 0 otherwise): per-filter parameter indices (or -1) for the factor on the shock
 * term, the factor on the SiFTO term and the SiFTO time offset (models.py:804-807, 913-916), and one piecewise-cubic
 * per filter: spline_coef[f][i][0..3] are the coefficients of (x - knot_i)^3..^0 on [knot_i, knot_i+1]; the
 * template is 0 outside [knot_0, knot_{n-1}] (models.py:717, 826).
 */
typedef struct lcf_problem {
    int32_t abi_version; /* LCF_ABI_VERSION */
    int32_t model;       /* lcf_model */
    int32_t n_par;       /* model parameters (without the optional intrinsic-scatter parameter); CUSTOM: the caller's */
                         /* (ARNETT: 3, MAGNETAR: 4, one more with leakage) */
    int32_t use_sigma;   /* 1: the last of n_dim = n_par + 1 parameters is sigma (models.py:128-130) */
    int32_t sigma_type;  /* LCF_SIGMA_RELATIVE | LCF_SIGMA_ABSOLUTE (models.py:121-126) */
    int32_t n_filters;   /* ARNETT, MAGNETAR: 0 -- no filters, filt_idx and every table pointer NULL */
    int64_t n_points;
    double consts[LCF_N_CONSTS];
    const double* t;          /* [n_points] observation times (lc['MJD'])                     models.py:117 */
    const double* y;          /* [n_points] observed luminosity density (lc['lum'])           models.py:118 */
    const double* dy;         /* [n_points] its uncertainty (lc['dlum'])                      models.py:119 */
    const int32_t* filt_idx;  /* [n_points] filter of each point, 0 <= . < n_filters          models.py:116 */
    const int32_t* tab_off;   /* [n_filters + 1] */
    const double* tab_a;      /* [tab_off[n_filters]] */
    const double* tab_w;      /* [tab_off[n_filters]] */
    /* Reddening, LCF_MODEL_SHOCK_COOLING3 only (NULL otherwise): A_lambda / E(B-V) of the extinction law at every
     * table sample, so that sample k is weighted by 10^(-0.4 E(B-V) tab_ext[k]) per walker
     * (filters.py:32-33, 308-310: extinction_law(freq, ebv) inside Filter.synthesize). */
    const double* tab_ext;    /* [tab_off[n_filters]] */
    /* Optional compressed companions (all NULL = none): per filter a shorter table (the Gauss quadrature of the full
     * table's own discrete measure, computed by the host packer) that reproduces the band sum to 2e-14 for every
     * temperature T >= ctab_tmin[i]; the engine switches per data point and uses the full table below it. */
    const int32_t* ctab_off;  /* [n_filters + 1] */
    const double* ctab_a;     /* [ctab_off[n_filters]] */
    const double* ctab_w;     /* [ctab_off[n_filters]] */
    const double* ctab_tmin;  /* [n_filters] kK; +inf = never use the compressed table of this filter */
    /* Optional second compressed level (all NULL = none; needs the first): a still shorter table per filter, valid
     * above a higher temperature htab_tmin[i] >= ctab_tmin[i].  Per data point the engine takes the shortest table
     * that is valid at the point's temperature: hot, else cool, else full. */
    const int32_t* htab_off;  /* [n_filters + 1] */
    const double* htab_a;     /* [htab_off[n_filters]] */
    const double* htab_w;     /* [htab_off[n_filters]] */
    const double* htab_tmin;  /* [n_filters] kK */
    /* Optional third level (NULL = none; not for LCF_MODEL_SHOCK_COOLING3): the band sum of every filter as a FUNCTION
     * of temperature -- ln S_f(T) as piecewise polynomials of degree 7 in u = ln T on itab_m equal intervals of width
     * itab_h from itab_u0 = ln(first temperature in kK), 8 monomial coefficients in s in [-1, 1] per interval, highest
     * power first -- valid for T >= itab_tmin[i] up to the last interval's end.  The host packer builds and proves them
     * (filters.interp_planck_table).  With it the engine evaluates a data point by one lookup, 7 fused multiply-adds
     * and one exponential wherever the point's temperature is inside the range; elsewhere it walks the sample tables. */
    const double* itab_coef;  /* [n_filters][itab_m][8] */
    const double* itab_tmin;  /* [n_filters] kK; +inf = no interpolant for this filter */
    int32_t itab_m;
    int32_t reserved2;
    double itab_u0, itab_h;
    const int32_t* filt_kasen_par; /* [n_filters] or NULL */
    const int32_t* filt_sifto_par; /* [n_filters] or NULL */
    const int32_t* filt_dt_par;    /* [n_filters] or NULL */
    int32_t n_knots;
    int32_t reserved;
    const double* spline_knots;    /* [n_knots] ascending */
    const double* spline_coef;     /* [n_filters][n_knots - 1][4] */
    const lcf_prior* priors;       /* [n_par + use_sigma] or NULL (then log_posterior == log_likelihood) */
} lcf_problem;

typedef struct lcf_engine lcf_engine;
typedef struct lcf_sampler lcf_sampler;

/* ---- library ------------------------------------------------------------------------------------------------ */
int32_t lcf_abi_version(void);
/* Human-readable description of the last failure on the calling thread ("" if none). */
const char* lcf_last_error(void);
/* Number of HIP devices visible (0 if none / no driver).  Never initialises a context on a device. */
int32_t lcf_device_count(void);

/* ---- engine --------------------------------------------------------------------------------------------------- */
/* Replaces the closure set-up of fitting.py:68-128 (photometry columns + model + priors captured once). */
lcf_status lcf_engine_create(const lcf_problem* problem, int32_t device, lcf_engine** out);
void lcf_engine_destroy(lcf_engine* e);
int32_t lcf_engine_ndim(const lcf_engine* e);
int64_t lcf_engine_npoints(const lcf_engine* e);
/* Planck samples of one log-likelihood evaluation over the full tables: sum over points of K_filter. */
int64_t lcf_engine_samples_per_eval(const lcf_engine* e);
/* Select the band-sum level: 0 = libm expm1 + divide over the full tables (reference-shaped), 1 = fused fast path
 * over the full tables, 2 = fused fast path over the Gauss-compressed tables where valid, 3 = the interpolants of
 * ln S_f(ln T) where a point's temperature is inside the range they are proved for, else level 2.  An engine starts
 * at the highest level its problem gave tables for (3 with itab_*, else 2 with ctab_*, else 1). */
lcf_status lcf_engine_set_variant(lcf_engine* e, int32_t variant);

/* Model.log_likelihood (models.py:93-136) for a block of n walkers.  Host pointers. out[n]. */
lcf_status lcf_log_likelihood(lcf_engine* e, int64_t n, const double* P, double* out);
/* log_posterior closure (fitting.py:121-128): -inf where a prior excludes the walker (likelihood skipped). */
lcf_status lcf_log_posterior(lcf_engine* e, int64_t n, const double* P, double* out);
/* Same with DEVICE pointers, enqueued on `stream` (a hipStream_t), no host sync.  NULL selects the engine's own
 * non-blocking stream, which is NOT ordered with the legacy default stream: pass a real stream to chain with other
 * work (the Python driver runs under a side stream for that reason). */
lcf_status lcf_log_likelihood_dev(lcf_engine* e, int64_t n, const double* dP, double* dout, void* stream);
lcf_status lcf_log_posterior_dev(lcf_engine* e, int64_t n, const double* dP, double* dout, void* stream);

/* Model.__call__ / evaluate (models.py:86-87, pointwise branch :1161-1162): y_fit[n][n_points], original point order. */
lcf_status lcf_model_evaluate(lcf_engine* e, int64_t n, const double* P, double* y_fit);
/* temperature_radius (models.py:231-269, 583-597, 727-755): T_K, R_bb as [n][n_points]. */
lcf_status lcf_temperature_radius(lcf_engine* e, int64_t n, const double* P, double* T_K, double* R_bb);
/* blackbody_to_filters pointwise (models.py:1131-1165): out[m] = L_nu(filter filt_idx[m]; T[m], R[m]). */
lcf_status lcf_blackbody_to_filters(lcf_engine* e, int64_t m, const int32_t* filt_idx, const double* T,
                                    const double* R, double* out);

/* Measurement hook for bench.py: average duration [ms] of the dominant kernel alone (the per-point likelihood
 * kernel over n walkers), reps back-to-back launches bracketed by HIP events on the engine's stream. */
lcf_status lcf_profile_loglike_kernel(lcf_engine* e, int64_t n, const double* P, int32_t reps, double* avg_ms);

/* ---- device-resident ensemble sampler (replaces emcee.EnsembleSampler for this path, fitting.py:130-145) -------- */
/* Goodman-Weare stretch move, red/blue halves, scale a.  RNG: Philox4x32-10 keyed by seed with counters
 * (walker, step, half) -- independent of how walkers are sharded over devices. */
lcf_status lcf_sampler_create(lcf_engine* e, int32_t n_walkers, uint64_t seed, double a, lcf_sampler** out);
void lcf_sampler_destroy(lcf_sampler* s);
/* coords[n_walkers][n_dim] host; evaluates the initial log-posterior on the device. */
lcf_status lcf_sampler_set_state(lcf_sampler* s, const double* coords);
lcf_status lcf_sampler_get_state(lcf_sampler* s, double* coords, double* log_prob);
/* Device memory for the chain of a later run of n_steps steps with store_chain, allocated now instead of inside that
 * run (emcee grows its backend inside run_mcmc, fitting.py:133-148; a caller that times a run reserves first). */
lcf_status lcf_sampler_reserve_chain(lcf_sampler* s, int64_t n_steps);
/* Red/blue colouring of each step.  RANDOM = emcee's randomize_split, generated on the device from (seed, step);
 * HOST = caller-provided perm[n_steps][n_walkers] int32 (the first half of each row is colour 0). */
enum { LCF_SPLIT_IDENTITY = 0, LCF_SPLIT_RANDOM = 1, LCF_SPLIT_HOST = 2 };
/* Run n_steps ensemble steps numbered from first_step (the step number is an RNG counter word). */
lcf_status lcf_sampler_run(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                           const int32_t* perm, int32_t store_chain);
/* The same split in two: enqueue the whole run on the engine's stream and return at once / wait for it and check.
 * Samplers on different engines (population mode: one transient each) run concurrently between the two calls. */
lcf_status lcf_sampler_run_async(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                 const int32_t* perm, int32_t store_chain);
lcf_status lcf_sampler_wait(lcf_sampler* s);
/* Population mode: run n samplers (independent transients with the same walker count, on one device) in lock step:
 * ONE launch per half-step covers all of them where every transient has shared epochs, tables staged in LDS and
 * proposal-independent tables (k_pop), else one proposal launch and one likelihood launch.  split_mode: identity or
 * random.  LCF_NO_POP=1 in the environment forces the two launches (tests). */
lcf_status lcf_population_run(lcf_sampler** samplers, int32_t n, int64_t first_step, int64_t n_steps,
                              int32_t split_mode, int32_t store_chain, double* elapsed_ms);
/* Chain of the last run: chain[n_steps][n_walkers][n_dim], log_prob[n_steps][n_walkers] (either may be NULL). */
lcf_status lcf_sampler_get_chain(lcf_sampler* s, double* chain, double* log_prob);
lcf_status lcf_sampler_get_naccepted(lcf_sampler* s, int64_t* n_accepted /* [n_walkers] */);
/* lcf_sampler_get_state and lcf_sampler_get_naccepted in ONE call (any pointer may be NULL): what a driver reads after
 * every run -- emcee's State and the acceptance counts (fitting.py:133, 145) -- for one trip through the binding. */
lcf_status lcf_sampler_get_snapshot(lcf_sampler* s, double* coords, double* log_prob, int64_t* n_accepted);
/* Device time of the last lcf_sampler_run in milliseconds (HIP events on the sampler's stream). */
double lcf_sampler_last_run_ms(const lcf_sampler* s);
/* 1 if half-steps of this sampler run as one launch (everything a workgroup needs fits in LDS), 0 if as
 * proposal + likelihood launches.  Same chain either way. */
int32_t lcf_sampler_one_launch(const lcf_sampler* s);
/* Which kernels a single-GPU run (lcf_sampler_run / _run_async) may use for a half-step.  All of them produce the
 * same chain bit for bit; the choice exists for tests and measurements.
 *   AUTO:   one workgroup per proposal that also accepts / rejects, resident for a whole block of half-steps
 *           (k_solo_run: ONE launch per up to 128 steps (256 half-steps), rows handed from workgroup to workgroup through a board of
 *           tagged rows in device memory) where a proposal's parts fit one workgroup; else one workgroup per
 *           (proposal, part) and launch (k_fused); else proposal + likelihood launches
 *   SOLO:   as AUTO, but one launch per half-step (k_solo)
 *   FUSED:  never k_solo        PHASES: always proposal + likelihood launches
 * Returns in *used (optional) what a run would use now: 3 = k_solo_run, 2 = k_solo, 1 = k_fused, 0 = separate launches.
 * (LCF_NO_RUN_KERNEL=1 in the environment: AUTO never picks k_solo_run -- for several processes sharing one GPU, whose
 * resident launches could keep each other's workgroups out.) */
enum { LCF_HALF_STEP_AUTO = 0, LCF_HALF_STEP_FUSED = 1, LCF_HALF_STEP_PHASES = 2, LCF_HALF_STEP_SOLO = 3 };
lcf_status lcf_sampler_set_half_step_kernel(lcf_sampler* s, int32_t choice, int32_t* used);

/* What the half-steps of the sampler's last run were executed by (-1: no run yet): separate proposal / likelihood
 * launches, k_fused, k_solo; for lcf_population_run resident workgroups for all transients (k_pop_run), one launch per
 * half-step for all transients (k_pop: a workgroup per four proposals, accept test included) or the two launches
 * k_step_multi + k_points_multi. */
enum { LCF_KERNEL_PHASES = 0, LCF_KERNEL_FUSED = 1, LCF_KERNEL_SOLO = 2, LCF_KERNEL_POPULATION = 3,
       LCF_KERNEL_POPULATION_PHASES = 4, LCF_KERNEL_RUN = 5 /* k_solo_run: a block of half-steps per launch */,
       LCF_KERNEL_POPULATION_RUN = 6 /* k_pop_run: the same for all transients of a population */ };
int32_t lcf_sampler_last_run_kernel(const lcf_sampler* s);
/* Launches of that kernel in the last single-GPU run (lcf_sampler_run / _run_async): two per step, or -- k_solo_run --
 * one per block of up to 128 steps (between ranks: 32); lcf_population_run: launches per run of the kernel it took. */
int64_t lcf_sampler_last_run_launches(const lcf_sampler* s);
/* The template instance <ND, NP, M, ranks> the last run's half-step kernel was launched with: ND the compile-time fit
 * dimension (0: the generic kernel, dimension at run time), NP the parts per workgroup (2, 4, or 8 = the 1024-thread
 * form; 0 for lcf_population_run, whose kernels take the parts at run time), M the model whose own kernel it was (0:
 * none), ranks 1 for a row-board run.  Four times -1 where no such kernel ran: k_fused, the separate launches, no run yet.
 * Host bookkeeping for tests and measurements: which row of the instantiation table a problem shape reaches. */
void lcf_sampler_last_run_instance(const lcf_sampler* s, int32_t out[4]);

/* Multi-GPU building blocks: one half-step split into phases so that the caller can all-gather the shard's new
 * log-probabilities (RCCL) between phase 2 and phase 3.  All enqueue on `stream` without host sync.
 *   1. propose:  every rank draws the same proposals for the whole active half (replicated, cheap)
 *   2. evaluate: this rank evaluates proposals [lo, hi) of the active half -> newlp[lo:hi)
 *   3. accept:   every rank applies the same accept/reject to the whole half given the gathered newlp[0:n/2) */
lcf_status lcf_sampler_begin(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                             const int32_t* perm, int32_t store_chain);
lcf_status lcf_sampler_propose(lcf_sampler* s, int64_t step, int32_t half, void* stream);
lcf_status lcf_sampler_evaluate(lcf_sampler* s, int32_t lo, int32_t hi, void* stream);
lcf_status lcf_sampler_accept(lcf_sampler* s, int64_t step, int32_t half, void* stream);
/* Phases 1 + 2 in one call (fewer launches: the thermal states of the shard ride on the proposal kernel). */
lcf_status lcf_sampler_half_step(lcf_sampler* s, int64_t step, int32_t half, int32_t lo, int32_t hi, void* stream);
/* Device pointer to newlp[n_walkers/2] (float64) for the collective. */
void* lcf_sampler_newlp_ptr(lcf_sampler* s);
/* The same half-step without the finalize launch: what the collective then carries is each proposal's ROW --
 * its partial chi^2 sums followed by its log-prior, *row_doubles float64 -- and the accept tests of the next launch add
 * a row up themselves (the protocol of lcf_sampler_run_sharded).  Use one protocol throughout a run.
 * lcf_sampler_rows_ptr: device pointer to rows[n_walkers/2][*row_doubles] of the half-step drawn last. */
lcf_status lcf_sampler_half_step_rows(lcf_sampler* s, int64_t step, int32_t half, int32_t lo, int32_t hi, void* stream);
void* lcf_sampler_rows_ptr(lcf_sampler* s, int32_t* row_doubles);
lcf_status lcf_sampler_check(lcf_sampler* s); /* syncs; returns LCF_ERR_NAN_LOGPROB if a NaN was seen */

/* ---- native multi-GPU run: RCCL bound at run time -------------------------------------------------------------- */
/* rccl_path: the librccl.so to dlopen (NULL/"" = the default search path; pass the one PyTorch ships when torch is
 * in the process).  One rank obtains an id, every rank creates its communicator with it (collective call). */
typedef struct { char internal[128]; } lcf_comm_id;
typedef struct lcf_comm lcf_comm;
/* Local, non-collective check that RCCL can be bound (call it on every rank and agree before the collective calls). */
lcf_status lcf_comm_probe(const char* rccl_path);
lcf_status lcf_comm_unique_id(const char* rccl_path, lcf_comm_id* out);
lcf_status lcf_comm_create(const char* rccl_path, const lcf_comm_id* id, int32_t n_ranks, int32_t rank, int32_t device,
                           lcf_comm** out);
void lcf_comm_destroy(lcf_comm* c);
/* Number of ranks as the communicator itself reports it (ncclCommCount), and this rank's index (ncclCommUserRank). */
lcf_status lcf_comm_count(const lcf_comm* c, int32_t* n_ranks, int32_t* rank);
/* Measurement hook for bench.py: average time [ms] of ONE in-place all-gather as lcf_sampler_run_sharded issues it per
 * half-step for sampler s (its rows, float64), `reps` of them back to back on the engine's stream between two HIP
 * events.  Collective: every rank calls it with the same arguments. */
lcf_status lcf_comm_time_allgather(lcf_comm* c, lcf_sampler* s, int32_t reps, double* avg_ms);
/* The whole run of lcf_sampler_run, sharded: this rank evaluates proposals [rank*w, (rank+1)*w) of each half-step
 * (w = n_walkers / 2 / n_ranks) and one in-place ncclAllGather per half-step (each proposal's partial chi^2 sums and
 * log-prior, which every rank then adds up in the same order) makes the ranks agree; enqueued on the
 * engine's stream without host synchronisation between half-steps.  Collective: same arguments on every rank. */
lcf_status lcf_sampler_run_sharded(lcf_sampler* s, lcf_comm* c, int64_t first_step, int64_t n_steps,
                                   int32_t split_mode, const int32_t* perm, int32_t store_chain);

/* ---- sharded run WITHOUT a collective: peer mailboxes (behind a switch until measured on a multi-GPU node) ---------- */
/* Every rank owns a mailbox in uncached device memory; a rank that has evaluated a proposal stores the numbers of its
 * row -- each as two 8-byte {data, generation} granules -- straight into every rank's mailbox (peers' memory mapped
 * through HIP IPC: xGMI writes on a node) and the accept tests of the next launch poll their own copy.  No kernel and
 * no host call sits between two half-steps.  Set-up: every rank exports its mailbox, the handles travel by any means
 * (the Python driver uses torch.distributed), every rank connects with the full list.  `local_ptrs` (instead of
 * handles): ranks emulated inside one process pass each other's device pointers.  At most 8 ranks. */
typedef struct { char internal[64]; } lcf_ipc_handle;
lcf_status lcf_sampler_mailbox_export(lcf_sampler* s, lcf_ipc_handle* out, void** local_ptr);
lcf_status lcf_sampler_mailbox_connect(lcf_sampler* s, int32_t n_ranks, int32_t rank, const lcf_ipc_handle* handles,
                                       void* const* local_ptrs);
/* The run of lcf_sampler_run_sharded over the mailboxes.  Every rank calls it with the same arguments, and only after
 * ALL ranks have returned from their previous run (barrier of the caller).  A rank whose peers' rows do not arrive
 * within 0.5 s returns LCF_ERR_STATE instead of waiting for ever. */
lcf_status lcf_sampler_run_peers(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                 const int32_t* perm, int32_t store_chain);
/* Enqueue only (lcf_sampler_wait completes it): lets one host thread drive several emulated ranks. */
lcf_status lcf_sampler_run_peers_async(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                       const int32_t* perm, int32_t store_chain);

/* Row boards: the sharded run in which nothing is replicated.  Rank r evaluates, accepts and commits the proposals
 * [r w, (r + 1) w) of every half-step with the one-workgroup-per-proposal kernel (k_solo) and stores each walker's new
 * row -- position, log-posterior, acceptance count, as {32 data bits, 32-bit half-step tag} words -- straight into
 * EVERY rank's board (uncached device memory, mapped through IPC: xGMI writes on a node); the serial head of a later
 * half-step polls its own board for exactly the versions of the two rows it needs.  No collective, no launch between
 * half-steps, no work about other ranks' walkers; every wait is bounded (0.5 s, then LCF_ERR_STATE).  When the run
 * ends, state, acceptance counts and (if stored) the chain are complete on every rank.  Same chain as every other
 * driver, bit for bit.  export / connect as for the mailboxes (local_ptrs: ranks emulated inside one process).
 * lcf_sampler_run_rows is collective in effect: same arguments on every rank, called after ALL ranks have returned
 * from the previous run, on samplers that have seen the same sequence of runs. */
lcf_status lcf_sampler_board_export(lcf_sampler* s, lcf_ipc_handle* out, void** local_ptr);
lcf_status lcf_sampler_board_connect(lcf_sampler* s, int32_t n_ranks, int32_t rank, const lcf_ipc_handle* handles,
                                     void* const* local_ptrs);
lcf_status lcf_sampler_run_rows(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                const int32_t* perm, int32_t store_chain);
lcf_status lcf_sampler_run_rows_async(lcf_sampler* s, int64_t first_step, int64_t n_steps, int32_t split_mode,
                                      const int32_t* perm, int32_t store_chain);

/* ---- per-epoch blackbody SED likelihood (bolometric.py:154-164: spectrum_mcmc's inner log_posterior) --------- */
/* For every epoch e, observations ep_off[e] .. ep_off[e+1]-1 (filter index, luminosity density y, uncertainty dy);
 * for every candidate (T [kK], R [1000 Rsun][, sigma]) of that epoch the Gaussian log-likelihood of the band-averaged
 * blackbody [f.synthesize(planck_fast, T, R) for f in filters].  precision 0 = float64 over the band tables sample by
 * sample, 1 = float32 over the band tables, 2 = float64 through the interpolants of ln S_f(ln T) where a candidate's
 * temperature is inside their proved range and over the band tables where it is not (0 when no interpolants were given). */
typedef struct lcf_sed lcf_sed;
/* ctab_*: optional Gauss-compressed companions of the band tables (all NULL = none), itab_*: optional interpolants of
 * ln S_f(ln T) (itab_coef NULL = none); both as in lcf_problem. */
lcf_status lcf_sed_create(int32_t n_filters, const int32_t* tab_off, const double* tab_a, const double* tab_w,
                          const int32_t* ctab_off, const double* ctab_a, const double* ctab_w,
                          const double* ctab_tmin, const double* itab_coef, const double* itab_tmin, int32_t itab_m,
                          double itab_u0, double itab_h, int32_t device, lcf_sed** out);
void lcf_sed_destroy(lcf_sed* s);
lcf_status lcf_sed_set_observations(lcf_sed* s, int64_t n_epochs, const int32_t* ep_off, const int32_t* filt_idx,
                                    const double* y, const double* dy);
/* cand[n_epochs][n_cand][n_par] (n_par = 2 or 3), out[n_epochs][n_cand]; kernel_ms (optional) receives the device
 * time of the kernel alone (HIP events on the engine's stream). */
lcf_status lcf_sed_log_likelihood(lcf_sed* s, int64_t n_cand, int32_t n_par, int32_t sigma_type, const double* cand,
                                  int32_t precision, int32_t use_compressed, double* out, double* kernel_ms);

/* ---- bolometric light curves (bolometric.py:483-534, 32-59, 422-453) ------------------------------------------ */
/* blackbody_lstsq for many epochs in one launch: for epoch e, points ep_off[e] .. ep_off[e+1]-1 (observed freq_eff
 * [THz], luminosity density lum [W/Hz]), the bounded, unweighted least-squares fit of planck_fast(freq (1+z), T, R,
 * cutoff_freq) from p0[e] = (T, R) within lo[e] <= (T, R) <= hi[e] (projected Levenberg-Marquardt, analytic Jacobian),
 * until no variable moves by more than xtol relative or max_iter iterations.  out[e][8] = T, R, cost = 1/2 sum r^2,
 * cov_TT, cov_TR, cov_RR (curve_fit's: pinv(J^T J) 2 cost / (m - 2), +inf when m <= 2), iterations, 0.
 * status[e]: 1 converged (step below xtol), 2 converged (projected gradient zero), 0 iteration cap, -1 no points or a
 * non-finite input or cost.  p0 outside [lo, hi] is LCF_ERR_INVALID_ARGUMENT. */
lcf_status lcf_bb_lstsq(int32_t device, int64_t n_epochs, const int32_t* ep_off, const double* freq, const double* lum,
                        const double* p0, const double* lo, const double* hi, double z, double cutoff_freq,
                        int32_t max_iter, double xtol, double* out, int32_t* status);
/* pseudo() and stefan_boltzmann() of n samples (T [kK], R [1000 Rsun]): L_pseudo[k] = 1e12 x the trapezoid (end
 * weights 1/2) of planck_fast((freq0 + j)(1+z), T, R, cutoff_freq) over j < n_grid, where the host passes
 * freq0 = I.freq_eff - I.dfreq/2 and n_grid = len(np.arange(freq0, U.freq_eff + U.dfreq/2)); L_bol[k] = 4 pi R^2
 * sigma_SB T^4 [W]. */
lcf_status lcf_bb_luminosity(int32_t device, int64_t n, const double* T, const double* R, double z, double freq0,
                             int32_t n_grid, double cutoff_freq, double* L_pseudo, double* L_bol);

/* ---- integrated autocorrelation time (emcee.autocorr.integrated_time, without its tol check) ------------------ */
/* Per parameter d: f[tau] = mean over walkers of the walker's autocorrelation at lag tau normalised by its lag 0,
 * taus = 2 cumsum(f) - 1, window[d] = argmin(k < c taus[k]) if any k satisfies it, else n_t - 1, and
 * tau[d] = taus[window[d]] (NaN with window n_t - 1 where a walker's series is constant).  Only the lags up to the
 * window are computed.  Host chain[n_t][n_w][n_d]; uploaded, processed and freed. */
lcf_status lcf_autocorr_time(int32_t device, const double* chain, int64_t n_t, int32_t n_w, int32_t n_d, double c,
                             double* tau, int64_t* window);
/* The same for the stored chains of n samplers (one device), read in place on the device: rows discard,
 * discard + thin, ... of each sampler's last stored run.  tau / window hold each sampler's n_dim entries one after
 * another.  LCF_ERR_STATE when a sampler has no stored chain; discard past the chain is LCF_ERR_INVALID_ARGUMENT. */
lcf_status lcf_samplers_autocorr_time(lcf_sampler** s, int32_t n, int64_t discard, int64_t thin, double c,
                                      double* tau, int64_t* window);

/* ---- posterior-predictive quantiles (what lightcurve_model_plot draws, fitting.py:337-360, over ALL samples) ---- */
/* `grid` is an evaluation engine built for the grid points (dummy photometry, no sigma, no priors; every (time,
 * filter) pair at most once).  For every point: the model values of all samples, NaNs dropped (n_valid of them
 * remain), sorted, interpolated linearly between the order statistics around h = (n_valid - 1) q / 100 -- NumPy's
 * nanpercentile, default method; NaN where n_valid = 0.  No value is stored per (sample, point): device memory beyond
 * the samples is at most workspace_bytes (LCF_ERR_INVALID_ARGUMENT, with the amount needed, if that is too little for
 * the samples' coefficients and one time of the grid) and the times are worked through in as many tiles as that takes.
 * Results do not depend on the tiling and are bitwise reproducible.
 * component: 0 = the model, 1 = the SiFTO term alone (companion-shocking models only): the template at the model's
 * stretch and offsets times the filter's factor, 0 outside the template (fitting.py:355-360).
 * q[n_q]: percentiles in [0, 100]; n_filters * n_q <= 512.
 * Quantiles of the model over n host samples P[n][ld] (the first n_par columns are used) on the points of `grid`: */
lcf_status lcf_predict_quantiles(lcf_engine* grid, const double* P, int64_t n, int32_t ld, int32_t component,
                                 const double* q, int32_t n_q, int64_t workspace_bytes,
                                 double* out /* [n_q][n_points] */, int64_t* n_valid /* [n_points] */);
/* The same over rows discard, discard + thin, ... of the sampler's last stored run, read in place (every walker of a
 * kept step is a sample, in the order of get_chain).  LCF_ERR_STATE without a stored chain, LCF_ERR_UNSUPPORTED when
 * sampler and grid engine are on different devices, LCF_ERR_INVALID_ARGUMENT for discard past the chain. */
lcf_status lcf_sampler_predict_quantiles(lcf_engine* grid, lcf_sampler* s, int64_t discard, int64_t thin,
                                         int32_t component, const double* q, int32_t n_q, int64_t workspace_bytes,
                                         double* out, int64_t* n_valid);

/* ---- colour bands and per-band peaks: the model's colours with their uncertainty, over ALL samples ---------------- */
/* `grid` is an evaluation engine on the dense grid, filter-major: point f * n_times + t is filter f of the engine at
 * the t-th of n_times distinct times (dummy photometry, no sigma, no priors; at most 16 filters).  Colour c is the pair
 * of engine filters a = pairs[2 c], b = pairs[2 c + 1] with the zero-point difference dzp[c] = m0_a - m0_b.  With
 * Y[f][t][s] the model value lcf_predict_quantiles ranks,
 *     C[c][t][s] = dzp[c] - 2.5 log10(Y[a][t][s] / Y[b][t][s])   if both values are finite and > 0, else NaN
 * (not exploded yet: Y == 0; NaN; a negative SiFTO tail), and out / n_valid are the percentiles and non-NaN counts of C
 * over the samples (definition, workspace, tiling and reproducibility as for lcf_predict_quantiles; n_c * n_q <= 512).
 * Every filter is evaluated once per (sample, time) and pass, whatever the number of colours it occurs in.
 * y_peak / peak_index (both or neither): per filter and sample the largest non-NaN Y over the times walked in ascending
 * order and the caller's index t of the first time it is attained (strict >; NaN and -1 when every value is NaN; 0 at
 * the earliest time for a sample that has not exploded anywhere).  The two arrays are results per sample and lie OUTSIDE
 * workspace_bytes: 12 n_filters n bytes of device memory while the call runs.
 * Every argument is checked before a device is asked for: a pair index outside the engine's filters is
 * LCF_ERR_INVALID_ARGUMENT; n_c * n_q > 512, more than 16 filters, and an engine of LCF_MODEL_CUSTOM or of a
 * central-engine model are LCF_ERR_UNSUPPORTED (the last two naming the route such an engine does take).
 * Over n host samples P[n][ld] (the first n_par columns are used): */
lcf_status lcf_predict_colors(lcf_engine* grid, const double* P, int64_t n, int32_t ld, int32_t n_c,
                              const int32_t* pairs /* [n_c][2] */, const double* dzp /* [n_c] */, const double* q,
                              int32_t n_q, int64_t workspace_bytes, double* out /* [n_q][n_c][n_times] */,
                              int64_t* n_valid /* [n_c][n_times] */, double* y_peak /* [n_filters][n] or NULL */,
                              int32_t* peak_index /* [n_filters][n] or NULL */);
/* The same over rows discard, discard + thin, ... of the sampler's last stored run, read in place; status codes as
 * for lcf_sampler_predict_quantiles. */
lcf_status lcf_sampler_predict_colors(lcf_engine* grid, lcf_sampler* s, int64_t discard, int64_t thin, int32_t n_c,
                                      const int32_t* pairs, const double* dzp, const double* q, int32_t n_q,
                                      int64_t workspace_bytes, double* out, int64_t* n_valid, double* y_peak,
                                      int32_t* peak_index);

/* ---- thermal bands and validity: T, R_bb, L_bol of the blackbody behind the light curves, over ALL samples -------- */
/* `grid` is an evaluation engine with one point per distinct time and any single filter (what temperature_radius is
 * evaluated on); the model is any but LCF_MODEL_BLACKBODY.  Per (sample, time): T [kK] and R_bb [1000 Rsun] as
 * lcf_temperature_radius returns them (for the companion-shocking models: of the shock component) and L_bol = 4 pi
 * sigma_SB R_bb^2 T^4 [W] of that pair.  Per time, over the samples: the percentiles q[n_q] of each of the three
 * (definition, workspace and reproducibility as for lcf_predict_quantiles; 3 * n_q <= 512), the number of non-NaN
 * values of each, the number of samples with T < T_floor (T is exactly 0 before a sample's explosion time: that is
 * cold), and the number with t_min(p) <= t <= t_max(p), the model's own validity window at opacity kappa = 1
 * (models.py:276-298, 414-430, 499-504, 634-657, 830-845; a NaN bound: not inside; ShockCooling2 has no lower bound).
 * All counts are exact integers.  Times are in the order the engine was given them.
 * Over n host samples P[n][ld] (the first n_par columns are used): */
lcf_status lcf_predict_thermal(lcf_engine* grid, const double* P, int64_t n, int32_t ld, const double* q, int32_t n_q,
                               double T_floor, int64_t workspace_bytes,
                               double* out /* [3][n_q][n_times]: T, R_bb, L_bol */,
                               int64_t* n_valid /* [3][n_times] */, int64_t* n_cold /* [n_times] */,
                               int64_t* n_inside /* [n_times] */);
/* The same over rows discard, discard + thin, ... of the sampler's last stored run, read in place; status codes as
 * for lcf_sampler_predict_quantiles. */
lcf_status lcf_sampler_predict_thermal(lcf_engine* grid, lcf_sampler* s, int64_t discard, int64_t thin, const double* q,
                                       int32_t n_q, double T_floor, int64_t workspace_bytes, double* out,
                                       int64_t* n_valid, int64_t* n_cold, int64_t* n_inside);

/* ---- corner histograms: what corner.corner counts for lightcurve_corner (fitting.py:241-253), over ALL samples ---- */
/* Two passes over the samples where they lie.  The range pass gives, per column, the minimum and the maximum of the
 * non-NaN values (NaN, NaN when there is none) and the number of NaNs.  The histogram pass counts v = x[d] - shift[d]
 * (one float64 subtraction) into `bins` bins per column whose bins + 1 edges the caller passes, ascending -- NumPy's
 * np.linspace(lo, hi, bins + 1) for its np.histogram / np.histogram2d: bin i holds edges[i] <= v < edges[i + 1], the
 * last bin also v == edges[bins]; a NaN, v < edges[0] or v > edges[bins] is in no bin (np.searchsorted(edges, v,
 * 'right') - 1 with the last edge folded in).  hist1d[d][i]: column d.  hist2d[p][i][j] for the pair p = a (a - 1) / 2
 * + b of columns b < a: the samples with column b in bin i AND column a in bin j -- H of np.histogram2d(x[:, b],
 * x[:, a]), the panel in row a, column b of the figure; a sample enters only with both coordinates in a bin.  All
 * counts are exact integers and do not depend on how the samples are split over workgroups.
 * 1 <= n_dim <= 16, 1 <= bins <= 128; hist2d may be NULL when n_dim == 1.
 * Over n host samples P[n][ld] (the first n_dim columns): */
lcf_status lcf_chain_range(int32_t device, const double* P, int64_t n, int32_t ld, int32_t n_dim,
                           double* lo /* [n_dim] */, double* hi /* [n_dim] */, int64_t* n_nan /* [n_dim] */);
lcf_status lcf_chain_hist(int32_t device, const double* P, int64_t n, int32_t ld, int32_t n_dim,
                          const double* shift /* [n_dim] */, const double* edges /* [n_dim][bins + 1] */, int32_t bins,
                          int64_t* hist1d /* [n_dim][bins] */, int64_t* hist2d /* [n_pairs][bins][bins] */);
/* The same over rows discard, discard + thin, ... of the last stored run of n_samplers samplers (one device), read in
 * place, in one sequence of launches; every walker of a kept step is a sample and every column of the chain is
 * counted.  Each sampler has its own n_dim, shift and edges; inputs and outputs of the samplers lie one after another
 * (lo / hi / n_nan / shift: n_dim entries each, edges: n_dim (bins + 1), hist1d: n_dim bins, hist2d: n_dim (n_dim -
 * 1) / 2 bins^2).  LCF_ERR_STATE when a sampler has no stored chain, LCF_ERR_INVALID_ARGUMENT for discard past the
 * chain, LCF_ERR_UNSUPPORTED when the samplers are on different devices. */
lcf_status lcf_samplers_chain_range(lcf_sampler** samplers, int32_t n_samplers, int64_t discard, int64_t thin,
                                    double* lo, double* hi, int64_t* n_nan);
lcf_status lcf_samplers_chain_hist(lcf_sampler** samplers, int32_t n_samplers, int64_t discard, int64_t thin,
                                   const double* shift, const double* edges, int32_t bins, int64_t* hist1d,
                                   int64_t* hist2d);

/* ---- chain history: the numbers of the chain plots of lightcurve_mcmc(show=True) (fitting.py:135-158) -------------- */
/* From a stored chain[n_t][n_w][n_dim] and its log-probabilities log_prob[n_t][n_w].  The kept steps are k = 0 ..
 * n_keep - 1 at stored step t_k = discard + k thin, n_keep = ceil((n_t - discard) / thin).
 * Ensemble bands: for every kept step and every column c -- c < n_dim a column of the chain, c == n_dim the
 * log-probability -- the values of the n_w walkers are ordered (-inf < ... < -0 < +0 < ... < +inf, infinities being
 * ordinary values; NaNs last, n_valid[k][c] values are none).  For each percentile q[i] in [0, 100]: h = (n_valid - 1)
 * (q[i] / 100), lo = floor(h), hi = min(lo + 1, n_valid - 1); stat_lo[i][k][c] and stat_hi[i][k][c] are the order
 * statistics of rank lo and hi, copies of input values.  The percentile is the caller's to interpolate, stat_lo +
 * (h - lo) (stat_hi - stat_lo) evaluated as NumPy evaluates it (np.nanpercentile, default method); the library does
 * not, because its arithmetic is contracted and would round differently.  n_valid == 0: both are NaN.  A NULL log_prob:
 * column n_dim has n_valid 0 and NaNs.
 * Moves: n_moved[k] is the number of walkers whose row at stored step t_k differs from their row at stored step t_k - 1
 * -- the step before in the STORED chain, not the kept step before -- two rows differing when the 64-bit pattern of
 * any column does (-0 and +0 differ; a NaN equals itself); -1 for t_k == 0, whose predecessor is not in the chain.  It
 * is the number of proposals accepted in that step.
 * Trace density: counts[d][i][j] is the number of (kept step k, walker) pairs with (k t_bins) / n_keep == i (integer
 * division) whose value in column d is in bin j of the v_bins bins between the ascending edges[d][0 .. v_bins]; bin
 * membership is that of lcf_chain_hist (edges[j] <= v < edges[j + 1], the last bin closed; a NaN and a value outside
 * are in no bin); no shift is applied.  Columns of the chain only.
 * All results are exact, bitwise reproducible and independent of how the work is split.
 * 1 <= n_dim <= 16, 1 <= n_q <= 16, 1 <= v_bins <= 256, 1 <= t_bins <= min(n_keep, 4096); n_w > 16384 is
 * LCF_ERR_UNSUPPORTED.  Over a host chain (uploaded whole, so that the first kept step has its predecessor, and freed): */
lcf_status lcf_chain_history(int32_t device, const double* chain, const double* log_prob /* or NULL */, int64_t n_t,
                             int32_t n_w, int32_t n_dim, int64_t discard, int64_t thin, const double* q, int32_t n_q,
                             double* stat_lo, double* stat_hi /* [n_q][n_keep][n_dim + 1] */,
                             int64_t* n_valid /* [n_keep][n_dim + 1] */, int64_t* n_moved /* [n_keep] */);
lcf_status lcf_chain_raster(int32_t device, const double* chain, int64_t n_t, int32_t n_w, int32_t n_dim,
                            int64_t discard, int64_t thin, int32_t t_bins,
                            const double* edges /* [n_dim][v_bins + 1] */, int32_t v_bins,
                            int64_t* counts /* [n_dim][t_bins][v_bins] */);
/* The same over the last stored run of n_samplers samplers (one device), chain and log-probabilities read in place, in
 * one sequence of launches.  Each sampler has its own n_dim, n_keep and edges; inputs and outputs of the samplers lie
 * one after another (stat_lo / stat_hi: n_q n_keep (n_dim + 1) entries each, n_valid: n_keep (n_dim + 1), n_moved:
 * n_keep, edges: n_dim (v_bins + 1), counts: n_dim t_bins v_bins).  Status codes as for lcf_samplers_chain_range. */
lcf_status lcf_samplers_chain_history(lcf_sampler** samplers, int32_t n_samplers, int64_t discard, int64_t thin,
                                      const double* q, int32_t n_q, double* stat_lo, double* stat_hi, int64_t* n_valid,
                                      int64_t* n_moved);
lcf_status lcf_samplers_chain_raster(lcf_sampler** samplers, int32_t n_samplers, int64_t discard, int64_t thin,
                                     int32_t t_bins, const double* edges, int32_t v_bins, int64_t* counts);

/* ---- parallel-tempered ensembles: degenerate posteriors and the log-evidence (emcee 2's PTSampler) ------------------ */
/* n_temps rungs k of inverse temperature betas[0] = 1 >= betas[1] >= ... >= betas[n_temps - 1] >= 0 (a ladder descends
 * strictly; between equal neighbours every swap is accepted, which the library allows and tests use), each an ensemble of
 * n_walkers walkers of its own; per walker the state keeps x, ln L(x) (likelihood only) and ln prior(x).  Rung k draws
 * from the sampler's generators (LCF_SPLIT_RANDOM colouring, z, partner, ln u) under seed + k 0x9E3779B97F4A7C15 (mod
 * 2^64), keyed by the absolute step.  Step s: for each half and all rungs at once, q = partner - (partner - x) z, ONE
 * likelihood call for the n_temps ceil(n_walkers / 2) proposals, accept iff ln prior(q) is finite, ln L(q) > -inf and
 * (n_dim - 1) ln z + betas[k] (ln L(q) - ln L(x)) + (ln prior(q) - ln prior(x)) > ln u (betas[k] = 0: no product is
 * formed); a NaN ln L(q) inside the prior ends the run with LCF_ERR_NAN_LOGPROB, outside it is ignored.  Then the pairs
 * (k, k + 1) with k = s (mod 2) swap slot by slot: ln u = log(u01(r0, r1)), (r0, r1, ., .) = Philox(counter (slot, s, 3,
 * k), key seed); accept iff (betas[k] - betas[k + 1]) (ln L[k + 1][i] - ln L[k][i]) > ln u; x, ln L and ln prior change
 * places, the move counts stay with the slot.
 * 1 <= n_temps <= 64 and 2 n_dim <= n_walkers <= 16384 (beyond: LCF_ERR_UNSUPPORTED).  The engine's priors decide what a
 * rung at beta = 0 samples: the caller makes sure they are proper. */
typedef struct lcf_tempered lcf_tempered;
lcf_status lcf_tempered_create(lcf_engine* e, int32_t n_temps, const double* betas, int32_t n_walkers, uint64_t seed,
                               double a, lcf_tempered** out);
void lcf_tempered_destroy(lcf_tempered* t);
/* coords[n_temps][n_walkers][n_dim] host.  A start row outside the prior is LCF_ERR_STATE, one whose likelihood is NaN
 * LCF_ERR_NAN_LOGPROB.  Clears the counts. */
lcf_status lcf_tempered_set_state(lcf_tempered* t, const double* coords);
/* coords[n_temps][n_walkers][n_dim], lnL / lnpr[n_temps][n_walkers] (any may be NULL) */
lcf_status lcf_tempered_get_state(lcf_tempered* t, double* coords, double* lnL, double* lnpr);
/* n_steps steps numbered from first_step.  store: 0 = nothing is stored (the stored chain stays), 1 = the run's steps
 * replace the stored chain, 2 = they are appended to it.  LCF_ERR_OUT_OF_MEMORY, before anything is allocated, when the
 * chain does not fit the device's free memory. */
lcf_status lcf_tempered_run(lcf_tempered* t, int64_t first_step, int64_t n_steps, int32_t store);
/* The stored chain: chain[n_stored][n_temps][n_walkers][n_dim], lnL[n_stored][n_temps][n_walkers] (either may be NULL). */
lcf_status lcf_tempered_get_chain(lcf_tempered* t, double* chain, double* lnL);
/* Since the last set_state: accepted moves per slot [n_temps][n_walkers], accepted and proposed swaps per pair (k, k + 1)
 * [n_temps - 1] (any may be NULL). */
lcf_status lcf_tempered_get_counts(lcf_tempered* t, int64_t* n_accepted, int64_t* swaps_accepted, int64_t* swaps_proposed);
/* out[k] = mean of ln L over the stored steps discard .. and all walkers of rung k, reduced on the device in a fixed
 * order (what thermodynamic integration needs of the chain). */
lcf_status lcf_tempered_mean_loglike(lcf_tempered* t, int64_t discard, double* out /* [n_temps] */);

/* An adaptive ladder (Vousden, Farr & Mandel 2016): lcf_tempered_run with the rungs moving on the device, in stream order,
 * until neighbouring pairs swap equally often.  Needs n_temps >= 3 and betas[n_temps - 1] == 0, finite lag > 0 and
 * time > 0 (otherwise LCF_ERR_INVALID_ARGUMENT, before any launch).  After the swaps of every odd step s, if every pair
 * was offered since the last adaptation (the window): A_k = accepted / offered swaps of pair k in the window,
 * kappa = lag / (t + lag) / time with t = t0 + (s - first_step) + 1, dT_k = (1 / beta_{k+1} - 1 / beta_k) exp(kappa (A_k -
 * A_{k+1})) for k = 0 .. n_temps - 3, then in this order T_0 = 1, T_{k+1} = T_k + dT_k, beta_{k+1} = 1 / T_{k+1}; the
 * window closes.  beta_0 = 1 and the last beta = 0 never move.  t0: the adapting steps this handle has made before (the
 * caller counts them).  An adapting run that follows an adapting run goes on in its window, so a run cut in two gives
 * the same ladders and chains; after lcf_tempered_run or lcf_tempered_set_state the window starts empty.  Gaps that round
 * away leave equal neighbours, which the driver takes. */
lcf_status lcf_tempered_run_adaptive(lcf_tempered* t, int64_t first_step, int64_t n_steps, int32_t store, double lag,
                                     double time, int64_t t0);
/* The ladder now: betas[n_temps]. */
lcf_status lcf_tempered_get_betas(lcf_tempered* t, double* betas);
/* betas[n_stored][n_temps]: the ladder every stored step was sampled under (before the adaptation that follows it). */
lcf_status lcf_tempered_get_beta_history(lcf_tempered* t, double* betas);
/* Stepping stones (Xie et al. 2011), per pair k and batch b of the stored steps discard + (b n) / n_batches .. (n the
 * steps kept): over ln L of rung k + 1, all walkers, max = the maximum m, sum = sum exp((beta_k - beta_{k+1}) (ln L - m))
 * (0 when m = -inf), count = the number of terms; each [n_temps - 1][n_batches], reduced on the device in a fixed order.
 * The ladder is the one step `discard` was sampled under.  1 <= n_batches <= n. */
lcf_status lcf_tempered_stepping_stones(lcf_tempered* t, int64_t discard, int32_t n_batches, double* max, double* sum,
                                        double* count);

/* Moves other than the stretch move (emcee's moves=): a step of a rung makes ONE kind of move in both of its half-steps.
 * With n_moves > 0, rung k at step s makes the first move m with um < cum_weights[m], um = u01(r0, r1) of Philox(counter
 * (0, s, 4, 0), key of rung k).  The colouring, the active walker of every slot and ln u stay the generators'; the new
 * numbers of walker w are P2 = Philox((w, s, half, 2)) and P3 = Philox((w, s, half, 3)) under the rung's key: ua =
 * u01(P2[0], P2[1]), ub = u01(P2[2], P2[3]), uc = u01(P3[0], P3[1]), ud = u01(P3[2], P3[3]).  c[0 .. n): the complementary
 * colour of the half-step, in the order of the step's permutation (what the stretch move's partner index points into).
 *   LCF_MOVE_STRETCH  as without moves.  params: unused.
 *   LCF_MOVE_DE       (ter Braak 2006; emcee's DEMove) params (sigma >= 0, gamma0 > 0).  j1 = min(int(ua n), n - 1),
 *                     j2 = min(int(ub (n - 1)), n - 2), j2 += (j2 >= j1); g = sqrt(-2 ln uc) cos(2 pi ud);
 *                     q = x + gamma0 (1 + sigma g) (c[j1] - c[j2]); log proposal factor 0.  Needs n >= 2.
 *   LCF_MOVE_SNOOKER  (ter Braak & Vrugt 2008; emcee's DESnookerMove) params (gammas > 0, unused).  j0, j1 as DE's j1, j2;
 *                     j2 = min(int(uc (n - 2)), n - 3), bumped past the smaller and then the larger of j0, j1.  z = c[j0],
 *                     d = x - z, u = d / |d|, q = x + u gammas (u.c[j1] - u.c[j2]); log proposal factor (n_dim - 1)
 *                     (ln |q - z| - ln |d|).  |d| = 0 or |q - z| = 0: never accepted.  Needs n >= 3.
 * The accept test takes the move's log proposal factor in place of (n_dim - 1) ln z; swaps, storing, adaptation and the
 * stepping stones are what they were.  cum_weights[n_moves]: ascending in (0, 1], the last exactly 1; params[n_moves][2].
 * n_moves = 0 (the pointers may be NULL) restores the default: the handle then launches what it launched before moves
 * existed.  At most LCF_MAX_MOVES entries.  Callable before the first run and between runs: waits for the engine's stream
 * and changes neither state nor counts.  LCF_ERR_INVALID_ARGUMENT (with the reason in lcf_last_error) for null pointers,
 * too many entries, unknown kinds, bad weights or parameters, and ensembles too small for a listed move (n is at least
 * n_walkers - ceil(n_walkers / 2)). */
#define LCF_MOVE_STRETCH 0
#define LCF_MOVE_DE 1
#define LCF_MOVE_SNOOKER 2
#define LCF_MAX_MOVES 8
lcf_status lcf_tempered_set_moves(lcf_tempered* t, int32_t n_moves, const int32_t* kinds, const double* cum_weights,
                                  const double* params /* [n_moves][2] */);
/* kinds[n_stored][n_temps]: the kind of move every rung made in every stored step (LCF_MOVE_STRETCH without moves). */
lcf_status lcf_tempered_get_move_history(lcf_tempered* t, int32_t* kinds);

/* ---- custom models: a user-written photosphere T(t), R(t), compiled at run time for the GPU ----------------------- */
/* What the reference's `Model` subclasses are to lightcurve_mcmc (models.py: temperature_radius, then
 * blackbody_to_filters), for the models the library has no kernel of its own for.  `source` is HIP device code that
 * defines, at global scope, the __device__ function lcf_user_state, returning void, of exactly the parameters
 *     (double t_in, const double* p, const double* consts, double z, double& T_kK, double& R_1000Rsun)
 * t_in: the observation time as the engine was given it (the function subtracts its explosion time and applies 1 + z as
 * its model requires); p: the n_par model parameters of the row (no fitted sigma); consts: lcf_problem.consts, all 12;
 * z: the engine's redshift for custom models (below).  Units are those of lcf_temperature_radius and
 * lcf_blackbody_to_filters.  Everything in csrc/lcf_device.h is visible, so lcf::pw -- the reference's power: base > 0 ?
 * base ** e : 0 -- makes "zero before the explosion" one call.  The model light curve is lcf_blackbody_to_filters of the
 * state at every point: T <= 0 or T >= 1e15 kK gives 0; a NaN T or R gives a NaN likelihood (LCF_ERR_NAN_LOGPROB at the
 * end of a run when inside the prior's support).  The function must return, and write nowhere but its two outputs.
 *
 * lcf_custom_compile: the program text is csrc/lcf_device.h, `#line 1 "user_model"`, the source, then the library's
 * kernels (csrc/lcf_custom_kernel.h, behind the key encoding of csrc/lcf_keys.h), compiled by hiprtc with the library's own code-generation flags for `arch`
 * ("gfx950"; NULL or "": the base name of the architecture of `device` -- with a name no device is needed).  hiprtc is
 * bound at run time: LCF_HIPRTC_LIB, <ROCM_PATH | HIP_PATH | /opt/rocm>/lib/libhiprtc.so, the directory the process's HIP
 * runtime was loaded from (PyTorch's lib), the loader's path; LCF_ERR_UNSUPPORTED with the paths tried when none loads.
 * A source that does not compile is LCF_ERR_INVALID_ARGUMENT, lcf_last_error carrying the compiler's log, in which the
 * source's lines are user_model:<line>.  Programs are cached per process by (source, arch): compiling the same pair
 * again returns the same handle.  The cache owns the programs; lcf_custom_destroy is the call that ends a caller's use
 * of a handle and frees nothing.
 * lcf_custom_log: the compiler's log of a successful compile (warnings; "" if none).
 * lcf_custom_code: the code object (*n_bytes long; n_bytes may be NULL), owned by the program. */
typedef struct lcf_custom lcf_custom;
lcf_status lcf_custom_compile(const char* source, const char* arch, int32_t device, lcf_custom** out);
const char* lcf_custom_log(const lcf_custom* c);
const void* lcf_custom_code(const lcf_custom* c, int64_t* n_bytes);
void lcf_custom_destroy(lcf_custom* c);
/* Attach a program to an engine created with LCF_MODEL_CUSTOM (any n_par with n_par + use_sigma <= 16; consts, band
 * tables, priors and sigma mode as for every model).  The program must have been compiled for the engine's device
 * architecture (LCF_ERR_INVALID_ARGUMENT otherwise); its module is loaded once per device.  The engine then serves
 * lcf_log_likelihood / lcf_log_posterior and their _dev forms, lcf_model_evaluate, lcf_temperature_radius (T and R as
 * the state function returned them) and, through lcf_log_likelihood_dev, lcf_tempered_*: one workgroup per (row, part of
 * the light curve), one lane per data point, the band sum chosen per point as lcf_blackbody_to_filters chooses it, sums
 * in a fixed order -- a row's value does not depend on the rows evaluated with it.  It also serves lcf_predict_custom
 * (below: the bands of the light curves, T, R and L over a whole chain).  Before a program is attached these calls
 * return LCF_ERR_STATE.  What is compiled per model -- lcf_sampler_create and with it every lcf_sampler_* and population
 * run, lcf_predict_quantiles, lcf_predict_thermal, lcf_predict_luminosity, lcf_sampler_predict_*,
 * lcf_profile_loglike_kernel -- returns LCF_ERR_UNSUPPORTED for such an engine, naming this route, and launches
 * nothing. */
lcf_status lcf_engine_set_custom(lcf_engine* e, lcf_custom* c);
/* The z handed to the state function (0 until set): the band tables carry 1 + z already, as for every model; the time
 * axis is the state function's own business. */
lcf_status lcf_engine_set_custom_redshift(lcf_engine* e, double z);

/* ---- central-engine models: a bolometric light curve L(t) [W] through Arnett's diffusion integral ----------------- */
/* LCF_MODEL_ARNETT and LCF_MODEL_MAGNETAR fit what calculate_bolometric produces: one luminosity per epoch, no filters.
 * The problem has n_filters = 0, filt_idx and all table pointers NULL, t = the epochs (MJD), y / dy = the bolometric
 * luminosity and its uncertainty in W; consts[0] = redshift z, consts[1] != 0 switches gamma-ray leakage on.
 * Parameters, in order (then sigma with use_sigma):
 *   ARNETT:    M_Ni [Msun], tau_m [d], (t_gamma [d] with leakage,) t_0 [d]
 *   MAGNETAR:  E_p [1e51 erg], t_p [d], tau_m [d], (t_gamma [d] with leakage,) t_0 [d]
 * With t = (MJD - t_0) / (1 + z): L = 0 for t <= 0, else
 *   L(t) = leak(t) int_0^t P(s) (2 s / tau_m^2) exp(-(t - s)(t + s) / tau_m^2) ds,
 *   leak = 1, or 1 - exp(-(t_gamma / t)^2) with leakage,
 *   ARNETT:    P(s) = M_Ni Msun [(e_Ni - e_Co) exp(-s / 8.8 d) + e_Co exp(-s / 111.3 d)] 1e-7 W, e_Ni = 3.9e10 and
 *              e_Co = 6.78e9 erg / s / g, Msun = 1.988409870698051e33 g
 *   MAGNETAR:  P(s) = E_p 1e51 / (t_p 86400) / (1 + s / t_p)^2 1e-7 W.
 * The integral is ONE fixed quadrature, part of the model's definition: the range is cut to [s_lo, t] with
 * s_lo = sqrt(max(0, t^2 - 40 tau_m^2)) (what is dropped is below e^-40 of the integrand's peak), split at
 * s_lo + (t - s_lo) / 8, and each piece takes 32 Gauss-Legendre nodes -- 64 nodes, the lanes of one wavefront.  Within
 * 1e-6 of the exact integral (measured: 4e-12) for 2 <= tau_m <= 60 d, 0.01 <= t <= 400 d, 1 <= t_p <= 100 d.
 * A non-finite parameter, tau_m <= 0, t_p <= 0 or t_gamma <= 0 gives NaN at every epoch.
 * Such an engine serves lcf_log_likelihood / lcf_log_posterior and their _dev forms, lcf_model_evaluate (L per epoch, in
 * the caller's order), through lcf_log_likelihood_dev, lcf_tempered_*, and lcf_predict_luminosity (below: the bands
 * and peaks of L(t) over a whole chain); a row's value does not depend on the rows evaluated with it.  What is compiled
 * per photometric model -- lcf_sampler_create and with it every lcf_sampler_* and population run, lcf_predict_quantiles,
 * lcf_predict_thermal, lcf_sampler_predict_*, lcf_temperature_radius, lcf_profile_loglike_kernel -- returns
 * LCF_ERR_UNSUPPORTED, naming this route, and launches nothing; lcf_blackbody_to_filters has no filter to index. */

/* ---- luminosity bands and peaks: L(t) of a central-engine model over ALL samples ---------------------------------- */
/* `grid` is a central-engine engine whose epochs are the grid times (dummy y / dy, no sigma, no priors).  Per (sample,
 * time): L [W], bit for bit what lcf_model_evaluate returns.  Per time, over the n host samples P[n][ld] (ld >= n_par;
 * the first n_par columns are used): the percentiles q[n_q] of L (NaNs dropped; NumPy's nanpercentile, default method;
 * NaN where no sample has a value; 1 <= n_q <= 512), n_valid = the samples whose L is not NaN, and n_dark = those
 * whose L is exactly +0: the sample has not exploded yet at that time.  All three in the order of the engine's epochs.
 * Per sample, when L_peak and i_peak are given (both or neither): L_peak = its largest non-NaN L over the epochs and
 * i_peak = the LOWEST epoch index at which it is attained; NaN and -1 for a sample that is NaN at every epoch.
 * Every (sample, time) pair is evaluated ONCE -- a value is a 64-node quadrature -- and kept as an 8-byte key while the
 * percentiles of its time are searched: device memory beyond the samples is at most workspace_bytes, the times being
 * worked through in tiles of as many times as fit, 8 n bytes each besides the searches' own (LCF_ERR_INVALID_ARGUMENT,
 * with the amount needed, if not even one time fits).  Results, the peaks included, do not depend on the tiling and
 * are bitwise reproducible.  An engine of another model: LCF_ERR_UNSUPPORTED, naming lcf_predict_quantiles. */
lcf_status lcf_predict_luminosity(lcf_engine* grid, const double* P, int64_t n, int32_t ld, const double* q, int32_t n_q,
                                  int64_t workspace_bytes, double* out /* [n_q][n_times] */,
                                  int64_t* n_valid /* [n_times] */, int64_t* n_dark /* [n_times] */,
                                  double* L_peak /* [n] or NULL */, int32_t* i_peak /* [n] or NULL */);

/* ---- bands of a custom model: its light curves, T, R and L over ALL samples ---------------------------------------- */
/* `grid` is an engine of LCF_MODEL_CUSTOM with a program attached (LCF_ERR_STATE without one) that holds the dense
 * filters x distinct-times grid, every (time, filter) pair once (dummy y / dy, no sigma, no priors;
 * LCF_ERR_INVALID_ARGUMENT for a pair held twice or missing).  Per (sample, time) the state function is called ONCE, and
 * its T [kK] and R [1000 Rsun] give n_filters + 3 series: the band luminosity of every filter -- lcf_model_evaluate's,
 * except that between the two forms of the band sum every sample chooses for itself (the main form where
 * a_max / T < 170, else the safe one: the same bits wherever a whole wavefront of lcf_model_evaluate takes the main
 * form) --, then T, R and L = 4 pi sigma_SB R^2 T^4 [W] of that pair.  A sample's
 * values do not depend on the samples evaluated with it.
 * Per (series, time), over the n host samples P[n][ld] (ld >= n_par; the first n_par columns are used): the percentiles
 * q[n_q] (NaNs dropped; NumPy's nanpercentile, default method; NaN where no sample has a value; 1 <= n_q <= 512) and
 * n_valid = the samples whose value is not NaN; per (filter, time) n_dark = the samples whose band luminosity is exactly
 * +0 (T <= 0: not exploded yet); per time, when n_cold is given and T_floor >= 0, n_cold = the samples with
 * T < T_floor (a NaN T is not cold, an exact 0 is; T_floor < 0 or NaN: nothing is counted and n_cold is zeroed).
 * Series in the order of the engine's filters, then T, R, L; times in ascending order.
 * Every value is kept as an 8-byte key while the percentiles of its time are searched: device memory beyond the
 * samples is at most workspace_bytes, the times being worked through in tiles of as many times as fit,
 * 8 n (n_filters + 3) bytes each besides the searches' own (LCF_ERR_INVALID_ARGUMENT, with the amount needed, if not even
 * one time fits).  Results do not depend on the tiling and are bitwise reproducible.  An engine of another model:
 * LCF_ERR_UNSUPPORTED, naming lcf_predict_quantiles / lcf_predict_luminosity. */
lcf_status lcf_predict_custom(lcf_engine* grid, const double* P, int64_t n, int32_t ld, const double* q, int32_t n_q,
                              double T_floor /* < 0 or NaN: no count */, int64_t workspace_bytes,
                              double* out /* [n_q][n_filters + 3][n_times] */,
                              int64_t* n_valid /* [n_filters + 3][n_times] */,
                              int64_t* n_dark /* [n_filters][n_times]: model value exactly +0 */,
                              int64_t* n_cold /* [n_times] or NULL */);

/* ---- upper limits: non-detections as censored terms of the likelihood ---------------------------------------------- */
/* By default a non-detection is what the reference makes of it: a row with y = 0 and dy = limit / nondetSigmas in the
 * Gaussian sum.  With limits attached, the engine `e` holds the DETECTIONS only and its log-likelihood gains, per limit
 * j, the probability that the flux was below the limit:
 *   ln L(p) = [the Gaussian log-likelihood of e's points] + sum_j ln Phi(z_j),   z_j = (L_lim[j] - m_j(p)) / sigma_j(p),
 * m_j(p) = the model at the limit's time and filter, bit for bit what lcf_model_evaluate(at, ...) returns;
 * sigma_j = dy[j] without use_sigma, else sqrt(dy[j]^2 + (s u_j)^2) with s the row's last column and u_j = dy[j]
 * (LCF_SIGMA_RELATIVE) or e's own median dy (LCF_SIGMA_ABSOLUTE); z is one subtraction and one division.
 * ln Phi(z) = log(erfcx(-z / sqrt 2) / 2) - z^2 / 2 for z <= 0 and log1p(-erfc(z / sqrt 2) / 2) for z > 0: accurate
 * in both tails (ln Phi(+inf) = 0, ln Phi(-inf) = -inf, -inf once z^2 overflows, NaN for a NaN model value).  The terms
 * are added in a fixed order: a row's value does not depend on the rows evaluated with it.  The sum belongs to the
 * likelihood: lcf_log_likelihood, lcf_log_posterior, their _dev forms and, through lcf_log_likelihood_dev,
 * lcf_tempered_* include it (a rung multiplies it by its beta); a row the prior excludes stays -inf.
 * Attach upper limits to a photometric engine: `at` is an engine of the same model, constants, n_par, use_sigma and
 * device on the limits' (t, filter) in the caller's order (its y, dy are not read); L_lim[n_lim], dy[n_lim] finite,
 * dy > 0, n_lim <= 2^20.  at = NULL or n_lim = 0 detaches.  The caller keeps `at` alive as long as `e` uses it, and
 * hands it to one engine only (its workspace holds the rows' coefficients between the launches).
 * What computes the likelihood inside kernels of its own would drop the limits silently and therefore returns
 * LCF_ERR_UNSUPPORTED for an engine with limits attached, naming the lcf_tempered_* route: lcf_sampler_create (and with
 * it every lcf_sampler_* and population run) and lcf_profile_loglike_kernel; so does attaching limits to an engine that
 * a live lcf_sampler uses, and to a central-engine model (a bolometric table has no non-detections).  Engines that do
 * not match, non-finite values and dy <= 0: LCF_ERR_INVALID_ARGUMENT. */
lcf_status lcf_engine_set_limits(lcf_engine* e, lcf_engine* at, int64_t n_lim, const double* L_lim, const double* dy);
/* out[n][n_lim]: ln Phi term of every (row, limit); rows as lcf_log_likelihood takes them.  LCF_ERR_STATE for an engine
 * without limits. */
lcf_status lcf_limit_terms(lcf_engine* e, int64_t n, const double* P, double* out);

/* ---- second component: a stretched template added to the model ----------------------------------------------------- */
/* A double-peaked light curve: the engine's model (a shock-cooling model, or a custom model) plus a second peak given as
 * a template per filter, which the fit may shift, stretch and scale -- what the companion-shocking models do with the
 * SiFTO template, for any photometric engine and any template.  With a template attached the model at point j, of
 * filter f, is
 *   m_j(p) = base_j(p[0 .. n_par)) + r_f S_f((t_j - t_max - dt_f) / s),
 * base_j bit for bit what lcf_model_evaluate of the engine without the template returns; S_f the piecewise cubic
 *   S_f(x) = ((c0 dx + c1) dx + c2) dx + c3,  dx = x - knots[i],  c = coef[f][i],  knots[i] <= x (< knots[i + 1]),
 * 0 for x outside [knots[0], knots[n_knots - 1]] and for a NaN x; the argument is evaluated as (t_j - t_max - dt_f) *
 * (1 / s), as the companion-shocking kernels do: s = 0 and a NaN s give an infinite or NaN argument, hence no template;
 * s < 0 mirrors the template; t is the observed time (not redshifted, as in the reference).  The likelihood is that of
 * every model (models.py:116-136) on m_j, with the engine's sigma mode, added in a fixed order: a row's value does
 * not depend on the rows evaluated with it.  A NaN model value gives NaN; a row the prior excludes stays -inf.
 * The rows gain n_extra >= 2 columns behind the model's own n_par, in front of sigma: lcf_engine_ndim then returns
 * n_par + n_extra + use_sigma (at most 16).  tmax_par and s_par are the columns of t_max and s; filt_factor_par[n_filters]
 * and filt_offset_par[n_filters] the columns of each filter's r_f and dt_f, -1 where the filter has none (r = 1,
 * dt = 0); all of them among the extra columns.  knots[n_knots] finite and strictly increasing, 4 <= n_knots <= 65536;
 * coef[n_filters][n_knots - 1][4], highest power first, finite.  priors: NULL, or the priors of ALL columns of the grown
 * row (they replace the ones the engine was created with).  knots = NULL or n_knots = 0 detaches: the engine is as it
 * was created, its own priors included.  Attach before anything that sizes itself by lcf_engine_ndim is created on the
 * engine (lcf_tempered_create).
 * Served: lcf_log_likelihood, lcf_log_posterior, their _dev forms (k_prepare, the engine's own model values into scratch
 * -- at most 256 MiB per pass, rows in chunks -- and one kernel more) and through them lcf_tempered_*; lcf_model_evaluate
 * (the sum), lcf_temperature_radius (the base model's) and lcf_template_evaluate.  What computes the likelihood inside
 * kernels of its own would drop the template silently and therefore returns LCF_ERR_UNSUPPORTED for such an engine,
 * naming the lcf_tempered_* route: lcf_sampler_create (and with it every lcf_sampler_* and population run),
 * lcf_profile_loglike_kernel and lcf_engine_set_limits (limits together with a template are out of scope); so does
 * attaching a template to an engine that a live lcf_sampler uses, that has limits attached, to a central-engine model (no
 * filters) and to a companion-shocking model (it has its template).  Everything else that does not fit:
 * LCF_ERR_INVALID_ARGUMENT. */
lcf_status lcf_engine_set_template(lcf_engine* e, int32_t n_knots, const double* knots, const double* coef,
                                   const int32_t* filt_factor_par, const int32_t* filt_offset_par, int32_t tmax_par,
                                   int32_t s_par, int32_t n_extra, const lcf_prior* priors);
enum { LCF_TEMPLATE_TOTAL = 1, LCF_TEMPLATE_BASE = 2, LCF_TEMPLATE_TEMPLATE = 3 };
/* out[n][n_points], the caller's order of the points: the model (LCF_TEMPLATE_TOTAL), the base model alone (_BASE) or the
 * template term alone (_TEMPLATE) of rows as lcf_log_likelihood takes them.  LCF_ERR_STATE for an engine without a
 * template. */
lcf_status lcf_template_evaluate(lcf_engine* e, int64_t n, const double* P, int32_t component, double* out);

/* ---- bands and features of a template fit: both components and their sum, over ALL samples ------------------------ */
/* `grid` is an evaluation engine with a second component attached, on the dense grid, filter-major: point f * n_times + t
 * is filter f of the engine at the t-th of n_times distinct times (dummy photometry, no sigma, no priors; at most 16
 * filters; the model one of the built-in shock-cooling models).  Per sample s (a row of n_par + n_extra columns, as
 * lcf_log_likelihood takes it), filter f and time t, defined exactly as lcf_template_evaluate defines them:
 *     B  = the base model's value (what lcf_predict_quantiles ranks for the engine without the template),
 *     Tm = r_f S_f((t - t_max - dt_f) * (1 / s)),    Y = B + Tm.
 * components: a non-empty sum of the LCF_TEMPLATE_MASK_* values; the n_comp components asked for come out in the order
 * total (Y), base (B), template (Tm).  out / n_valid are the percentiles q[n_q] and the non-NaN counts of each over the
 * samples (definition, workspace, tiling and reproducibility as for lcf_predict_quantiles; n_comp * n_filters * n_q <=
 * 512), n_dark the samples whose B is exactly +0.0: the shock has not started.  Nothing is stored per (sample, time).
 * Every argument is checked before a device is asked for: LCF_ERR_STATE for an engine without a template,
 * LCF_ERR_UNSUPPORTED for an engine of LCF_MODEL_CUSTOM or of a central-engine model (naming the route such an engine
 * does take), for more than 16 filters and for more than 512 searches; everything else LCF_ERR_INVALID_ARGUMENT. */
enum { LCF_TEMPLATE_MASK_TOTAL = 1, LCF_TEMPLATE_MASK_BASE = 2, LCF_TEMPLATE_MASK_TEMPLATE = 4 };
lcf_status lcf_predict_template(lcf_engine* grid, const double* P, int64_t n, int32_t ld, int32_t components,
                                const double* q, int32_t n_q, int64_t workspace_bytes,
                                double* out /* [n_q][n_comp][n_points] */, int64_t* n_valid /* [n_comp][n_points] */,
                                int64_t* n_dark /* [n_points] */);
/* Per sample and filter of the same grid, over the times walked in ascending order; the first occurrence always wins,
 * comparisons are on values and a NaN never wins one.  indices[0], [1]: where the largest non-NaN B and the largest
 * non-NaN Tm are (-1: none); [2]: the first time with Tm > B (-1: none); [3]: where the smallest non-NaN Y over the
 * times from indices[0] to indices[1] inclusive is, defined only when 0 <= indices[0] < indices[1] in the walk (else -1).
 * values[0], [1], [2]: B, Tm and Y there, NaN where the index is -1.  Indices are the caller's t.  One launch over all
 * samples, (64 + 40 n_filters) n bytes of device memory beyond the samples; checks and status codes as above. */
lcf_status lcf_template_features(lcf_engine* grid, const double* P, int64_t n, int32_t ld,
                                 double* values /* [3][n_filters][n] */, int32_t* indices /* [4][n_filters][n] */);

#ifdef __cplusplus
}
#endif
#endif /* LCF_H */
