#!/usr/bin/env python3
"""Cost of a parallel-tempered fit on the GPU: time per step, and where the device time goes.

A configs[1]-shaped fit (ShockCooling on the config2 light curve, 1024 walkers) with a ladder of K = 8 rungs
(``default_betas(5, 8, Tmax=inf)``: the last rung samples the prior): ``--warmup`` unstored steps, then ``--steps``
stored steps, timed by a host clock around ``run_mcmc`` (which returns when the device has finished).  Reported: ms
per step and walker-steps/s over all rungs.  For orientation, K times what one step of ``EnsembleSampler`` costs at
the same walker count on its per-launch path (proposal and likelihood launches per half-step, ``'phases'``) -- what K
separate ensembles would cost launch by launch -- and on its resident path.

The split of the device time between the new kernels (``k_t_*``) and the existing likelihood kernels comes from a
separate ``rocprofv3 --kernel-trace --stats`` run of this script (nothing else collected); ``--kernel-stats CSV``
reads that run's kernel statistics and adds the split to the report.

``--adapt`` measures the adaptive ladder and the stepping stones instead (default ``--json
profiles/tempered_adaptive.json``): the same configuration frozen and adapting, interleaved ``--repeats`` times; what
``log_evidence(method='stepping_stone')`` costs on the stored chain (one ``k_t_stone`` launch and its copies, host
clock); and, at 8 and 16 rungs, the swap fractions and the log-evidence by both methods on the fixed ladder and on the
ladder adapted during ``--burn`` steps.

Usage:  python tools/tempered_timing.py [--steps 300] [--json profiles/tempered_timing.json] [--kernel-stats CSV]
        python tools/tempered_timing.py --adapt [--repeats 5] [--burn 1000]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.sampler import EnsembleSampler, TemperedSampler, default_betas  # noqa: E402

PRIORS = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.5)]
LO, HI = np.array([1., 0.3, 2., 1.5, 0.]), np.array([1.5, 0.7, 4., 2.5, 0.2])
LIKELIHOOD_KERNELS = ('k_prepare', 'k_points', 'k_finalize', 'k_thermal')
GENERATORS = ('k_make_perm', 'k_draws')


def lc_case():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'config2.npz'))
    return {'MJD': g['cfg2__t'], 'filter': [str(n) for n in g['cfg2__names']], 'lum': g['cfg2__y'], 'dlum': g['cfg2__dy']}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def kernel_split(path):
    """Device time by group from the kernel statistics of a rocprofv3 run: {'tempered_ns', 'likelihood_ns', ...}."""
    groups = {'tempered_ns': 0, 'likelihood_ns': 0, 'generators_ns': 0, 'other_ns': 0}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name, ns = row['Name'], int(float(row['TotalDurationNs']))
            if '::k_t_' in name:
                groups['tempered_ns'] += ns
            elif any(f'::{k}' in name for k in LIKELIHOOD_KERNELS):
                groups['likelihood_ns'] += ns
            elif any(f'::{k}' in name for k in GENERATORS):
                groups['generators_ns'] += ns
            else:
                groups['other_ns'] += ns
    total = sum(groups.values())
    groups['tempered_share'] = groups['tempered_ns'] / total if total else None
    groups['likelihood_share'] = groups['likelihood_ns'] / total if total else None
    return groups


def run(walkers, ntemps, steps, warmup, compare=True):
    lc, model = lc_case(), M.ShockCooling(redshift=0.)
    eng = model.engine_for(lc, priors=PRIORS)
    rng = np.random.default_rng(1)
    betas = default_betas(eng.ndim, ntemps, Tmax=np.inf)
    s = TemperedSampler(walkers, eng.ndim, eng, betas=betas, seed=1)
    s.run_mcmc(LO + (HI - LO) * rng.random((ntemps, walkers, eng.ndim)), warmup, store=False)
    sec = timed(lambda: s.run_mcmc(None, steps))
    res = {'walkers': walkers, 'ntemps': ntemps, 'betas': [float(b) for b in betas], 'steps': steps, 'warmup': warmup,
           'n_points': int(eng.npoints), 'proposals_per_likelihood_launch': ntemps * ((walkers + 1) // 2),
           'launches_per_step': 2 * (1 + 3 + 1) + 1,
           'ms_per_step': 1e3 * sec / steps, 'walker_steps_per_s': ntemps * walkers * steps / sec,
           'acceptance_per_rung': [float(a) for a in s.acceptance_fraction.mean(axis=1)],
           'swap_acceptance': [float(a) for a in s.swap_acceptance_fraction],
           'mean_log_like': [float(m) for m in s.mean_log_like(discard=steps // 2)]}
    lnZ, dlnZ = s.log_evidence(discard=steps // 2)
    res['log_evidence'] = [lnZ, dlnZ]
    if compare:
        x0 = LO + (HI - LO) * rng.random((walkers, eng.ndim))
        for kernel, key in (('phases', 'ensemble_phases_ms_per_step'), ('auto', 'ensemble_resident_ms_per_step')):
            e = EnsembleSampler(walkers, eng.ndim, eng, seed=1)
            e._native.set_half_step_kernel(kernel)
            e.run_mcmc(x0, warmup, store=False)
            res[key] = 1e3 * timed(lambda: e.run_mcmc(None, steps)) / steps
        res['K_x_ensemble_phases_ms_per_step'] = ntemps * res['ensemble_phases_ms_per_step']
        res['K_x_ensemble_resident_ms_per_step'] = ntemps * res['ensemble_resident_ms_per_step']
    return res


def evidence_case(eng, walkers, ntemps, burn, steps, adapt, lag, time_):
    """Burn in (adapting or not), store ``steps`` frozen steps: the ladder, swap fractions and both log-evidences."""
    rng = np.random.default_rng(1)
    start = default_betas(eng.ndim, ntemps, Tmax=np.inf)
    s = TemperedSampler(walkers, eng.ndim, eng, betas=start, seed=1, adaptation_lag=lag, adaptation_time=time_)
    s.run_mcmc(LO + (HI - LO) * rng.random((ntemps, walkers, eng.ndim)), burn, store=False, adapt=adapt)
    burn_swaps = s.swap_acceptance_fraction
    s.reset()
    s.run_mcmc(None, steps)
    ti, ss = s.log_evidence(), s.log_evidence(method='stepping_stone')
    res = {'ntemps': ntemps, 'adapted': bool(adapt), 'betas': [float(b) for b in s.betas],
           'swap_acceptance_burn_in': [float(a) for a in burn_swaps],
           'swap_acceptance_stored': [float(a) for a in s.swap_acceptance_fraction],
           'mean_log_like': [float(m) for m in s.mean_log_like()],
           'lnZ_thermodynamic': list(ti), 'lnZ_stepping_stone': list(ss)}
    s.close()
    return res


def run_adaptive(walkers, ntemps, steps, warmup, repeats, burn, lag, time_):
    lc, model = lc_case(), M.ShockCooling(redshift=0.)
    eng = model.engine_for(lc, priors=PRIORS)
    rng = np.random.default_rng(1)
    betas = default_betas(eng.ndim, ntemps, Tmax=np.inf)
    x0 = LO + (HI - LO) * rng.random((ntemps, walkers, eng.ndim))
    samplers = {}
    for mode in ('frozen', 'adapting'):
        s = TemperedSampler(walkers, eng.ndim, eng, betas=betas, seed=1, adaptation_lag=lag, adaptation_time=time_)
        s.run_mcmc(x0, warmup, store=False, adapt=mode == 'adapting')
        samplers[mode] = s
    ms = {'frozen': [], 'adapting': []}
    for _ in range(repeats):          # interleaved: both modes see the same drift of the machine
        for mode, s in samplers.items():
            s.reset()
            ms[mode].append(1e3 * timed(lambda: s.run_mcmc(None, steps, adapt=mode == 'adapting')) / steps)
    res = {'walkers': walkers, 'ntemps': ntemps, 'steps': steps, 'warmup': warmup, 'repeats': repeats,
           'n_points': int(eng.npoints), 'adaptation_lag': lag, 'adaptation_time': time_,
           'launches_per_step': {'frozen': 11, 'adapting': 11.5},
           'ms_per_step': {m: {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'runs': v}
                           for m, v in ms.items()}}
    f = samplers['frozen']
    f.log_evidence(method='stepping_stone')           # (allocates the partials once)
    stone = [1e3 * timed(lambda: f.log_evidence(method='stepping_stone')) for _ in range(repeats)]
    mean = [1e3 * timed(lambda: f.log_evidence()) for _ in range(repeats)]
    res['log_evidence_ms'] = {'stored_steps': steps, 'batches': 8, 'stepping_stone': float(np.median(stone)),
                              'thermodynamic': float(np.median(mean))}
    for s in samplers.values():
        s.close()
    res['evidence'] = [evidence_case(eng, walkers, k, burn, steps, adapt, lag, time_)
                       for k in (8, 16) for adapt in (False, True)]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--adapt', action='store_true', help='measure the adaptive ladder and the stepping stones')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--burn', type=int, default=1000, help='--adapt: burn-in steps of the evidence cases')
    ap.add_argument('--lag', type=float, default=1000.)
    ap.add_argument('--time', type=float, default=10.)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--walkers', type=int, default=1024)
    ap.add_argument('--ntemps', type=int, default=8)
    ap.add_argument('--no-compare', action='store_true', help='the tempered run alone (the run to profile)')
    ap.add_argument('--kernel-stats', default=None, help='kernel statistics (CSV) of a rocprofv3 --kernel-trace --stats run')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if a.adapt:
        res = run_adaptive(a.walkers, a.ntemps, a.steps, a.warmup, a.repeats, a.burn, a.lag, a.time)
        a.json = a.json or os.path.join(ROOT, 'profiles', 'tempered_adaptive.json')
    else:
        res = run(a.walkers, a.ntemps, a.steps, a.warmup, compare=not a.no_compare)
    if a.kernel_stats:
        res['device_time'] = kernel_split(a.kernel_stats)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
