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

``--moves LIST`` (``stretch``, ``de``, ``snooker``, ``mix`` -- 0.8 DE / 0.2 snooker -- or ``all``, comma-separated;
default ``--json profiles/moves_timing.json``) measures the moves of ``TemperedSampler(moves=)`` instead: ms per step of
the same fit for the sampler without moves (``default``) and for each listed move, medians of ``--repeats`` alternating
repetitions; with ``--parent DIR`` (a built checkout of the parent commit) the default path of this tree next to the
parent's, each repetition a fresh process, alternating; and ``get_autocorr_time`` of the cold chain (``--autocorr-steps``
stored steps after ``--burn``) for the default sampler, DE and the mixture.

Usage:  python tools/tempered_timing.py [--steps 300] [--json profiles/tempered_timing.json] [--kernel-stats CSV]
        python tools/tempered_timing.py --adapt [--repeats 5] [--burn 1000]
        python tools/tempered_timing.py --moves all [--parent DIR] [--repeats 5] [--burn 1000] [--autocorr-steps 2000]"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--package-root DIR, the child processes of --parent: the package of that tree, the golden light curve of this one)
PACKAGE_ROOT = sys.argv[sys.argv.index('--package-root') + 1] if '--package-root' in sys.argv[:-1] else ROOT
sys.path.insert(0, PACKAGE_ROOT)
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


def move_list(name):
    from lightcurve_fitting_amd.sampler import DEMove, DESnookerMove, StretchMove
    return {'default': None, 'stretch': StretchMove(), 'de': DEMove(), 'snooker': DESnookerMove(),
            'mix': [(DEMove(), 0.8), (DESnookerMove(), 0.2)]}[name]


def stats(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'runs': [float(x) for x in v]}


def default_path_once(walkers, ntemps, steps, warmup):
    """ms per step of the sampler without moves, through nothing the parent commit lacks (a child of --parent)."""
    eng = M.ShockCooling(redshift=0.).engine_for(lc_case(), priors=PRIORS)
    s = TemperedSampler(walkers, eng.ndim, eng, betas=default_betas(eng.ndim, ntemps, Tmax=np.inf), seed=1)
    s.run_mcmc(LO + (HI - LO) * np.random.default_rng(1).random((ntemps, walkers, eng.ndim)), warmup, store=False)
    return 1e3 * timed(lambda: s.run_mcmc(None, steps)) / steps


def run_moves(names, walkers, ntemps, steps, warmup, repeats, burn, autocorr_steps, parent):
    eng = M.ShockCooling(redshift=0.).engine_for(lc_case(), priors=PRIORS)
    betas = default_betas(eng.ndim, ntemps, Tmax=np.inf)
    x0 = LO + (HI - LO) * np.random.default_rng(1).random((ntemps, walkers, eng.ndim))
    new = lambda name: TemperedSampler(walkers, eng.ndim, eng, betas=betas, seed=1,
                                       **({} if name == 'default' else {'moves': move_list(name)}))
    samplers = {name: new(name) for name in ['default'] + names}
    for s in samplers.values():
        s.run_mcmc(x0, warmup, store=False)
    ms = {name: [] for name in samplers}
    for _ in range(repeats):          # interleaved: every sampler sees the same drift of the machine
        for name, s in samplers.items():
            s.reset()
            ms[name].append(1e3 * timed(lambda: s.run_mcmc(None, steps)) / steps)
    res = {'walkers': walkers, 'ntemps': ntemps, 'steps': steps, 'warmup': warmup, 'repeats': repeats,
           'n_points': int(eng.npoints), 'mix': '0.8 DEMove + 0.2 DESnookerMove',
           'ms_per_step': {name: stats(v) for name, v in ms.items()},
           'acceptance_cold_rung': {name: float(s.acceptance_fraction[0].mean()) for name, s in samplers.items()}}
    for s in samplers.values():
        s.close()
    if parent:
        runs = {'this_commit': [], 'parent_commit': []}
        for _ in range(repeats):      # a fresh process each, alternating
            for key, root in (('this_commit', ROOT), ('parent_commit', os.path.abspath(parent))):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--default-path-once', '--walkers', str(walkers),
                                      '--ntemps', str(ntemps), '--steps', str(steps), '--warmup', str(warmup),
                                      '--package-root', root], check=True, capture_output=True, text=True, timeout=300)
                runs[key].append(float(out.stdout.strip().splitlines()[-1]))
        res['default_path_ms_per_step'] = {k: stats(v) for k, v in runs.items()}
    res['autocorr'] = {}
    for name in [n for n in ('default', 'de', 'mix') if n in samplers]:
        s = new(name)
        s.run_mcmc(x0, burn, store=False)
        s.run_mcmc(None, autocorr_steps)
        tau = s.get_autocorr_time(quiet=True)
        res['autocorr'][name] = {'burn': burn, 'steps': autocorr_steps, 'tau': [float(t) for t in np.atleast_1d(tau)],
                                 'steps_over_tau_max': float(autocorr_steps / np.max(tau)),
                                 'acceptance_cold_rung': float(s.acceptance_fraction[0].mean())}
        s.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--moves', default=None, help='measure these moves: stretch, de, snooker, mix (comma-separated) or all')
    ap.add_argument('--parent', default=None, help='--moves: a built checkout of the parent commit to time the default path of')
    ap.add_argument('--autocorr-steps', type=int, default=2000)
    ap.add_argument('--default-path-once', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--package-root', default=None, help=argparse.SUPPRESS)
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
    if a.default_path_once:
        print(default_path_once(a.walkers, a.ntemps, a.steps, a.warmup))
        return
    if a.moves:
        names = ['stretch', 'de', 'snooker', 'mix'] if a.moves == 'all' else a.moves.split(',')
        res = run_moves(names, a.walkers, a.ntemps, a.steps, a.warmup, a.repeats, a.burn, a.autocorr_steps, a.parent)
        a.json = a.json or os.path.join(ROOT, 'profiles', 'moves_timing.json')
    elif a.adapt:
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
