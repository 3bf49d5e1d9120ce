#!/usr/bin/env python3
"""Cost of ``luminosity_predictive()`` after an Arnett fit, on the GPU, next to the only route there was before it.

The chain is a REAL fit: ``lightcurve_mcmc`` of the 40-epoch Arnett curve of the tests (exact integral at M_Ni = 0.07,
tau_m = 12 d, t_0 = -5 d, 2 % noise) with 1024 walkers, 2000 stored steps after 1000 of burn-in, one rung at beta = 1.
The bands of L(t) on 1000 times, the dark counts and every sample's peak are timed (a) over the whole chain, 2 048 000
samples -- 2e9 values, each a 64-node quadrature -- and (b) at ``thin=100`` (20 480 samples), where the earlier route --
``model(t, *flat.T)`` (every value over PCIe), ``np.nanpercentile`` and ``np.nanargmax`` on the host -- is timed on the
same samples and the results are compared.  At (b) both routes are medians of ``--reps`` ALTERNATING repetitions after one
warm-up each, with their ranges; the new call is expected not to be slower (the earlier route does every evaluation
the new one does, then a download and a host sort), and ``thinned.not_slower`` says whether the ranges bear that out.
The whole-chain rate is given next to the 2e9 values/s that ``profiles/central_timing.json`` implies for the bare
evaluation (2.6e7 nodes in 0.19 ms): the ceiling of a call that evaluates every value once.  Every number is a host
clock around a call that returns host arrays.

``k_lq_eval``'s share of the device time comes from a separate ``rocprofv3 --kernel-trace --stats`` run of this script
with ``--profile`` (the fit and ONE whole-chain call, nothing else), whose kernel statistics ``--kernel-stats`` folds
into the result.

Usage:  python tools/luminosity_timing.py [--reps 5] [--kernel-stats stats.csv] [--json profiles/luminosity_timing.json]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import central_reference as C  # noqa: E402
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.fitting import lightcurve_mcmc, luminosity_predictive  # noqa: E402

TRUTH = np.array([0.07, 12., -5.])
BARE_VALUES_PER_S = 2.6e7 / 0.19e-3 / 64       # profiles/central_timing.json: 100 epochs x 4096 rows x 64 nodes in 0.19 ms


def arnett_curve(noise=0.02):
    mjd = np.linspace(0., 90., 40)
    exact = np.array([C.truth('arnett', t - TRUTH[2], TRUTH[:1], TRUTH[1]) for t in mjd])
    deviates = np.random.default_rng(11).standard_normal(40)
    return {'MJD': mjd, 'L_bol': exact * (1. + noise * deviates), 'dL_bol': noise * exact}


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def summary(ms):
    return {'median': float(np.median(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms)), 'runs': [float(v) for v in ms]}


def rel_diff(got, want):
    with np.errstate(all='ignore'):
        d = np.abs(got - want) / np.abs(want)
    return float(np.nanmax(np.where(got == want, 0., d)))


def kernel_split(path):
    """Device time of one whole-chain call by kernel, from the kernel statistics of a rocprofv3 run with --profile."""
    names = ('k_lq_eval', 'k_kq_pass', 'k_lq_peak', 'k_pq_pick', 'k_pq_finish')
    ns = dict.fromkeys(names, 0)
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            for name in names:
                if '::' + name + '(' in row['Name']:
                    ns[name] += int(float(row['TotalDurationNs']))
    total = sum(ns.values())
    return {'ns': ns, 'call_kernels_ms': total / 1e6, 'k_lq_eval_share': ns['k_lq_eval'] / total if total else None}


def fit(walkers, steps, burnin):
    lc, model = arnett_curve(), M.Arnett()
    priors = [M.UniformPrior(0.001, 1.), M.UniformPrior(2., 60.), M.UniformPrior(-30., -0.01)]
    np.random.seed(5)
    sampler = lightcurve_mcmc(lc, model, priors=priors, p_lo=[0.05, 9., -7.], p_up=[0.09, 15., -3.], nwalkers=walkers,
                              nsteps=steps, nsteps_burnin=burnin, seed=1)
    return lc, model, sampler


def run(reps, walkers, steps, burnin, num, thin):
    lc, model, sampler = fit(walkers, steps, burnin)
    res = {'model': 'Arnett', 'chain': 'lightcurve_mcmc fit (TemperedSampler, one rung at beta = 1)', 'walkers': walkers,
           'steps': steps, 'times': num, 'reps': reps, 'bare_evaluation_values_per_s': BARE_VALUES_PER_S}

    full = luminosity_predictive(lc, model, sampler, num=num)                          # (warm-up: the grid engine)
    ms = [timed_ms(lambda: luminosity_predictive(lc, model, sampler, num=num)) for _ in range(reps)]
    values = full.n_samples * len(full.t)
    rate = values / (np.median(ms) * 1e-3)
    summ = full.peak_summary((15.87, 50., 84.14))
    res['whole_chain'] = {'samples': full.n_samples, 'values': values, 'ms': summary(ms), 'values_per_s': rate,
                          'share_of_bare_evaluation_rate': rate / BARE_VALUES_PER_S,
                          'L_peak_W': summ['L_peak'].tolist(), 't_rise_d': summ['t_rise'].tolist(),
                          'n_peak_first': full.n_peak_first, 'n_peak_last': full.n_peak_last}

    flat = np.ascontiguousarray(sampler.get_chain(thin=thin, flat=True))
    distinct = np.unique(full.t)

    def new_route():
        return luminosity_predictive(lc, model, flat, num=num)

    def old_route():
        L = model(distinct, *flat.T)                               # (num, S) float64 across PCIe
        return np.nanpercentile(L, full.percentiles, axis=1), np.nanargmax(L, axis=0), np.nanmax(L, axis=0)
    thinned = new_route()
    want, where, top = old_route()
    assert len(flat) == thinned.n_samples
    err = rel_diff(thinned.luminosity, want)
    assert err <= 2e-11, err
    assert np.array_equal(where, thinned.peak_index) and np.array_equal(top, thinned.L_peak)
    new_ms, old_ms = [], []
    for _ in range(reps):          # alternating: both see the same drift of the machine
        new_ms.append(timed_ms(new_route))
        old_ms.append(timed_ms(old_route))
    values = thinned.n_samples * len(thinned.t)
    res['thinned'] = {'thin': thin, 'samples': thinned.n_samples, 'values': values, 'ms': summary(new_ms),
                      'values_per_s': values / (np.median(new_ms) * 1e-3),
                      'evaluate_plus_nanpercentile_plus_nanargmax_ms': summary(old_ms),
                      'ratio_old_over_new': float(np.median(old_ms) / np.median(new_ms)),
                      'not_slower': bool(np.median(new_ms) <= np.median(old_ms) and max(new_ms) <= max(old_ms)
                                         and min(new_ms) <= min(old_ms)),
                      'ranges_disjoint': bool(max(new_ms) < min(old_ms)),
                      'max_rel_diff': err, 'values_the_old_route_moves_MB': values * 8 / 1e6}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--kernel-stats', default=None, help='kernel statistics (CSV) of a rocprofv3 --kernel-trace --stats run '
                                                         'of this script with --profile')
    ap.add_argument('--profile', action='store_true', help='the fit and ONE whole-chain call, for the profiler')
    ap.add_argument('--small', action='store_true', help='tiny shapes (a quick check of the script itself)')
    a = ap.parse_args()
    shape = (64, 200, 50, 50, 10) if a.small else (1024, 2000, 1000, 1000, 100)
    if a.profile:
        lc, model, sampler = fit(*shape[:3])
        print(luminosity_predictive(lc, model, sampler, num=shape[3]))
        return
    res = run(a.reps, *shape)
    if a.kernel_stats:
        res['whole_chain']['device_time'] = kernel_split(a.kernel_stats)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
