#!/usr/bin/env python3
"""Cost of ``color_predictive()`` after a fit, on the GPU, next to ``posterior_predictive`` and the host route.

After the configs[1]-shaped fit the other timing tools use (ShockCooling, 1024 walkers, 2000 stored steps after 1000 of
burn-in, 3000-point light curve, through ``lightcurve_mcmc``):

1. the whole chain (2 048 000 samples, read where they lie), the colours B-V, g-r, r-i, U-B and V-r (6 filters) on 1000
   times, with and without ``peak``;
2. in the same session ``posterior_predictive`` on the same six filters and times;
3. at ``thin=100`` (20 480 samples) the host route -- ``model(t, filters, *flat.T)`` (every value over PCIe), the NumPy
   formula of the colours, ``np.nanpercentile`` and ``np.nanargmax`` -- on the same samples, and how closely the two
   agree.

The three whole-chain calls alternate, ``--reps`` rounds after one warm-up round; medians are reported and the range
of every series is kept.  Every number is a host clock around a call that returns host arrays (the device work is
complete when it returns).  Kernel shares come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.

Usage:  python tools/color_timing.py [--reps 5] [--json profiles/color_timing.json]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.fitting import color_predictive, lightcurve_mcmc, posterior_predictive  # noqa: E402

COLORS = ('B-V', 'g-r', 'r-i', 'U-B', 'V-r')
PRIORS = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.5)]
LO, HI = [1., 0.3, 2., 1.5, 0.], [1.5, 0.7, 4., 2.5, 0.2]


def lc_case():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'config2.npz'))
    return {'MJD': g['cfg2__t'], 'filter': [str(n) for n in g['cfg2__names']], 'lum': g['cfg2__y'], 'dlum': g['cfg2__dy']}


def clock_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms)),
            'all_ms': [float(v) for v in ms]}


def host_route(model, t, filters, index, dzp, percentiles, flat):
    """model(...), the colours, nanpercentile, nanargmax: what there was before color_predictive."""
    Y = model(t, filters, *flat.T)                                  # (nf, nt, S) float64 across PCIe
    bands = []
    for (a, b), d in zip(index, dzp):
        ok = np.isfinite(Y[a]) & np.isfinite(Y[b]) & (Y[a] > 0.) & (Y[b] > 0.)
        ratio = np.divide(Y[a], Y[b], out=np.ones_like(Y[a]), where=ok)
        bands.append(np.nanpercentile(np.where(ok, d - 2.5 * np.log10(ratio), np.nan), percentiles, axis=-1))
    at = np.nanargmax(Y, axis=1)                                    # (nf, S)
    return np.stack(bands, axis=1), np.take_along_axis(Y, at[:, None, :], axis=1)[:, 0].T, at.T


def run(reps, walkers, steps, burnin, num, thin):
    lc, model = lc_case(), M.ShockCooling(redshift=0.)
    sampler = lightcurve_mcmc(lc, model, priors=PRIORS, p_lo=LO, p_up=HI, nwalkers=walkers, nsteps=steps,
                              nsteps_burnin=burnin, seed=1)
    res = {'walkers': walkers, 'steps': steps, 'colors': list(COLORS), 'filters': 6, 'times': num, 'reps': reps,
           'note': 'host clocks around calls that return host arrays; the three whole-chain calls alternate'}

    calls = {'color_with_peak': lambda: color_predictive(lc, model, sampler, colors=COLORS, num=num),
             'color_without_peak': lambda: color_predictive(lc, model, sampler, colors=COLORS, num=num, peak=False),
             'posterior_predictive': None}
    full = calls['color_with_peak']()                               # (warm-up: builds the grid engine)
    assert sampler._chain_on_device == steps and len(full.filters) == 6
    calls['posterior_predictive'] = lambda: posterior_predictive(lc, model, sampler, num=num, filters_to_model=full.filters)
    ms = {name: [] for name in calls}
    for r in range(reps + 1):
        for name, fn in calls.items():
            t, _ = clock_ms(fn)
            if r:
                ms[name].append(t)
    res['whole_chain'] = {'samples': full.n_samples, **{name: summary(v) for name, v in ms.items()}}
    med = {name: res['whole_chain'][name]['median_ms'] for name in calls}
    res['whole_chain']['ratio_color_over_posterior_predictive'] = med['color_without_peak'] / med['posterior_predictive']
    res['whole_chain']['peak_costs_ms'] = med['color_with_peak'] - med['color_without_peak']
    res['whole_chain']['all_valid'] = bool(np.all(full.n_valid == full.n_samples))
    res['whole_chain']['n_peak_first'] = [int(v) for v in full.n_peak_first]
    res['whole_chain']['n_peak_last'] = [int(v) for v in full.n_peak_last]

    new = [clock_ms(lambda: color_predictive(lc, model, sampler, colors=COLORS, num=num, thin=thin)) for _ in range(reps + 1)]
    thinned = new[0][1]
    flat = sampler.get_chain(thin=thin, flat=True)
    assert len(flat) == thinned.n_samples
    where = {f: i for i, f in enumerate(thinned.filters)}
    index = [(where[a], where[b]) for a, b in thinned.colors]
    dzp = [a.m0 - b.m0 for a, b in thinned.colors]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        old = [clock_ms(lambda: host_route(model, thinned.t, thinned.filters, index, dzp, thinned.percentiles, flat))
               for _ in range(max(2, min(reps, 3)))]
    want, y_peak, at = old[0][1]
    res['thinned'] = {'thin': thin, 'samples': thinned.n_samples, 'color_predictive': summary([t for t, _ in new[1:]]),
                      'host_route': summary([t for t, _ in old[1:]]),
                      'max_abs_diff_mag': float(np.nanmax(np.abs(thinned.color - want))),
                      'max_rel_diff_y_peak': float(np.nanmax(np.abs(thinned.y_peak - y_peak) / np.abs(y_peak))),
                      'peak_index_equal_fraction': float(np.mean(thinned.peak_index == at)),
                      'values_the_host_route_moves_MB': thinned.n_samples * 6 * num * 8 / 1e6}
    res['thinned']['ratio_host_over_new'] = (res['thinned']['host_route']['median_ms'] /
                                             res['thinned']['color_predictive']['median_ms'])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--small', action='store_true', help='tiny shapes (a quick check of the script itself)')
    a = ap.parse_args()
    res = run(a.reps, 64, 200, 50, 50, 10) if a.small else run(a.reps, 1024, 2000, 1000, 1000, 100)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
