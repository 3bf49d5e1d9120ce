#!/usr/bin/env python3
"""Cost of ``thermal_predictive()`` after a fit, on the GPU, next to the only route there was before it.

After the configs[1]-shaped fit of ``tools/predictive_timing.py`` (ShockCooling, 1024 walkers, 2000 stored steps after
1000 of burn-in) the bands of T, R and L_bol and the validity counters on 1000 times are timed (a) over the whole chain,
2 048 000 samples read where they lie in device memory, and (b) at ``thin=100`` (20 480 samples), where the earlier
route -- ``model.temperature_radius(t, *flat.T)`` (every T and R over PCIe), ``stefan_boltzmann`` and
``np.nanpercentile`` on the host -- is timed on the same samples and the results are compared.  For scale,
``posterior_predictive()`` is timed on the same times with ONE filter: the thermal call runs the same passes without
the band evaluation, for three series instead of one.  Every number is a host clock around a call that returns host
arrays; each is the median of ``--reps`` calls after one warm-up call.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script.

Usage:  python tools/thermal_timing.py [--reps 5] [--json profiles/thermal_timing.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.bolometric import stefan_boltzmann  # noqa: E402
from lightcurve_fitting_amd.fitting import lightcurve_mcmc, posterior_predictive, thermal_predictive  # noqa: E402
from predictive_timing import HI, LO, PRIORS, lc_case, median_ms  # noqa: E402


def rel_diff(got, want):
    with np.errstate(all='ignore'):
        d = np.abs(got - want) / np.abs(want)
    return float(np.nanmax(np.where(got == want, 0., d)))


def run(reps, walkers, steps, burnin, num, thin):
    lc, model = lc_case(), M.ShockCooling(redshift=0.)
    sampler = lightcurve_mcmc(lc, model, priors=PRIORS, p_lo=LO, p_up=HI, nwalkers=walkers, nsteps=steps,
                              nsteps_burnin=burnin, seed=1)
    res = {'walkers': walkers, 'steps': steps, 'times': num, 'series': 3,
           'note': 'pairs = samples x times; a pair gives three values (T, R, L_bol) and feeds two counters'}

    full = thermal_predictive(lc, model, sampler, num=num)                              # (warm-up: builds the grid engine)
    assert sampler._chain_on_device == steps
    ms = median_ms(lambda: thermal_predictive(lc, model, sampler, num=num), reps)
    pairs = full.n_samples * len(full.t)
    res['whole_chain'] = {'samples': full.n_samples, 'ms': ms, 'ms_per_series': ms / 3, 'pairs_per_s': pairs / (ms * 1e-3),
                          'frac_cold_max': float(np.nanmax(full.frac_cold)),
                          'frac_inside_min': float(full.frac_inside.min())}
    one = [next(iter(dict.fromkeys(lc['filter'])))]
    posterior_predictive(lc, model, sampler, num=num, filters_to_model=one)
    lc_ms = median_ms(lambda: posterior_predictive(lc, model, sampler, num=num, filters_to_model=one), reps)
    res['whole_chain']['posterior_predictive_one_filter_ms'] = lc_ms

    thinned = thermal_predictive(lc, model, sampler, num=num, thin=thin)
    ms = median_ms(lambda: thermal_predictive(lc, model, sampler, num=num, thin=thin), reps)
    flat = sampler.get_chain(thin=thin, flat=True)
    assert len(flat) == thinned.n_samples

    def old_route():
        T, R = model.temperature_radius(thinned.t, *flat.T)         # 2 x (num, S) float64 across PCIe
        L = stefan_boltzmann(T, R)
        return [np.nanpercentile(X, thinned.percentiles, axis=-1) for X in (T, R, L)], np.sum(T < 8.12, axis=-1)
    want, cold = old_route()
    old_ms = median_ms(old_route, max(1, min(reps, 3)))
    err = max(rel_diff(got, w) for got, w in zip((thinned.temperature, thinned.radius, thinned.luminosity), want))
    assert err <= 2e-11, err
    assert np.array_equal(cold, thinned.n_cold)
    posterior_predictive(lc, model, sampler, num=num, thin=thin, filters_to_model=one)
    lc_ms = median_ms(lambda: posterior_predictive(lc, model, sampler, num=num, thin=thin, filters_to_model=one), reps)
    pairs = thinned.n_samples * len(thinned.t)
    res['thinned'] = {'thin': thin, 'samples': thinned.n_samples, 'ms': ms, 'ms_per_series': ms / 3,
                      'pairs_per_s': pairs / (ms * 1e-3), 'posterior_predictive_one_filter_ms': lc_ms,
                      'temperature_radius_plus_nanpercentile_ms': old_ms, 'ratio_old_over_new': old_ms / ms,
                      'max_rel_diff': err, 'values_the_old_route_moves_MB': 2 * pairs * 8 / 1e6}
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
