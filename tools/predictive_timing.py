#!/usr/bin/env python3
"""Cost of ``posterior_predictive()`` after a fit, on the GPU, next to the only route there was before it.

After the configs[1]-shaped fit (ShockCooling, 1024 walkers, 2000 stored steps after 1000 of burn-in, through
``lightcurve_mcmc``) the percentile bands on 6 filters x 1000 times are timed (a) over the whole chain, 2 048 000
samples read where they lie in device memory, and (b) at ``thin=100`` (20 480 samples), where the earlier route --
``model(t, filters, *flat.T)`` (every value over PCIe) followed by ``np.nanpercentile`` on the host -- is timed on the
same samples and both results are compared.  Every number is a host clock around a call that returns host arrays (the
device work is complete when it returns); each is the median of ``--reps`` calls after one warm-up call.  Kernel times
come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.

Usage:  python tools/predictive_timing.py [--reps 5] [--json profiles/predictive_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.fitting import lightcurve_mcmc, posterior_predictive  # noqa: E402


def lc_case():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'config2.npz'))
    return {'MJD': g['cfg2__t'], 'filter': [str(n) for n in g['cfg2__names']], 'lum': g['cfg2__y'], 'dlum': g['cfg2__dy']}


PRIORS = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.5)]
LO, HI = [1., 0.3, 2., 1.5, 0.], [1.5, 0.7, 4., 2.5, 0.2]
PASSES_DOC = 'point evaluations = samples x grid points, counted once (every pass evaluates all of them again)'


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def run(reps, walkers, steps, burnin, num, thin):
    lc, model = lc_case(), M.ShockCooling(redshift=0.)
    sampler = lightcurve_mcmc(lc, model, priors=PRIORS, p_lo=LO, p_up=HI, nwalkers=walkers, nsteps=steps,
                              nsteps_burnin=burnin, seed=1)
    res = {'walkers': walkers, 'steps': steps, 'filters': 6, 'times': num, 'note': PASSES_DOC}

    full = posterior_predictive(lc, model, sampler, num=num)                            # (warm-up: builds the grid engine)
    assert sampler._chain_on_device == steps and len(full.filters) == 6
    ms = median_ms(lambda: posterior_predictive(lc, model, sampler, num=num), reps)
    pairs = full.n_samples * full.quantiles[0].size
    res['whole_chain'] = {'samples': full.n_samples, 'ms': ms, 'point_evaluations_per_s': pairs / (ms * 1e-3),
                          'all_valid': bool(np.all(full.n_valid == full.n_samples))}

    thinned = posterior_predictive(lc, model, sampler, num=num, thin=thin)
    ms = median_ms(lambda: posterior_predictive(lc, model, sampler, num=num, thin=thin), reps)
    flat = sampler.get_chain(thin=thin, flat=True)
    assert len(flat) == thinned.n_samples

    def old_route():
        y = model(thinned.t, thinned.filters, *flat.T)            # (6, num, S) float64 across PCIe
        return np.nanpercentile(y, thinned.percentiles, axis=-1)
    want = old_route()
    old_ms = median_ms(old_route, max(1, min(reps, 3)))
    err = float(np.max(np.abs(thinned.quantiles - want) / np.abs(want)))
    assert err <= 2e-11, err
    pairs = thinned.n_samples * thinned.quantiles[0].size
    res['thinned'] = {'thin': thin, 'samples': thinned.n_samples, 'ms': ms, 'point_evaluations_per_s': pairs / (ms * 1e-3),
                      'model_plus_nanpercentile_ms': old_ms, 'ratio_old_over_new': old_ms / ms, 'max_rel_diff': err,
                      'values_the_old_route_moves_MB': pairs * 8 / 1e6}
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
