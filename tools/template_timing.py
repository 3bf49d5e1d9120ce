#!/usr/bin/env python3
"""Cost of a second component (``models.WithTemplate``) on the GPU: ShockCooling4 with and without the SiFTO template.

The light curve is the headline fit's (configs[1]: 3000 points).  In one process, for the plain ``ShockCooling4`` and for
``WithTemplate(ShockCooling4, sifto_template(), factors=('r',), offsets=('U',))``: ``TemperedSampler(betas=[1.])`` at
``--walkers`` walkers -- the route ``lightcurve_mcmc`` takes for such a model -- ``--warmup`` unstored steps, then
``--steps`` steps timed by a host clock around ``run_mcmc`` (which returns when the device has finished), in ms per step;
and ``lcf_log_likelihood_dev`` alone on ``--rows`` rows, ``--reps`` calls between two events on one stream, in ms per call.
``--repeats`` repetitions ALTERNATING between the two engines, so that both see the same drift of the machine; medians and
all runs are reported.  With the template a likelihood call writes the model values of every (row, point) to scratch and
reads them back in ``k_template`` (98 MB each way at 4096 x 3000) instead of summing in the points kernel.  There is no
gate on any of it.

Usage:  python tools/template_timing.py [--steps 200] [--json profiles/template_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.sampler import TemperedSampler  # noqa: E402
from tools.limits_timing import likelihood_ms, summary  # noqa: E402

BASE_PRIORS = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.5)]
BASE_LO, BASE_HI = np.array([1., 0.3, 2., 1.5, 0.]), np.array([1.5, 0.7, 4., 2.5, 0.2])
KINDS = ('plain', 'template')


def light_curve():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'config2.npz'))
    return {'MJD': g['cfg2__t'], 'filter': [str(n) for n in g['cfg2__names']], 'lum': g['cfg2__y'], 'dlum': g['cfg2__dy']}


def run(walkers, steps, warmup, rows, reps, repeats):
    lc = light_curve()
    t_mid = float(np.median(lc['MJD']))
    base = M.ShockCooling4(redshift=0.)
    models = {'plain': base, 'template': M.WithTemplate(base, M.sifto_template(), lc, factors=('r',), offsets=('U',))}
    # the template's box: its peak in the middle of the light curve, 103 days of template stretched over a few days
    lo = {'plain': BASE_LO, 'template': np.concatenate([BASE_LO, [t_mid - 0.5, 0.03, 0.8, -0.2]])}
    hi = {'plain': BASE_HI, 'template': np.concatenate([BASE_HI, [t_mid + 0.5, 0.06, 1.2, 0.2]])}
    priors = {'plain': BASE_PRIORS, 'template': BASE_PRIORS + [M.UniformPrior(t_mid - 5., t_mid + 5.), M.UniformPrior(0.01, 1.),
                                                             M.UniformPrior(0., 5.), M.UniformPrior(-2., 2.)]}
    engines, samplers, P = {}, {}, {}
    for k in KINDS:
        nd = len(lo[k])
        x0 = lo[k] + (hi[k] - lo[k]) * np.random.default_rng(1).random((1, walkers, nd))
        P[k] = np.ascontiguousarray(lo[k] + (hi[k] - lo[k]) * np.random.default_rng(2).random((rows, nd)))
        engines[k] = models[k].engine_for(lc, priors=priors[k])
        assert engines[k].ndim == nd
        samplers[k] = TemperedSampler(walkers, nd, engines[k], betas=[1.], seed=1)
        samplers[k].run_mcmc(x0, warmup, store=False)
    step_ms, like_ms = {k: [] for k in KINDS}, {k: [] for k in KINDS}
    for _ in range(repeats):           # alternating: both engines see the same drift of the machine
        for k in KINDS:
            t0 = time.perf_counter()
            samplers[k].run_mcmc(None, steps, store=False)
            step_ms[k].append(1e3 * (time.perf_counter() - t0) / steps)
        for k in KINDS:
            like_ms[k].append(likelihood_ms(engines[k], P[k], reps))
    npts = len(lc['MJD'])
    res = {'model': 'ShockCooling4', 'template': 'sifto_template(), factors r, offsets U', 'light_curve':
           f'configs[1]: {npts} points', 'sampler': 'TemperedSampler(betas=[1.])', 'walkers': walkers, 'steps': steps,
           'rows': rows, 'reps': reps, 'repeats': repeats, 'scratch_bytes_per_call': rows * npts * 8, 'engines': {}}
    for k in KINDS:
        res['engines'][k] = {'ndim': engines[k].ndim, 'ms_per_step': summary(step_ms[k]),
                             'log_likelihood_dev_ms': summary(like_ms[k]),
                             'acceptance': float(samplers[k].acceptance_fraction.mean())}
    res['extra'] = {'ms_per_step': float(np.median(step_ms['template']) - np.median(step_ms['plain'])),
                    'share_of_step': float(np.median(step_ms['template']) / np.median(step_ms['plain']) - 1.),
                    'log_likelihood_dev_ms': float(np.median(like_ms['template']) - np.median(like_ms['plain']))}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--walkers', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--rows', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    res = run(a.walkers, a.steps, a.warmup, a.rows, a.reps, a.repeats)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
