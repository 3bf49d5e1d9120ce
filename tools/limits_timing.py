#!/usr/bin/env python3
"""Cost of upper limits (``nondet='censored'``) on the GPU: the same fit with 0, 1, 8 and 64 limits attached.

The light curve is the headline fit's (configs[1]: 3000 points, ShockCooling); the limits are non-detections in the
three days before its first epoch, in its six filters in turn.  For each number of limits, in one process: the route
``lightcurve_mcmc(..., nondet='censored')`` takes -- ``TemperedSampler(betas=[1.])`` at ``--walkers`` walkers,
``--warmup`` unstored steps, then ``--steps`` steps timed by a host clock around ``run_mcmc`` (which returns when the
device has finished), in ms per step -- and ``lcf_log_likelihood_dev`` alone on ``--rows`` rows, ``--reps`` calls between
two events on one stream, in ms per call.  ``--repeats`` repetitions ALTERNATING between the engines, so that all see the
same drift of the machine; medians and all runs are reported.  With limits a likelihood call is three or four launches
more (the limit engine's coefficients, its thermal states where it shares epochs, its points, ``k_limits``); the engine
with ONE limit pays those launches for next to no work, so its difference from the engine without limits is the launches'
share of what 8 and 64 limits cost.  There is no gate on any of it.

Usage:  python tools/limits_timing.py [--steps 200] [--json profiles/limits_timing.json]"""
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

PRIORS = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.5)]
LO, HI = np.array([1., 0.3, 2., 1.5, 0.]), np.array([1.5, 0.7, 4., 2.5, 0.2])
COUNTS = (0, 1, 8, 64)


def lc_case(n_lim):
    """The configs[1] light curve with ``n_lim`` non-detections in front of it (none: no ``nondet`` column)."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'config2.npz'))
    t, names, y, dy = g['cfg2__t'], [str(n) for n in g['cfg2__names']], g['cfg2__y'], g['cfg2__dy']
    if n_lim == 0:
        return {'MJD': t, 'filter': names, 'lum': y, 'dlum': dy}
    filters = list(dict.fromkeys(names))
    t_lim = np.linspace(t.min() - 3., t.min() - 0.05, n_lim)
    return {'MJD': np.concatenate([t_lim, t]), 'filter': [filters[k % len(filters)] for k in range(n_lim)] + names,
            'lum': np.concatenate([np.zeros(n_lim), y]), 'dlum': np.concatenate([np.full(n_lim, 0.02 * np.median(y)), dy]),
            'nondet': np.arange(n_lim + len(t)) < n_lim}


def likelihood_ms(eng, P_host, reps):
    """ms per ``lcf_log_likelihood_dev`` call on the rows (in device memory): ``reps`` calls between two events."""
    import torch
    rows = len(P_host)
    P = torch.from_numpy(P_host).cuda()
    out = torch.empty(rows, dtype=torch.float64, device='cuda')
    stream = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        eng.log_likelihood_dev(rows, P.data_ptr(), out.data_ptr(), stream.cuda_stream)      # (workspace, first launch)
        a.record(stream)
        for _ in range(reps):
            eng.log_likelihood_dev(rows, P.data_ptr(), out.data_ptr(), stream.cuda_stream)
        b.record(stream)
    b.synchronize()
    assert bool(torch.isfinite(out).all())
    return a.elapsed_time(b) / reps


def summary(ms):
    return {'median': float(np.median(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms)), 'runs': [float(v) for v in ms]}


def run(walkers, steps, warmup, rows, reps, repeats):
    model = M.ShockCooling(redshift=0.)
    model.max_bound_engines = len(COUNTS)
    rng = np.random.default_rng(1)
    x0 = LO + (HI - LO) * rng.random((1, walkers, 5))
    P = np.ascontiguousarray(LO + (HI - LO) * np.random.default_rng(2).random((rows, 5)))
    engines, samplers = {}, {}
    for n in COUNTS:
        engines[n] = model.engine_for(lc_case(n), priors=PRIORS, nondet='censored')
        assert getattr(engines[n], 'nlimits', 0) == n
        samplers[n] = TemperedSampler(walkers, 5, engines[n], betas=[1.], seed=1)
        samplers[n].run_mcmc(x0, warmup, store=False)
    step_ms, like_ms = {n: [] for n in COUNTS}, {n: [] for n in COUNTS}
    for _ in range(repeats):           # alternating: every engine sees the same drift of the machine
        for n in COUNTS:
            t0 = time.perf_counter()
            samplers[n].run_mcmc(None, steps, store=False)
            step_ms[n].append(1e3 * (time.perf_counter() - t0) / steps)
        for n in COUNTS:
            like_ms[n].append(likelihood_ms(engines[n], P, reps))
    res = {'model': 'ShockCooling', 'light_curve': 'configs[1]: 3000 points', 'sampler': 'TemperedSampler(betas=[1.])',
           'walkers': walkers, 'steps': steps, 'rows': rows, 'reps': reps, 'repeats': repeats, 'limits': {}}
    for n in COUNTS:
        res['limits'][str(n)] = {'ms_per_step': summary(step_ms[n]), 'log_likelihood_dev_ms': summary(like_ms[n]),
                                 'acceptance': float(samplers[n].acceptance_fraction.mean())}
    base_s, base_l = np.median(step_ms[0]), np.median(like_ms[0])
    res['extra'] = {str(n): {'ms_per_step': float(np.median(step_ms[n]) - base_s),
                             'share_of_step': float(np.median(step_ms[n]) / base_s - 1.),
                             'log_likelihood_dev_ms': float(np.median(like_ms[n]) - base_l)} for n in COUNTS[1:]}
    res['extra_launches_ms_per_step'] = res['extra']['1']['ms_per_step']     # (one limit: the launches, next to no work)
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
