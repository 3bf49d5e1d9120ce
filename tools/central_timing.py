#!/usr/bin/env python3
"""Cost of the central-engine models (``Arnett``, ``Magnetar``) on the GPU, next to their NumPy restatement on the host.

On a 100-epoch bolometric light curve, for each of the two models in one process: the route ``lightcurve_mcmc`` takes --
``TemperedSampler(betas=[1.])`` at ``--walkers`` walkers, ``--warmup`` unstored steps, then ``--steps`` steps timed by a
host clock around ``run_mcmc`` (which returns when the device has finished), in ms per step -- then
``lcf_log_likelihood_dev`` alone on ``--rows`` rows, ``--reps`` calls between two events on one stream, in ms per call,
and the restatement (``tests/central_reference.py``: the same rule in NumPy) on the same rows on the host, in ms per
call, with the number of cores this process may use.  ``--repeats`` repetitions, alternating between the models and
between device and host, so that all see the same drift of the machine; medians and all runs are reported, and the ratio
host / device of the medians.  There is nothing else to compare a new kernel with, and no gate on the ratio.

Usage:  python tools/central_timing.py [--steps 200] [--json profiles/central_timing.json]"""
import argparse
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
from lightcurve_fitting_amd.sampler import TemperedSampler  # noqa: E402

N_EPOCHS = 100
CASES = {
    'arnett': dict(model=M.Arnett, truth=[0.07, 12., -5.], lo=[0.05, 9., -7.], hi=[0.09, 15., -3.],
                   priors=[(0.001, 1.), (2., 60.), (-30., -0.01)]),
    'magnetar': dict(model=M.Magnetar, truth=[0.2, 10., 12., -5.], lo=[0.1, 5., 9., -7.], hi=[0.4, 20., 15., -3.],
                     priors=[(0.001, 10.), (1., 100.), (2., 60.), (-30., -0.01)]),
}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def summary(runs):
    return {'median': float(np.median(runs)), 'min': float(min(runs)), 'max': float(max(runs)), 'runs': [float(r) for r in runs]}


def light_curve(kind):
    """The model's own curve at the case's truth, 2 % noise."""
    rng = np.random.default_rng(3)
    mjd = np.linspace(0., 150., N_EPOCHS)
    exact = C.luminosity(kind, mjd, [CASES[kind]['truth']])[0]
    return {'MJD': mjd, 'L_bol': exact * (1. + 0.02 * rng.standard_normal(N_EPOCHS)), 'dL_bol': 0.02 * exact}


def rows_of(kind, rows):
    lo, hi = np.array(CASES[kind]['lo']), np.array(CASES[kind]['hi'])
    return lo + (hi - lo) * np.random.default_rng(2).random((rows, len(lo)))


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
    return a.elapsed_time(b) / reps, out.cpu().numpy()


def run(walkers, steps, warmup, rows, reps, repeats):
    cores = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else os.cpu_count()
    res = {'n_epochs': N_EPOCHS, 'walkers': walkers, 'steps': steps, 'warmup': warmup, 'rows': rows, 'reps': reps,
           'repeats': repeats, 'host_cores': int(cores)}
    lcs = {k: light_curve(k) for k in CASES}
    models = {k: c['model']() for k, c in CASES.items()}
    priors = {k: [M.UniformPrior(lo, hi) for lo, hi in c['priors']] for k, c in CASES.items()}
    engines = {k: m.engine_for(lcs[k], priors=priors[k]) for k, m in models.items()}
    blocks = {k: rows_of(k, rows) for k in CASES}
    samplers = {}
    for k, eng in engines.items():
        nd = eng.ndim
        x0 = rows_of(k, walkers)[None, :, :]
        samplers[k] = TemperedSampler(walkers, nd, eng, betas=[1.], seed=1)
        samplers[k].run_mcmc(x0, warmup, store=False)
    step_ms = {k: [] for k in CASES}
    dev_ms, host_ms, parity = {k: [] for k in CASES}, {k: [] for k in CASES}, {}
    for _ in range(repeats):          # alternating: all see the same drift of the machine
        for k, s in samplers.items():
            step_ms[k].append(1e3 * timed(lambda: s.run_mcmc(None, steps, store=False)) / steps)
    for _ in range(repeats):
        for k, eng in engines.items():
            ms, got = likelihood_ms(eng, blocks[k], reps)
            dev_ms[k].append(ms)
            lc = lcs[k]
            want = []
            host_ms[k].append(1e3 * timed(lambda: want.append(C.log_likelihood(k, lc['MJD'], lc['L_bol'], lc['dL_bol'],
                                                                               blocks[k]))))
            parity[k] = float(np.max(np.abs(got - want[0]) / np.abs(want[0])))
    res['tempered_ms_per_step'] = {k: summary(v) for k, v in step_ms.items()}
    res['log_likelihood_dev_ms'] = {k: summary(v) for k, v in dev_ms.items()}
    res['restatement_host_ms'] = {k: summary(v) for k, v in host_ms.items()}
    res['ratio_host_over_device'] = {k: res['restatement_host_ms'][k]['median'] / res['log_likelihood_dev_ms'][k]['median']
                                     for k in CASES}
    res['parity_relative'] = parity
    res['acceptance'] = {k: float(s.acceptance_fraction.mean()) for k, s in samplers.items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--walkers', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--rows', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'central_timing.json'))
    a = ap.parse_args()
    res = run(a.walkers, a.steps, a.warmup, a.rows, a.reps, a.repeats)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
