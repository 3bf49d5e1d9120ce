#!/usr/bin/env python3
"""Cost of a custom model on the GPU, next to the built-in model it restates.

On the configs[1] light curve (3000 points) a ``CustomModel`` whose source restates ShockCooling2 and the built-in
``ShockCooling2``, in one process: both through ``TemperedSampler(betas=[1.])`` at ``--walkers`` walkers -- ``--warmup``
unstored steps, then ``--steps`` steps timed by a host clock around ``run_mcmc`` (which returns when the device has
finished), in ms per step -- then ``lcf_log_likelihood_dev`` alone on ``--rows`` rows for each, ``--reps`` calls between
two events on one stream, in ms per call.  ``--repeats`` repetitions, alternating between the two, so that both see the
same drift of the machine; medians and all runs are reported, and the ratios custom / built-in of the medians.  The
compile time of the source, cold and from the cache, comes first.  The user's function is the user's cost: there is no
gate on any ratio.

Where the device time goes comes from a separate ``rocprofv3 --kernel-trace --stats`` run of this script with nothing else
collected; ``--kernel-stats CSV`` reads that run's kernel statistics and adds the split to the report.

Usage:  python tools/custom_timing.py [--steps 200] [--json profiles/custom_timing.json] [--kernel-stats CSV]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import engine as E, models as M  # noqa: E402
from lightcurve_fitting_amd.sampler import TemperedSampler  # noqa: E402

# ShockCooling2 (models.py:403-406) as a user writes it; consts = A, a, alpha, epsilon_1, epsilon_2
SOURCE = r'''
__device__ void lcf_user_state(double t_in, const double* p, const double* consts, double z,
                               double& T_kK, double& R_1000Rsun) {
    const double t = t_in - p[3];
    T_kK = p[0] * lcf::pw(t, 2. * consts[3] - 0.5);
    const double L = p[1] * exp(-lcf::pw(consts[1] * t / p[2], consts[2])) * lcf::pw(t, -2. * consts[4]) * 1e42;
    R_1000Rsun = lcf::kC3 * sqrt(L) * lcf::pw(T_kK, -2.);
}
'''
NAMES = ['T_1', 'L_1', 't_\\mathrm{tr}', 't_0']
PRIORS = [M.UniformPrior(0., 100.), M.UniformPrior(0., 100.), M.UniformPrior(0., 100.), M.UniformPrior(-1., 0.5)]
LO, HI = np.array([15., 1., 5., 0.]), np.array([25., 3., 15., 0.2])


def lc_case():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'config2.npz'))
    return {'MJD': g['cfg2__t'], 'filter': [str(n) for n in g['cfg2__names']], 'lum': g['cfg2__y'], 'dlum': g['cfg2__dy']}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def summary(runs):
    return {'median': float(np.median(runs)), 'min': float(min(runs)), 'max': float(max(runs)), 'runs': [float(r) for r in runs]}


def likelihood_ms(eng, rows, reps):
    """ms per ``lcf_log_likelihood_dev`` call on ``rows`` device rows: ``reps`` calls between two events of one stream."""
    import torch
    rng = np.random.default_rng(2)
    P = torch.from_numpy(LO + (HI - LO) * rng.random((rows, eng.ndim))).cuda()
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


def kernel_split(path):
    """Device time by kernel group from the kernel statistics of a rocprofv3 run."""
    groups = {'custom_points_ns': 0, 'k_points_ns': 0, 'prepare_finalize_ns': 0, 'tempered_ns': 0, 'other_ns': 0}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name, ns = row['Name'], int(float(row['TotalDurationNs']))
            key = ('custom_points_ns' if 'lcf_custom_points' in name else 'k_points_ns' if '::k_points' in name
                   else 'prepare_finalize_ns' if '::k_prepare' in name or '::k_finalize' in name
                   else 'tempered_ns' if '::k_t_' in name else 'other_ns')
            groups[key] += ns
    return groups


def run(walkers, steps, warmup, rows, reps, repeats):
    lc = lc_case()
    consts = M.ShockCooling2(redshift=0.)._consts()[:5]
    res = {'walkers': walkers, 'steps': steps, 'warmup': warmup, 'rows': rows, 'reps': reps, 'repeats': repeats}
    cold = timed(lambda: E.CustomProgram(SOURCE))
    res['compile_s'] = {'cold': cold, 'cached': timed(lambda: E.CustomProgram(SOURCE))}
    models = {'custom': M.CustomModel(SOURCE, NAMES, consts=consts, redshift=0.), 'builtin': M.ShockCooling2(redshift=0.)}
    engines = {k: m.engine_for(lc, priors=PRIORS) for k, m in models.items()}
    res['n_points'] = int(engines['custom'].npoints)
    rng = np.random.default_rng(1)
    x0 = LO + (HI - LO) * rng.random((1, walkers, 4))
    samplers = {}
    for k, eng in engines.items():
        samplers[k] = TemperedSampler(walkers, 4, eng, betas=[1.], seed=1)
        samplers[k].run_mcmc(x0, warmup, store=False)
    step_ms, like_ms = {k: [] for k in engines}, {k: [] for k in engines}
    for _ in range(repeats):          # alternating: both see the same drift of the machine
        for k, s in samplers.items():
            step_ms[k].append(1e3 * timed(lambda: s.run_mcmc(None, steps, store=False)) / steps)
    for _ in range(repeats):
        for k, eng in engines.items():
            like_ms[k].append(likelihood_ms(eng, rows, reps))
    res['tempered_ms_per_step'] = {k: summary(v) for k, v in step_ms.items()}
    res['log_likelihood_dev_ms'] = {k: summary(v) for k, v in like_ms.items()}
    for key in ('tempered_ms_per_step', 'log_likelihood_dev_ms'):
        res[key]['ratio_custom_over_builtin'] = res[key]['custom']['median'] / res[key]['builtin']['median']
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
    ap.add_argument('--kernel-stats', default=None, help='kernel statistics (CSV) of a rocprofv3 --kernel-trace --stats run')
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'custom_timing.json'))
    a = ap.parse_args()
    res = run(a.walkers, a.steps, a.warmup, a.rows, a.reps, a.repeats)
    if a.kernel_stats:
        res['device_time'] = kernel_split(a.kernel_stats)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
