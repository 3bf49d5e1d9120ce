#!/usr/bin/env python3
"""Engine creation and the bench lines of this tree against a checkout of another commit (its parent), on one GPU.

Two shapes: the headline fit's light curve (configs[1]: 500 epochs x UBVgri = 3000 points) and the population's (32
engines of 100 epochs x UBVgri = 600 points).  Three measurements, each in ``--runs`` fresh processes per tree,
ALTERNATING between the trees so that both see the same drift of the machine:

* ``create``: seconds ``lcf_engine_create`` takes (``Engine.timings['create_s']``: the host's plan, the one upload, the
  problem's image; the band tables are packed before it) -- the median over nine engines on the 3000-point light curve
  after a first one (which loads the library's code objects), and the sum over the 32 engines of 600 points;
* ``mcmc`` and ``population``: ``value`` of ``bench.py --gpus 1`` (``--workload population`` for the second) without the
  CPU baseline and the end-to-end block.

``within_parent_spread``: this tree's median lies between the other tree's fastest and slowest run.  The other tree must
be built (``make -C lightcurve_fitting_amd/csrc``).

Usage:  python tools/engine_plan_timing.py --parent ../parent-checkout [--runs 5] [--json profiles/engine_plan_timing.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = list('UBVgri')


def child_create(tree):
    """In a fresh process, on the library of ``tree``: the creation times of both shapes as one JSON line."""
    sys.path.insert(0, tree)
    from lightcurve_fitting_amd import models as M
    rng = np.random.default_rng(11)

    def create_s(n_epochs):
        t = np.repeat(np.sort(rng.uniform(0.5, 10., n_epochs)), 6)
        y = 1e20 * (1. + 0.05 * rng.standard_normal(len(t)))
        eng = M.ShockCooling(redshift=0.).make_engine(t, BANDS * n_epochs, y, 0.05 * np.abs(y))
        eng.log_likelihood(np.array([[1.2, 0.5, 3.0, 2.0, 0.1]]))      # (the engine works)
        return eng.timings['create_s']
    create_s(500)
    fit = [create_s(500) for _ in range(9)]
    population = [create_s(100) for _ in range(32)]
    print(json.dumps({'fit_3000_points_create_s': float(np.median(fit)), 'population_32x600_points_create_s': float(np.sum(population))}))


def fresh(tree, what, steps, timeout):
    """One measurement in a fresh process of ``tree`` -> dict of its numbers."""
    env = dict(os.environ, LCF_BENCH_NO_E2E='1')
    if what == 'create':
        cmd = [sys.executable, os.path.abspath(__file__), '--child', tree]
    else:
        cmd = [sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', str(steps[what]), '--warmup', '20',
               '--no-cpu-baseline'] + (['--workload', 'population'] if what == 'population' else [])
    t0 = time.perf_counter()
    done = subprocess.run(cmd, cwd=tree, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, check=True)
    line = json.loads(done.stdout.decode().strip().splitlines()[-1])
    out = line if what == 'create' else {what + '_walker_steps_per_s': line['value']}
    print(f'{what:10s} {os.path.basename(tree.rstrip("/")):12s} {time.perf_counter() - t0:6.1f} s  {out}', file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent', help='a built checkout of the commit to compare with')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--mcmc-steps', type=int, default=1000)
    ap.add_argument('--population-steps', type=int, default=300)
    ap.add_argument('--timeout', type=float, default=240., help='seconds a child process may take')
    ap.add_argument('--json', default=None)
    ap.add_argument('--child', metavar='TREE', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_create(a.child)
    trees = {'parent': os.path.abspath(a.parent), 'head': ROOT}
    steps = {'mcmc': a.mcmc_steps, 'population': a.population_steps}
    runs = {name: {} for name in trees}
    for what in ('create', 'mcmc', 'population'):
        for _ in range(a.runs):
            for name, tree in trees.items():
                for key, value in fresh(tree, what, steps, a.timeout).items():
                    runs[name].setdefault(key, []).append(value)
    res = {'runs_per_tree': a.runs, 'order': 'alternating fresh processes, parent first', 'steps': steps, 'measurements': {}}
    for key in runs['head']:
        p, h = runs['parent'][key], runs['head'][key]
        res['measurements'][key] = {
            'parent': {'median': float(np.median(p)), 'min': min(p), 'max': max(p), 'runs': p},
            'head': {'median': float(np.median(h)), 'min': min(h), 'max': max(h), 'runs': h},
            'within_parent_spread': bool(min(p) <= np.median(h) <= max(p))}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
