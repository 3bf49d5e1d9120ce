#!/usr/bin/env python3
"""Cost of ``chain_history()`` after a fit, on the GPU, next to the only route there was before it.

After the configs[1]-shaped fit (ShockCooling, 1024 walkers, 2000 stored steps after 1000 of burn-in, through
``lightcurve_mcmc``) the numbers of the chain plot -- five percentiles across the walkers per step and column, the
log-probability included, the walkers that moved per step, and the 512 x 64 trace raster of every column -- are computed
over the whole chain where it lies in device memory.  The earlier route -- ``get_chain`` + ``get_log_prob`` (the chain
over PCIe), ``np.percentile`` over the walker axis, the comparison of the rows' bit patterns for the moves and one
``np.histogram`` per step bin and column on the host -- is then timed on the same chain in the same process, download
included, and every number of both routes is asserted equal.  Every time is a host clock around a call that returns
host arrays (the device work is complete when it returns); the device route is the median of ``--reps`` calls after one
warm-up call, the download (which happens once) the one call there is.  Kernel times come from a separate ``rocprofv3
--kernel-trace --stats`` run of this script.

Usage:  python tools/history_timing.py [--reps 5] [--json profiles/history_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.fitting import chain_history, lightcurve_mcmc  # noqa: E402

PASSES = 3   # the steps pass, the range pass and the raster pass each read every kept row once


def lc_case():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'config2.npz'))
    return {'MJD': g['cfg2__t'], 'filter': [str(n) for n in g['cfg2__names']], 'lum': g['cfg2__y'], 'dlum': g['cfg2__dy']}


PRIORS = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.5)]
LO, HI = [1., 0.3, 2., 1.5, 0.], [1.5, 0.7, 4., 2.5, 0.2]


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def numpy_history(x, lp, res):
    """The host route on the chain ``x`` (n_t, n_w, n_dim) and ``lp`` (n_t, n_w), on the bins of ``res``: ``(bands,
    log-probability bands, moves, raster, ms of the three parts)``."""
    t0 = time.perf_counter()
    bands = np.percentile(x, res.percentiles, axis=1)
    lp_bands = np.percentile(lp, res.percentiles, axis=1)
    t1 = time.perf_counter()
    bits = x.view(np.int64)
    moved = np.concatenate([[-1], np.any(bits[1:] != bits[:-1], axis=2).sum(axis=1)])
    t2 = time.perf_counter()
    e = res.step_edges
    counts = np.array([[np.histogram(x[a:b, :, d].ravel(), bins=res.edges[d])[0] for a, b in zip(e[:-1], e[1:])]
                       for d in range(x.shape[2])])
    t3 = time.perf_counter()
    return bands, lp_bands, moved, counts, [1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)]


def run(reps, walkers, steps, burnin):
    lc, model = lc_case(), M.ShockCooling(redshift=0.)
    sampler = lightcurve_mcmc(lc, model, priors=PRIORS, p_lo=LO, p_up=HI, nwalkers=walkers, nsteps=steps,
                              nsteps_burnin=burnin, seed=1)
    # the device route, while the chain is still where the run left it
    got = chain_history(model, sampler)                                                 # (warm-up)
    gpu_ms = median_ms(lambda: chain_history(model, sampler), reps)
    assert sampler._chain_on_device == steps and len(sampler._chain_host) == 0          # nothing was downloaded

    # the host route: the download (once), then NumPy
    t0 = time.perf_counter()
    x, lp = sampler.get_chain(), sampler.get_log_prob()
    download_ms = 1e3 * (time.perf_counter() - t0)
    bands, lp_bands, moved, counts, _ = numpy_history(x, lp, got)                        # (warm-up, and the comparison)
    equal = bool(np.array_equal(got.quantiles, bands) and np.array_equal(got.log_prob_quantiles, lp_bands)
                 and np.array_equal(got.n_moved, moved) and np.array_equal(got.counts, counts))
    assert equal, 'the numbers of the two routes differ'
    parts = np.median([numpy_history(x, lp, got)[4] for _ in range(max(1, min(reps, 3)))], axis=0)
    chain_bytes = x.size * 8 + lp.size * 8
    res = {'walkers': walkers, 'steps': steps, 'columns': sampler.ndim, 'percentiles': len(got.percentiles),
           't_bins': int(got.counts.shape[1]), 'v_bins': int(got.counts.shape[2]), 'chain_MB': chain_bytes / 1e6,
           'ms': gpu_ms, 'chain_bytes_read_per_s': PASSES * chain_bytes / (gpu_ms * 1e-3), 'download_ms': download_ms,
           'numpy_percentile_ms': float(parts[0]), 'numpy_moves_ms': float(parts[1]),
           'numpy_histogram_ms': float(parts[2]), 'numpy_route_ms': download_ms + float(parts.sum()),
           'equal_numbers': equal, 'accepted_per_step_mean': float(got.n_moved[1:].mean())}
    res['ratio_numpy_over_gpu'] = res['numpy_route_ms'] / gpu_ms
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--small', action='store_true', help='tiny shapes (a quick check of the script itself)')
    a = ap.parse_args()
    res = run(a.reps, 64, 200, 50) if a.small else run(a.reps, 1024, 2000, 1000)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
