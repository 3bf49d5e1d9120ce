#!/usr/bin/env python3
"""Cost of ``posterior_corner()`` after a fit, on the GPU, next to the only route there was before it.

After the configs[1]-shaped fit (ShockCooling, 1024 walkers, 2000 stored steps after 1000 of burn-in, through
``lightcurve_mcmc``) every histogram of the corner plot -- 5 marginals and 10 pairs at 20 bins -- is counted (a) over the
whole chain, 2 048 000 samples read where they lie in device memory, and (b) at ``thin=100`` (20 480 samples).  The
earlier route -- ``get_chain(flat=True)`` (the chain over PCIe), ``np.histogram`` per column and ``np.histogram2d``
per pair on the host -- is then timed on the same samples, download included, and every count of both routes is
asserted equal.  Every number is a host clock around a call that returns host arrays (the device work is complete when
it returns); each is the median of ``--reps`` calls after one warm-up call, the download (which happens once) the one
call there is.  The bytes of chain read per second -- both passes -- stand next to the HBM peak of the MI355X
(8 TB/s).  Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.

Usage:  python tools/corner_timing.py [--reps 5] [--json profiles/corner_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.fitting import lightcurve_mcmc, posterior_corner  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8e12
PASSES = 2   # the range pass and the histogram pass each read every kept row once


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


def numpy_corner(flat, res):
    """The host route on the rows ``flat``: the offset, then one NumPy call per panel on the ranges of ``res``."""
    x = flat - res.offsets if np.any(res.offsets) else flat
    bins, n_dim = res.hist1d.shape[1], x.shape[1]
    t0 = time.perf_counter()
    h1 = [np.histogram(x[:, d], bins=bins, range=tuple(res.range[d]))[0] for d in range(n_dim)]
    t1 = time.perf_counter()
    h2 = {(a, b): np.histogram2d(x[:, b], x[:, a], bins=bins, range=[tuple(res.range[b]), tuple(res.range[a])])[0]
          for a in range(1, n_dim) for b in range(a)}
    t2 = time.perf_counter()
    return h1, h2, 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def equal_counts(res, h1, h2):
    return bool(np.array_equal(res.hist1d, h1) and all(np.array_equal(res.hist2d[a, b], h) for (a, b), h in h2.items()))


def run(reps, walkers, steps, burnin, thin):
    lc, model = lc_case(), M.ShockCooling(redshift=0.)
    sampler = lightcurve_mcmc(lc, model, priors=PRIORS, p_lo=LO, p_up=HI, nwalkers=walkers, nsteps=steps,
                              nsteps_burnin=burnin, seed=1)
    n_dim = sampler.ndim
    res = {'walkers': walkers, 'steps': steps, 'columns': n_dim, 'pairs': n_dim * (n_dim - 1) // 2, 'bins': 20,
           'hbm_peak_bytes_per_s': HBM_PEAK_BYTES_PER_S}

    # (a), (b): the device route, while the chain is still where the run left it
    full = posterior_corner(model, sampler)                                             # (warm-up)
    full_ms = median_ms(lambda: posterior_corner(model, sampler), reps)
    thinned = posterior_corner(model, sampler, thin=thin)
    thin_ms = median_ms(lambda: posterior_corner(model, sampler, thin=thin), reps)
    assert sampler._chain_on_device == steps and len(sampler._chain_host) == 0          # nothing was downloaded

    # the host route: the download (once), then NumPy per panel
    t0 = time.perf_counter()
    flat = sampler.get_chain(flat=True)
    download_ms = 1e3 * (time.perf_counter() - t0)
    assert len(flat) == full.n_samples == walkers * steps
    for tag, got, rows, ms in (('whole_chain', full, flat, full_ms),
                               ('thinned', thinned, sampler.get_chain(thin=thin, flat=True), thin_ms)):
        assert len(rows) == got.n_samples
        h1, h2, _, _ = numpy_corner(rows, got)                                          # (warm-up, and the comparison)
        equal = equal_counts(got, h1, h2)
        assert equal, f'{tag}: the counts of the two routes differ'
        t1d, t2d = [], []
        for _ in range(max(1, min(reps, 3))):
            _, _, a, b = numpy_corner(rows, got)
            t1d.append(a)
            t2d.append(b)
        t1d, t2d = float(np.median(t1d)), float(np.median(t2d))
        chain_bytes = rows.size * 8
        entry = {'samples': got.n_samples, 'ms': ms, 'chain_MB': chain_bytes / 1e6,
                 'chain_bytes_read_per_s': PASSES * chain_bytes / (ms * 1e-3),
                 'fraction_of_hbm_peak': PASSES * chain_bytes / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S,
                 'numpy_histogram_ms': t1d, 'numpy_histogram2d_ms': t2d, 'equal_counts': equal}
        if tag == 'whole_chain':
            entry['download_ms'] = download_ms
            entry['numpy_route_ms'] = download_ms + t1d + t2d
        else:   # (the thinned rows are a slice of the chain already on the host)
            entry['numpy_route_ms_without_download'] = t1d + t2d
            entry['numpy_route_ms'] = download_ms + t1d + t2d
        entry['ratio_numpy_over_gpu'] = entry['numpy_route_ms'] / ms
        res[tag] = entry
    res['thinned']['thin'] = thin
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--small', action='store_true', help='tiny shapes (a quick check of the script itself)')
    a = ap.parse_args()
    res = run(a.reps, 64, 200, 50, 10) if a.small else run(a.reps, 1024, 2000, 1000, 100)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
