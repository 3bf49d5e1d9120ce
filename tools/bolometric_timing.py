#!/usr/bin/env python3
"""Phase timings of ``bolometric.calculate_bolometric`` on the GPU, next to the host's NumPy / scipy for the same phases.

Phases: host grouping and binning (group_by_epoch + calcFlux / bin / calcMag / calcAbsMag / calcLum), the least-squares
launch (k_bb_lstsq, with the k_bb_lum call for the optimum's L), the population MCMC, the luminosity launch over every
chain sample (k_bb_lum), and the percentiles / table.  Host comparisons: scipy's curve_fit per epoch (the reference's
blackbody_lstsq arithmetic; skipped when scipy does not import) and the host pseudo() over the same samples.

Usage:  python tools/bolometric_timing.py [--epochs 2000] [--json out.json]
Light curves: the included SN 2016bkv (tests/golden/config1.npz, dm = 30.79, z = 0.002) and a synthetic one of
``--epochs`` epochs in UBVgri.  Every number is a host clock around work that ends in a device synchronise."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import bolometric as B  # noqa: E402
from lightcurve_fitting_amd.filters import c1, c2, filtdict  # noqa: E402
from lightcurve_fitting_amd.lightcurve import LC  # noqa: E402
from lightcurve_fitting_amd.models import Blackbody, LogUniformPrior, UniformPrior  # noqa: E402
from lightcurve_fitting_amd.sampler import PopulationSampler  # noqa: E402


def sn2016bkv():
    c = np.load(os.path.join(ROOT, 'tests', 'golden', 'config1.npz'))
    return LC({'MJD': c['cfg1__MJD'], 'mag': c['cfg1__mag'], 'dmag': c['cfg1__dmag'], 'filter': c['cfg1__filter'],
               'nondet': c['cfg1__nondet'], 'source': c['cfg1__source']}, meta={'dm': 30.79, 'redshift': 0.002})


def synthetic(n_epochs, seed=0):
    rng = np.random.default_rng(seed)
    names = ['U', 'B', 'V', 'g', 'r', 'i']
    days = 100. + 1.5 * np.arange(n_epochs)
    T = 12. * np.exp(-(days - 100.) / 400.) + 5.
    R = 1. + 0.02 * (days - 100.)
    mjd = np.repeat(days, len(names)) + rng.uniform(-0.1, 0.1, n_epochs * len(names))
    filt = names * n_epochs
    nu = np.array([filtdict[n].freq_eff for n in filt])
    lum = c2 * np.repeat(R, 6) ** 2 * nu ** 3 / np.expm1(c1 * nu / np.repeat(T, 6))
    lum *= 1 + 0.05 * rng.standard_normal(len(lum))
    mag = np.array([filtdict[n].m0 for n in filt]) + 90.19 - 2.5 * np.log10(lum)
    return LC({'MJD': mjd, 'mag': mag, 'dmag': np.full(len(mag), 0.054), 'filter': filt}, meta={'dm': 0.})


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def phases(lc, nwalkers=10, burnin=200, steps=100, seed=1):
    z = lc.meta.get('redshift', 0.)
    r = {}

    def prep():
        sub = lc[np.isfinite(lc['dmag']) & (lc['dmag'] > 0.)]
        eps = [B._prepare_epoch(e) for e in B.group_by_epoch(sub)]
        return [e for e in eps if len(set(e.where(nondet=False)['filter'])) >= 3]
    epochs, r['host_group_bin_s'] = clock(prep)
    r['epochs'] = len(epochs)
    B.blackbody_lstsq_epochs(epochs[:1], z)    # (warm-up: code objects, device context)
    ls, r['k_bb_lstsq_s'] = clock(lambda: B.blackbody_lstsq_epochs(epochs, z))
    r['lstsq_converged'] = int(np.sum(ls['status'] > 0))
    r['lstsq_iterations_max'] = int(ls['niter'].max())
    p0 = np.column_stack([ls['temp'], ls['radius']])
    p0[~np.isfinite(p0)] = 10.

    def mcmc():
        rng = np.random.default_rng(seed)
        priors = [UniformPrior(1., 100.), LogUniformPrior(0.01, 1000.)]
        problems = [(Blackbody(redshift=z), {'MJD': np.zeros(len(e)), 'filter': list(e['filter']), 'lum': e['lum'],
                                             'dlum': e['dlum']}, priors) for e in epochs]
        x0 = {k: np.maximum(rng.normal(size=(nwalkers, 2)) + p0[k], 1.) for k in range(len(epochs))}
        pop = PopulationSampler(problems, nwalkers, seed=seed)
        pop.run_mcmc(x0, burnin, store=False)
        for s in pop.samplers.values():
            s.reset()
        pop.run_mcmc(None, steps)
        return np.stack([pop[k].flatchain for k in range(len(epochs))])
    chains, r['mcmc_s'] = clock(mcmc)
    r['samples'] = int(chains.shape[0] * chains.shape[1])
    B.luminosity_samples(chains[:1, :10, 0], chains[:1, :10, 1], z)
    (Lp, Lb), r['k_bb_lum_s'] = clock(lambda: B.luminosity_samples(chains[:, :, 0], chains[:, :, 1], z))

    def table():
        B.median_and_unc(np.moveaxis(chains, 1, 0))
        B.median_and_unc(Lp.T), B.median_and_unc(Lb.T)
        return [B.integrate_sed(e) for e in epochs]
    _, r['percentiles_table_s'] = clock(table)
    # host comparisons for the same phases
    flat_T, flat_R = chains[:, :, 0].ravel(), chains[:, :, 1].ravel()
    n_host = min(len(flat_T), 200000)
    _, t = clock(lambda: B.pseudo(flat_T[:n_host], flat_R[:n_host], z))
    r['host_pseudo_s'] = t * len(flat_T) / n_host
    r['host_pseudo_extrapolated_from'] = n_host
    try:
        from scipy.optimize import curve_fit

        def host_lstsq():
            for e in epochs:
                def planck(nu, T, R):
                    return c2 * R ** 2 * nu ** 3 / np.expm1(c1 * nu / T)
                try:
                    curve_fit(planck, e['freq'] * (1 + z), e['lum'], p0=(10., 10.), bounds=([1., 0.01], [100., 1000.]))
                except RuntimeError:
                    pass
        _, r['host_curve_fit_s'] = clock(host_lstsq)
    except ImportError:
        r['host_curve_fit_s'] = None
    _, r['calculate_bolometric_s'] = clock(lambda: B.calculate_bolometric(lc, seed=seed))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=2000)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import warnings
    warnings.simplefilter('ignore')
    res = {'SN2016bkv': phases(sn2016bkv()), f'synthetic_{args.epochs}': phases(synthetic(args.epochs))}
    for k, v in res.items():
        print(k, json.dumps(v))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
