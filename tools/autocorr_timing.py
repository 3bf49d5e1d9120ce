#!/usr/bin/env python3
"""Cost of ``get_autocorr_time()`` after a fit, on the GPU, next to what it replaces.

Two workloads: the configs[1]-shaped fit (ShockCooling, 1024 walkers, 2000 steps after 1000 of burn-in, through
``lightcurve_mcmc``) and a population of 32 transients x 512 walkers x 2000 steps.  For each: the device call on the
chain in HBM (``get_autocorr_time``), ``get_chain()`` alone (the copy over PCIe the call avoids) and emcee's estimator
restated in NumPy (one FFT per walker and parameter) on that chain.  Every GPU number is a host clock around work that
ends in a device synchronise; each is the median of ``--reps`` calls after one warm-up call.  Kernel times come from a
separate ``rocprofv3 --kernel-trace --stats`` run of this script.

Usage:  python tools/autocorr_timing.py [--reps 5] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.fitting import lightcurve_mcmc  # noqa: E402
from lightcurve_fitting_amd.sampler import PopulationSampler  # noqa: E402


def numpy_integrated_time(x, c=5.):
    """emcee's estimator in NumPy (zero-padded FFT per walker and parameter), without the tol check."""
    n_t, n_w, n_d = x.shape
    n = 1 << int(np.ceil(np.log2(n_t)))
    tau = np.empty(n_d)
    for d in range(n_d):
        f = np.zeros(n_t)
        for k in range(n_w):
            y = x[:, k, d]
            g = np.fft.fft(y - y.mean(), n=2 * n)
            acf = np.fft.ifft(g * np.conjugate(g))[:n_t].real
            f += acf / acf[0]
        f /= n_w
        taus = 2. * np.cumsum(f) - 1.
        m = np.arange(n_t) < c * taus
        tau[d] = taus[np.argmin(m) if np.any(m) else n_t - 1]
    return tau


def lc_case():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'shockcooling.npz'))
    return {'MJD': g['scb__t'], 'filter': [str(n) for n in g['scb__names']], 'lum': g['scb__y'], 'dlum': g['scb__dy']}


PRIORS = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.2)]
LO, HI = [1., 0.5, 2., 1., -0.5], [2., 1.5, 4., 3., 0.]


def median_ms(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def single(reps, walkers, steps, burnin):
    sampler = lightcurve_mcmc(lc_case(), M.ShockCooling(redshift=0.01), priors=PRIORS, p_lo=LO, p_up=HI,
                              nwalkers=walkers, nsteps=steps, nsteps_burnin=burnin, seed=1)
    tau = sampler.get_autocorr_time(tol=0)                              # (warm-up)
    dev_ms = median_ms(lambda: sampler.get_autocorr_time(tol=0), reps)
    assert sampler._chain_on_device == steps
    copy_ms = median_ms(lambda: sampler._native.get_chain(), reps)          # the copy get_chain() makes
    chain = sampler.get_chain()
    t0 = time.perf_counter()
    ref = numpy_integrated_time(chain)
    np_ms = 1e3 * (time.perf_counter() - t0)
    return {'walkers': walkers, 'steps': steps, 'chain_MB': chain.nbytes / 1e6, 'tau': tau.tolist(),
            'max_rel_vs_numpy': float(np.max(np.abs(tau - ref) / np.abs(ref))), 'get_autocorr_time_ms': dev_ms,
            'get_chain_ms': copy_ms, 'numpy_ms': np_ms, 'numpy_over_device': np_ms / dev_ms,
            'copy_over_device': copy_ms / dev_ms}


def population(reps, n_trans, walkers, steps):
    lc = lc_case()
    problems = [(M.ShockCooling(redshift=0.01 + 0.001 * k), lc, PRIORS) for k in range(n_trans)]
    rng = np.random.default_rng(2)
    x0 = {k: rng.uniform(LO, HI, (walkers, 5)) for k in range(n_trans)}
    pop = PopulationSampler(problems, walkers, seed=5)
    pop.run_mcmc(x0, 1000, store=False)
    pop.run_mcmc(None, steps)
    pop.get_autocorr_time(tol=0)
    dev_ms = median_ms(lambda: pop.get_autocorr_time(tol=0), reps)
    copy_ms = median_ms(lambda: [s._native.get_chain() for s in pop.samplers.values()], reps)
    t0 = time.perf_counter()
    numpy_integrated_time(pop[0].get_chain())
    np_one_ms = 1e3 * (time.perf_counter() - t0)
    return {'transients': n_trans, 'walkers': walkers, 'steps': steps, 'get_autocorr_time_ms': dev_ms,
            'get_chain_all_ms': copy_ms, 'numpy_ms_estimated': np_one_ms * n_trans,
            'numpy_over_device': np_one_ms * n_trans / dev_ms, 'copy_over_device': copy_ms / dev_ms}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--small', action='store_true', help='tiny shapes (a quick check of the script itself)')
    a = ap.parse_args()
    if a.small:
        res = {'single': single(a.reps, 64, 200, 50), 'population': population(a.reps, 3, 64, 200)}
    else:
        res = {'single': single(a.reps, 1024, 2000, 1000), 'population': population(a.reps, 32, 512, 2000)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
