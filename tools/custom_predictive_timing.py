#!/usr/bin/env python3
"""Cost of ``custom_predictive()`` after a fit of a custom model, on the GPU, next to the only route there was before it.

The chain is a REAL fit: the README's temperature-floor model (``CustomModel``) on the configs[1] light curve (3000
points) through ``TemperedSampler(betas=[1.])`` with 1024 walkers, 2000 stored steps after 300 of burn-in.  The bands
of the six filters' light curves and of T, R and L on 1000 times are timed (a) over the whole chain, 2 048 000 samples --
2e9 calls of the state function, 1.2e10 band luminosities, 1.8e10 keys -- and (b) at ``thin=100`` (20 480 samples),
where the earlier route -- ``model(t, filters, *flat.T)`` (every value over PCIe), ``model.temperature_radius``,
``stefan_boltzmann`` and ``np.nanpercentile`` on the host -- is timed on the same samples and the results are compared.
At (b) both routes are medians of ``--reps`` ALTERNATING repetitions after one warm-up each, with their ranges.  The
whole-chain rate, in band luminosities per second, is given next to the rate ``profiles/custom_timing.json`` implies for
the likelihood kernel of the ShockCooling2 restatement (4096 rows x 3000 points in 0.358 ms: one call of the state
function AND one band luminosity per point; the floor model's function is that one plus an ``fmax``).  There is no gate
on any of it.  Every number is a host clock around a call that returns host arrays.

``lcf_custom_keys``'s share of the device time comes from a separate ``rocprofv3 --kernel-trace --stats`` run of this
script with ``--profile`` (the fit and ONE whole-chain call, nothing else), whose kernel statistics ``--kernel-stats``
folds into the result.

Usage:  python tools/custom_predictive_timing.py [--reps 5] [--kernel-stats stats.csv]
                                                 [--json profiles/custom_predictive_timing.json]"""
import argparse
import csv
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.bolometric import stefan_boltzmann  # noqa: E402
from lightcurve_fitting_amd.fitting import custom_predictive  # noqa: E402
from lightcurve_fitting_amd.sampler import TemperedSampler  # noqa: E402

# the README's example ("A model of your own"): the ShockCooling2 luminosity law with a temperature floor
SOURCE = r'''
__device__ void lcf_user_state(double t_in, const double* p, const double* consts, double z,
                               double& T_kK, double& R_1000Rsun) {
    const double t = t_in - p[3];                                        // p = T_1, L_1, t_tr, t_0, T_floor
    T_kK = fmax(p[0] * lcf::pw(t, 2. * consts[3] - 0.5), p[4]);          // consts = A, a, alpha, eps_1, eps_2
    const double L = p[1] * exp(-lcf::pw(consts[1] * t / p[2], consts[2])) * lcf::pw(t, -2. * consts[4]) * 1e42;
    R_1000Rsun = lcf::kC3 * sqrt(L) * lcf::pw(T_kK, -2.);
}
'''
NAMES = ['T_1', 'L_1', 't_\\mathrm{tr}', 't_0', 'T_\\mathrm{floor}']
PRIORS = [M.UniformPrior(0., 100.), M.UniformPrior(0., 100.), M.UniformPrior(0., 100.), M.UniformPrior(-1., 0.5),
          M.UniformPrior(0., 5.)]
LO, HI = np.array([15., 1., 5., 0., 0.5]), np.array([25., 3., 15., 0.2, 2.])
T_FLOOR = 1.                                          # [kK] the floor asked about: samples colder than it per time
LIKELIHOOD_POINTS_PER_S = 4096 * 3000 / 0.358e-3      # profiles/custom_timing.json: lcf_log_likelihood_dev, custom


def lc_case():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'config2.npz'))
    return {'MJD': g['cfg2__t'], 'filter': [str(n) for n in g['cfg2__names']], 'lum': g['cfg2__y'], 'dlum': g['cfg2__dy']}


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def summary(ms):
    return {'median': float(np.median(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms)), 'runs': [float(v) for v in ms]}


def rel_diff(got, want):
    with np.errstate(all='ignore'):
        d = np.abs(got - want) / np.abs(want)
    return float(np.nanmax(np.where(got == want, 0., d)))


def kernel_split(path):
    """Device time of one whole-chain call by kernel, from the kernel statistics of a rocprofv3 run with --profile."""
    names = ('lcf_custom_keys', 'k_kq_pass', 'k_pq_pick', 'k_pq_finish')
    ns = dict.fromkeys(names, 0)
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            for name in names:
                if name in row['Name']:
                    ns[name] += int(float(row['TotalDurationNs']))
    total = sum(ns.values())
    return {'ns': ns, 'call_kernels_ms': total / 1e6, 'lcf_custom_keys_share': ns['lcf_custom_keys'] / total if total else None}


def fit(walkers, steps, burnin):
    lc = lc_case()
    consts = M.ShockCooling2(redshift=0.)._consts()[:5]
    model = M.CustomModel(SOURCE, NAMES, consts=consts, redshift=0.)
    sampler = TemperedSampler(walkers, 5, model.engine_for(lc, priors=PRIORS), betas=[1.], seed=1)
    x0 = LO + (HI - LO) * np.random.default_rng(1).random((1, walkers, 5))
    sampler.run_mcmc(x0, burnin, store=False)
    sampler.run_mcmc(None, steps)
    return lc, model, sampler


def run(reps, walkers, steps, burnin, num, thin):
    lc, model, sampler = fit(walkers, steps, burnin)
    res = {'model': 'CustomModel: ShockCooling2 luminosity law with a temperature floor (README)',
           'chain': 'TemperedSampler, one rung at beta = 1', 'walkers': walkers, 'steps': steps, 'times': num, 'reps': reps,
           'T_floor_kK': T_FLOOR, 'likelihood_kernel_points_per_s': LIKELIHOOD_POINTS_PER_S}
    kw = dict(num=num, T_floor=T_FLOOR)

    full = custom_predictive(lc, model, sampler, **kw)                                 # (warm-up: the grid engine)
    ms = [timed_ms(lambda: custom_predictive(lc, model, sampler, **kw)) for _ in range(reps)]
    nf, nt = len(full.filters), len(full.t)
    states, values = full.n_samples * nt, full.n_samples * nt * nf
    rate = values / (np.median(ms) * 1e-3)
    res['whole_chain'] = {'samples': full.n_samples, 'filters': nf, 'state_evaluations': states, 'band_luminosities': values,
                          'keys': full.n_samples * nt * (nf + 3), 'ms': summary(ms), 'band_luminosities_per_s': rate,
                          'state_evaluations_per_s': states / (np.median(ms) * 1e-3),
                          'share_of_likelihood_kernel_rate': rate / LIKELIHOOD_POINTS_PER_S,
                          'max_frac_cold': float(np.nanmax(full.frac_cold))}

    flat = np.ascontiguousarray(sampler.get_chain(thin=thin, flat=True))
    names = [f.name for f in full.filters]

    def new_route():
        return custom_predictive(lc, model, flat, **kw)

    def old_route():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            T, R = model.temperature_radius(full.t, *flat.T)       # (num, S) each
            Y = model(full.t, names, *flat.T)                      # (nf, num, S) float64 across PCIe; the model keeps
            q = full.percentiles                                   # ONE evaluation grid: the one new_route wants, last
            return (np.nanpercentile(Y, q, axis=-1), np.nanpercentile(T, q, axis=-1), np.nanpercentile(R, q, axis=-1),
                    np.nanpercentile(stefan_boltzmann(T, R), q, axis=-1), np.sum(T < T_FLOOR, axis=-1))
    thinned = new_route()
    want = old_route()
    assert len(flat) == thinned.n_samples
    errs = {name: rel_diff(getattr(thinned, name), w)
            for name, w in zip(('quantiles', 'temperature', 'radius', 'luminosity'), want)}
    assert max(errs.values()) <= 1e-10, errs
    assert np.array_equal(thinned.n_cold, want[4])
    new_ms, old_ms = [], []
    for _ in range(reps):          # alternating: both see the same drift of the machine
        new_ms.append(timed_ms(new_route))
        old_ms.append(timed_ms(old_route))
    values = thinned.n_samples * nt * nf
    res['thinned'] = {'thin': thin, 'samples': thinned.n_samples, 'band_luminosities': values, 'ms': summary(new_ms),
                      'band_luminosities_per_s': values / (np.median(new_ms) * 1e-3),
                      'evaluate_plus_temperature_radius_plus_nanpercentile_ms': summary(old_ms),
                      'ratio_old_over_new': float(np.median(old_ms) / np.median(new_ms)),
                      'ranges_disjoint': bool(max(new_ms) < min(old_ms)),
                      'max_rel_diff': errs, 'values_the_old_route_moves_MB': thinned.n_samples * nt * (nf + 2) * 8 / 1e6}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--kernel-stats', default=None, help='kernel statistics (CSV) of a rocprofv3 --kernel-trace --stats run '
                                                         'of this script with --profile')
    ap.add_argument('--profile', action='store_true', help='the fit and ONE whole-chain call, for the profiler')
    ap.add_argument('--small', action='store_true', help='tiny shapes (a quick check of the script itself)')
    a = ap.parse_args()
    shape = (64, 200, 50, 50, 10) if a.small else (1024, 2000, 300, 1000, 100)
    if a.profile:
        lc, model, sampler = fit(*shape[:3])
        print(custom_predictive(lc, model, sampler, num=shape[3], T_floor=T_FLOOR))
        return
    res = run(a.reps, *shape)
    if a.kernel_stats:
        res['whole_chain']['device_time'] = kernel_split(a.kernel_stats)
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
