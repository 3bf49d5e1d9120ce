#!/usr/bin/env python3
"""Golden vectors of the bolometric workflow (tests/golden/bolometric.npz), from the REFERENCE's own functions.

Imports the reference through the stand-ins of ``make_golden.py`` and calls ``bolometric.blackbody_lstsq``,
``integrate_sed``, ``calc_colors``, ``median_and_unc`` and ``lightcurve.binflux`` on synthetic inputs and on the
SN 2016bkv light curve of ``tests/golden/config1.npz``.  ``curve_fit`` inside the reference's module is wrapped only
to record the covariance it returns (the 7-tuple leaves out cov_TR).  Only data go into the fixture.

Usage:  python tools/refgen/make_golden_bolometric.py [--ref /root/reference]
"""
import argparse
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import GOLD, import_reference  # noqa: E402

NAMES = ['U', 'B', 'V', 'g', 'r', 'i', 'UVW1', 'UVM2', 'UVW2']


def table(Table, filters, names, **cols):
    """Stand-in table with a ``filter`` column of the reference's Filter objects and a ``where(filter=)``."""

    class Epoch(Table):
        def where(self, filter=None):
            return Sel(self, np.array([x == filter for x in self['filter']]))

    class Sel:   # epoch1.where(filter=f)[['absmag', 'dmag', 'nondet']][0] -> (absmag, dmag, nondet) of the first row
        def __init__(self, t, mask):
            self.t, self.mask = t, mask

        def __getitem__(self, keys):
            return [tuple(np.asarray(self.t[k])[self.mask][i] for k in keys) for i in range(int(self.mask.sum()))]

    t = Epoch()
    fobj = np.empty(len(names), dtype=object)
    fobj[:] = [filters.filtdict[n] for n in names]
    t['filter'] = fobj
    for k, v in cols.items():
        t[k] = np.asarray(v)
    return t


def gen_lstsq(bolometric, filters, models, Table, out, n=300):
    import scipy.optimize
    record = []

    def recording_curve_fit(*args, **kwargs):
        popt, pcov = scipy.optimize.curve_fit(*args, **kwargs)
        record.append(pcov)
        return popt, pcov
    bolometric.curve_fit = recording_curve_fit
    rng = np.random.default_rng(2024)
    ep_off, freq, lum, names_all = [0], [], [], []
    rows = []   # z, cutoff, p0 T, p0 R, T_lo, R_lo, T_hi, R_hi, T_true, R_true
    res = []    # temp, radius, dtemp, drad, lum, dlum, L_opt, covTR, cost
    for k in range(n):
        m = 2 if k % 50 == 7 else int(rng.integers(3, 10))
        names = list(rng.choice(NAMES, m, replace=False))
        T0, R0 = rng.uniform(3., 40.), np.exp(rng.uniform(np.log(0.3), np.log(50.)))
        z = (0., 0.03)[k % 2]
        cut = (np.inf, 700.)[(k // 2) % 2]
        T_range, R_range, p0 = (1., 100.), (0.01, 1000.), (10., 10.)
        if k % 25 == 11:        # optimum on the upper temperature bound
            T_range, p0 = (1., 0.5 * T0), (0.25 * T0, 10.)
        f = np.array([filters.filtdict[x].freq_eff.value for x in names])
        y = models.planck_fast(f * (1. + z), T0, R0, cut) * (1. + 0.05 * rng.standard_normal(m))
        if k % 7 == 3 and m > 3:   # a non-detection row
            y[int(rng.integers(m))] = 0.
        ep = table(Table, filters, names, freq=f, lum=y)
        try:
            r = bolometric.blackbody_lstsq(ep, z, p0, T_range, R_range, cut)
            pcov = record[-1]
            cost = 0.5 * np.sum((models.planck_fast(f * (1. + z), r[0], r[1], cut) - y) ** 2)
            res.append(list(r) + [pcov[0, 1], cost])
        except RuntimeError:
            res.append([np.nan] * 9)
        rows.append([z, cut, *p0, T_range[0], R_range[0], T_range[1], R_range[1], T0, R0])
        ep_off.append(ep_off[-1] + m)
        freq.extend(f)
        lum.extend(y)
        names_all.extend(names)
    out['ls/ep_off'] = np.array(ep_off)
    out['ls/freq'] = np.array(freq)
    out['ls/lum'] = np.array(lum)
    out['ls/filter'] = np.array(names_all)
    out['ls/setup'] = np.array(rows)
    out['ls/result'] = np.array(res)


def gen_host(bolometric, filters, Table, out, n=60):
    rng = np.random.default_rng(7)
    colors = ['U-B', 'B-V', 'g-r', 'r-i', 'UVW2-V']
    out['host/colors'] = np.array(colors)
    ep_off, names_all, lum, absmag, dmag, nondet = [0], [], [], [], [], []
    L_int, cm, cd, clo, cup = [], [], [], [], []
    for k in range(n):
        m = int(rng.integers(2, 9))
        names = list(rng.choice(NAMES, m, replace=False))
        y = rng.uniform(1e19, 1e21, m)
        am = rng.uniform(-19., -15., m)
        dm = rng.uniform(0.01, 0.2, m)
        nd = rng.uniform(size=m) < 0.2
        dm[nd] = np.nan
        f = np.array([filters.filtdict[x].freq_eff.value for x in names])
        df = np.array([filters.filtdict[x].dfreq.value for x in names])
        ep = table(Table, filters, names, freq=f, dfreq=df, lum=y, absmag=am, dmag=dm, nondet=nd)
        ep['freq'].unit = bolometric.u.THz
        ep['dfreq'].unit = bolometric.u.THz
        ep['lum'].unit = bolometric.u.W / bolometric.u.Hz
        c = bolometric.calc_colors(ep, colors)      # (before integrate_sed, which sorts the epoch in place)
        L_int.append(bolometric.integrate_sed(ep))
        cm.append(c[0]), cd.append(c[1]), clo.append(c[2]), cup.append(c[3])
        ep_off.append(ep_off[-1] + m)
        names_all.extend(names), lum.extend(y), absmag.extend(am), dmag.extend(dm), nondet.extend(nd)
    out['host/ep_off'] = np.array(ep_off)
    out['host/filter'] = np.array(names_all)
    for k, v in (('lum', lum), ('absmag', absmag), ('dmag', dmag), ('nondet', nondet)):
        out[f'host/{k}'] = np.array(v)
    out['host/L_int'] = np.array(L_int)
    out['host/color_mags'] = np.array(cm, dtype=float)
    out['host/color_dmags'] = np.array(cd, dtype=float)
    out['host/color_lolims'] = np.array(clo, dtype=bool)
    out['host/color_uplims'] = np.array(cup, dtype=bool)
    x = rng.lognormal(0., 1., (1000, 3))
    out['host/samples'] = x
    for p in (68., 95., 100.):
        out[f'host/median_and_unc_{p:g}'] = np.array(bolometric.median_and_unc(x, p))


def gen_binflux(lightcurve, filters, out):
    """binflux of SN 2016bkv's rows (tests/golden/config1.npz), grouped by (filter, source), at two bin sizes."""
    d = np.load(os.path.join(GOLD, 'config1.npz'))
    mjd, mag, dmag = d['cfg1__MJD'], d['cfg1__mag'], d['cfg1__dmag']
    names, src, nondet = d['cfg1__filter'], d['cfg1__source'], d['cfg1__nondet']
    zp = np.array([filters.filtdict[x].m0 for x in names])
    flux, dflux = lightcurve.mag2flux(mag, dmag, zp, nondet, 3.)
    out['bin/flux'], out['bin/dflux'] = flux, dflux
    keys = sorted(set(zip(names, src)))
    for delta in (0.3, np.inf):
        parts = []
        for j, (fn, s) in enumerate(keys):
            sel = (names == fn) & (src == s)
            t, f, df = lightcurve.binflux(mjd[sel], flux[sel], dflux[sel], delta)
            parts.append(np.column_stack([np.full(len(t), j), t, f, df]))
        out[f'bin/delta_{delta:g}'] = np.concatenate(parts)
    out['bin/key_filter'] = np.array([k[0] for k in keys])
    out['bin/key_source'] = np.array([k[1] for k in keys])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    args = ap.parse_args()
    models, filters, bolometric, lightcurve, Table = import_reference(args.ref)
    warnings.simplefilter('ignore')
    out = {}
    gen_lstsq(bolometric, filters, models, Table, out)
    gen_host(bolometric, filters, Table, out)
    gen_binflux(lightcurve, filters, out)
    path = os.path.join(GOLD, 'bolometric.npz')
    np.savez_compressed(path, **{k.replace('/', '__'): v for k, v in out.items()})
    print(f'bolometric: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB; '
          f'least squares failed on {int(np.isnan(out["ls/result"][:, 0]).sum())} of {len(out["ls/result"])} epochs')


if __name__ == '__main__':
    main()
