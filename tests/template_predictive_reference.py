"""Bands and features of a template fit in NumPy (a helper, not a test): the definition ``fitting.template_predictive`` is
held to, on top of ``template_reference``.

Per sample ``s``, filter ``f`` and grid time ``i``: ``B`` the base model's value (the oracle's, through
``limits_reference.model_values``), ``Tm = r_f S_f((t_i - t_max - dt_f) / s)`` (``template_reference.template_values``) and
``Y = B + Tm``.  The bands are ``np.nanpercentile`` over the samples; the features are plain loops over the times in
ascending order, per (sample, filter): the first occurrence always wins, comparisons are on values, a NaN never wins."""
import warnings

import numpy as np

import limits_reference as L
import template_reference as T
from oracle import lcf_oracle as O

FILTERS = T.FILTERS
GRID_T = np.array([0.05, 0.5, 1.5, 3., 5., 6.5, 8., 9.5, 11., 14., 20., 60.])
PERCENTILES = (0., 15.87, 50., 84.14, 100.)
KINDS = ('ShockCooling2', 'ShockCooling', 'ShockCooling4', 'ShockCooling3')
TEMPLATES = ('sifto', 'four', 'bump')
COMPONENTS = ('total', 'base', 'template')
# a base column whose NaN makes every base value of an exploded row NaN (the luminosity scale; the shock velocity): the
# reference's power() turns a NaN in most other columns into a zero or a finite light curve
NAN_COLUMN = {'ShockCooling2': 1, 'ShockCooling': 0, 'ShockCooling4': 0, 'ShockCooling3': 0}
_memo = {}


def grid_case(kind, template):
    """``template_reference.case`` with a template column for every one of the six filters: its own where the light
    curve has the filter, else the column scaled to an explicit peak (``scale``: what ``WithTemplate`` is then given)."""
    c = T.case(kind, template)
    names = np.asarray([str(n) for n in c['names']])
    peaks = {nm: (float(np.max(c['y'][names == nm])) if nm in c['scaled'] else 1e35) for nm in FILTERS}
    scaled = T.scaled_columns(c['template'], FILTERS, scale=peaks)
    for nm in c['scaled']:       # (the same expression on the same numbers)
        assert np.array_equal(scaled[nm], c['scaled'][nm])
    return dict(c, scaled=scaled, scale=None if all(nm in c['scaled'] for nm in FILTERS) else peaks)


def tiled_rows(c, n=2100, jitter=0., seed=7):
    """The case's 37 rows without sigma, repeated to ``n`` samples (every value then ties ``n / 37`` times), or every
    column jittered by a relative ``jitter`` (distinct values)."""
    P37 = T.rows(c, False)
    P = np.ascontiguousarray(P37[np.arange(n) % len(P37)])
    if jitter:
        P = P * (1. + jitter * np.random.default_rng(seed).uniform(-1., 1., P.shape))
    return P


def values(c, P, t=GRID_T, filters=FILTERS):
    """``(B, Tm, Y)``, each (nf, nt, n), of the rows ``P`` (n, n_par) on the dense grid."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    nf, nt, nb = len(filters), len(t), c['n_base']
    tt, nn = np.tile(np.asarray(t, dtype=np.float64), nf), np.repeat(list(filters), nt)
    with np.errstate(all='ignore'):
        B = L.model_values(c['base'], tt, [O.band(n) for n in nn], P[:, :nb])
        Tm = T.template_values(c['epochs'], c['scaled'], tt, nn, P, nb)
        Y = B + Tm
    return tuple(v.reshape(nf, nt, len(P)) for v in (B, Tm, Y))


def reference_values(kind, template, rows='tiled'):
    """The memoised ``(case, P, B, Tm, Y)`` of a case on the grid: ``rows`` is ``'plain'`` (the 37 rows), ``'tiled'``
    (2100 samples, ties), ``'jitter'`` (2100 distinct samples) or ``'nan'`` (the 37 rows and two more: one with a base
    column NaN, one with ``r_r`` NaN)."""
    key = (kind, template, rows)
    if key not in _memo:
        c = grid_case(kind, template)
        if rows == 'plain':
            P = T.rows(c, False)
        elif rows == 'nan':
            P37 = T.rows(c, False)
            exploded = int(np.argmax(P37[:, L.KINDS[kind][2]] < 0.))   # a row with t_0 < 0: on the whole grid
            P = np.concatenate([P37, P37[[exploded, 5]]])
            P[-2, NAN_COLUMN[kind]] = np.nan        # a base column
            P[-1, c['n_base'] + 2] = np.nan         # r_r
        else:
            P = tiled_rows(c, jitter=1e-3 if rows == 'jitter' else 0.)
        if rows == 'tiled':      # (the oracle once per distinct row)
            B, Tm, Y = (v[..., np.arange(len(P)) % T.N_ROWS] for v in values(c, T.rows(c, False)))
        else:
            B, Tm, Y = values(c, P)
        for v in (B, Tm, Y):
            v.setflags(write=False)
        _memo[key] = (c, P, B, Tm, Y)
    return _memo[key]


def bands(V, percentiles=PERCENTILES):
    """``(quantiles (nq, nf, nt), n_valid (nf, nt))`` of values ``V`` (nf, nt, n)."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)   # (every sample NaN: NaN)
        return np.nanpercentile(V, percentiles, axis=-1), np.sum(~np.isnan(V), axis=-1)


def n_dark(B):
    """(nf, nt): the samples whose base value is exactly ``+0.0``."""
    return np.sum((B == 0.) & ~np.signbit(B), axis=-1)


def features_of(b, tm):
    """The features of one (sample, filter): ``b``, ``tm`` (nt,) over ascending times.  Returns ``((y_peak_base,
    y_peak_template, y_dip), (i_peak_base, i_peak_template, i_cross, i_dip))``."""
    nan = float('nan')
    y_b, i_b, y_t, i_t, i_x = nan, -1, nan, -1, -1
    for i in range(len(b)):
        if b[i] == b[i] and (i_b < 0 or b[i] > y_b):
            y_b, i_b = b[i], i
        if tm[i] == tm[i] and (i_t < 0 or tm[i] > y_t):
            y_t, i_t = tm[i], i
        if i_x < 0 and tm[i] > b[i]:
            i_x = i
    y_d, i_d = nan, -1
    if 0 <= i_b < i_t:
        for i in range(i_b, i_t + 1):
            y = b[i] + tm[i]
            if y == y and (i_d < 0 or y < y_d):
                y_d, i_d = y, i
    return (y_b, y_t, y_d), (i_b, i_t, i_x, i_d)


def features(B, Tm):
    """``(values (3, nf, n), indices (4, nf, n) int32)`` of ``B``, ``Tm`` (nf, nt, n)."""
    nf, _, n = B.shape
    vals, idx = np.empty((3, nf, n)), np.empty((4, nf, n), dtype=np.int32)
    with np.errstate(all='ignore'):
        for f in range(nf):
            for s in range(n):
                vals[:, f, s], idx[:, f, s] = features_of(B[f, :, s].tolist(), Tm[f, :, s].tolist())
    return vals, idx


def features_brute(B, Tm):
    """The same, restated with array operations (what ``features`` is checked against)."""
    nf, nt, n = B.shape
    vals, idx = np.full((3, nf, n), np.nan), np.full((4, nf, n), -1, dtype=np.int32)
    steps = np.arange(nt)
    with np.errstate(all='ignore'):
        Y = B + Tm
        for f in range(nf):
            for s in range(n):
                b, tm, y = B[f, :, s], Tm[f, :, s], Y[f, :, s]
                for k, v in ((0, b), (1, tm)):
                    ok = ~np.isnan(v)
                    if ok.any():
                        vals[k, f, s] = np.max(v[ok])
                        idx[k, f, s] = steps[ok & (v == vals[k, f, s])][0]
                above = steps[tm > b]
                if len(above):
                    idx[2, f, s] = above[0]
                lo, hi = idx[0, f, s], idx[1, f, s]
                if 0 <= lo < hi:
                    inside = (steps >= lo) & (steps <= hi) & ~np.isnan(y)
                    if inside.any():
                        vals[2, f, s] = np.min(y[inside])
                        idx[3, f, s] = steps[inside & (y == vals[2, f, s])][0]
    return vals, idx
