"""A shock model plus a stretched template in NumPy (a helper, not a test): the definition ``models.WithTemplate`` is
held to.

At a data point ``j`` of filter ``f``::

    m_j(p)  = base_j(p_base) + r_f * S_f((t_j - t_max - dt_f) / s)
    ln L(p) = -1/2 sum_j [ln(2 pi sigma_j^2) + ((y_j - m_j) / sigma_j)^2]          (models.py:116-136)

``S_f`` is ``scipy.interpolate.CubicSpline(epochs, scaled_f, extrapolate=False)`` with NaN (outside the epochs, or a NaN
argument) mapped to 0 -- what the reference does with SiFTO (models.py:717, 816-826); ``scaled_f`` the template column
of ``f`` times ``max(y over the filter's rows) / max(column)`` (models.py:701-717), or times an explicit peak value.  The
base model's values are the oracle's, through ``limits_reference.model_values``.  Rows are ``[base ..., t_max, s,
r_X for X in factors ..., dt_X for X in offsets ..., (sigma)]``."""
import numpy as np
from scipy.interpolate import CubicSpline

import limits_reference as L
from oracle import lcf_oracle as O

Z = L.Z
FILTERS = L.FILTERS
N_ROWS = L.N_ROWS
FACTORS, OFFSETS = ('r',), ('U',)
T_MAX, STRETCH = 8., 0.25           # the truth's t_max and s: powers of two, so that points can lie exactly on knots
_memo = {}


# ---- the three templates --------------------------------------------------------------------------------------------
def templates(which):
    """``(epochs, {column: values})``: ``'sifto'`` (103 knots 1 d apart: the uniform path), ``'four'`` (the smallest
    not-a-knot spline, non-uniform: the search path) and ``'bump'`` (12 non-uniform knots under a Gaussian bump)."""
    if which == 'sifto':
        tab = O.sifto_table()
        return tab[:, 0].copy(), {c: tab[:, k].copy() for k, c in enumerate(O._SIFTO_COLS) if k}
    if which == 'four':
        epochs = np.array([-10., -2., 3., 30.])
        return epochs, {c: np.array([0.1, 0.8, 1., 0.05]) * (1. + 0.1 * k) for k, c in enumerate(FILTERS)}
    if which == 'bump':
        epochs = np.array([-20., -14., -9., -6., -3.5, -1.5, 0., 2., 4.5, 8., 14., 24.])
        return epochs, {c: np.exp(-0.5 * ((epochs - 0.5 * k) / (6. + k)) ** 2.) for k, c in enumerate(FILTERS)}
    raise ValueError(which)


def scaled_columns(template, names, y=None, columns=None, scale='peak'):
    """{filter name: scaled column} for the distinct ``names`` of a light curve (models.py:701-717): the column
    ``columns.get(name, char)`` times ``peak / max(column)``, ``peak`` the largest ``y`` among the filter's rows
    (``scale='peak'``) or ``scale[name]``."""
    epochs, cols = template
    names = np.asarray([str(n) for n in names])
    out = {}
    for nm in dict.fromkeys(names.tolist()):
        column = (columns or {}).get(nm, O.band(nm).char)
        if column not in cols:
            raise Exception('No template for filter ' + nm)
        col = np.asarray(cols[column], dtype=np.float64)
        peak = np.max(np.asarray(y, dtype=np.float64)[names == nm]) if isinstance(scale, str) else scale[nm]
        out[nm] = col * peak / np.max(col)
    return out


def split_rows(P, n_base, factors=FACTORS, offsets=OFFSETS):
    """``(t_max, s, {char: r}, {char: dt})`` of rows ``P`` (n, >= n_base + 2 + len(factors) + len(offsets))."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    k = n_base + 2
    fac = {c: P[:, k + i] for i, c in enumerate(factors)}
    off = {c: P[:, k + len(factors) + i] for i, c in enumerate(offsets)}
    return P[:, n_base], P[:, n_base + 1], fac, off


def template_argument(t, names, P, n_base, factors=FACTORS, offsets=OFFSETS):
    """(npoints, n): ``(t - t_max - dt) / s``."""
    t_max, s, _, off = split_rows(P, n_base, factors, offsets)
    t = np.asarray(t, dtype=np.float64)
    zero = np.zeros(len(t_max))
    dt = np.array([off.get(O.band(str(nm)).char, zero) for nm in names])
    with np.errstate(all='ignore'):
        return ((t[:, None] - t_max) - dt) / s


def template_values(epochs, scaled, t, names, P, n_base, factors=FACTORS, offsets=OFFSETS):
    """(npoints, n): ``r_f S_f((t - t_max - dt_f) / s)`` for the rows ``P``; ``scaled``: :func:`scaled_columns`."""
    _, _, fac, _ = split_rows(P, n_base, factors, offsets)
    x = template_argument(t, names, P, n_base, factors, offsets)
    out = np.empty_like(x)
    one = np.ones(x.shape[1])
    for j, nm in enumerate(names):
        with np.errstate(all='ignore'):
            v = CubicSpline(epochs, scaled[str(nm)], extrapolate=False)(x[j])
        v[np.isnan(v)] = 0.
        out[j] = v * fac.get(O.band(str(nm)).char, one)
    return out


def model_values(base, epochs, scaled, t, bands, names, P, n_base, factors=FACTORS, offsets=OFFSETS):
    """(npoints, n): base + template."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    with np.errstate(all='ignore'):
        return L.model_values(base, np.asarray(t), bands, P[:, :n_base]) + \
            template_values(epochs, scaled, t, names, P, n_base, factors, offsets)


def gaussian_log_likelihood(m, y, dy, sigma=None, sigma_type='relative'):
    """models.py:116-136 for model values ``m`` (npoints, n); ``sigma`` (n,) or None."""
    y, dy = np.asarray(y, dtype=np.float64)[:, None], np.asarray(dy, dtype=np.float64)[:, None]
    s = dy if sigma is None else np.sqrt(dy ** 2. + ((dy if sigma_type == 'relative' else np.median(dy)) * sigma) ** 2.)
    with np.errstate(all='ignore'):
        return -0.5 * np.sum(np.log(2 * np.pi * s ** 2.) + ((y - m) / s) ** 2., axis=0)


def log_likelihood(c, P, use_sigma=False, sigma_type='relative', factors=FACTORS, offsets=OFFSETS, base=None):
    """(n,): the log-likelihood of the rows ``P`` (n, ndim) on the case ``c``."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    m = model_values(base or c['base'], c['epochs'], c['scaled'], c['t'], c['bands'], c['names'], P, c['n_base'], factors,
                     offsets)
    return gaussian_log_likelihood(m, c['y'], c['dy'], P[:, -1] if use_sigma else None, sigma_type)


# ---- the case -----------------------------------------------------------------------------------------------------------
def oracle_base(kind):
    if kind == 'ShockCooling4':
        return (kind, O.ShockCooling4Oracle(Z))
    return (kind, O.ShockCoolingOracle(z=Z, n=1.5))


def case(kind='ShockCooling2', template='sifto', npts=60):
    """``npts`` points in six filters over 0.3 ... 40 d about a truth -- ``kind``'s of ``limits_reference.KINDS`` plus a
    template of explicit peak values at ``t_max = 8``, ``s = 0.25``, ``r_r = 0.8``, ``dt_U = 1.5`` -- with 5 % errors, so
    that ``scale='peak'`` then rescales from the noisy data.  The first three points lie, for the truth, exactly on an
    interior knot, the first and the last knot (filters without an offset); 37 rows (with a sigma column) about the
    truth, row 0 the truth itself."""
    key = (kind, template, npts)
    if key in _memo:
        return _memo[key]
    rng = np.random.default_rng(170)
    epochs, cols = templates(template)
    base = oracle_base(kind)
    truth_base, spread, i_t0 = L.KINDS[kind]
    n_base = len(truth_base)
    on_knots = T_MAX + STRETCH * epochs[[len(epochs) // 2, 0, -1]]
    t = np.concatenate([on_knots, np.sort(rng.uniform(0.3, 40., max(npts, 60) - 3))])[:npts]
    names = np.concatenate([['B', 'g', 'V'], rng.choice(FILTERS, max(npts, 60) - 3)])[:npts]
    bands = [O.band(n) for n in names]
    truth = np.concatenate([truth_base, [T_MAX, STRETCH, 0.8, 1.5]])
    base_true = L.model_values(base, t, bands, truth[None, :n_base])[:, 0]
    # explicit peak values: a second peak as bright as the shock component is around the dip, per filter
    dip = L.model_values(base, np.full(6, 5.), [O.band(n) for n in FILTERS], truth[None, :n_base])[:, 0]
    true_scaled = scaled_columns((epochs, cols), FILTERS, scale=dict(zip(FILTERS, 2. * dip)))
    tau_true = template_values(epochs, true_scaled, t, names, truth[None], n_base)[:, 0]
    ytrue = base_true + tau_true
    y = ytrue * (1. + 0.05 * rng.standard_normal(npts))
    dy = 0.05 * ytrue
    scaled = scaled_columns((epochs, cols), names, y)      # what scale='peak' makes of the noisy data

    cols_p = [rng.uniform(a, b, N_ROWS) for a, b in spread]
    cols_p.insert(i_t0, rng.uniform(-1., 1., N_ROWS))
    P = np.column_stack(cols_p + [rng.uniform(5., 11., N_ROWS), rng.uniform(0.15, 0.4, N_ROWS),
                                  rng.uniform(0.5, 1.5, N_ROWS), rng.uniform(-2., 2., N_ROWS),
                                  rng.uniform(0.1, 1., N_ROWS)])
    P[0, :-1] = truth

    # so that a degenerate case cannot hide an error: for the truth row ...
    x = template_argument(t, names, truth[None], n_base)[:, 0]
    if npts >= 3:     # ... points exactly on an interior knot, on the first and on the last
        assert x[0] == epochs[len(epochs) // 2] and x[1] == epochs[0] and x[2] == epochs[-1]
    else:
        assert x[0] == epochs[len(epochs) // 2]
    if npts >= 60:
        inside = (x >= epochs[0]) & (x <= epochs[-1])
        assert np.any(x < epochs[0]) and np.any(x > epochs[-1])          # ... points before the first knot, after the last
        share = tau_true[inside] / ytrue[inside]
        assert np.sum((share > 1e-3) & (share < 0.99)) >= 0.5 * inside.sum(), share
        assert inside.sum() >= 10
    quantity = 'flux' if kind == 'ShockCooling3' else 'lum'
    lc = {'MJD': t, 'filter': [str(n) for n in names], quantity: y, 'd' + quantity: dy}
    c = dict(kind=kind, template=(epochs, cols), epochs=epochs, scaled=scaled, t=t, names=names, bands=bands, y=y, dy=dy,
             P=P, lc=lc, base=base, truth=truth, n_base=n_base, n_par=len(truth), quantity=quantity)
    _memo[key] = c
    return c


def rows(c, use_sigma):
    return np.ascontiguousarray(c['P'] if use_sigma else c['P'][:, :-1])


# ---- Kasen's companion shock as a base (models.py:752-755): what CompanionShocking{,2} add SiFTO to -----------------
KASEN_NAMES = ['t_0', 'a', 'M v^7']


def kasen_state(t_in, P):
    """``T = 25 (a^36 Mv t^-74)^(1/144)``, ``R = 2.7 (Mv t^7)^(1/9)``: (npoints, n) each."""
    P = np.atleast_2d(P)
    T, R = O.kasen_temperature_radius(t_in, P[:, 0], P[:, 1], P[:, 2])
    return np.reshape(T, (len(t_in), -1)), np.reshape(R, (len(t_in), -1))


# ---- sampling: the tempered restatement with this likelihood --------------------------------------------------------
def tempered_log_like(pb, block):
    """What tests/tempered_reference.py calls for the likelihood: (n, D) -> (n,), no prior."""
    return log_likelihood(pb, np.atleast_2d(block))
