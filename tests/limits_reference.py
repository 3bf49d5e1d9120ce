"""Censored non-detections in NumPy (a helper, not a test): the definition ``nondet='censored'`` is held to.

The rows of a light curve whose ``nondet`` is true are the limits ``j``, the others the detections ``i``::

    ln L(p) = [the Gaussian log-likelihood of models.py:116-136 over the detections]
              + sum_j ln Phi((L_lim,j - m_j(p)) / sigma_j(p))

with ``L_lim,j = nondetSigmas * dy_j``, ``m_j`` the model at the limit's time and filter, ``sigma_j = dy_j`` or, with a
fitted scatter ``s``, ``sqrt(dy_j^2 + (s u_j)^2)``, ``u_j = dy_j`` ('relative') or the median ``dy`` of the detections
('absolute').  The model values are the oracle's; ``ln Phi`` is ``scipy.special.log_ndtr`` (within 1.5e-13 relative of
the exact value for z in [-1e4, 37]: good for sums at 1e-11), and :func:`log_ndtr_exact` is the exact one, mpmath at 60
digits, for the test of the device function alone."""
import mpmath
import numpy as np
from scipy.special import erfc, log_ndtr

from oracle import lcf_oracle as O

Z = 0.01
FILTERS = ['U', 'B', 'V', 'g', 'r', 'i']
N_ROWS = 37
NONDET_SIGMAS = 3.


def log_ndtr_exact(z):
    """``ln Phi(z)`` rounded from 60 digits: ``log(ncdf(z))`` for ``z <= 0`` and ``log1p(-ncdf(-z))`` for ``z > 0`` (the
    plain form rounds to 0 from z = 17 at this precision)."""
    out = np.empty(np.shape(z))
    with mpmath.workdps(60):
        for k, v in np.ndenumerate(np.asarray(z, dtype=np.float64)):
            x = mpmath.mpf(float(v))
            out[k] = float(mpmath.log(mpmath.ncdf(x)) if x <= 0 else mpmath.log1p(-mpmath.ncdf(-x)))
    return out


def log_ndtr_naive(z):
    """What an accurate ``ln Phi`` must not be: ``log(erfc(-z / sqrt 2) / 2)``."""
    with np.errstate(all='ignore'):
        return np.log(0.5 * erfc(-np.asarray(z, dtype=np.float64) / np.sqrt(2.)))


def z_sweep():
    """130 values of z over -1e4 ... 37: both tails, 0, +-1e-3, +-1 and both sides of -38.5."""
    fixed = [-1e4, -3e3, -1e3, -300., -100., -38.6, -38.5, -38.4, -1., -1e-3, 0., 1e-3, 1., 5., 8.3, 17., 37.]
    rest = np.concatenate([-np.geomspace(1e-2, 5e3, 50), np.linspace(0.05, 36.5, 63)])
    out = np.sort(np.concatenate([fixed, rest]))
    assert len(out) == 130 and len(np.unique(out)) == 130
    return out


def model_values(model, t, bands, P):
    """Oracle model values (npoints, n) for the rows ``P`` (n, n_par).  ``model``: an oracle pair ``(kind, oracle)`` as
    ``lcf_oracle.evaluate`` takes it, or ``('custom', state, z)`` with ``state(t, P) -> T, R`` of shape (npoints, n)."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    if len(t) == 1:   # (the oracle's front end squeezes a single point's axis away: it takes light curves)
        return model_values(model, np.repeat(t, 2), list(bands) * 2, P)[:1]
    with np.errstate(all='ignore'):
        if model[0] == 'custom':
            T, R = model[1](t, P)
            return O.blackbody_to_filters_batch(bands, T, R, model[2])
        if model[0] == 'CompanionShocking' or len(P) == 1:   # (one parameter vector at a time)
            return np.column_stack([O.evaluate(model, t, bands, p) for p in P])
        return O.evaluate(model, t, bands, P.T)


def limit_terms(model, t, bands, dy, nondet, P, use_sigma=False, sigma_type='relative', nondet_sigmas=NONDET_SIGMAS):
    """(n, n_lim): ``ln Phi`` of every (row, limit), the limits in the order of the light curve's ``nondet`` rows."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    t, dy, lim = np.asarray(t), np.asarray(dy, dtype=np.float64), np.asarray(nondet, dtype=bool)
    n_par = P.shape[1] - bool(use_sigma)
    m = model_values(model, t[lim], [b for b, k in zip(bands, lim) if k], P[:, :n_par])      # (n_lim, n)
    d = dy[lim][:, None]
    sigma = d
    if use_sigma:
        unit = d if sigma_type == 'relative' else np.median(dy[~lim])
        sigma = np.sqrt(d ** 2. + (P[:, -1] * unit) ** 2.)
    with np.errstate(all='ignore'):
        return log_ndtr((nondet_sigmas * d - m) / sigma).T


def gaussian_part(model, t, bands, y, dy, nondet, P, use_sigma=False, sigma_type='relative'):
    """(n,): models.py:116-136 over the detections alone."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    det = ~np.asarray(nondet, dtype=bool)
    t, y, dy = np.asarray(t)[det], np.asarray(y, dtype=np.float64)[det][:, None], np.asarray(dy, dtype=np.float64)[det][:, None]
    n_par = P.shape[1] - bool(use_sigma)
    m = model_values(model, t, [b for b, k in zip(bands, det) if k], P[:, :n_par])
    sigma = dy
    if use_sigma:
        sigma = np.sqrt(dy ** 2. + ((dy if sigma_type == 'relative' else np.median(dy)) * P[:, -1]) ** 2.)
    with np.errstate(all='ignore'):
        return -0.5 * np.sum(np.log(2 * np.pi * sigma ** 2.) + ((y - m) / sigma) ** 2., axis=0)


def log_likelihood(model, t, bands, y, dy, nondet, P, use_sigma=False, sigma_type='relative',
                   nondet_sigmas=NONDET_SIGMAS):
    """(n,): the censored log-likelihood of the rows ``P`` (n, ndim)."""
    with np.errstate(all='ignore'):
        return gaussian_part(model, t, bands, y, dy, nondet, P, use_sigma, sigma_type) + np.sum(
            limit_terms(model, t, bands, dy, nondet, P, use_sigma, sigma_type, nondet_sigmas), axis=1)


# ---- the case -----------------------------------------------------------------------------------------------------------
# kind -> truth (the explosion time last, at 0.1 d), spread of the 37 rows about it, index of the explosion time
KINDS = {
    'ShockCooling2': ([20., 2., 10., 0.1], [(15., 25.), (1., 3.), (5., 15.)], 3),
    'ShockCooling': ([1.2, 0.5, 3.0, 2.0, 0.1], [(1., 1.5), (0.3, 0.7), (2., 4.), (1.5, 2.5)], 4),
    'ShockCooling4': ([1.2, 0.5, 3.0, 2.0, 0.1], [(1., 1.5), (0.3, 0.7), (2., 4.), (1.5, 2.5)], 4),
    'ShockCooling3': ([1.1, 0.6, 2.5, 1.8, 25., 0.15, 0.1], [(0.9, 1.3), (0.4, 0.8), (2., 3.), (1.5, 2.1), (20., 30.),
                                                               (0.05, 0.25)], 6),
    'CompanionShocking': ([0.1, 0.5, 1.2, 17., 1.05, 0.95, 0.9, 0.6], None, 0),
}
_memo = {}


def limit_times(n_lim):
    """The recipe of the 13 limits on a grid of ``n_lim``: 7 in 13 before the explosion, over -3 ... 0.05 d, the others
    on the rise, over 0.12 ... 0.28 d (one limit: on the rise)."""
    n_pre = 7 * n_lim // 13
    return np.linspace(-3., 0.05, n_pre), np.linspace(0.12, 0.28, n_lim - n_pre)


def oracle_model(kind, bands=None, y=None):
    if kind == 'CompanionShocking':
        return (kind, O.CompanionShockingOracle(bands, y, Z, 1))
    if kind == 'ShockCooling4':
        return (kind, O.ShockCooling4Oracle(Z))
    return (kind, O.ShockCoolingOracle(z=Z, n=1.5))


def case(kind='ShockCooling2', n_lim=13):
    """60 detections over 0.3 ... 9 d in six filters about the truth (5 % errors, ``default_rng(160)``: for ShockCooling2
    the photometry of ``test_gpu_custom.sc2_case(60)``) and ``n_lim`` limits: those before the explosion with
    ``dy = 0.02 median(ytrue)`` and the model exactly 0 at the truth, those on the rise with a 3-sigma limit equal to the
    true model value.  The rows of the light curve are shuffled, so that the limits lie among the detections.  37 rows
    (with a sigma column) whose explosion times run from before the first limit to after some detections."""
    if (kind, n_lim) in _memo:
        return _memo[kind, n_lim]
    rng = np.random.default_rng(160)
    npts = 60
    t = np.sort(rng.uniform(0.3, 9., npts))
    names = rng.choice(FILTERS, npts)
    truth, spread, i_t0 = KINDS[kind]
    truth = np.array(truth)
    t_pre, t_rise = limit_times(n_lim)
    t_lim = np.concatenate([t_pre, t_rise])
    names_lim = np.array([FILTERS[k % 6] for k in range(n_lim)])
    t_all, names_all = np.concatenate([t, t_lim]), np.concatenate([names, names_lim])
    bands_all = [O.band(n) for n in names_all]
    if kind == 'CompanionShocking':   # (the template is scaled to the observed peak: data from a smooth stand-in first)
        guess = 2e20 * np.exp(-0.5 * ((t_all - 17.) / 12.) ** 2)
        ytrue_all = O.evaluate(oracle_model(kind, bands_all, guess), t_all, bands_all, truth)
    else:
        ytrue_all = O.evaluate(oracle_model(kind), t_all, bands_all, truth)
    ytrue = ytrue_all[:npts]
    y = ytrue * (1. + 0.05 * rng.standard_normal(npts))
    dy = 0.05 * ytrue
    # (the companion models' SN Ia template is there before the shock: only their shock component is exactly 0)
    assert kind == 'CompanionShocking' or np.all(ytrue_all[npts:npts + len(t_pre)] == 0.)
    assert np.all(ytrue_all[npts + len(t_pre):] > 0.)
    dy_lim = np.concatenate([np.full(len(t_pre), 0.02 * np.median(ytrue)), ytrue_all[npts + len(t_pre):] / NONDET_SIGMAS])
    y_all, dy_all = np.concatenate([y, np.zeros(n_lim)]), np.concatenate([dy, dy_lim])
    nondet = np.concatenate([np.zeros(npts, dtype=bool), np.ones(n_lim, dtype=bool)])
    order = np.random.default_rng(1000 + n_lim).permutation(npts + n_lim)
    t_all, names_all, y_all, dy_all, nondet = t_all[order], names_all[order], y_all[order], dy_all[order], nondet[order]
    bands_all = [bands_all[k] for k in order]
    if kind == 'CompanionShocking':
        lo = truth - [3.6, 0.1, 0.3, 1., 0.03, 0.05, 0.05, 0.1]
        hi = truth + [2.4, 0.1, 0.3, 1., 0.03, 0.05, 0.05, 0.1]
        P = rng.uniform(lo, hi, (N_ROWS, len(truth)))
    else:
        cols = [rng.uniform(a, b, N_ROWS) for a, b in spread]
        cols.insert(i_t0, rng.uniform(-3.5, 2.5, N_ROWS))
        P = np.column_stack(cols)
    P = np.column_stack([P, rng.uniform(0.1, 1., N_ROWS)])
    P[:, i_t0] = rng.permutation(np.linspace(-3.5, 2.5, N_ROWS))
    P[0, :-1] = truth
    t0 = P[:, i_t0]
    assert np.any(t0 > t_all[~nondet].min()) and np.any(t0 < t_all.min())     # after some detections, before every row
    quantity = 'flux' if kind == 'ShockCooling3' else 'lum'
    lc = {'MJD': t_all, 'filter': [str(n) for n in names_all], quantity: y_all, 'd' + quantity: dy_all, 'nondet': nondet}
    model = oracle_model(kind, bands_all, y_all)
    c = dict(kind=kind, t=t_all, names=names_all, bands=bands_all, y=y_all, dy=dy_all, nondet=nondet, P=P, lc=lc,
             model=model, truth=truth, n_par=len(truth))
    _memo[kind, n_lim] = c
    return c


def rows(c, use_sigma):
    return np.ascontiguousarray(c['P'] if use_sigma else c['P'][:, :-1])


def without_limits(c):
    """The light curve of the detections alone (no ``nondet`` column)."""
    det = ~c['nondet']
    return {k: ([x for x, d in zip(v, det) if d] if isinstance(v, list) else v[det]) for k, v in c['lc'].items()
            if k != 'nondet'}


# ---- sampling: the tempered restatement with the censored likelihood ----------------------------------------------------
def censored_log_like(pb, block):
    """What tests/tempered_reference.py calls for the likelihood: (n, D) -> (n,), no prior."""
    return log_likelihood(pb['model'], pb['t'], pb['bands'], pb['y'], pb['dy'], pb['nondet'], np.atleast_2d(block))


def gaussian_log_like(pb, block):
    """The same light curve without its limits."""
    return gaussian_part(pb['model'], pb['t'], pb['bands'], pb['y'], pb['dy'], pb['nondet'], np.atleast_2d(block))
