"""Per-epoch blackbody SED likelihoods on the MI355X and the small closed-form helpers around them.

Mirrors the part of the reference's ``bolometric.py`` that shares the hot path's primitive
(SURVEY.md section 8 row a11 / "next" row 1):

* :func:`spectrum_log_likelihood` -- the inner ``log_posterior`` of ``spectrum_mcmc`` without its priors
  (``bolometric.py:154-164``): ``[f.synthesize(planck_fast, T, R) for f in filters]`` + Gaussian likelihood, batched
  over (epoch x candidate) on the device, float64 or float32;
* :func:`pseudo` (``bolometric.py:32-59``), :func:`stefan_boltzmann` (``bolometric.py:422-453``): closed-form,
  one NumPy expression each, evaluated on the host once per result table (not a hot loop).

and the bolometric light curve (``bolometric.py:383-416, 456-605, 648-832``):

* :func:`calculate_bolometric` -- the reference's workflow step for step, with its three loops over epochs and samples
  batched into three device phases: one :func:`blackbody_lstsq_epochs` launch (``k_bb_lstsq``) for every epoch's
  ``curve_fit``, one population MCMC for every epoch's ``spectrum_mcmc``, one :func:`luminosity_samples` launch
  (``k_bb_lum``) for ``pseudo`` / ``stefan_boltzmann`` of every posterior sample;
* :func:`group_by_epoch`, :func:`median_and_unc`, :func:`integrate_sed`, :func:`calc_colors` (host, as the reference).
"""
import os
import warnings

import numpy as np

from . import engine as _eng
from .filters import PackedTables, as_filter, c1, c2, filtdict
from .lightcurve import LC, _group_rows

DEPRECATED_BOLOMETRIC_COLNAMES = [  # (old, new)   bolometric.py:22-30
    ('L_opt', 'L'),
    ('lum', 'L_bol'),
    ('dlum', 'dL_bol'),
    ('dtemp0', 'dtemp_mcmc0'),
    ('dtemp1', 'dtemp_mcmc1'),
    ('dradius0', 'dradius_mcmc0'),
    ('dradius1', 'dradius_mcmc1'),
]

#: Stefan-Boltzmann constant in W (1000 Rsun)^-2 kK^-4 (bolometric.py:419)
sigma_sb = 2.744452656619892e+28


def stefan_boltzmann(temp, radius, dtemp=None, drad=None, covTR=None):
    """Blackbody luminosity [W] (and its uncertainty) from T [kK] and R [1000 Rsun] (bolometric.py:422-453)."""
    lum = 4 * np.pi * radius ** 2 * sigma_sb * temp ** 4
    if dtemp is None or drad is None or covTR is None:
        return lum
    dlum = 8 * np.pi * sigma_sb * (radius ** 2 * temp ** 8 * drad ** 2 + 4 * radius ** 4 * temp ** 6 * dtemp ** 2
                                   + 4 * radius ** 3 * temp ** 7 * covTR) ** 0.5
    return lum, dlum


def pseudo(temp, radius, z, filter0=filtdict['I'], filter1=filtdict['U'], cutoff_freq=np.inf):
    """Planck spectrum integrated on a 1-THz grid between two filters [W] (bolometric.py:32-59)."""
    freq0 = filter0.freq_eff - filter0.dfreq / 2.
    freq1 = filter1.freq_eff + filter1.dfreq / 2.
    nu = np.arange(freq0, freq1) * (1. + z)
    temp = np.asarray(temp, dtype=float)
    radius = np.asarray(radius, dtype=float)
    with np.errstate(all='ignore'):
        inv_t = np.where(temp > 0., 1. / np.where(temp > 0., temp, 1.), 0.)
        occ = np.exp(c1 * np.multiply.outer(inv_t, nu)) - 1.
        occ = np.where(occ > 0., 1. / np.where(occ > 0., occ, 1.), 0.)
        lnu = c2 * np.multiply.outer(radius ** 2, nu ** 3 * np.minimum(1., cutoff_freq / nu)) * occ
    tw = np.ones(len(nu))
    tw[[0, -1]] = 0.5
    return np.sum(lnu * tw, axis=-1) * 1e12


class SpectrumLikelihood:
    """Observed SEDs of many epochs resident on the GPU; evaluates candidate blackbodies per epoch.

    Parameters
    ----------
    epochs : sequence of (filters, y, dy)
        Per epoch: the filters (objects or aliases), the observed luminosity densities [W/Hz] and uncertainties.
    z : float
        Redshift between the blackbody and the observed filters.
    """

    def __init__(self, epochs, z=0., cutoff_freq=np.inf, device=0):
        filts = [[as_filter(f) for f in e[0]] for e in epochs]
        uniq = list(dict.fromkeys(f for fl in filts for f in fl))
        lookup = {f: i for i, f in enumerate(uniq)}
        tabs = PackedTables(uniq, z=z, cutoff_freq=cutoff_freq)
        self.engine = _eng.SedEngine(tabs.off, tabs.a, tabs.w, device=device,
                                     ctab=(tabs.coff, tabs.ca, tabs.cw, tabs.ctmin),
                                     itab=tabs.interpolants(below=10))   # from 0.94 kK: the priors start at 1 kK
        self.itab_tmin = tabs.interpolants(below=10)[1]
        off = np.concatenate([[0], np.cumsum([len(fl) for fl in filts])])
        idx = np.array([lookup[f] for fl in filts for f in fl], dtype=np.int32)
        y = np.concatenate([np.asarray(e[1], dtype=float) for e in epochs]) if len(epochs) else np.zeros(0)
        dy = np.concatenate([np.asarray(e[2], dtype=float) for e in epochs]) if len(epochs) else np.zeros(0)
        self.engine.set_observations(off, idx, y, dy)
        self.n_epochs = len(epochs)
        self.samples_per_candidate = np.array([sum(tabs.off[lookup[f] + 1] - tabs.off[lookup[f]] for f in fl)
                                               for fl in filts])

    #: arithmetic of the device kernel: 'f64' = float64 through the interpolants of ln S_f(ln T) (the light-curve
    #: engine's default level; sample tables outside their range), 'f64-tables' = float64 sample by sample (the
    #: reference's own sum), 'f32' = float32 sample by sample (BASELINE configs[3] as specified)
    PRECISIONS = {'f64': 2, 'f64-tables': 0, 'f32': 1}

    def __call__(self, candidates, sigma_type='relative', precision='f64', compressed=True):
        """``candidates``: (n_epochs, n_cand, 2|3) of (T, R[, sigma]) -> log-likelihoods (n_epochs, n_cand).
        ``compressed``: use the Gauss-compressed band tables where they are valid (same sums to 2e-14)."""
        if sigma_type not in ('relative', 'absolute'):
            raise Exception('sigma_type must either be "relative" or "absolute"')
        st = _eng.SIGMA_RELATIVE if sigma_type == 'relative' else _eng.SIGMA_ABSOLUTE
        return self.engine.log_likelihood(candidates, st, self.PRECISIONS[precision], compressed)


def spectrum_log_likelihood(filters, y, dy, T, R, z=0., sigma=None, sigma_type='relative', precision='f64'):
    """Log-likelihood of one epoch's SED for arrays of candidate (T, R[, sigma])."""
    T = np.atleast_1d(np.asarray(T, dtype=float))
    cols = [T, np.broadcast_to(np.asarray(R, dtype=float), T.shape)]
    if sigma is not None:
        cols.append(np.broadcast_to(np.asarray(sigma, dtype=float), T.shape))
    like = SpectrumLikelihood([(filters, y, dy)], z=z)
    return like(np.stack(cols, axis=-1)[None], sigma_type, precision)[0]


def blackbody_grid_fit(epochs, z=0., T_grid=None, R_grid=None, precision='f64', device=0):
    """Per-epoch blackbody fit on a dense (T, R) grid: the device evaluates every epoch's log-likelihood surface in
    one launch; the posterior moments under the reference's default priors -- uniform in T, log-uniform in R
    (``bolometric.py:729``) -- give the estimates the reference gets from ``curve_fit`` / a short MCMC per epoch.

    Returns a dict of arrays over epochs: ``temp, radius`` (maximum likelihood), ``temp_mean, dtemp, radius_mean,
    dradius, covTR`` (posterior moments), ``lum, dlum`` (Stefan-Boltzmann at the posterior mean) and ``lnL_max``."""
    T_grid = np.linspace(1., 100., 128) if T_grid is None else np.asarray(T_grid, dtype=float)
    R_grid = np.geomspace(0.01, 1000., 128) if R_grid is None else np.asarray(R_grid, dtype=float)
    like = SpectrumLikelihood(epochs, z=z, device=device)
    TT, RR = np.meshgrid(T_grid, R_grid, indexing='ij')
    cand = np.broadcast_to(np.stack([TT.ravel(), RR.ravel()], axis=-1), (like.n_epochs, TT.size, 2))
    lnl = like(np.ascontiguousarray(cand), precision=precision)                 # (n_epochs, nT * nR)
    best = np.argmax(lnl, axis=1)
    # quadrature weights: uniform prior in T -> dT; log-uniform prior in R -> d(ln R) on the geometric grid
    wT = np.gradient(T_grid)
    wR = np.gradient(np.log(R_grid))
    w = np.exp(lnl - lnl.max(axis=1, keepdims=True)) * np.outer(wT, wR).ravel()
    w /= w.sum(axis=1, keepdims=True)
    Tm, Rm = w @ TT.ravel(), w @ RR.ravel()
    dT = np.sqrt(np.maximum(w @ TT.ravel() ** 2 - Tm ** 2, 0.))
    dR = np.sqrt(np.maximum(w @ RR.ravel() ** 2 - Rm ** 2, 0.))
    cov = w @ (TT.ravel() * RR.ravel()) - Tm * Rm
    lum, dlum = stefan_boltzmann(Tm, Rm, dT, dR, cov)
    return dict(temp=TT.ravel()[best], radius=RR.ravel()[best], temp_mean=Tm, dtemp=dT, radius_mean=Rm, dradius=dR,
                covTR=cov, lum=lum, dlum=dlum, lnL_max=lnl[np.arange(len(best)), best])


def spectrum_mcmc_population(epochs, priors=None, z=0., nwalkers=10, burnin_steps=200, steps=100, T_range=(1., 100.),
                             R_range=(0.01, 1000.), seed=0, use_sigma=False, sigma_type='relative'):
    """``spectrum_mcmc`` (bolometric.py:87-190) for MANY epochs at once: one (T, R[, sigma]) ensemble per epoch, all
    running in lock step on the device (population mode).  Defaults follow the reference (10 walkers, 200 burn-in +
    100 steps, uniform prior on T, log-uniform on R).  Returns ``chains[n_epochs][steps * nwalkers, ndim]``."""
    from .models import Blackbody, LogUniformPrior, UniformPrior
    from .sampler import PopulationSampler
    ndim = 3 if use_sigma else 2
    if priors is None:
        priors = [UniformPrior(*T_range), LogUniformPrior(*R_range)] + ([UniformPrior(0., 10.)] if use_sigma else [])
    if nwalkers < 2 * ndim:
        raise ValueError('nwalkers must be at least 2 * ndim')
    problems, x0 = [], {}
    rng = np.random.default_rng(seed)
    for k, (filts, y, dy) in enumerate(epochs):
        lc = {'MJD': np.zeros(len(y)), 'filter': list(filts), 'lum': np.asarray(y, float), 'dlum': np.asarray(dy, float)}
        model = Blackbody(redshift=z)
        if use_sigma:
            model.input_names.append('\\sigma')
        problems.append((model, lc, priors, dict(use_sigma=use_sigma, sigma_type=sigma_type)))
        # starting guesses: uniform over the prior ranges like the reference (bolometric.py:166)
        cols = [rng.uniform(*T_range, nwalkers), np.exp(rng.uniform(*np.log(R_range), nwalkers))]
        if use_sigma:
            cols.append(rng.uniform(0., 1., nwalkers))
        x0[k] = np.column_stack(cols)
    pop = PopulationSampler(problems, nwalkers, seed=seed)
    pop.run_mcmc(x0, burnin_steps, store=False)
    for s in pop.samplers.values():
        s.reset()
    pop.run_mcmc(None, steps)
    return [pop[k].flatchain for k in range(len(epochs))]


# ---------------------------------------------------------------------------------------------------------------
# bolometric light curves (bolometric.py:383-832)
# ---------------------------------------------------------------------------------------------------------------
def _grid(filter0=filtdict['I'], filter1=filtdict['U']):
    """(freq0, n_grid) of :func:`pseudo`'s 1-THz grid."""
    freq0 = filter0.freq_eff - filter0.dfreq / 2.
    freq1 = filter1.freq_eff + filter1.dfreq / 2.
    return freq0, len(np.arange(freq0, freq1))


def group_by_epoch(lc, res=1., also_group_by=()):
    """Single-epoch SEDs of a light curve, sorted by median MJD (bolometric.py:383-416).

    Manual epochs go in an ``'epoch'`` column; rows without one (NaN, or all rows when there is no such column) get
    ``round(x - frac + round(frac)) * res`` with ``x = MJD / res`` and ``frac`` the median fractional part of ``x``.
    ``lc['epoch']`` is set, as in the reference."""
    epochs = np.asarray(lc['epoch'], dtype=float).copy() if 'epoch' in lc else np.full(len(lc), np.nan)
    missing = np.isnan(epochs)
    if missing.any():
        x = np.asarray(lc['MJD'], dtype=float)[missing] / res
        frac = np.median(x - np.trunc(x))
        epochs[missing] = np.round(x - frac + np.round(frac)) * res
    lc['epoch'] = epochs
    groups = [lc[rows] for rows in _group_rows(lc, ['epoch'] + list(also_group_by))]
    mjdavg = [np.median(g['MJD']) for g in groups]
    return [groups[i] for i in np.argsort(mjdavg)]


def median_and_unc(x, perc_contained=68.):
    """Median and the distances to the edges of the equal-tailed interval holding ``perc_contained`` % of ``x``
    (along axis 0) (bolometric.py:456-480)."""
    q = 50. + np.array([-perc_contained / 2., 0., perc_contained / 2.])
    percentiles = np.percentile(x, q, axis=0)
    median = percentiles[1]
    lower, upper = np.diff(percentiles, axis=0)
    return median, lower, upper


def integrate_sed(epoch1):
    """Trapezoid of the SED, closed by zeros one filter width beyond the outermost filters [W] (bolometric.py:537-556).
    Needs ``'freq'``, ``'dfreq'`` [THz] and ``'lum'`` [W/Hz]; the epoch is not reordered."""
    order = np.argsort(np.asarray(epoch1['freq'], dtype=float))
    f = np.asarray(epoch1['freq'], dtype=float)[order]
    df = np.asarray(epoch1['dfreq'], dtype=float)[order]
    lum = np.asarray(epoch1['lum'], dtype=float)[order]
    freqs = np.concatenate([[f[0] - df[0]], f, [f[-1] + df[-1]]])
    lums = np.concatenate([[0.], lum, [0.]])
    trapezoid = getattr(np, 'trapezoid', None) or np.trapz   # (NumPy 2 renamed it)
    return trapezoid(lums, freqs) * 1e12


def calc_colors(epoch1, colors):
    """Colours ``'X-Y'`` of an epoch from its ``absmag`` / ``dmag`` / ``nondet`` (bolometric.py:559-605): lists of
    colours, uncertainties, lower-limit and upper-limit flags.  The first row of each filter counts."""
    mags, dmags, lolims, uplims = [], [], [], []
    filts = list(epoch1['filter'])
    for color in colors:
        f0, f1 = [filtdict[f] for f in color.split('-')]
        if f0 in filts and f1 in filts:
            i0, i1 = filts.index(f0), filts.index(f1)
            m0, dm0, n0 = epoch1['absmag'][i0], epoch1['dmag'][i0], bool(epoch1['nondet'][i0])
            m1, dm1, n1 = epoch1['absmag'][i1], epoch1['dmag'][i1], bool(epoch1['nondet'][i1])
            mags.append(np.nan if n0 and n1 else m0 - m1)
            dmags.append((dm0 ** 2. + dm1 ** 2.) ** 0.5)
            lolims.append(n0)
            uplims.append(n1)
        else:
            mags.append(np.nan)
            dmags.append(np.nan)
            lolims.append(True)
            uplims.append(True)
    return mags, dmags, lolims, uplims


def luminosity_samples(T, R, z=0., cutoff_freq=np.inf, device=0):
    """``(pseudo(T, R, z, cutoff_freq=...), stefan_boltzmann(T, R))`` of every sample in one device launch
    (``k_bb_lum``): the 1-THz trapezoid from I's blue edge to U's red edge and 4 pi R^2 sigma T^4, both in W."""
    T = np.asarray(T, dtype=float)
    R = np.broadcast_to(np.asarray(R, dtype=float), T.shape)
    freq0, n_grid = _grid()
    Lp, Lb = _eng.bb_luminosity(T.ravel(), R.ravel(), z, freq0, n_grid, cutoff_freq, device=device)
    return Lp.reshape(T.shape), Lb.reshape(T.shape)


#: k_bb_lstsq's iteration cap and step tolerance (relative)
LSTSQ_MAX_ITER = 500
LSTSQ_XTOL = 1e-12


def blackbody_lstsq_epochs(epochs, z, p0=None, T_range=(1., 100.), R_range=(0.01, 1000.), cutoff_freq=np.inf,
                           device=0):
    """:func:`blackbody_lstsq` of many epochs in ONE device launch.

    ``epochs``: sequence of (freq [THz, observed freq_eff], lum [W/Hz]) pairs, or of tables with those columns.
    ``p0``: (T, R) for all epochs or an (n_epochs, 2) array; default (10, 10).  Returns a dict of arrays over epochs:
    ``temp, radius, dtemp, dradius, covTR, L_bol, dL_bol, L`` (the reference's 7-tuple plus the covariance; NaN where the
    fit did not converge), ``cost`` (1/2 sum of squared residuals), ``niter`` and ``status`` (``engine.bb_lstsq``)."""
    pairs = [(e['freq'], e['lum']) if not isinstance(e, tuple) else e for e in epochs]
    n = len(pairs)
    p0 = np.broadcast_to(np.asarray([10., 10.] if p0 is None else p0, dtype=float), (n, 2))
    lo, hi = np.array([T_range[0], R_range[0]], float), np.array([T_range[1], R_range[1]], float)
    if np.any(p0 < lo) or np.any(p0 > hi):
        raise ValueError('`x0` is infeasible.')   # (scipy's least_squares)
    off = np.concatenate([[0], np.cumsum([len(f) for f, _ in pairs])]).astype(np.int32)
    freq = np.concatenate([np.asarray(f, float) for f, _ in pairs]) if n else np.zeros(0)
    lum = np.concatenate([np.asarray(y, float) for _, y in pairs]) if n else np.zeros(0)
    out, status = _eng.bb_lstsq(off, freq, lum, p0, lo, hi, z, cutoff_freq, LSTSQ_MAX_ITER, LSTSQ_XTOL, device=device)
    ok = status > 0
    T, R = np.where(ok, out[:, 0], np.nan), np.where(ok, out[:, 1], np.nan)
    with np.errstate(invalid='ignore'):
        dT, dR = np.sqrt(out[:, 3]), np.sqrt(out[:, 5])
    covTR = out[:, 4]
    Lp, Lb = luminosity_samples(np.where(ok, T, 0.), np.where(ok, R, 0.), z, cutoff_freq, device=device)
    _, dLb = stefan_boltzmann(T, R, dT, dR, covTR)
    nan = np.where(ok, 1., np.nan)
    return dict(temp=T, radius=R, dtemp=dT * nan, dradius=dR * nan, covTR=covTR * nan, L_bol=Lb * nan,
                dL_bol=dLb * nan, L=Lp * nan, cost=out[:, 2], niter=out[:, 6].astype(int), status=status)


def blackbody_lstsq(epoch1, z, p0=None, T_range=(1., 100.), R_range=(0.01, 1000.), cutoff_freq=np.inf):
    """Least-squares blackbody fit of one epoch (bolometric.py:483-534), on the device: ``(temp, radius, dtemp, drad,
    lum, dlum, L_opt)``.  Raises ``RuntimeError`` if the fit does not converge, as ``curve_fit`` does."""
    r = blackbody_lstsq_epochs([epoch1], z, p0, T_range, R_range, cutoff_freq)
    if r['status'][0] <= 0:
        raise RuntimeError('Optimal parameters not found: the iteration limit was reached or the data are not finite.')
    return tuple(float(r[k][0]) for k in ('temp', 'radius', 'dtemp', 'dradius', 'L_bol', 'dL_bol', 'L'))


def output_colnames(colors=(), use_src=False):
    """Column names of :func:`calculate_bolometric`'s table, in order (bolometric.py:717-728, 827-829)."""
    return (['MJD', 'dMJD0', 'dMJD1', 'temp', 'radius', 'dtemp', 'dradius', 'L_bol', 'dL_bol', 'L',
             'temp_mcmc', 'radius_mcmc', 'dtemp_mcmc0', 'dtemp_mcmc1', 'dradius_mcmc0', 'dradius_mcmc1',
             'L_bol_mcmc', 'dL_bol_mcmc0', 'dL_bol_mcmc1', 'L_mcmc', 'dL_mcmc0', 'dL_mcmc1', 'L_int', 'npoints']
            + list(colors) + [f'd({c})' for c in colors] + [f'lolims({c})' for c in colors]
            + [f'uplims({c})' for c in colors] + ['filts'] + (['source'] if use_src else [])
            + [old for old, _ in DEPRECATED_BOLOMETRIC_COLNAMES])


def _prepare_epoch(epoch1):
    """calcFlux, bin(delta=inf), calcMag, calcAbsMag, calcLum, freq / dfreq (bolometric.py:734-744)."""
    epoch1.calcFlux()
    epoch1 = epoch1.bin(delta=np.inf)
    epoch1.calcMag()
    epoch1.calcAbsMag()
    epoch1.calcLum()
    epoch1['freq'] = np.array([f.freq_eff for f in epoch1['filter']], dtype=float)
    epoch1['dfreq'] = np.array([f.dfreq for f in epoch1['filter']], dtype=float)
    return epoch1


def calculate_bolometric(lc, z=0., outpath='.', res=1., nwalkers=10, burnin_steps=200, steps=100, priors=None,
                         save_table_as=None, min_nfilt=3, cutoff_freq=np.inf, show=False, colors=None, do_mcmc=True,
                         save_chains=False, use_sigma=False, sigma_type='relative', also_group_by=(), seed=None,
                         device=0):
    """The bolometric light curve of a table of broadband photometry (bolometric.py:648-832).

    Same arguments, steps and output table as the reference's, with its per-epoch loops batched on the device: the
    ``curve_fit`` of every epoch in one ``k_bb_lstsq`` launch, the MCMC of every epoch in one population run, and
    ``pseudo`` / ``stefan_boltzmann`` of every posterior sample in one ``k_bb_lum`` launch.  The redshift comes from
    ``lc.meta['redshift']`` (``z`` is deprecated, as in the reference); ``lc.meta['dm']`` is the distance modulus.

    ``seed`` (extension): the key of the walkers' starting guesses and of the sampler; ``None`` draws it from NumPy's
    global generator, so ``np.random.seed`` reproduces a call.  ``show`` produces no plots (a warning says so);
    ``save_chains`` writes ``outpath/{mjdavg:.3f}.npy`` per epoch.

    Stated deviation: the reference gives an epoch with one detected filter a KDE prior made from the previous epoch's
    chain (bolometric.py:751-753); that replaces ``priors[0]``, and the next epoch then fails on ``priors[0].p_min``.
    Such epochs (only possible with ``min_nfilt <= 1``) are skipped here with a warning.

    Returns an :class:`~lightcurve_fitting_amd.lightcurve.LC` with the reference's columns (:func:`output_colnames`),
    including the deprecated aliases; values the reference masks are NaN (a missing ``filts`` / ``source`` is '')."""
    from .models import Blackbody, GaussianPrior, LogUniformPrior, UniformPrior
    from .sampler import PopulationSampler
    if z:
        warnings.warn('The z keyword is deprecated. Include the redshift in `lc.meta["redshift"]` instead.')
    z = lc.meta.get('redshift', z)
    if show:
        warnings.warn('show=True: plots are not produced by this package')
    colors = [] if colors is None else list(colors)
    if sigma_type not in ('relative', 'absolute'):
        raise Exception('sigma_type must either be "relative" or "absolute"')
    if priors is None:
        priors = [UniformPrior(1., 100.), LogUniformPrior(0.01, 1000.)]
        if use_sigma:
            priors.append(GaussianPrior(0., 10.))
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))
    use_src = 'source' in lc.colnames

    # host: grouping, binning, magnitudes -> luminosities (bolometric.py:732-749)
    dmag = np.asarray(lc['dmag'], dtype=float)
    lc = lc[np.isfinite(dmag) & (dmag > 0.)]
    epochs, nfilts, filtstrs = [], [], []
    for epoch1 in group_by_epoch(lc, res, also_group_by):
        epoch1 = _prepare_epoch(epoch1)
        filts = set(epoch1.where(nondet=False)['filter'])
        nfilt = len(filts)
        if nfilt < min_nfilt:
            continue
        if nfilt <= 1:
            warnings.warn(f'epoch at MJD {np.median(epoch1["MJD"]):.3f} has one detected filter: skipped (the '
                          f'reference\'s KDE-prior path is not reproduced)')
            continue
        epochs.append(epoch1)
        nfilts.append(nfilt)
        filtstrs.append(''.join(f.char for f in sorted(filts)))
    n = len(epochs)

    # device phase 1: every epoch's least-squares fit (bolometric.py:757-764)
    T_range = (priors[0].p_min, priors[0].p_max)
    R_range = (priors[1].p_min, priors[1].p_max)
    ls = blackbody_lstsq_epochs(epochs, z, (10., 10.), T_range, R_range, cutoff_freq, device=device)
    p0 = np.where(np.isfinite(ls['temp'])[:, None], np.column_stack([ls['temp'], ls['radius']]), 10.)

    ndim = 3 if use_sigma else 2
    mc = {k: np.full(n, np.nan) for k in ('temp_mcmc', 'radius_mcmc', 'dtemp_mcmc0', 'dtemp_mcmc1', 'dradius_mcmc0',
                                           'dradius_mcmc1', 'L_bol_mcmc', 'dL_bol_mcmc0', 'dL_bol_mcmc1', 'L_mcmc',
                                           'dL_mcmc0', 'dL_mcmc1')}
    if do_mcmc and n:
        # starting guesses N(0, 1) + p0, values <= 0 -> 1, |N(0, 1)| for sigma (bolometric.py:766-772)
        rng = np.random.default_rng(seed)
        x0 = {}
        for k in range(n):
            g = rng.normal(size=(nwalkers, 2)) + p0[k]
            g[g <= 0.] = 1.
            if use_sigma:
                g = np.append(g, np.abs(rng.normal(size=(nwalkers, 1))), axis=1)
            x0[k] = g
        # device phase 2: one population MCMC over all epochs (bolometric.py:776-790)
        problems = []
        for e in epochs:
            model = Blackbody(redshift=z, cutoff_freq=cutoff_freq)
            if use_sigma:
                model.input_names.append('\\sigma')
            data = {'MJD': np.zeros(len(e)), 'filter': list(e['filter']), 'lum': e['lum'], 'dlum': e['dlum']}
            problems.append((model, data, priors[:ndim], dict(use_sigma=use_sigma, sigma_type=sigma_type)))
        pop = PopulationSampler(problems, nwalkers, seed=seed, device=device)
        pop.run_mcmc(x0, burnin_steps, store=False)
        for s in pop.samplers.values():
            s.reset()
        pop.run_mcmc(None, steps)
        chains = np.stack([pop[k].flatchain for k in range(n)])          # (n, nwalkers * steps, ndim)
        if save_chains:
            os.makedirs(outpath, exist_ok=True)
            for k, e in enumerate(epochs):
                np.save(os.path.join(outpath, f'{np.median(e["MJD"]):.3f}.npy'), chains[k])
        # device phase 3: pseudo / stefan_boltzmann of every sample (bolometric.py:793-794)
        L_samples, Lbol_samples = luminosity_samples(chains[:, :, 0], chains[:, :, 1], z, cutoff_freq, device=device)
        # medians and intervals over (epoch, sample) at once (bolometric.py:797-799)
        (mc['temp_mcmc'], mc['radius_mcmc']), (mc['dtemp_mcmc0'], mc['dradius_mcmc0']), \
            (mc['dtemp_mcmc1'], mc['dradius_mcmc1']) = [a.T for a in median_and_unc(
                np.moveaxis(chains[:, :, :2], 1, 0))]
        mc['L_bol_mcmc'], mc['dL_bol_mcmc0'], mc['dL_bol_mcmc1'] = median_and_unc(Lbol_samples.T)
        mc['L_mcmc'], mc['dL_mcmc0'], mc['dL_mcmc1'] = median_and_unc(L_samples.T)

    # host: MJD, direct integration and colours (bolometric.py:754-755, 806-813)
    mjd = np.array([median_and_unc(e['MJD'], 100.) for e in epochs]).reshape(n, 3)
    L_int = np.array([integrate_sed(e) for e in epochs])
    # (the reference's integrate_sed sorts its epoch by frequency in place before the colours are taken)
    col = [calc_colors(e[np.argsort(e['freq'], kind='stable')], colors) for e in epochs]
    cols = {'MJD': mjd[:, 0], 'dMJD0': mjd[:, 1], 'dMJD1': mjd[:, 2],
            'temp': ls['temp'], 'radius': ls['radius'], 'dtemp': ls['dtemp'], 'dradius': ls['dradius'],
            'L_bol': ls['L_bol'], 'dL_bol': ls['dL_bol'], 'L': ls['L']}
    cols.update(mc)
    cols['L_int'] = L_int
    cols['npoints'] = np.array(nfilts, dtype=int)
    for j, c in enumerate(colors):
        cols[c] = np.array([r[0][j] for r in col], dtype=float)
    for j, c in enumerate(colors):
        cols[f'd({c})'] = np.array([r[1][j] for r in col], dtype=float)
    for j, c in enumerate(colors):
        cols[f'lolims({c})'] = np.array([r[2][j] for r in col], dtype=bool)
    for j, c in enumerate(colors):
        cols[f'uplims({c})'] = np.array([r[3][j] for r in col], dtype=bool)
    cols['filts'] = np.array(filtstrs, dtype=object)
    if use_src:
        cols['source'] = np.array([e['source'][0] for e in epochs], dtype=object)
    for old, new in DEPRECATED_BOLOMETRIC_COLNAMES:
        cols[old] = cols[new]
    t0 = LC.__new__(LC)
    t0.columns = {k: np.asarray(v) for k, v in cols.items()}
    t0.meta, t0.nondetSigmas, t0.groupby = {}, 3., {'filter', 'source'}
    warnings.warn('Some column names in the output table have changed (see documentation). Please update your code!')
    if save_table_as is not None and n:
        write_fixed_width_two_line(t0, save_table_as)
    return t0


def _cell(v):
    if isinstance(v, (bool, np.bool_)):
        return 'True' if v else 'False'
    if isinstance(v, (float, np.floating)):
        return '--' if np.isnan(v) else repr(float(v))
    return str(v) if str(v) else '--'


def write_fixed_width_two_line(table, path):
    """astropy's ``ascii.fixed_width_two_line`` layout: a header row, a row of dashes, then the rows, every column
    padded to its widest cell and separated by two spaces; a masked (NaN / empty) cell is ``--``."""
    names = table.colnames
    cells = [[_cell(v) for v in table[k]] for k in names]
    widths = [max([len(k)] + [len(c) for c in col]) for k, col in zip(names, cells)]
    lines = ['  '.join(k.rjust(w) for k, w in zip(names, widths)),
             '  '.join('-' * w for w in widths)]
    for i in range(len(table)):
        lines.append('  '.join(col[i].rjust(w) for col, w in zip(cells, widths)))
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
