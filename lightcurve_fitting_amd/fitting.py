"""``lightcurve_mcmc`` counterpart (reference fitting.py:16-168): same keyword signature, checks and return
conventions; the ensemble runs on the MI355X instead of inside emcee's Python loop.

Plotting (``show`` / ``save_plot_as``, ``lightcurve_corner``, ``lightcurve_model_plot``) stays outside the package: the
figures only consume ``sampler.chain`` / ``sampler.flatchain``, which the returned object provides.  The NUMBERS behind
``lightcurve_model_plot`` (fitting.py:337-360) are here: :func:`posterior_predictive` gives the percentile bands of
the model light curves -- and, for the companion-shocking models, of the SiFTO term the reference draws dashed -- over
every sample of the chain instead of 100 random draws, computed on the device without storing a value per (sample,
grid point).  :func:`thermal_predictive` does the same for what those light curves are made from -- the blackbody
temperature, radius and bolometric luminosity -- and counts, time by time, the samples that are colder than the models
allow or outside their validity window: the check the reference's usage guide asks for after every shock-cooling fit.
:func:`luminosity_predictive` is the first of the two for the central-engine models, :func:`custom_predictive` both of
them for a model the user wrote (``CustomModel``).
The numbers behind ``lightcurve_corner`` (fitting.py:241-253) are :func:`posterior_corner`: the marginal histogram of
every parameter, the joint histogram of every pair and the counts of the contour levels, with the reference's ``t_0``
offset, counted on the device over every sample.  The numbers behind the chain plots of ``lightcurve_mcmc(show=True)``
(fitting.py:135-158) are :func:`chain_history`: per step the percentile bands of the walker ensemble and the number of
walkers that moved, and the (step, value) raster of every walker's trace; with ``show`` or ``save_plot_as`` the
burn-in's is kept as ``sampler.burnin_history`` before the burn-in chain is dropped.
"""
import warnings

import numpy as np

from .models import (BaseCentralEngine, BaseCompanionShocking, Blackbody, CustomModel, Model, UniformPrior, WithTemplate,
                     _column)
from .filters import as_filter
from .sampler import EnsembleSampler

PRIOR_WARNING = 'The p_max/p_min keywords are deprecated. Use the priors keyword instead.'
MODEL_KWARGS_WARNING = 'The model_kwargs keyword is deprecated. These are now included in the model intialization.'


def make_log_posterior(lc, model, priors=None, use_sigma=False, sigma_type='relative', nondet='gaussian'):
    """The ``log_posterior`` callable that the reference builds inside ``lightcurve_mcmc`` (fitting.py:121-128), backed
    by the device engine.  ``f(p)`` with ``p`` of shape ``(ndim,)`` returns a float, exactly like the reference's
    closure; with a C-contiguous ``(n, ndim)`` block it returns ``(n,)`` -- the form
    ``emcee.EnsembleSampler(nwalkers, ndim, f, vectorize=True)`` calls once per half-step.  ``nondet='censored'``
    (extension): non-detections enter as upper limits, see ``Model.log_likelihood``."""
    engine = model.engine_for(lc, use_sigma=use_sigma, sigma_type=sigma_type, priors=priors, nondet=nondet)

    def log_posterior(p):
        p = np.asarray(p, dtype=np.float64)
        out = engine.log_posterior(p)
        return float(out[0]) if p.ndim == 1 else out

    log_posterior.engine = engine
    return log_posterior


def _prepare_photometry(lc, model):
    """The column the model is fitted to, derived from the magnitudes when ``lc`` knows how (fitting.py:68-72)."""
    if not hasattr(lc, 'calcAbsMag'):
        return                                           # plain column stores (dict of arrays) carry it already
    for method in {'flux': ('calcFlux',), 'lum': ('calcAbsMag', 'calcLum')}.get(model.output_quantity, ()):
        getattr(lc, method)()


def _bound_vector(values, ndim, fill, *, deprecated=False, name=None, fallback=None):
    """One of the four length-``ndim`` keyword vectors of ``lightcurve_mcmc`` as a float array.

    ``None`` -> ``fallback`` if given, else ``ndim`` copies of ``fill``; a wrong length raises with the reference's
    message (the deprecation text for ``p_min`` / ``p_max``, which also warn when they are used at all)."""
    if values is None:
        return np.full(ndim, fill) if fallback is None else fallback
    if len(values) != ndim:
        raise Exception(PRIOR_WARNING if deprecated else '{} must have length {:d}'.format(name, ndim))
    if deprecated:
        warnings.warn(PRIOR_WARNING)
    return np.asarray(values, dtype=float).copy()


def _resolve_priors(priors, p_min, p_max, ndim):
    if priors is None:
        return [UniformPrior(lo, hi) for lo, hi in zip(p_min, p_max)]
    if len(priors) != ndim:
        raise Exception('priors must have length {:d}'.format(ndim))
    return priors


def _check_start_box(names, priors, p_lo, p_up):
    """The box the walkers start in must lie inside the priors' support (fitting.py:113-119)."""
    for k, (param, prior) in enumerate(zip(names, priors)):
        for label, guess, limit_name, limit, outside in (('p_lo', p_lo[k], 'p_min', prior.p_min, p_lo[k] < prior.p_min),
                                                         ('p_up', p_up[k], 'p_max', prior.p_max, p_up[k] > prior.p_max)):
            if outside:
                raise Exception(f'starting guess for {param} ({label} = {guess}) is outside prior '
                                f'({limit_name} = {limit})')


def lightcurve_mcmc(lc, model, priors=None, p_min=None, p_max=None, p_lo=None, p_up=None,
                    nwalkers=100, nsteps=1000, nsteps_burnin=1000, model_kwargs=None,
                    show=False, save_plot_as='', save_sampler_as='', use_sigma=False, sigma_type='relative',
                    seed=None, ntemps=None, betas=None, Tmax=None, adapt=False, moves=None, nondet='gaussian'):
    """Fit an analytical model to observed photometry with an affine-invariant ensemble sampler on the GPU.

    Arguments as in the reference (fitting.py:16-58).  ``seed`` (extension) keys the counter-based RNG; by default
    it is drawn from NumPy's global generator, which also provides the starting guesses (fitting.py:132), so
    ``np.random.seed`` makes a run reproducible exactly as it does for the reference.

    ``ntemps`` / ``betas`` / ``Tmax`` (extension; all None: the call is what it always was): fit with a
    parallel-tempered ensemble, :class:`~lightcurve_fitting_amd.sampler.TemperedSampler`, of ``nwalkers`` walkers per
    rung -- for degenerate or multi-modal posteriors, and for the log-evidence (``sampler.log_evidence()``).  Every
    rung starts uniform in the starting box; ``chain`` / ``flatchain`` of the returned sampler are the cold rung's.
    ``adapt=True`` (tempered fits only, ``ValueError`` otherwise; needs ``ntemps >= 3`` and ``Tmax=inf``): the ladder
    adapts during the burn-in until neighbouring rungs swap equally often, and is frozen for the stored run, so that
    ``sampler.log_evidence(method='stepping_stone')`` is over one ladder.

    ``moves`` (extension; emcee's argument: a move, or a list of moves or ``(move, weight)`` pairs of
    :class:`~lightcurve_fitting_amd.sampler.StretchMove`, :class:`~lightcurve_fitting_amd.sampler.DEMove` and
    :class:`~lightcurve_fitting_amd.sampler.DESnookerMove`), for posteriors with curved or narrow ridges: when given, the
    fit goes through :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` too -- on one rung at ``beta = 1`` unless a
    ladder is asked for as well -- and the keyword is passed on to it; None is not passed on.

    A :class:`~lightcurve_fitting_amd.models.CustomModel` is always fitted by that sampler -- without the tempering
    arguments on one rung at ``beta = 1``, which makes the ensemble sampler's moves -- because the resident sampler's
    kernels are compiled per built-in model; ``chain``, ``flatchain``, ``get_autocorr_time`` are the same,
    ``acceptance_fraction`` has a leading axis of length one.  So are the central-engine models
    (:class:`~lightcurve_fitting_amd.models.Arnett`, :class:`~lightcurve_fitting_amd.models.Magnetar`), whose ``lc`` is a
    bolometric light curve (``MJD``, ``L_bol``, ``dL_bol``; no magnitudes are converted).

    ``nondet`` (extension; ``'gaussian'``: the call is what it always was): with ``'censored'`` the rows of ``lc`` whose
    ``nondet`` is true are upper limits -- each adds ``ln Phi((limit - model) / sigma)`` to the likelihood instead of
    entering the Gaussian sum as a measurement of zero (``Model.log_likelihood`` has the definition).  The resident
    sampler's kernels compute the likelihood themselves and do not know the term, so a light curve that has such rows
    is fitted by :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` as well -- on one rung at ``beta = 1`` unless
    a ladder or ``moves`` is asked for -- and a ladder tempers the term with the rest of the likelihood.  Without a
    true ``nondet`` row the fit is the default one.

    A :class:`~lightcurve_fitting_amd.models.WithTemplate` model (a shock model plus a stretched template) is fitted by
    :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` for the same reason, on one rung at ``beta = 1`` unless a
    ladder or ``moves`` is asked for; ``nondet='censored'`` with it raises ``ValueError`` (out of scope).

    Returns the sampler (``.chain`` (nwalkers, nsteps, ndim), ``.flatchain``, ``.run_mcmc``, ``.reset``).
    """
    import time
    marks = [('call', time.perf_counter())]
    if model_kwargs is not None:
        raise Exception(MODEL_KWARGS_WARNING)
    if adapt and ntemps is None and betas is None and Tmax is None:
        raise ValueError('adapt=True adapts a temperature ladder: give ntemps, betas or Tmax')
    _prepare_photometry(lc, model)
    if use_sigma and model.input_names[-1] != '\\sigma':   # the intrinsic-scatter parameter joins the model's own
        model.input_names.append('\\sigma')
        model.units.append('')
    ndim = model.nparams

    p_min = _bound_vector(p_min, ndim, -np.inf, deprecated=True)
    p_max = _bound_vector(p_max, ndim, np.inf, deprecated=True)
    p_lo = _bound_vector(p_lo, ndim, None, name='p_lo', fallback=p_min)
    if p_up is None:
        raise Exception('p_up must have length {:d}'.format(ndim))
    p_up = _bound_vector(p_up, ndim, None, name='p_up')
    priors = _resolve_priors(priors, p_min, p_max, ndim)
    _check_start_box(model.input_names, priors, p_lo, p_up)

    # log_posterior of fitting.py:121-128 lives on the device: priors are baked into the engine
    marks.append(('checks', time.perf_counter()))
    engine = model.engine_for(lc, use_sigma=use_sigma, sigma_type=sigma_type, priors=priors, nondet=nondet)
    marks.append(('engine', time.perf_counter()))
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2 ** 31 + int(np.random.randint(0, 2 ** 31 - 1))
    if (isinstance(model, (CustomModel, BaseCentralEngine, WithTemplate)) or moves is not None
            or getattr(engine, 'nlimits', 0)) and ntemps is None and betas is None and Tmax is None:
        # the resident sampler's kernels are compiled per photometric model, make the stretch move and know neither
        # upper limits nor a second component: one rung is the same ensemble
        betas = [1.]
    if ntemps is not None or betas is not None or Tmax is not None:
        from .sampler import TemperedSampler
        sampler = TemperedSampler(nwalkers, ndim, engine, ntemps=ntemps, betas=betas, Tmax=Tmax, seed=seed,
                                  names=model.input_names, **({} if moves is None else {'moves': moves}))
        start = p_lo + (p_up - p_lo) * np.random.rand(sampler.ntemps, nwalkers, ndim)
        marks.append(('sampler', time.perf_counter()))
        sampler.run_mcmc(start, nsteps_burnin, store=False, adapt=bool(adapt))
        marks.append(('burn_in', time.perf_counter()))
        if show or save_plot_as:
            warnings.warn('chain plots are not produced by the MI355X engine; plot sampler.chain with the reference tools')
        sampler.run_mcmc(None, nsteps)
        return _finish_mcmc(sampler, engine, marks, save_sampler_as)
    sampler = EnsembleSampler(nwalkers, ndim, engine, seed=seed)

    start = p_lo + (p_up - p_lo) * np.random.rand(nwalkers, ndim)      # uniform in the starting box
    marks.append(('sampler', time.perf_counter()))
    burned_in = sampler.run_mcmc(start, nsteps_burnin)
    marks.append(('burn_in', time.perf_counter()))
    if show or save_plot_as:
        warnings.warn('chain plots are not produced by the MI355X engine; plot sampler.chain with the reference tools')
        # the left column of the reference's figure (fitting.py:135-158): the burn-in chain is gone after reset()
        # (no burn-in, or more walkers than chain_history takes: the call goes on as it always has, without it)
        from . import engine as _eng
        if sampler.iteration > 0 and nwalkers <= _eng.HISTORY_MAX_WALKERS:
            sampler.burnin_history = chain_history(model, sampler, use_sigma=bool(use_sigma))
    sampler.reset()                                                    # keep only the post-burn-in chain
    sampler.run_mcmc(burned_in.coords, nsteps, skip_initial_state_check=True)
    return _finish_mcmc(sampler, engine, marks, save_sampler_as)


def _finish_mcmc(sampler, engine, marks, save_sampler_as):
    """The end of ``lightcurve_mcmc`` for either sampler: the call's timings, and the flatchain saved if asked."""
    import time
    marks.append(('run', time.perf_counter()))
    #: seconds of this call, phase by phase, up to the chain complete in HBM (it crosses PCIe when it is first read):
    #: argument checks and photometry; the engine (band tables packed on the host + device engine created; ~0 when the
    #: model already holds an engine for this photometry); sampler and starting positions; burn-in; the stored run
    sampler.timings = {name: t - t0 for (name, t), (_, t0) in zip(marks[1:], marks[:-1])}
    sampler.timings['total'] = marks[-1][1] - marks[0][1]
    sampler.timings['engine_parts'] = dict(getattr(engine, 'timings', {}))
    if save_sampler_as:
        print('saving sampler.flatchain as ' + save_sampler_as)
        np.save(save_sampler_as, sampler.flatchain)
    return sampler


# ---------------------------------------------------------------------------------------------------------------
# posterior-predictive light-curve bands (the numbers of lightcurve_model_plot, reference fitting.py:337-360)
# ---------------------------------------------------------------------------------------------------------------
def quantile_ranks(n_valid, q):
    """Which order statistics percentile ``q`` of ``n_valid`` sorted values lies between, and how far: ``(lo, hi,
    gamma)`` with ``h = (n_valid - 1) * q / 100``, ``lo = floor(h)``, ``hi = min(lo + 1, n_valid - 1)`` and
    ``gamma = h - lo`` -- NumPy's default (``'linear'``) method, and the definition the device kernels implement
    (``k_pq_pick``).  Arguments broadcast."""
    n = np.asarray(n_valid, dtype=np.int64)
    h = (n - 1) * (np.asarray(q, dtype=np.float64) / 100.)
    lo = np.floor(h)
    gamma = h - lo
    lo = lo.astype(np.int64)
    return lo, np.minimum(lo + 1, n - 1), gamma


def quantile_lerp(a, b, gamma):
    """The value ``gamma`` of the way from order statistic ``a`` to the next one ``b``, in the form NumPy evaluates it
    (and ``k_pq_finish`` does): from ``a`` below one half, from ``b`` above; ``a`` itself where ``gamma`` is 0."""
    a, b, gamma = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                                      np.asarray(gamma, dtype=np.float64))
    with np.errstate(invalid='ignore'):
        diff = b - a
        out = np.where(gamma >= 0.5, b - diff * (1. - gamma), a + diff * gamma)
    return np.where(gamma == 0., a, out)


def _predictive_times(lc, t, tmin, tmax, num, xscale):
    """The times of :func:`predictive_grid`."""
    if t is not None:
        times = np.array(t, dtype=np.float64).ravel()
    else:
        if tmin is None:
            tmin = np.min(_column(lc, 'MJD'))
        if tmax is None:
            tmax = np.max(_column(lc, 'MJD'))
        if xscale not in ('linear', 'log'):
            raise ValueError("xscale must be 'linear' or 'log'")
        times = np.geomspace(tmin, tmax, int(num)) if xscale == 'log' else np.linspace(tmin, tmax, int(num))
    if len(times) == 0 or not np.all(np.isfinite(times)):
        raise ValueError('the grid needs at least one time, all finite')
    return times


def predictive_grid(lc, t=None, tmin=None, tmax=None, num=1000, xscale='linear', filters_to_model=None):
    """The ``filters x times`` grid of ``lightcurve_model_plot`` (fitting.py:340-348): ``t`` if given, else ``num``
    points from ``tmin`` to ``tmax`` (default: the range of ``lc['MJD']``), equally spaced (``xscale='linear'``) or
    geometrically (``'log'``); the filters of ``filters_to_model``, else the distinct filters of ``lc``, sorted.
    Returns ``(times, filters)``."""
    times = _predictive_times(lc, t, tmin, tmax, num, xscale)
    if filters_to_model is None:
        filters = sorted(set(as_filter(f) for f in _column(lc, 'filter')))
    else:
        filters = [as_filter(f) for f in filters_to_model]
    if len(filters) == 0:
        raise ValueError('the grid needs at least one filter')
    return times, filters


class PosteriorPredictive:
    """Result of :func:`posterior_predictive`: ``t`` (nt,), ``filters`` (nf Filter objects), ``percentiles`` (nq,),
    ``quantiles`` (nq, nf, nt), ``n_valid`` (nf, nt) -- the samples whose model value at the point is not NaN -- and
    ``n_samples``."""
    __slots__ = ('t', 'filters', 'percentiles', 'quantiles', 'n_valid', 'n_samples')

    def __init__(self, t, filters, percentiles, quantiles, n_valid, n_samples):
        self.t, self.filters, self.percentiles = t, filters, percentiles
        self.quantiles, self.n_valid, self.n_samples = quantiles, n_valid, n_samples

    def __repr__(self):
        return (f'<PosteriorPredictive: {len(self.percentiles)} percentiles x {len(self.filters)} filters x '
                f'{len(self.t)} times over {self.n_samples} samples>')


def _predictive_samples(samples, discard, thin):
    """``(sampler or None, host array or None, n_samples, n_columns)`` after the checks that need no device."""
    if isinstance(samples, EnsembleSampler) or (hasattr(samples, '_native') and hasattr(samples, 'get_chain')):
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1:
            raise ValueError('need discard >= 0 and thin >= 1')
        if samples.iteration == 0:
            raise ValueError('no chain is stored: run the sampler with store=True first')
        n_t = len(range(discard, samples.iteration, thin))
        if n_t == 0:
            raise ValueError(f'discard={discard} leaves no steps of the {samples.iteration} stored')
        return samples, None, n_t * samples.nwalkers, samples.ndim
    if discard != 0 or thin != 1:
        raise ValueError('discard and thin apply to a sampler; slice the array of samples instead')
    P = np.ascontiguousarray(samples, dtype=np.float64)
    if P.ndim != 2:
        raise ValueError('samples must be a sampler or an array of shape (n_samples, n_columns)')
    if P.shape[0] == 0:
        raise ValueError('no samples')
    return None, P, P.shape[0], P.shape[1]


def _percentile_array(percentiles):
    q = np.array(percentiles, dtype=np.float64).ravel()
    if q.size == 0:
        raise ValueError('percentiles must not be empty')
    if not np.all((q >= 0.) & (q <= 100.)):
        raise ValueError('percentiles must be in the range [0, 100]')
    return q


def _refuse_custom(model, what):
    """The predictive kernels are compiled per built-in photometric model: a ``CustomModel`` and the central-engine
    models (``Arnett``, ``Magnetar``) are refused before anything is built, and so is a ``WithTemplate`` model."""
    _refuse_template(model, what)
    if isinstance(model, CustomModel):
        from .engine import LcfError
        raise LcfError(5, f'{what} is compiled per built-in model and does not take a CustomModel; its fit (the '
                          'tempered route, TemperedSampler) gives the chain, custom_predictive the bands of its light '
                          'curves, T, R and L over that chain, and model(t, filters, *p) evaluates any of its rows')
    if isinstance(model, BaseCentralEngine):
        from .engine import LcfError
        raise LcfError(5, f'{what} is compiled per photometric model and does not take a central-engine model (Arnett, '
                          'Magnetar); its fit (the tempered route, TemperedSampler) gives the chain, model(t, *p) '
                          'evaluates any of its rows, and luminosity_predictive gives the bands of L(t)')


def _refuse_template(model, what):
    """The predictive kernels evaluate the model themselves and do not know a second component."""
    if isinstance(model, WithTemplate):
        from .engine import LcfError
        raise LcfError(5, f'{what} computes the model in kernels of its own, which do not know a second component: '
                          'template_predictive gives the bands of a WithTemplate model, of its two terms, and the dip '
                          'and hand-over between them, over the chain its fit (the tempered route, TemperedSampler) '
                          'gives; its colours and thermal bands are out of scope, and model(t, f, *p) on a thinned chain '
                          'evaluates its rows (model.components(t, f, *p) the two terms)')


def _model_samples(model, samples, discard, thin, use_sigma):
    """:func:`_predictive_samples` and the column count ``model`` wants: ``(sampler or None, host array or None,
    n_samples)``."""
    sampler, P, n_samples, n_col = _predictive_samples(samples, discard, thin)
    want = model.n_model_params + int(bool(use_sigma))
    if n_col != want:
        raise ValueError(f'the samples have {n_col} columns, the model takes {model.n_model_params}'
                         + (' and one for sigma' if use_sigma else ''))
    return sampler, P, n_samples


def _sample_source(sampler, P, discard, thin):
    """What the native call reads: the sampler's chain where it lies when its whole stored chain is the last run's, else
    the host rows."""
    if sampler is not None and not (len(sampler._chain_host) == 0 and sampler._chain_on_device > 0):
        P, sampler = sampler.get_chain(discard=int(discard), thin=int(thin), flat=True), None
    return sampler._native if sampler is not None else P


def posterior_predictive(lc, model, samples, percentiles=(15.87, 50., 84.14), t=None, tmin=None, tmax=None,
                         num=1000, xscale='linear', filters_to_model=None, discard=0, thin=1, use_sigma=False,
                         component='model', workspace_bytes=None):
    """Percentile bands of the model light curves over ALL samples of a chain, on the dense ``filters x times`` grid
    of ``lightcurve_model_plot`` (fitting.py:337-360; see :func:`predictive_grid` for ``t`` ... ``filters_to_model``).

    ``samples``: the sampler ``lightcurve_mcmc`` returned -- rows ``discard::thin`` of its stored chain, read where
    they lie in device memory when the whole stored chain is the last run's, else uploaded from ``get_chain`` -- or a
    host array ``(n_samples, n_columns)`` such as a saved ``flatchain`` (``discard`` / ``thin`` do not apply).
    ``use_sigma``: the last column is the intrinsic scatter and does not enter the model (fitting.py:349-352).
    ``component``: ``'model'``, or ``'sifto'`` for the SiFTO term of a companion-shocking model alone (the template at the
    sample's stretch and offsets times the filter's factor, 0 outside the template; fitting.py:355-360).

    For every grid point the values of all samples are taken, NaNs dropped (``n_valid`` remain), and the percentiles
    interpolated linearly between order statistics: ``np.nanpercentile(Y, percentiles, axis=samples)`` with NumPy's
    default method, NaN where ``n_valid`` is 0.  No value is stored per (sample, point): device memory beyond the
    samples stays below ``workspace_bytes`` (default 1 GiB), the times being worked through in tiles.  Results are
    bitwise reproducible and do not depend on ``workspace_bytes``.  Returns a :class:`PosteriorPredictive`."""
    from . import engine as _eng
    _refuse_custom(model, 'posterior_predictive')
    q = _percentile_array(percentiles)
    if component not in ('model', 'sifto'):
        raise ValueError("component must be 'model' or 'sifto'")
    if component == 'sifto' and not isinstance(model, BaseCompanionShocking):
        raise ValueError("component='sifto' needs a companion-shocking model")
    sampler, P, n_samples = _model_samples(model, samples, discard, thin, use_sigma)
    times, filters = predictive_grid(lc, t, tmin, tmax, num, xscale, filters_to_model)
    if len(filters) > _eng.PREDICT_MAX_SEARCHES:
        raise ValueError(f'at most {_eng.PREDICT_MAX_SEARCHES} filters')

    grid_engine, shape = Model._eval_engine(model, times, filters, False)   # the dense grid, filter-major
    source = _sample_source(sampler, P, discard, thin)
    comp = _eng.COMPONENT_SIFTO if component == 'sifto' else _eng.COMPONENT_MODEL
    per_call = max(1, _eng.PREDICT_MAX_SEARCHES // len(filters))
    quantiles, n_valid = [], None
    for k in range(0, len(q), per_call):
        out, n_valid = _eng.predict_quantiles(grid_engine, source, q[k:k + per_call], comp, workspace_bytes,
                                              discard=int(discard), thin=int(thin))
        quantiles.append(out)
    quantiles = np.concatenate(quantiles).reshape((len(q),) + shape)
    return PosteriorPredictive(times, filters, q, quantiles, n_valid.reshape(shape), n_samples)


# ---------------------------------------------------------------------------------------------------------------
# colour bands and per-band peaks (the model's side of calc_colors / plot_color_curves, bolometric.py:559-605)
# ---------------------------------------------------------------------------------------------------------------
class ColorPredictive:
    """Result of :func:`color_predictive`: ``t`` (nt,), ``colors`` (nc pairs of Filter objects), ``color_names`` (nc
    strings ``'X-Y'``), ``filters`` (nf Filter objects: the distinct filters of the colours, sorted), ``percentiles``
    (nq,), ``color`` [mag] (nq, nc, nt), ``n_valid`` (nc, nt) -- the samples that have the colour at the time -- and
    ``n_samples``.  With ``peak=True``, per sample and filter over the times in ascending order: ``y_peak`` (n, nf) in
    the model's ``output_quantity``, ``peak_index`` (n, nf) int32 into ``t`` (-1: NaN everywhere), ``t_peak`` (n, nf),
    ``M_peak`` (n, nf) [mag] (NaN where ``y_peak`` is not positive), and the counts ``n_peak_first`` / ``n_peak_last``
    (nf,) of samples that peak at an edge of the grid (their true peak may lie outside it); else all ``None``."""
    __slots__ = ('t', 'colors', 'color_names', 'filters', 'percentiles', 'color', 'n_valid', 'n_samples', 'y_peak',
                 'peak_index', 't_peak', 'M_peak', 'n_peak_first', 'n_peak_last')

    def __init__(self, t, colors, color_names, filters, percentiles, color, n_valid, n_samples):
        self.t, self.colors, self.color_names, self.filters = t, colors, color_names, filters
        self.percentiles, self.color, self.n_valid, self.n_samples = percentiles, color, n_valid, n_samples
        self.y_peak = self.peak_index = self.t_peak = self.M_peak = self.n_peak_first = self.n_peak_last = None

    def set_peaks(self, y_peak, peak_index, zero_points):
        """Attach the peaks: ``y_peak`` / ``peak_index`` (n, nf) as the device returns them, ``zero_points`` (nf,) the
        magnitude of a unit value per filter.  Everything else follows on the host."""
        y_peak = np.asarray(y_peak, dtype=np.float64)
        peak_index = np.asarray(peak_index, dtype=np.int32)
        self.y_peak, self.peak_index = y_peak, peak_index
        self.t_peak = np.where(peak_index < 0, np.nan, np.asarray(self.t)[np.maximum(peak_index, 0)])
        with np.errstate(invalid='ignore', divide='ignore'):
            mag = np.asarray(zero_points, dtype=np.float64) - 2.5 * np.log10(y_peak)
        self.M_peak = np.where(y_peak > 0., mag, np.nan)
        self.n_peak_first = np.sum(peak_index == 0, axis=0)
        self.n_peak_last = np.sum(peak_index == len(self.t) - 1, axis=0)

    def peak_summary(self, percentiles=(15.87, 50., 84.14)):
        """``{'M_peak': (nq, nf), 't_peak': (nq, nf)}``: ``np.nanpercentile`` over the samples, per filter."""
        if self.peak_index is None:
            raise ValueError('the peaks were not computed: call color_predictive with peak=True')
        q = _percentile_array(percentiles)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)   # (every sample NaN: NaN)
            return {name: np.nanpercentile(getattr(self, name), q, axis=0) for name in ('M_peak', 't_peak')}

    def __repr__(self):
        return (f'<ColorPredictive: {len(self.percentiles)} percentiles x {len(self.colors)} colours x '
                f'{len(self.t)} times over {self.n_samples} samples'
                + ('' if self.peak_index is None else f', with peaks in {len(self.filters)} filters') + '>')


def parse_colors(colors):
    """The colours of :func:`color_predictive`: each ``'X-Y'``, split at the first ``-`` and looked up in ``filtdict``
    (as ``calc_colors`` does), or a ``(filter, filter)`` pair of names or ``Filter`` objects.  Returns ``(pairs, names,
    filters, index, dzp)``: the (Filter, Filter) pairs, their ``'X-Y'`` names, the distinct filters sorted, the pairs
    as indices (nc, 2) into them, and ``m0_a - m0_b`` per colour.  ``ValueError`` for an empty list, an unknown filter,
    a filter without a zero point, a colour of a filter with itself and more than 16 distinct filters."""
    from .engine import COLOR_MAX_FILTERS
    from .filters import Filter, filtdict
    if isinstance(colors, str):
        colors = [colors]
    colors = list(colors)
    if len(colors) == 0:
        raise ValueError('colors must not be empty')

    def lookup(f, color):
        if isinstance(f, Filter):
            return f
        try:
            return filtdict[str(f)]
        except KeyError:
            raise ValueError(f'colour {color!r}: unrecognised filter {f!r}') from None

    pairs = []
    for color in colors:
        if isinstance(color, str):
            if '-' not in color:
                raise ValueError(f"colour {color!r} is not of the form 'X-Y'")
            ends = color.split('-', 1)
        else:
            ends = list(color)
            if len(ends) != 2:
                raise ValueError(f'colour {color!r} is not a pair of filters')
        a, b = lookup(ends[0], color), lookup(ends[1], color)
        for f in (a, b):
            if not np.isfinite(f.m0):
                raise ValueError(f'colour {color!r}: filter {f.name!r} has no zero point')
        if a == b:
            raise ValueError(f'colour {color!r} is of a filter with itself')
        pairs.append((a, b))
    filters = sorted(set(f for pair in pairs for f in pair))
    if len(filters) > COLOR_MAX_FILTERS:
        raise ValueError(f'the colours name {len(filters)} distinct filters: at most {COLOR_MAX_FILTERS}')
    where = {f: i for i, f in enumerate(filters)}
    index = np.array([[where[a], where[b]] for a, b in pairs], dtype=np.int32)
    dzp = np.array([a.m0 - b.m0 for a, b in pairs], dtype=np.float64)
    return pairs, [f'{a.name}-{b.name}' for a, b in pairs], filters, index, dzp


def color_predictive(lc, model, samples, colors=('B-V', 'g-r', 'r-i'), percentiles=(15.87, 50., 84.14), t=None,
                     tmin=None, tmax=None, num=1000, xscale='linear', discard=0, thin=1, use_sigma=False, peak=True,
                     workspace_bytes=None):
    """Percentile bands of the model's colour curves over ALL samples of a chain, and every sample's peak in every
    filter the colours name: the model's side of ``calc_colors`` / ``plot_color_curves``, with its uncertainty.

    ``samples``, ``discard``, ``thin``, ``use_sigma``, ``workspace_bytes`` and the time grid ``t`` ... ``xscale`` as in
    :func:`posterior_predictive`; ``model``: every model it takes.  ``colors``: see :func:`parse_colors`; the grid's
    filters are the distinct filters of all colours, sorted, and a filter may occur in several colours.

    With ``Y[f, t, s] = model(t, filters, *p_s)`` -- the value :func:`posterior_predictive` ranks, in the model's
    ``output_quantity`` -- the colour ``(a, b)`` of a sample at a time is ``(m0_a - m0_b) - 2.5 log10(Y_a / Y_b)`` where
    both values are finite and positive, else NaN (not exploded yet; a NaN; a negative SiFTO tail), and ``color`` is
    ``np.nanpercentile`` of it over the samples: a property of the two filters' joint distribution, sample by sample,
    not a difference of per-filter percentiles.  ``n_valid`` counts the samples that have the colour; ``color`` is NaN
    where none has.  With ``peak=True`` the largest non-NaN ``Y`` of every (sample, filter) and the first time it is
    attained, the times walked in ascending order (``np.nanargmax`` on a sorted grid): a sample that has not exploded
    anywhere has ``y_peak == 0`` at the earliest time.  ``M_peak = zp - 2.5 log10(y_peak)`` with ``zp`` the filter's
    ``M0`` for a ``'lum'`` model and ``m0`` for a ``'flux'`` one.  Nothing is stored per (sample, time) except the
    peaks, 12 bytes per (sample, filter) beyond ``workspace_bytes`` (``engine.color_workspace``).  Results are bitwise
    reproducible and do not depend on ``workspace_bytes``.  Returns a :class:`ColorPredictive`."""
    from . import engine as _eng
    _refuse_custom(model, 'color_predictive')
    q = _percentile_array(percentiles)
    pairs, names, filters, index, dzp = parse_colors(colors)
    if len(pairs) > _eng.PREDICT_MAX_SEARCHES:
        raise ValueError(f'at most {_eng.PREDICT_MAX_SEARCHES} colours')
    sampler, P, n_samples = _model_samples(model, samples, discard, thin, use_sigma)
    times, _ = predictive_grid(lc, t, tmin, tmax, num, xscale, filters)

    grid_engine, _ = Model._eval_engine(model, times, filters, False)   # the dense grid, filter-major
    source = _sample_source(sampler, P, discard, thin)
    per_call = max(1, _eng.PREDICT_MAX_SEARCHES // len(pairs))
    bands, n_valid, y_peak, i_peak = [], None, None, None
    for k in range(0, len(q), per_call):
        out, n_valid, y_pk, i_pk = _eng.predict_colors(grid_engine, source, index, dzp, q[k:k + per_call],
                                                       workspace_bytes, peak=bool(peak) and k == 0,
                                                       discard=int(discard), thin=int(thin))
        bands.append(out)
        if k == 0:
            y_peak, i_peak = y_pk, i_pk
    res = ColorPredictive(times, pairs, names, filters, q, np.concatenate(bands), n_valid, n_samples)
    if peak:
        zero = [f.M0 if model.output_quantity == 'lum' else f.m0 for f in filters]
        res.set_peaks(y_peak.T, i_peak.T, zero)      # (views: the device's [filter][sample] arrays are not copied)
    return res


# ---------------------------------------------------------------------------------------------------------------
# thermal bands and validity (temperature_radius over the whole chain; t_min / t_max, the 0.7 eV floor)
# ---------------------------------------------------------------------------------------------------------------
class ThermalPredictive:
    """Result of :func:`thermal_predictive`: ``t`` (nt,), ``percentiles`` (nq,); ``temperature`` [kK], ``radius``
    [1000 Rsun] and ``luminosity`` [W], each (nq, nt); ``n_valid`` (3, nt) -- the non-NaN values of the three, in that
    order; ``n_cold`` (nt,) -- samples with a temperature below ``T_floor``; ``n_inside`` (nt,) -- samples whose validity
    window holds the time; ``n_samples``."""
    __slots__ = ('t', 'percentiles', 'temperature', 'radius', 'luminosity', 'n_valid', 'n_cold', 'n_inside', 'n_samples')

    def __init__(self, t, percentiles, temperature, radius, luminosity, n_valid, n_cold, n_inside, n_samples):
        self.t, self.percentiles = t, percentiles
        self.temperature, self.radius, self.luminosity = temperature, radius, luminosity
        self.n_valid, self.n_cold, self.n_inside = n_valid, n_cold, n_inside
        self.n_samples = n_samples

    @property
    def frac_cold(self):
        """Fraction of the samples with a temperature that are below the floor, per time (NaN where none has one)."""
        with np.errstate(invalid='ignore', divide='ignore'):
            return self.n_cold / self.n_valid[0]

    @property
    def frac_inside(self):
        """Fraction of all samples whose validity window holds the time, per time."""
        return self.n_inside / self.n_samples

    def __repr__(self):
        return (f'<ThermalPredictive: {len(self.percentiles)} percentiles x {len(self.t)} times over '
                f'{self.n_samples} samples>')


def _thermal_filter(model):
    """Any filter the model can build an engine for: the thermal state does not depend on it."""
    f = model._any_filter()
    if isinstance(model, BaseCompanionShocking) and f not in model.sifto:
        f = next(iter(model.sifto))
    return f


def thermal_predictive(lc, model, samples, percentiles=(15.87, 50., 84.14), t=None, tmin=None, tmax=None,
                       num=1000, xscale='linear', discard=0, thin=1, use_sigma=False, T_floor=8.12,
                       workspace_bytes=None):
    """Percentile bands of the blackbody temperature [kK], radius [1000 Rsun] and bolometric luminosity [W] behind the
    model light curves over ALL samples of a chain, and how many samples the model is valid for, time by time.

    ``samples``, ``discard``, ``thin``, ``use_sigma``, ``workspace_bytes`` and the time grid ``t`` ... ``xscale`` as in
    :func:`posterior_predictive`.  ``model``: any of the seven reference models; for the companion-shocking models the
    quantities are those of the shock component.  T and R are ``model.temperature_radius`` of every (sample, time)
    pair, the luminosity ``bolometric.stefan_boltzmann(T, R)`` of that pair (not of the T and R percentiles); the
    percentiles of each are ``np.nanpercentile(..., axis=samples)``, NaN where no sample has a value.

    The models hold above ``T_floor`` (0.7 eV = 8.12 kK) and inside ``model.t_min(p) <= t <= model.t_max(p)`` (opacity
    kappa = 1; ``ShockCooling2`` has no lower bound): ``n_cold[t]`` counts the samples with T < ``T_floor`` -- T is
    exactly 0 before a sample's explosion time, which counts -- and ``n_inside[t]`` those whose window holds ``t``; a
    NaN bound holds nothing.  Nothing is stored per (sample, time) and all counts are exact.  Returns a
    :class:`ThermalPredictive`."""
    from . import engine as _eng
    _refuse_custom(model, 'thermal_predictive')
    if isinstance(model, Blackbody):
        raise ValueError('the Blackbody model has no thermal evolution or validity window')
    q = _percentile_array(percentiles)
    sampler, P, n_samples = _model_samples(model, samples, discard, thin, use_sigma)
    filt = _thermal_filter(model)
    times, _ = predictive_grid(lc, t, tmin, tmax, num, xscale, [filt])
    distinct, where = np.unique(times, return_inverse=True)     # the engine holds one point per distinct time

    grid_engine, _ = Model._eval_engine(model, distinct, [filt] * len(distinct))
    source = _sample_source(sampler, P, discard, thin)
    per_call = _eng.PREDICT_MAX_SEARCHES // _eng.THERMAL_SERIES
    parts = [_eng.predict_thermal(grid_engine, source, q[k:k + per_call], T_floor, workspace_bytes,
                                  discard=int(discard), thin=int(thin)) for k in range(0, len(q), per_call)]
    quantiles = np.concatenate([part[0] for part in parts], axis=1)[:, :, where]
    _, n_valid, n_cold, n_inside = parts[0]
    return ThermalPredictive(times, q, quantiles[0], quantiles[1], quantiles[2], n_valid[:, where], n_cold[where],
                             n_inside[where], n_samples)


# ---------------------------------------------------------------------------------------------------------------
# luminosity bands and peaks (the central-engine models: does the fit go through the data, L_peak, t_rise)
# ---------------------------------------------------------------------------------------------------------------
class LuminosityPredictive:
    """Result of :func:`luminosity_predictive`: ``t`` (nt,), ``percentiles`` (nq,), ``luminosity`` [W] (nq, nt);
    ``n_valid`` (nt,) -- the samples whose ``L`` at the time is not NaN; ``n_dark`` (nt,) -- those whose ``L`` is exactly
    ``+0.0``: not exploded yet; ``n_samples``.  With ``peak=True``, per sample over the distinct times in ascending
    order: ``peak_index`` (int32, into ``np.unique(t)``; -1: NaN everywhere), ``L_peak`` [W], ``t_peak`` [MJD],
    ``t_rise`` [d, rest frame], and the counts ``n_peak_first`` / ``n_peak_last`` of samples that peak at an edge of
    the grid (their true peak may lie outside it); else all ``None``."""
    __slots__ = ('t', 'percentiles', 'luminosity', 'n_valid', 'n_dark', 'n_samples', 'peak_index', 'L_peak', 't_peak',
                 't_rise', 'n_peak_first', 'n_peak_last')

    def __init__(self, t, percentiles, luminosity, n_valid, n_dark, n_samples, peak_index=None, L_peak=None,
                 t_peak=None, t_rise=None, n_peak_first=None, n_peak_last=None):
        self.t, self.percentiles, self.luminosity = t, percentiles, luminosity
        self.n_valid, self.n_dark, self.n_samples = n_valid, n_dark, n_samples
        self.peak_index, self.L_peak, self.t_peak, self.t_rise = peak_index, L_peak, t_peak, t_rise
        self.n_peak_first, self.n_peak_last = n_peak_first, n_peak_last

    @property
    def frac_dark(self):
        """Fraction of the samples with a value that have not exploded yet, per time (NaN where none has one)."""
        with np.errstate(invalid='ignore', divide='ignore'):
            return self.n_dark / self.n_valid

    def peak_summary(self, percentiles=None):
        """``{'L_peak': ..., 't_peak': ..., 't_rise': ...}``: ``np.nanpercentile`` of the per-sample arrays at
        ``percentiles`` (default: those of the bands)."""
        if self.peak_index is None:
            raise ValueError('the peaks were not computed: call luminosity_predictive with peak=True')
        q = self.percentiles if percentiles is None else _percentile_array(percentiles)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)   # (every sample NaN: NaN)
            return {name: np.nanpercentile(getattr(self, name), q) for name in ('L_peak', 't_peak', 't_rise')}

    def __repr__(self):
        return (f'<LuminosityPredictive: {len(self.percentiles)} percentiles x {len(self.t)} times over '
                f'{self.n_samples} samples' + ('' if self.peak_index is None else ', with peaks') + '>')


def luminosity_predictive(lc, model, samples, percentiles=(15.87, 50., 84.14), t=None, tmin=None, tmax=None, num=1000,
                          xscale='linear', discard=0, thin=1, use_sigma=False, peak=True, workspace_bytes=None):
    """Percentile bands of the bolometric light curve ``L(t)`` [W] of a central-engine model (``Arnett``,
    ``Magnetar``) over ALL samples of a chain, and every sample's peak: what :func:`posterior_predictive` is for the
    photometric models, plus the two numbers quoted from such a fit.

    ``samples``: a host array ``(n_samples, n_columns)`` (``discard`` / ``thin`` do not apply), or the
    :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` that ``lightcurve_mcmc`` returned -- any object with its
    ``get_chain`` --: rows ``discard::thin`` of its cold rung, uploaded.  ``use_sigma``: the last column is the scatter
    and does not enter the model.  The time grid ``t`` ... ``xscale`` as in :func:`predictive_grid`, without filters.

    ``luminosity`` is ``np.nanpercentile(L, percentiles, axis=samples)`` of ``L[s, t] = model(t, *p_s)``, bit for bit
    those values, NaN where no sample has one.  With ``peak=True`` the largest non-NaN ``L`` of every sample over the
    distinct grid times, the first time it is attained (``np.nanargmax``), and ``t_rise = (t_peak - t_0) / (1 + z)``.
    Every (sample, time) value is evaluated once on the device and kept there as an 8-byte key while the percentiles of
    its time are searched; the times are worked through in tiles that keep device memory beyond the samples below
    ``workspace_bytes`` (default 1 GiB; ``engine.luminosity_workspace``).  Results are bitwise reproducible and do not
    depend on ``workspace_bytes``.  Returns a :class:`LuminosityPredictive`."""
    from . import engine as _eng
    _refuse_template(model, 'luminosity_predictive')
    if not isinstance(model, BaseCentralEngine):
        raise _eng.LcfError(5, 'luminosity_predictive takes a central-engine model (Arnett, Magnetar); the bands of a '
                               'photometric model are posterior_predictive and thermal_predictive')
    q = _percentile_array(percentiles)
    if not isinstance(samples, np.ndarray) and hasattr(samples, 'get_chain'):
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1:
            raise ValueError('need discard >= 0 and thin >= 1')
        samples = samples.get_chain(discard=discard, thin=thin, flat=True)
        if len(samples) == 0:
            raise ValueError(f'discard={discard} leaves no steps of the stored chain')
        discard, thin = 0, 1
    _, P, n_samples = _model_samples(model, samples, discard, thin, use_sigma)
    times = _predictive_times(lc, t, tmin, tmax, num, xscale)
    distinct, where = np.unique(times, return_inverse=True)     # ascending: "first" below is the earliest time

    grid_engine = model._grid_engine(distinct)
    per_call = _eng.PREDICT_MAX_SEARCHES
    parts = [_eng.predict_luminosity(grid_engine, P, q[k:k + per_call], workspace_bytes, peak=bool(peak) and k == 0)
             for k in range(0, len(q), per_call)]
    bands = np.concatenate([part[0] for part in parts])[:, where]
    _, n_valid, n_dark, L_peak, i_peak = parts[0]
    res = LuminosityPredictive(times, q, bands, n_valid[where], n_dark[where], n_samples)
    if peak:
        none = i_peak < 0
        res.peak_index, res.L_peak = i_peak, L_peak
        res.t_peak = np.where(none, np.nan, distinct[np.maximum(i_peak, 0)])
        res.t_rise = (res.t_peak - P[:, model.n_model_params - 1]) / (1. + model.z)
        res.n_peak_first = int(np.sum(i_peak == 0))
        res.n_peak_last = int(np.sum(i_peak == len(distinct) - 1))
    return res


# ---------------------------------------------------------------------------------------------------------------
# bands of a custom model (its light curves and the T, R, L behind them: does the fit go through the data, and is the
# photosphere the user wrote physical over the whole chain)
# ---------------------------------------------------------------------------------------------------------------
class CustomPredictive:
    """Result of :func:`custom_predictive`: ``t`` (nt,), ``filters`` (nf Filter objects), ``percentiles`` (nq,),
    ``n_samples``; ``quantiles`` (nq, nf, nt) of the model light curves, ``n_valid`` (nf, nt) -- the samples whose
    value is not NaN -- and ``n_dark`` (nf, nt) -- those whose value is exactly ``+0.0``: no photosphere yet;
    ``temperature`` [kK], ``radius`` [1000 Rsun] and ``luminosity`` [W], each (nq, nt), with ``n_valid_thermal`` (3, nt)
    in that order; with a ``T_floor``, ``n_cold`` (nt,) -- the samples with a temperature below it -- else ``None``."""
    __slots__ = ('t', 'filters', 'percentiles', 'n_samples', 'quantiles', 'n_valid', 'n_dark', 'temperature', 'radius',
                 'luminosity', 'n_valid_thermal', 'n_cold')

    def __init__(self, t, filters, percentiles, n_samples, quantiles, n_valid, n_dark, temperature, radius, luminosity,
                 n_valid_thermal, n_cold=None):
        self.t, self.filters, self.percentiles, self.n_samples = t, filters, percentiles, n_samples
        self.quantiles, self.n_valid, self.n_dark = quantiles, n_valid, n_dark
        self.temperature, self.radius, self.luminosity = temperature, radius, luminosity
        self.n_valid_thermal, self.n_cold = n_valid_thermal, n_cold

    @property
    def frac_cold(self):
        """Fraction of the samples with a temperature that are below the floor, per time (NaN where none has one);
        ``None`` without a ``T_floor``."""
        if self.n_cold is None:
            return None
        with np.errstate(invalid='ignore', divide='ignore'):
            return self.n_cold / self.n_valid_thermal[0]

    def __repr__(self):
        return (f'<CustomPredictive: {len(self.percentiles)} percentiles x ({len(self.filters)} filters + T, R, L) x '
                f'{len(self.t)} times over {self.n_samples} samples>')


def custom_predictive(lc, model, samples, percentiles=(15.87, 50., 84.14), t=None, tmin=None, tmax=None, num=1000,
                      xscale='linear', filters_to_model=None, discard=0, thin=1, use_sigma=False, T_floor=None,
                      workspace_bytes=None):
    """Percentile bands of the light curves of a :class:`~lightcurve_fitting_amd.models.CustomModel` over ALL samples
    of a chain, on the dense ``filters x times`` grid of :func:`predictive_grid`, and of the temperature [kK], radius
    [1000 Rsun] and bolometric luminosity [W] its state function returned for them: :func:`posterior_predictive` and
    :func:`thermal_predictive` for the models the user writes.

    ``samples``: a host array ``(n_samples, n_columns)`` (``discard`` / ``thin`` do not apply), or any object with
    ``get_chain`` -- the :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` that ``lightcurve_mcmc`` returned --:
    rows ``discard::thin`` of its cold rung, uploaded.  ``use_sigma``: the last column is the scatter and does not enter
    the model.  ``T_floor`` [kK]: count per time the samples colder than it (``n_cold``, ``frac_cold``; a temperature of
    exactly 0 -- no photosphere yet -- counts, a NaN does not); ``None``: no count.

    Every band is ``np.nanpercentile(values, percentiles, axis=samples)`` with NumPy's default method, NaN where no
    sample has a value: of ``model(t, filters, *p)``, of ``model.temperature_radius(t, *p)`` and of
    ``bolometric.stefan_boltzmann(T, R)`` of every (sample, time) pair.  The state function is evaluated once per pair
    on the device and its ``nf + 3`` values are kept there as 8-byte keys while the percentiles of their time are
    searched; the times are worked through in tiles that keep device memory beyond the samples below
    ``workspace_bytes`` (default 1 GiB; ``engine.custom_workspace``).  A sample's values do not depend on the samples
    evaluated with it; results are bitwise reproducible and do not depend on ``workspace_bytes``.  Returns a
    :class:`CustomPredictive`."""
    from . import engine as _eng
    _refuse_template(model, 'custom_predictive')
    if not isinstance(model, CustomModel):
        raise _eng.LcfError(5, 'custom_predictive takes a CustomModel; the bands of a built-in photometric model are '
                               'posterior_predictive and thermal_predictive, those of a central-engine model '
                               'luminosity_predictive')
    q = _percentile_array(percentiles)
    if not isinstance(samples, np.ndarray) and hasattr(samples, 'get_chain'):
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1:
            raise ValueError('need discard >= 0 and thin >= 1')
        samples = samples.get_chain(discard=discard, thin=thin, flat=True)
        if len(samples) == 0:
            raise ValueError(f'discard={discard} leaves no steps of the stored chain')
        discard, thin = 0, 1
    _, P, n_samples = _model_samples(model, samples, discard, thin, use_sigma)
    times, filters = predictive_grid(lc, t, tmin, tmax, num, xscale, filters_to_model)
    distinct, where = np.unique(times, return_inverse=True)     # the engine holds every (time, filter) pair once
    held = list(dict.fromkeys(filters))
    which = [held.index(f) for f in filters]

    grid_engine, _ = Model._eval_engine(model, distinct, held, False)   # the dense grid, filter-major
    nf = len(held)
    per_call = _eng.PREDICT_MAX_SEARCHES
    parts = [_eng.predict_custom(grid_engine, P, q[k:k + per_call], T_floor if k == 0 else None, workspace_bytes)
             for k in range(0, len(q), per_call)]
    bands = np.concatenate([part[0] for part in parts])[:, :, where]
    _, n_valid, n_dark, n_cold = parts[0]
    n_valid = n_valid[:, where]
    return CustomPredictive(times, filters, q, n_samples, bands[:, :nf][:, which], n_valid[:nf][which],
                            n_dark[:, where][which], bands[:, nf], bands[:, nf + 1], bands[:, nf + 2], n_valid[nf:],
                            None if n_cold is None else n_cold[where])


# ---------------------------------------------------------------------------------------------------------------
# bands and features of a template fit (a WithTemplate model: how much of the light is shock cooling and how much the
# second peak, when the second component takes over, where and how deep the dip between the peaks is)
# ---------------------------------------------------------------------------------------------------------------
class TemplatePredictive:
    """Result of :func:`template_predictive`: ``t`` (nt,), ``filters`` (nf Filter objects), ``percentiles`` (nq,),
    ``n_samples``, ``components`` (the names asked for, in the order total, base, template); ``quantiles[c]`` (nq, nf, nt)
    and ``n_valid[c]`` (nf, nt) -- the samples whose value is not NaN -- per component ``c`` (also ``.total``, ``.base``,
    ``.template``: ``None`` where not asked for); ``n_dark`` (nf, nt): the samples whose base term is exactly ``+0.0``,
    the shock has not started.  With ``features=True``, per filter and sample (nf, n), over the times in ascending order
    (the first occurrence wins, comparisons are on values, a NaN never wins): ``y_peak_base`` / ``i_peak_base`` and
    ``y_peak_template`` / ``i_peak_template`` -- the largest non-NaN base and template term and its index into ``t``
    (NaN and -1: none); ``i_cross`` -- the first index with template > base (-1: none); ``y_dip`` / ``i_dip`` -- the
    smallest non-NaN sum from the base's peak to the template's inclusive, defined only when the base peaks first (else
    NaN and -1); the times ``t_peak_base``, ``t_peak_template``, ``t_cross``, ``t_dip`` (NaN where the index is -1) and the
    counts ``n_cross_none``, ``n_dip_none`` (nf,); else all ``None``."""
    FEATURE_TIMES = ('t_peak_base', 't_peak_template', 't_cross', 't_dip')
    FEATURE_VALUES = ('y_peak_base', 'y_peak_template', 'y_dip')
    FEATURE_INDICES = ('i_peak_base', 'i_peak_template', 'i_cross', 'i_dip')
    __slots__ = ('t', 'filters', 'percentiles', 'n_samples', 'components', 'quantiles', 'n_valid', 'n_dark',
                 'n_cross_none', 'n_dip_none') + FEATURE_TIMES + FEATURE_VALUES + FEATURE_INDICES

    def __init__(self, t, filters, percentiles, n_samples, components, quantiles, n_valid, n_dark):
        self.t, self.filters, self.percentiles, self.n_samples = t, filters, percentiles, n_samples
        self.components, self.quantiles, self.n_valid, self.n_dark = components, quantiles, n_valid, n_dark
        for name in self.__slots__[8:]:
            setattr(self, name, None)

    total = property(lambda self: self.quantiles.get('total'))
    base = property(lambda self: self.quantiles.get('base'))
    template = property(lambda self: self.quantiles.get('template'))

    def set_features(self, values, indices):
        """Attach the features: ``values`` (3, nf, n) and ``indices`` (4, nf, n) into ``t``, in the order of
        ``FEATURE_VALUES`` / ``FEATURE_INDICES``.  The times and the counts follow on the host."""
        t = np.asarray(self.t, dtype=np.float64)
        for name, v in zip(self.FEATURE_VALUES, values):
            setattr(self, name, v)
        for name, t_name, i in zip(self.FEATURE_INDICES, self.FEATURE_TIMES, indices):
            setattr(self, name, i)
            setattr(self, t_name, np.where(i < 0, np.nan, t[np.maximum(i, 0)]))
        self.n_cross_none = np.sum(self.i_cross < 0, axis=1)
        self.n_dip_none = np.sum(self.i_dip < 0, axis=1)

    def feature_summary(self, percentiles=(15.87, 50., 84.14)):
        """``{name: (nq, nf)}`` for the four times and the three values: ``np.nanpercentile`` over the samples, per
        filter (NaN where no sample has the feature)."""
        if self.i_cross is None:
            raise ValueError('the features were not computed: call template_predictive with features=True')
        q = _percentile_array(percentiles)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)   # (every sample NaN: NaN)
            return {name: np.nanpercentile(getattr(self, name), q, axis=1)
                    for name in self.FEATURE_TIMES + self.FEATURE_VALUES}

    def __repr__(self):
        return (f'<TemplatePredictive: {len(self.percentiles)} percentiles x {len(self.components)} components x '
                f'{len(self.filters)} filters x {len(self.t)} times over {self.n_samples} samples'
                + ('' if self.i_cross is None else ', with features') + '>')


def _template_model(model):
    """``template_predictive`` takes a ``WithTemplate`` over a built-in shock-cooling base; everything else is refused
    before anything is built, naming the function that does take it."""
    from .engine import LcfError
    if isinstance(model, WithTemplate):
        if isinstance(model.base, CustomModel):
            raise LcfError(5, 'template_predictive computes the base model in kernels compiled per built-in model, and the '
                              'base of this WithTemplate is a CustomModel, compiled at run time: out of scope; '
                              'model(t, f, *p) and model.components(t, f, *p) on a thinned chain evaluate its rows and '
                              'their two terms')
        return
    if isinstance(model, CustomModel):
        route = 'custom_predictive gives the bands of a CustomModel'
    elif isinstance(model, BaseCentralEngine):
        route = 'luminosity_predictive gives the bands of a central-engine model (Arnett, Magnetar)'
    else:
        route = (f'posterior_predictive gives the bands of a {type(model).__name__} (thermal_predictive and '
                 'color_predictive its T, R, L and colours)')
    raise LcfError(5, f'template_predictive takes a WithTemplate model, which has two terms to tell apart; {route}')


def template_predictive(lc, model, samples, percentiles=(15.87, 50., 84.14), t=None, tmin=None, tmax=None, num=1000,
                        xscale='linear', filters_to_model=None, discard=0, thin=1, use_sigma=False,
                        components=('total', 'base', 'template'), features=True, workspace_bytes=None):
    """Percentile bands of a :class:`~lightcurve_fitting_amd.models.WithTemplate` fit over ALL samples of a chain, on the
    dense ``filters x times`` grid of :func:`predictive_grid` -- of the model, of its base term and of its template term
    -- and, per sample, what only the two curves jointly tell: the two peaks, when the template takes over, and the dip
    between the peaks.

    ``model``: a ``WithTemplate`` whose base is a ``ShockCooling``, ``ShockCooling2``, ``ShockCooling3`` or
    ``ShockCooling4`` (a ``CustomModel`` base and every other model raise ``LcfError`` naming their route).  ``samples``:
    a host array ``(n_samples, n_columns)`` (``discard`` / ``thin`` do not apply), or any object with ``get_chain`` -- the
    :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` that ``lightcurve_mcmc`` returned --: rows ``discard::thin``
    of its cold rung, uploaded.  ``use_sigma``: the last column is the scatter and does not enter the model.
    ``components``: which of ``'total'``, ``'base'``, ``'template'`` to rank.

    Per sample, filter ``f`` and time, exactly as ``model.components`` defines them: ``B`` the base model's value,
    ``Tm = r_f S_f((t - t_max - dt_f) (1 / s))`` the template term and ``Y = B + Tm``.  Every band is
    ``np.nanpercentile(values, percentiles, axis=samples)`` with NumPy's default method, NaN where no sample has a value;
    no value is stored per (sample, time): device memory beyond the samples stays below ``workspace_bytes`` (default
    1 GiB; ``engine.template_workspace``), the times being worked through in tiles.  With ``features`` one more launch
    walks every sample's curves (:class:`TemplatePredictive` has the definitions; 40 bytes per (sample, filter)).  At most
    16 distinct filters.  Results are bitwise reproducible and do not depend on ``workspace_bytes``.  Returns a
    :class:`TemplatePredictive`."""
    from . import engine as _eng
    _template_model(model)
    q = _percentile_array(percentiles)
    names, _ = _eng.template_components(components)
    if not isinstance(samples, np.ndarray) and hasattr(samples, 'get_chain'):
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1:
            raise ValueError('need discard >= 0 and thin >= 1')
        samples = samples.get_chain(discard=discard, thin=thin, flat=True)
        if len(samples) == 0:
            raise ValueError(f'discard={discard} leaves no steps of the stored chain')
        discard, thin = 0, 1
    _, P, n_samples = _model_samples(model, samples, discard, thin, use_sigma)
    times, filters = predictive_grid(lc, t, tmin, tmax, num, xscale, filters_to_model)
    distinct, first, where = np.unique(times, return_index=True, return_inverse=True)   # every (time, filter) pair once
    held = list(dict.fromkeys(filters))
    which = [held.index(f) for f in filters]
    if len(held) > _eng.TEMPLATE_MAX_FILTERS:
        raise ValueError(f'the grid has {len(held)} distinct filters: template_predictive takes at most '
                         f'{_eng.TEMPLATE_MAX_FILTERS} per call')

    grid_engine, _ = Model._eval_engine(model, distinct, held, False)   # the dense grid, filter-major, template attached
    per_call = max(1, _eng.PREDICT_MAX_SEARCHES // (len(names) * len(held)))
    parts = [_eng.predict_template(grid_engine, P, q[k:k + per_call], names, workspace_bytes)
             for k in range(0, len(q), per_call)]
    bands = np.concatenate([part[0] for part in parts])[:, :, which][..., where]
    _, n_valid, n_dark, _ = parts[0]
    n_valid = n_valid[:, which][..., where]
    res = TemplatePredictive(times, filters, q, n_samples, names, {c: bands[:, k] for k, c in enumerate(names)},
                             {c: n_valid[k] for k, c in enumerate(names)}, n_dark[which][:, where])
    if features:
        values, indices = _eng.template_features(grid_engine, P)
        # (an index is into the distinct times, ascending: to the first place of that time in t)
        indices = np.where(indices < 0, -1, first[np.maximum(indices, 0)]).astype(np.int32)
        res.set_features(values[:, which], indices[:, which])
    return res


# ---------------------------------------------------------------------------------------------------------------
# corner histograms (what corner.corner counts for lightcurve_corner, fitting.py:241-253, over the whole chain)
# ---------------------------------------------------------------------------------------------------------------
#: corner.hist2d's default contour levels: the mass inside 0.5, 1, 1.5 and 2 sigma of a two-dimensional Gaussian
CORNER_LEVELS = tuple(1. - np.exp(-0.5 * np.arange(0.5, 2.1, 0.5) ** 2))
#: the columns lightcurve_corner shifts by ``t0_offset`` (fitting.py:243)
CORNER_TIME_NAMES = ('t_0', 't_\\mathrm{max}')


class CornerData:
    """Result of :func:`posterior_corner` for P columns: ``names`` and ``labels`` (P strings each), ``offsets`` (P,) --
    what was subtracted from each column -- ``range`` (P, 2) and ``edges`` (P, bins + 1) in shifted coordinates,
    ``hist1d`` (P, bins) and ``hist2d`` (P, P, bins, bins), int64 -- ``hist2d[a, b]`` for ``b < a`` is
    ``np.histogram2d(x[:, b], x[:, a])[0]``, the panel in row ``a``, column ``b`` of the figure, zero elsewhere --
    ``levels`` (n_levels,), ``contour_levels`` (P, P, n_levels) -- the counts at which the contours of that panel are
    drawn, NaN where there is no panel or no sample in it -- ``n_samples`` and ``n_nan`` (P,)."""
    __slots__ = ('names', 'labels', 'offsets', 'range', 'edges', 'hist1d', 'hist2d', 'levels', 'contour_levels',
                 'n_samples', 'n_nan')

    def __init__(self, names, labels, offsets, range, edges, hist1d, hist2d, levels, contour_levels, n_samples, n_nan):
        self.names, self.labels, self.offsets, self.range, self.edges = names, labels, offsets, range, edges
        self.hist1d, self.hist2d, self.levels, self.contour_levels = hist1d, hist2d, levels, contour_levels
        self.n_samples, self.n_nan = n_samples, n_nan

    def pair(self, a, b):
        """``(H, x_edges, y_edges, V)`` of the panel with column ``b`` on the horizontal and column ``a`` on the vertical
        axis, ``a != b`` in either order: ``H[i, j]`` counts the samples with column ``b`` in bin ``i`` and column ``a``
        in bin ``j`` (``np.histogram2d(x[:, b], x[:, a])``), ``V`` the counts of the contour levels."""
        n = len(self.names)
        a, b = int(a), int(b)
        if not (0 <= a < n and 0 <= b < n) or a == b:
            raise IndexError(f'pair({a}, {b}): need two different columns below {n}')
        if b < a:
            return self.hist2d[a, b], self.edges[b], self.edges[a], self.contour_levels[a, b]
        return self.hist2d[b, a].T, self.edges[b], self.edges[a], self.contour_levels[b, a]

    def __repr__(self):
        return (f'<CornerData: {len(self.names)} columns x {self.hist1d.shape[1]} bins over {self.n_samples} samples>')


def corner_contour_levels(H, levels=CORNER_LEVELS):
    """The counts at which ``corner.hist2d`` draws the contours that enclose the fractions ``levels`` of the samples
    of a two-dimensional histogram ``H``: flatten ``H`` and sort it descending, take the cumulative sum normalised to 1,
    and let ``V[i]`` be the last sorted count whose cumulative share is ``<= levels[i]`` -- the largest count if none
    is; sort ``V``, multiply the first of two equal neighbours by ``1 - 1e-4`` for as long as there are any, and sort
    again.  NaN for every level when ``H`` is empty."""
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    Hflat = np.sort(np.asarray(H, dtype=np.float64).ravel())[::-1]
    total = Hflat.sum()
    if not total > 0.:
        return np.full(len(levels), np.nan)
    sm = np.cumsum(Hflat) / total
    V = np.empty(len(levels))
    for i, v0 in enumerate(levels):
        inside = Hflat[sm <= v0]
        V[i] = inside[-1] if len(inside) else Hflat[0]
    V.sort()
    m = np.diff(V) == 0
    while np.any(m):
        V[np.where(m)[0][0]] *= 1. - 1e-4
        m = np.diff(V) == 0
    V.sort()
    return V


def _column_names(model, n_col, use_sigma):
    """``(names, labels)`` of the ``n_col`` columns of a chain: the model's parameter names and axis labels, with
    ``'\\sigma'`` for the last column if ``use_sigma`` -- the model itself is left as it is --, or ``p0, p1, ...``
    without a model.  ``ValueError`` when the model takes another number of columns, or for more than 16."""
    from . import engine as _eng
    if model is None:
        names = [f'p{i}' for i in np.arange(n_col)]
        labels = list(names)
    else:
        want = model.n_model_params + int(bool(use_sigma))
        if n_col != want:
            raise ValueError(f'the samples have {n_col} columns, the model takes {model.n_model_params}'
                             + (' and one for sigma' if use_sigma else ''))
        # (the model's own parameters: the first n_model_params of the instance's lists -- a CustomModel has no others)
        names = list(model.input_names[:model.n_model_params]) + (['\\sigma'] if use_sigma else [])
        units = list(model.units[:model.n_model_params]) + ([''] if use_sigma else [])
        labels = ['${}$ ({})'.format(var, unit) if unit else '${}$'.format(var) for var, unit in zip(names, units)]
    if not 1 <= n_col <= _eng.CORNER_MAX_DIM:
        raise ValueError(f'the samples must have from 1 to {_eng.CORNER_MAX_DIM} columns')
    return names, labels


class _CornerPlan:
    """What :func:`posterior_corner` settles before the device is touched: names, labels, bins, levels, the time columns
    and the caller's ranges; then, from the columns' extremes, the offsets, ranges and edges."""

    def __init__(self, model, n_col, bins, range, levels, t0_offset, use_sigma):
        from . import engine as _eng
        if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= _eng.CORNER_MAX_BINS:
            raise ValueError(f'bins must be an integer from 1 to {_eng.CORNER_MAX_BINS}')
        self.bins = int(bins)
        if model is None and t0_offset is not None:
            raise ValueError('t0_offset needs a model: without one no column is known to be a time')
        self.names, self.labels = _column_names(model, n_col, use_sigma)
        self.time_columns = [self.names.index(var) for var in CORNER_TIME_NAMES if var in self.names] \
            if model is not None else []
        if t0_offset is not None and not np.isfinite(t0_offset):
            raise ValueError('t0_offset must be finite')
        self.t0_offset = None if t0_offset is None else float(t0_offset)
        self.levels = np.array(CORNER_LEVELS if levels is None else levels, dtype=np.float64).ravel()
        if self.levels.size == 0 or not np.all((self.levels > 0.) & (self.levels <= 1.)):
            raise ValueError('levels must be fractions in (0, 1]')
        self.user_range = [None] * n_col
        if range is not None:
            if len(range) != n_col:
                raise ValueError(f'range needs one entry per column: {n_col}, got {len(range)}')
            for d, r in enumerate(range):
                if r is None:
                    continue
                lo, hi = (float(v) for v in r)
                if not (np.isfinite(lo) and np.isfinite(hi)) or hi < lo:
                    raise ValueError(f'range of column {d} ({self.names[d]}): need finite lo <= hi')
                self._refuse_degenerate(d, lo, hi)
                self.user_range[d] = (lo, hi)

    def _refuse_degenerate(self, d, lo, hi):
        if lo == hi:   # corner: "It looks like the parameter(s) in column(s) ... have no dynamic range."
            raise ValueError(f'column {d} ({self.names[d]}) has no dynamic range: its range is ({lo}, {hi})')

    def settle(self, lo, hi):
        """``(offsets, range, edges, labels)`` from the columns' smallest and largest non-NaN values ``lo``, ``hi``
        (unshifted).  The offset is the reference's: for each time column in turn, the floor of the first one's
        minimum unless the caller gave it; subtracted, and written into the label, where it is not zero."""
        n_col = len(self.names)
        offsets, labels, t0 = np.zeros(n_col), list(self.labels), self.t0_offset
        for var, i in zip([v for v in CORNER_TIME_NAMES if v in self.names], self.time_columns):
            if t0 is None:
                t0 = np.floor(lo[i])
                if not np.isfinite(t0):
                    raise ValueError(f'column {i} ({var}) has no finite minimum to take t0_offset from')
            if t0 != 0.:
                offsets[i] = t0
                formatted = '{:f}'.format(t0).rstrip('0').rstrip('.')
                labels[i] = f'${var} - {formatted}$ (d)'
        rng = np.empty((n_col, 2))
        for d in np.arange(n_col):
            if self.user_range[d] is not None:
                rng[d] = self.user_range[d]
                continue
            rng[d] = lo[d] - offsets[d], hi[d] - offsets[d]   # (rounding is monotone: the extremes of x - offset)
            if not np.all(np.isfinite(rng[d])):
                raise ValueError(f'column {d} ({self.names[d]}) has no finite range: ({rng[d, 0]}, {rng[d, 1]})')
            self._refuse_degenerate(d, rng[d, 0], rng[d, 1])
        edges = np.array([np.linspace(r[0], r[1], self.bins + 1) for r in rng])
        return offsets, rng, edges, labels

    def data(self, offsets, rng, edges, labels, hist1d, pairs, n_samples, n_nan):
        n_col, n_lev = len(self.names), len(self.levels)
        hist2d = np.zeros((n_col, n_col, self.bins, self.bins), dtype=np.int64)
        contours = np.full((n_col, n_col, n_lev), np.nan)
        for a in np.arange(1, n_col):
            for b in np.arange(a):
                hist2d[a, b] = pairs[a * (a - 1) // 2 + b]
                contours[a, b] = corner_contour_levels(hist2d[a, b], self.levels)
        return CornerData(self.names, labels, offsets, rng, edges, hist1d, hist2d, self.levels, contours, n_samples,
                          n_nan)


def posterior_corner(model, samples, bins=20, range=None, levels=None, t0_offset=None, discard=0, thin=1,
                     use_sigma=False):
    """Every histogram of the corner plot of ``lightcurve_corner`` (fitting.py:241-253) over ALL samples of a chain:
    the marginal histogram of every column, the joint histogram of every pair of columns and the counts at which the
    contours of each pair are drawn.  Drawing them is left to the caller.

    ``samples``, ``discard``, ``thin`` as in :func:`posterior_predictive`: a sampler's chain is read where it lies in
    device memory when the whole stored chain is the last run's, else uploaded from ``get_chain``; or a host array
    ``(n_samples, n_columns)``.  ``model``: the fitted model -- its parameter names and axis labels, with
    ``'\\sigma'`` for the last column if ``use_sigma`` -- or ``None``: columns ``p0, p1, ...``, no offset.

    ``t0_offset`` (fitting.py:241-251): the columns named ``t_0`` and ``t_\\mathrm{max}`` are counted as
    ``x - t0_offset``, by default the floor of the minimum of the first of them; where it is not zero the axis label
    becomes ``$t_0 - <offset>$ (d)``.  ``range``: per column ``None`` -- the smallest and largest non-NaN shifted
    value, corner's default -- or ``(lo, hi)`` in shifted coordinates; a column without dynamic range raises
    ``ValueError``, as corner refuses it.  The bins are NumPy's for ``np.linspace(lo, hi, bins + 1)``: bin ``i`` holds
    ``edges[i] <= v < edges[i + 1]``, the last also ``v == hi``; NaNs (``n_nan`` per column) and values outside the
    range are in no bin, and a sample enters a pair's histogram only with both coordinates in a bin.  Every count
    equals ``np.histogram`` / ``np.histogram2d`` on the same samples.

    ``levels``: the fractions of the samples the contours enclose, default ``1 - exp(-0.5 [0.5, 1, 1.5, 2]^2)``; their
    counts per pair follow ``corner.hist2d`` (:func:`corner_contour_levels`).  No smoothing, no weights.  Returns a
    :class:`CornerData`."""
    from . import engine as _eng
    sampler, P, n_samples, n_col = _predictive_samples(samples, discard, thin)
    plan = _CornerPlan(model, n_col, bins, range, levels, t0_offset, use_sigma)
    source = _sample_source(sampler, P, discard, thin)
    kw = dict(discard=int(discard), thin=int(thin), device=0 if model is None else model.device)
    lo, hi, n_nan = _eng.chain_range(source, **kw)
    offsets, rng, edges, labels = plan.settle(lo, hi)
    hist1d, pairs = _eng.chain_hist(source, offsets, edges, **kw)
    return plan.data(offsets, rng, edges, labels, hist1d, pairs, n_samples, n_nan)


# ---------------------------------------------------------------------------------------------------------------
# chain history (the numbers of the chain plots of lightcurve_mcmc(show=True), reference fitting.py:135-158)
# ---------------------------------------------------------------------------------------------------------------
#: the default bands of :func:`chain_history`: the extremes, the median and the central 68 %
HISTORY_PERCENTILES = (0., 15.87, 50., 84.14, 100.)
#: step bins of the trace raster unless the caller says otherwise (or the chain has fewer kept steps)
HISTORY_T_BINS = 512


class ChainHistory:
    """Result of :func:`chain_history` for ``n_keep`` kept steps of ``n_walkers`` walkers and P columns: ``steps``
    (n_keep,) -- the stored step ``t_k`` of every kept step -- ``percentiles`` (nq,), ``quantiles`` (nq, n_keep, P) and
    ``log_prob_quantiles`` (nq, n_keep) -- the percentiles across the walkers, NaN where no walker has a value --
    ``n_valid`` (n_keep, P + 1) -- the non-NaN values per step and column, the log-probability last -- ``n_moved``
    (n_keep,) -- the walkers whose row differs from the stored step before, -1 for stored step 0 -- ``frac_moved``
    (that over ``n_walkers``, NaN where ``n_moved`` is -1), ``counts`` (P, t_bins, v_bins), int64 -- the (kept step,
    walker) pairs per step bin and value bin -- ``step_edges`` (t_bins + 1,) -- step bin ``i`` holds the kept steps
    ``step_edges[i] <= k < step_edges[i + 1]`` -- ``edges`` (P, v_bins + 1), ``range`` (P, 2), ``names`` and
    ``labels`` (P strings each)."""
    __slots__ = ('steps', 'percentiles', 'quantiles', 'log_prob_quantiles', 'n_valid', 'n_moved', 'frac_moved',
                 'counts', 'step_edges', 'edges', 'range', 'names', 'labels', 'n_walkers')

    def __init__(self, steps, percentiles, quantiles, log_prob_quantiles, n_valid, n_moved, counts, step_edges, edges,
                 range, names, labels, n_walkers):
        self.steps, self.percentiles = steps, percentiles
        self.quantiles, self.log_prob_quantiles, self.n_valid, self.n_moved = quantiles, log_prob_quantiles, n_valid, n_moved
        self.frac_moved = np.where(n_moved < 0, np.nan, n_moved / n_walkers)
        self.counts, self.step_edges, self.edges, self.range = counts, step_edges, edges, range
        self.names, self.labels, self.n_walkers = names, labels, n_walkers

    def __repr__(self):
        return (f'<ChainHistory: {len(self.percentiles)} percentiles x {len(self.steps)} steps x {len(self.names)} '
                f'columns of {self.n_walkers} walkers; raster {self.counts.shape[1]} x {self.counts.shape[2]}>')


def _bin_count(value, name, most):
    if isinstance(value, bool) or int(value) != value or not 1 <= int(value) <= most:
        raise ValueError(f'{name} must be an integer from 1 to {most}')
    return int(value)


class _HistoryPlan:
    """What :func:`chain_history` settles before the device is touched -- names, labels, percentiles, the kept steps,
    both bin counts and the caller's ranges -- and what it makes of the device's answers."""

    def __init__(self, model, n_t, n_w, n_col, percentiles, t_bins, v_bins, range, discard, thin, use_sigma):
        from . import engine as _eng
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1:
            raise ValueError('need discard >= 0 and thin >= 1')
        if n_t < 1 or n_w < 1:
            raise ValueError('the chain needs at least one step and one walker')
        self.steps = np.arange(discard, n_t, thin, dtype=np.int64)
        if len(self.steps) == 0:
            raise ValueError(f'discard={discard} leaves no steps of the {n_t} stored')
        if n_w > _eng.HISTORY_MAX_WALKERS:
            raise ValueError(f'at most {_eng.HISTORY_MAX_WALKERS} walkers, got {n_w}')
        if use_sigma is None:   # a chain with one column more than its model has parameters carries sigma
            use_sigma = model is not None and n_col == model.n_model_params + 1
        self.names, self.labels = _column_names(model, n_col, use_sigma)
        self.n_walkers, self.discard, self.thin = int(n_w), discard, thin
        self.percentiles = _percentile_array(percentiles)
        if len(self.percentiles) > _eng.HISTORY_MAX_PERCENTILES:
            raise ValueError(f'at most {_eng.HISTORY_MAX_PERCENTILES} percentiles')
        n_keep = len(self.steps)
        self.v_bins = _bin_count(v_bins, 'v_bins', _eng.HISTORY_MAX_VBINS)
        self.t_bins = min(n_keep, HISTORY_T_BINS) if t_bins is None else \
            _bin_count(t_bins, 't_bins', min(n_keep, _eng.HISTORY_MAX_TBINS))
        #: step bin i holds the kept steps k with (k * t_bins) // n_keep == i
        self.step_edges = -(-(np.arange(self.t_bins + 1, dtype=np.int64) * n_keep) // self.t_bins)
        self.user_range = [None] * n_col
        if range is not None:
            if len(range) != n_col:
                raise ValueError(f'range needs one entry per column: {n_col}, got {len(range)}')
            for d, r in enumerate(range):
                if r is None:
                    continue
                lo, hi = (float(v) for v in r)
                if not (np.isfinite(lo) and np.isfinite(hi)) or not lo < hi:
                    raise ValueError(f'range of column {d} ({self.names[d]}) has no extent: need finite lo < hi, got '
                                     f'({lo}, {hi})')
                self.user_range[d] = (lo, hi)

    @property
    def needs_extremes(self):
        return any(r is None for r in self.user_range)

    def settle(self, lo=None, hi=None):
        """``(range, edges)``: the caller's range, else the column's smallest and largest non-NaN value ``lo``, ``hi`` over
        the kept rows -- widened by one half either way when they are equal, as ``np.histogram`` widens it."""
        n_col = len(self.names)
        rng = np.empty((n_col, 2))
        for d in np.arange(n_col):
            if self.user_range[d] is not None:
                rng[d] = self.user_range[d]
                continue
            rng[d] = lo[d], hi[d]
            if not np.all(np.isfinite(rng[d])):
                raise ValueError(f'column {d} ({self.names[d]}) has no finite range: ({rng[d, 0]}, {rng[d, 1]})')
            if rng[d, 0] == rng[d, 1]:
                rng[d] = rng[d, 0] - 0.5, rng[d, 1] + 0.5
        return rng, np.array([np.linspace(r[0], r[1], self.v_bins + 1) for r in rng])

    def data(self, stat_lo, stat_hi, n_valid, n_moved, counts, rng, edges):
        """The order statistics ``stat_lo``, ``stat_hi`` (nq, n_keep, P + 1) interpolated as NumPy interpolates them."""
        _, _, gamma = quantile_ranks(np.maximum(n_valid, 1)[None], self.percentiles[:, None, None])
        quantiles = np.where(n_valid[None] > 0, quantile_lerp(stat_lo, stat_hi, gamma), np.nan)
        return ChainHistory(self.steps, self.percentiles, quantiles[:, :, :-1], quantiles[:, :, -1], n_valid, n_moved,
                            counts, self.step_edges, edges, rng, self.names, self.labels, self.n_walkers)


def chain_history(model, samples, percentiles=HISTORY_PERCENTILES, t_bins=None, v_bins=64, range=None, log_prob=None,
                  discard=0, thin=1, use_sigma=None):
    """The numbers of the chain plots of ``lightcurve_mcmc(..., show=True)`` (fitting.py:135-158), which draw every
    walker's trace, one panel per parameter: whether burn-in was long enough and whether walkers are stuck.  Drawing
    them is left to the caller.

    ``samples``: a sampler -- its stored chain and log-probabilities, read where they lie in device memory when the
    whole stored chain is the last run's, else uploaded from ``get_chain`` / ``get_log_prob`` -- or a host chain
    ``(n_t, n_w, n_dim)`` with an optional ``log_prob`` ``(n_t, n_w)``.  The kept steps are ``k = 0 .. n_keep - 1`` at
    stored step ``t_k = discard + k * thin``.  ``model``, ``use_sigma``: names and labels as in
    :func:`posterior_corner` (``use_sigma=None``: a chain with one column more than the model has parameters carries
    sigma); the ``t_0`` column and its label are left as they are, as the reference's chain plot leaves them.

    Ensemble bands: ``quantiles[:, k, d]`` is ``np.nanpercentile(chain[t_k, :, d], percentiles)`` across the walkers,
    NumPy's default method, bit for bit (the device sorts and selects, the interpolation is NumPy's own arithmetic);
    ``log_prob_quantiles`` the same for the log-probability.  NaN where ``n_valid`` is 0; infinities are ordinary
    values.  At most 16 percentiles, at most 16384 walkers.

    Moves: ``n_moved[k]`` is the number of walkers whose row at stored step ``t_k`` differs, in any bit, from their
    row at stored step ``t_k - 1`` -- the predecessor in the stored chain, not the kept step before: the number of
    proposals accepted in that step.  -1 for ``t_k == 0``.

    Trace density: ``counts[d, i, j]`` is the number of (kept step, walker) pairs with step bin ``i = (k * t_bins) //
    n_keep`` (``t_bins`` defaults to ``min(n_keep, 512)``, at most 4096) and the value of column ``d`` in bin ``j`` of
    ``np.linspace(lo, hi, v_bins + 1)`` (``v_bins`` at most 256) -- ``np.histogram``'s bins, the last closed; NaNs and
    values outside are in no bin.  ``range``: per column ``None`` -- the extremes of the kept rows -- or ``(lo, hi)``.

    Results are exact and bitwise reproducible.  Returns a :class:`ChainHistory`."""
    from . import engine as _eng
    is_sampler = isinstance(samples, EnsembleSampler) or (hasattr(samples, '_native') and hasattr(samples, 'get_chain'))
    if is_sampler:
        if log_prob is not None:
            raise ValueError('log_prob goes with a host chain; a sampler brings its own')
        if samples.iteration == 0:
            raise ValueError('no chain is stored: run the sampler with store=True first')
        n_t, n_w, n_col = samples.iteration, samples.nwalkers, samples.ndim
        device = samples.engine.device
    else:
        x = np.ascontiguousarray(samples, dtype=np.float64)
        if x.ndim != 3:
            raise ValueError('samples must be a sampler or a chain of shape (n_t, n_w, n_dim)')
        n_t, n_w, n_col = x.shape
        if log_prob is not None:
            log_prob = np.ascontiguousarray(log_prob, dtype=np.float64)
            if log_prob.shape != (n_t, n_w):
                raise ValueError(f'log_prob must have shape {(n_t, n_w)}, got {log_prob.shape}')
        device = 0 if model is None else model.device
    plan = _HistoryPlan(model, n_t, n_w, n_col, percentiles, t_bins, v_bins, range, discard, thin, use_sigma)
    kw = dict(discard=plan.discard, thin=plan.thin, device=device)
    if is_sampler and len(samples._chain_host) == 0 and samples._chain_on_device > 0:
        source = rows = samples._native
        stats = _eng.chain_history(source, plan.percentiles, **kw)
    else:
        if is_sampler:
            x, log_prob = samples.get_chain(), samples.get_log_prob()
        source, rows = x, x[plan.discard::plan.thin].reshape(-1, n_col)
        stats = _eng.chain_history(source, plan.percentiles, log_prob=log_prob, **kw)
    lo = hi = None
    if plan.needs_extremes:
        lo, hi, _ = _eng.chain_range(rows, **(kw if rows is source else dict(device=device)))
    rng, edges = plan.settle(lo, hi)
    counts = _eng.chain_raster(source, plan.t_bins, edges, **kw)
    return plan.data(*stats, counts, rng, edges)
