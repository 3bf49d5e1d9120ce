"""Host-side mirror of the reference's model / prior interface, backed by the MI355X engine.

Same class names, constructor arguments, ``input_names``, call signatures and error behaviour as
``/root/reference/lightcurve_fitting/models.py`` for the likelihood path:

* ``Model.log_likelihood(lc, p, use_sigma=False, sigma_type='relative')``   (reference models.py:93-136)
* ``Model.__call__(t_in, f, *params)`` / ``evaluate``                        (models.py:86-87, per-model evaluate)
* ``temperature_radius``                                                     (models.py:231-269, 583-597, 727-755)
* ``UniformPrior`` / ``LogUniformPrior`` / ``GaussianPrior``                 (models.py:1048-1098)
* ``blackbody_to_filters``                                                   (models.py:1131-1165, ebv = 0)

All arithmetic on walkers runs in the HIP kernels (``csrc/``) through the C ABI (``include/lcf.h``).  This module
only marshals: it extracts the photometry columns, packs band tables, bakes the model's construction-time
constants, computes the SiFTO spline coefficients once, and caches one engine per (light curve, sigma mode).
There is no NumPy fallback for the model mathematics: without the native library and a GPU these calls raise.

Extension over the reference: ``p`` may be a C-contiguous ``(n, ndim)`` block (what emcee passes with
``vectorize=True``); the result then has shape ``(n,)``.  ``nondet='censored'`` (``log_likelihood``, ``engine_for``;
``limit_terms``) makes the rows whose ``nondet`` is true upper limits instead of measurements of zero.
``WithTemplate`` adds a stretched template -- a second peak -- to a shock model or a ``CustomModel``.
"""
import numpy as np

from . import engine as _eng
from .spline import not_a_knot_coefficients  # noqa: F401  (re-exported)
from .filters import Filter, PackedTables, as_filter, filtdict, _tables

# module-level constants with the reference's names (models.py:10-12, 1101-1102)
k_B = 0.08617333262145178
c3 = 5.38477047522316e-19
c4 = 8.357743635931361e-47
c1 = 0.0479924307336622
c2 = 281739904251.4432


# ---------------------------------------------------------------------------------------------------------------
# priors (models.py:1048-1098)
# ---------------------------------------------------------------------------------------------------------------
class Prior:
    """Base prior: ``__call__`` returns ``logp(p)`` strictly inside ``(p_min, p_max)`` and ``-inf`` otherwise."""
    kind = _eng.PRIOR_UNIFORM

    def __init__(self, p_min=-np.inf, p_max=np.inf):
        self.p_min = p_min
        self.p_max = p_max

    def __call__(self, p):
        if self.p_min < p < self.p_max:
            return self.logp(p)
        return -np.inf

    def logp(self, p):
        raise NotImplementedError

    def descriptor(self):
        """(kind, p_min, p_max, mean, stddev) as the C ABI wants it."""
        return (self.kind, float(self.p_min), float(self.p_max), float(getattr(self, 'mean', 0.)),
                float(getattr(self, 'stddev', 1.)))


class UniformPrior(Prior):
    """dP/dp proportional to 1."""
    kind = _eng.PRIOR_UNIFORM

    def logp(self, p):
        return np.zeros_like(p)


class LogUniformPrior(Prior):
    """dP/dp proportional to 1/p."""
    kind = _eng.PRIOR_LOG_UNIFORM

    def __init__(self, p_min=0., p_max=np.inf):
        if p_min < 0.:
            raise ValueError('a log-uniform prior cannot have negative limits')
        super().__init__(p_min, p_max)

    def logp(self, p):
        return -np.log(p)


class GaussianPrior(Prior):
    """Gaussian centred on ``mean`` with standard deviation ``stddev`` (unnormalised), truncated to the bounds."""
    kind = _eng.PRIOR_GAUSSIAN

    def __init__(self, p_min=-np.inf, p_max=np.inf, mean=0., stddev=1.):
        super().__init__(p_min, p_max)
        self.mean = mean
        self.stddev = stddev

    def logp(self, p):
        return -0.5 * ((p - self.mean) / self.stddev) ** 2.


# ---------------------------------------------------------------------------------------------------------------
# light-curve access (duck typed: astropy Table, lightcurve_fitting_amd.lightcurve.LC, dict of arrays)
# ---------------------------------------------------------------------------------------------------------------
def _column(lc, name):
    col = lc[name]
    return np.asarray(getattr(col, 'data', col))


def _photometry(lc, quantity):
    t = np.asarray(_column(lc, 'MJD'), dtype=np.float64)
    y = np.asarray(_column(lc, quantity), dtype=np.float64)
    dy = np.asarray(_column(lc, 'd' + quantity), dtype=np.float64)
    filts = [as_filter(f) for f in _column(lc, 'filter')]
    return t, filts, y, dy


class _BoundEngine:
    """An engine together with the photometry it was created from (host copies, for the content check)."""
    __slots__ = ('engine', 'mode', 't', 'filters', 'y', 'dy')

    def __init__(self, engine, mode, t, filters, y, dy):
        self.engine, self.mode = engine, mode
        self.t, self.y, self.dy = t.copy(), y.copy(), dy.copy()
        self.filters = filters.copy()

    def holds(self, t, filters, y, dy):
        """True if the engine's photometry equals these columns (NaNs compare equal to NaNs)."""
        if t.shape != self.t.shape:
            return False
        for mine, theirs in ((self.y, y), (self.dy, dy), (self.t, t)):
            if mine.shape != theirs.shape or not np.array_equal(mine, theirs, equal_nan=True):
                return False
        return filters.shape == self.filters.shape and bool(np.all(filters == self.filters))


NONDET_MODES = ('gaussian', 'censored')


def _check_nondet_mode(nondet):
    if nondet not in NONDET_MODES:
        raise ValueError(f"nondet must be 'gaussian' (a non-detection is a measurement of zero, as in the reference) or "
                         f"'censored' (an upper limit: the probability that the flux was below it), not {nondet!r}")


def _nondet_mask(lc):
    """The ``nondet`` column of ``lc`` as a boolean array, or None when ``lc`` has none or no row of it is true."""
    names = getattr(lc, 'colnames', None)
    if not ('nondet' in names if names is not None else 'nondet' in lc):
        return None
    mask = np.asarray(_column(lc, 'nondet')).astype(bool)
    return mask if mask.any() else None


class LimitSplit:
    """The rows of a light curve split by its ``nondet`` column (``nondet='censored'``): ``det`` / ``lim`` are the
    boolean masks of the detections and the upper limits, ``dy`` the limits' ``d<quantity>`` (which ``calcLum`` /
    ``calcFlux`` set to ``limit / nondetSigmas``), ``L_lim = nondetSigmas * dy`` the limits themselves, and
    ``sigma_unit_abs`` the median ``d<quantity>`` of the detections (the unit of an ``'absolute'`` fitted sigma)."""

    def __init__(self, lc, quantity, mask=None):
        mask = _nondet_mask(lc) if mask is None else mask
        dy = np.asarray(_column(lc, 'd' + quantity), dtype=np.float64)
        if mask is None:
            mask = np.zeros(len(dy), dtype=bool)
        if mask.shape != dy.shape:
            raise ValueError('the nondet column must have one entry per row')
        if mask.all():
            raise ValueError("nondet='censored' needs at least one detection: every row of the light curve is a "
                             "non-detection")
        self.lim, self.det = mask, ~mask
        self.nondet_sigmas = float(getattr(lc, 'nondetSigmas', 3.))
        self.dy = dy[mask]
        self.L_lim = self.nondet_sigmas * self.dy
        self.sigma_unit_abs = float(np.median(dy[self.det]))


def _index_filters(filts):
    """Distinct filters (first-seen order) and the per-point index into them."""
    uniq = list(dict.fromkeys(filts))
    lookup = {f: i for i, f in enumerate(uniq)}
    return uniq, np.array([lookup[f] for f in filts], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------
class Model:
    """An analytical model, defined by its parameters and evaluated on the GPU."""

    input_names = []
    units = []
    output_quantity = 'lum'
    model_id = None
    #: E(B-V) is a model parameter: band-table weights are reddened per walker (full tables only)
    reddened = False
    #: photometry-bound engines one model keeps (each holds a copy of a light curve on the device)
    max_bound_engines = 8
    #: cutoff frequency [THz] of a modified blackbody (filters.py:308-310); only Blackbody takes another value
    cutoff_freq = np.inf

    def __init__(self, lc=None, redshift=0.):
        if redshift:
            self.z = redshift
        elif lc is not None and 'redshift' in getattr(lc, 'meta', {}):
            self.z = lc.meta['redshift']
        else:
            self.z = 0.
        # instance-level copies: lightcurve_mcmc(use_sigma=True) appends '\\sigma' (fitting.py:74-76)
        self.input_names = list(type(self).input_names)
        self.units = list(type(self).units)
        self._engines = {}   # evaluation engines (model grids), keyed by the (times, filters) they were built for
        self._bound = []     # engines bound to photometry, most recently used first (see engine_for)
        self.device = 0

    @property
    def nparams(self):
        return len(self.input_names)

    @property
    def n_model_params(self):
        return len(type(self).input_names)

    @property
    def axis_labels(self):
        return ['${}$ ({})'.format(var, unit) if unit else '${}$'.format(var)
                for var, unit in zip(self.input_names, self.units)]

    def __repr__(self):
        return f'<{self.__class__.__name__}: z={self.z:.3f}>'

    def __call__(self, *args, **kwargs):
        return self.evaluate(*args, **kwargs)

    # --- hooks for subclasses ----------------------------------------------------------------------------------
    def _consts(self):
        return []

    def _companion_tables(self, uniq_filters):
        return None

    # --- engine management -------------------------------------------------------------------------------------
    def make_engine(self, t, filts, y, dy, use_sigma=False, sigma_type='relative', priors=None, device=None):
        """Build a device engine for explicit photometry arrays (``filts``: Filter objects or aliases)."""
        if sigma_type == 'relative':
            st = _eng.SIGMA_RELATIVE
        elif sigma_type == 'absolute':
            st = _eng.SIGMA_ABSOLUTE
        else:
            raise Exception('sigma_type must either be "relative" or "absolute"')
        import time
        t0 = time.perf_counter()
        filts = [as_filter(f) for f in filts]
        uniq, idx = _index_filters(filts)
        tabs = PackedTables(uniq, z=self.z, cutoff_freq=self.cutoff_freq, compress=not self.reddened,
                            reddening=self.reddened)
        t1 = time.perf_counter()
        pri = None if priors is None else [p.descriptor() for p in priors]
        eng = _eng.Engine(self.model_id, self.n_model_params, self._consts(), t, y, dy, idx, tabs.off, tabs.a, tabs.w,
                          use_sigma=use_sigma, sigma_type=st, priors=pri,
                          companion=self._companion_tables(uniq), device=self.device if device is None else device,
                          ctab=None if self.reddened else (tabs.coff, tabs.ca, tabs.cw, tabs.ctmin),
                          htab=None if self.reddened else (tabs.hoff, tabs.ha, tabs.hw, tabs.htmin),
                          itab=None if self.reddened else (tabs.icoef, tabs.itmin, tabs.iu0, tabs.ih),
                          tab_ext=tabs.ext)
        eng.tables, eng.filt_idx = tabs, idx   # what was packed (measurement tools count the samples a fit executes)
        #: seconds: band tables packed on the host (their levels shipped or built: tabs.levels_from) / engine created
        eng.timings = {'tables_s': t1 - t0, 'create_s': time.perf_counter() - t1, 'levels': sorted(set(tabs.levels_from))}
        return eng

    def engine_for(self, lc, use_sigma=False, sigma_type='relative', priors=None, nondet='gaussian'):
        """Engine bound to the photometry ``lc`` holds NOW (sigma mode and prior set as given).

        The reference reads the light-curve columns on every ``log_likelihood`` call (models.py:116-119); an engine
        copies them to the device once.  Engines are therefore cached by the CONTENT of the four columns, compared on
        every call: editing ``lc['lum']`` in place, or a new light-curve object at a recycled address, gets a new
        engine.  An engine that leaves the cache is only dropped, never destroyed here -- samplers and closures that
        were handed it keep it alive.

        ``nondet='censored'`` (extension; see :meth:`log_likelihood`): the engine holds the rows whose ``nondet`` is
        false, with the true rows attached as upper limits (a second engine on their times and filters); the cache key
        gains the mode, the column's content and ``nondetSigmas``.  Without a true ``nondet`` row it is the plain engine."""
        if sigma_type not in ('relative', 'absolute'):
            raise Exception('sigma_type must either be "relative" or "absolute"')
        _check_nondet_mode(nondet)
        t = np.asarray(_column(lc, 'MJD'), dtype=np.float64)
        y = np.asarray(_column(lc, self.output_quantity), dtype=np.float64)
        dy = np.asarray(_column(lc, 'd' + self.output_quantity), dtype=np.float64)
        filt_col = np.asarray(_column(lc, 'filter'), dtype=object)
        mode = (bool(use_sigma), sigma_type, None if priors is None else tuple(p.descriptor() for p in priors))
        split = None
        mask = _nondet_mask(lc) if nondet == 'censored' else None
        if mask is not None:
            split = LimitSplit(lc, self.output_quantity, mask)
            mode += ('censored', mask.tobytes(), split.nondet_sigmas)
        for k, bound in enumerate(self._bound):
            if bound.mode == mode and bound.holds(t, filt_col, y, dy):
                if k:  # most recently used first
                    self._bound.insert(0, self._bound.pop(k))
                return bound.engine
        filts = [as_filter(f) for f in filt_col]
        if split is None:
            eng = self.make_engine(t, filts, y, dy, use_sigma, sigma_type, priors)
        else:
            det, lim = np.nonzero(split.det)[0], np.nonzero(split.lim)[0]
            eng = self.make_engine(t[det], [filts[i] for i in det], y[det], dy[det], use_sigma, sigma_type, priors)
            at = self.make_engine(t[lim], [filts[i] for i in lim], np.zeros(len(lim)), split.dy, use_sigma, sigma_type)
            eng.set_limits(at, split.L_lim, split.dy)
        self._bound.insert(0, _BoundEngine(eng, mode, t, filt_col, y, dy))
        del self._bound[self.max_bound_engines:]
        return eng

    # --- the reference's public surface --------------------------------------------------------------------------
    def log_likelihood(self, lc, p, use_sigma=False, sigma_type='relative', nondet='gaussian'):
        """Gaussian log-likelihood of the photometry in ``lc`` given parameters ``p`` (models.py:93-136).

        ``p`` 1-D -> float; ``p`` of shape (n, ndim) -> array (n,).

        ``nondet`` (extension): ``'gaussian'``, the default, is the reference's treatment -- a row whose ``nondet`` is
        true enters with ``y = 0`` and ``dy = limit / nondetSigmas`` like a measurement of zero.  ``'censored'`` makes it
        an upper limit: the Gaussian sum runs over the detections only, and every non-detection ``j`` adds
        ``ln Phi((L_lim,j - m_j(p)) / sigma_j(p))``, the probability that the flux was below the limit -- with
        ``L_lim,j = nondetSigmas * dy_j``, ``m_j`` the model at its time and filter, ``sigma_j = dy_j`` or, with
        ``use_sigma``, ``sqrt(dy_j^2 + (s u_j)^2)`` where ``u_j = dy_j`` (``'relative'``) or the detections' median ``dy``
        (``'absolute'``).  ``lc`` needs a boolean ``nondet`` column for it (an ``LC`` or a dict); without one, or without
        a true row, the call is the default one.  No detection at all raises ``ValueError``."""
        eng = self.engine_for(lc, use_sigma, sigma_type, nondet=nondet)
        p = np.asarray(p, dtype=np.float64)
        out = eng.log_likelihood(p)
        return float(out[0]) if p.ndim == 1 else out

    def limit_terms(self, lc, p, use_sigma=False, sigma_type='relative'):
        """The censored term ``ln Phi((L_lim,j - m_j(p)) / sigma_j(p))`` of every non-detection of ``lc``, in the order
        of its ``nondet`` rows: which limits a fit with ``nondet='censored'`` leans on.

        ``p`` 1-D -> (n_lim,); ``p`` of shape (n, ndim) -> (n, n_lim).  Their sum over the limits plus the
        log-likelihood of the detections alone is ``log_likelihood(..., nondet='censored')``."""
        eng = self.engine_for(lc, use_sigma, sigma_type, nondet='censored')
        p = np.asarray(p, dtype=np.float64)
        out = eng.limit_terms(p) if getattr(eng, 'nlimits', 0) else np.empty((len(eng._block(p)), 0))
        return out[0] if p.ndim == 1 else out

    def _eval_engine(self, t_in, f, scalar_params=True):
        """Engine for model evaluation at (t, f): pointwise when the lengths agree and the parameters are scalars
        (``T.ndim == 1 and len(T) == len(filters)``, models.py:1161), else the dense filters x times grid
        (models.py:1163-1164).  Returns (engine, grid_shape or None)."""
        t_in = np.atleast_1d(np.asarray(t_in, dtype=np.float64))
        single = isinstance(f, (Filter, str))
        filts = [as_filter(f)] if single else [as_filter(x) for x in f]
        if not single and scalar_params and t_in.ndim == 1 and len(t_in) == len(filts):
            t, fl, shape = t_in, filts, None
        else:
            t = np.tile(t_in.ravel(), len(filts))
            fl = [x for x in filts for _ in range(t_in.size)]
            shape = (len(filts), t_in.size)
        key = ('eval', t.tobytes(), tuple(x.name for x in fl))
        eng = self._engines.get(key)
        if eng is None:
            eng = self.make_engine(t, fl, np.zeros(len(t)), np.ones(len(t)))
            self._engines = {key: eng}  # one evaluation grid at a time; the old engine dies with its last reference
        return eng, shape

    def evaluate(self, t_in, f, *params):
        """Model light curve(s).  Scalar parameters -> (npoints,) [pointwise, when ``len(t_in) == len(f)``] or
        (nfilters, ntimes) [grid]; array parameters of length n -> the grid with a trailing axis of length n, as in
        the reference (whose pointwise branch needs a one-dimensional temperature)."""
        if len(params) != self.n_model_params:
            raise TypeError(f'{type(self).__name__} takes {self.n_model_params} parameters, got {len(params)}')
        cols = np.broadcast_arrays(*[np.asarray(x, dtype=np.float64) for x in params])
        scalar = cols[0].ndim == 0
        eng, shape = self._eval_engine(t_in, f, scalar)
        P = np.column_stack([np.atleast_1d(c).ravel() for c in cols])
        y = eng.evaluate(P)  # (n, npoints)
        y = y[0] if scalar else y.T
        if shape is not None:
            y = y.reshape(shape if scalar else shape + (len(P),))
        return y

    def temperature_radius(self, t_in, *params):
        """Blackbody temperature [kK] and radius [1000 Rsun] at times ``t_in`` (same broadcasting as evaluate)."""
        t_in = np.atleast_1d(np.asarray(t_in, dtype=np.float64))
        eng, _ = self._eval_engine(t_in, [self._any_filter()] * len(t_in))
        n_tr = self._n_tr_params()
        cols = np.broadcast_arrays(*[np.asarray(x, dtype=np.float64) for x in params[:n_tr]])
        scalar = cols[0].ndim == 0
        P = np.column_stack([np.atleast_1d(c).ravel() for c in cols])
        if P.shape[1] < self.n_model_params:  # parameters that do not enter T, R
            P = np.column_stack([P, np.ones((len(P), self.n_model_params - P.shape[1]))])
        T, R = eng.temperature_radius(P)
        return (T[0], R[0]) if scalar else (T.T, R.T)

    def _n_tr_params(self):
        return self.n_model_params

    @staticmethod
    def _any_filter():
        return filtdict['r']


class BaseShockCooling(Model):
    """Sapir & Waxman (2017) / Rabinak & Waxman (2011) shock cooling; constants per models.py:192-226."""

    def __init__(self, lc=None, redshift=0., n=1.5, RW=False):
        super().__init__(lc, redshift=redshift)
        if n == 1.5:
            self.n, self.A, self.a, self.alpha = 1.5, 0.94, 1.67, 0.8
            self.epsilon_1, self.epsilon_2, self.L_0, self.T_0, self.Tph_to_Tcol = 0.027, 0.086, 2.0e42, 1.61, 1.1
        elif n == 3.:
            self.n, self.A, self.a, self.alpha = 3., 0.79, 4.57, 0.73
            self.epsilon_1, self.epsilon_2, self.L_0, self.T_0, self.Tph_to_Tcol = 0.016, 0.175, 2.1e42, 1.69, 1.0
        else:
            raise ValueError('n can only be 1.5 or 3')
        self.epsilon_T = 2 * self.epsilon_1 - 0.5
        self.epsilon_L = -2 * self.epsilon_2
        self.RW = bool(RW)
        if RW:
            self.a = 0.
            self.Tph_to_Tcol = 1.2

    def __repr__(self):
        return f'<{self.__class__.__name__}: z={self.z:.3f}, n={self.n:.1f}, RW={self.RW}>'

    def _consts(self):
        return [self.A, self.a, self.alpha, self.epsilon_1, self.epsilon_2, self.L_0, self.T_0, self.Tph_to_Tcol]

    @staticmethod
    def t_min(p, kappa=1.):
        """Minimum validity time (models.py:276-287)."""
        v_s, f_rho_M, R = p[0], p[2], p[3]
        t_exp = p[4] if len(p) > 4 else 0.
        return 0.2 * R / v_s * np.maximum(0.5, R ** 0.4 * (f_rho_M * kappa) ** -0.2 * v_s ** -0.7) + t_exp

    @staticmethod
    def t_max(p, kappa=1.):
        """Maximum validity time (models.py:290-298)."""
        R = p[3]
        t_exp = p[4] if len(p) > 4 else 0.
        return 7.4 * (R / kappa) ** 0.55 + t_exp


class ShockCooling(BaseShockCooling):
    """Physical parameters v_s, M_env, f_rho M, R, t_0 (models.py:301-353)."""
    model_id = _eng.MODEL_SHOCK_COOLING
    input_names = ['v_\\mathrm{s*}', 'M_\\mathrm{env}', 'f_\\rho M', 'R', 't_0']
    units = ['10^8.5 cm/s', 'Msun', 'Msun', '10^13 cm', 'd']


class ShockCooling2(BaseShockCooling):
    """Scaling parameters T_1, L_1, t_tr, t_0 (models.py:356-430)."""
    model_id = _eng.MODEL_SHOCK_COOLING2
    input_names = ['T_1', 'L_1', 't_\\mathrm{tr}', 't_0']
    units = ['kK', '10^42 erg/s', 'd', 'd']

    @staticmethod
    def t_min(p, kappa=1.):
        return NotImplemented

    def t_max(self, p, kappa=1.):
        T_1 = p[0]
        t_exp = p[3] if len(p) > 3 else 0.
        return (8.12 / T_1) ** (self.epsilon_T ** -1) + t_exp


class ShockCooling3(BaseShockCooling):
    """``ShockCooling`` with the luminosity distance d_L [Mpc] and the reddening E(B-V) as free parameters; fits
    ``'flux'`` instead of ``'lum'`` (models.py:433-504): ``flux = c4 * Lnu(E(B-V)) / d_L ** 2``, the blackbody being
    reddened sample by sample inside the band integral with the Fitzpatrick (1999) law, R_V = 3.1
    (``extinction.py``; that law is third-party arithmetic for the reference -- see its header for how it is pinned)."""
    model_id = _eng.MODEL_SHOCK_COOLING3
    input_names = ['v_\\mathrm{s*}', 'M_\\mathrm{env}', 'f_\\rho M', 'R', 'd_L', 'E(B-V)', 't_0']
    units = ['10^8.5 cm/s', 'Msun', 'Msun', '10^13 cm', 'Mpc', 'mag', 'd']
    output_quantity = 'flux'
    reddened = True

    def temperature_radius(self, t_in, v_s, M_env, f_rho_M, R, t_exp=0.):
        """Same (T, R) as ``ShockCooling`` (``BaseShockCooling.temperature_radius``, models.py:231-269)."""
        one = np.ones_like(np.asarray(v_s, dtype=np.float64))
        return super().temperature_radius(t_in, v_s, M_env, f_rho_M, R, one, 0. * one, t_exp * one)

    @staticmethod
    def t_min(p, kappa=1.):
        return BaseShockCooling.t_min([p[0], p[1], p[2], p[3], p[6] if len(p) > 6 else 0.], kappa=kappa)

    @staticmethod
    def t_max(p, kappa=1.):
        return BaseShockCooling.t_max([p[0], p[1], p[2], p[3], p[6] if len(p) > 6 else 0.], kappa=kappa)


class ShockCooling4(Model):
    """Morag, Sapir & Waxman (2023) form (models.py:507-657), quirks of the reference included."""
    model_id = _eng.MODEL_SHOCK_COOLING4
    input_names = ['v_\\mathrm{s*}', 'M_\\mathrm{env}', 'f_\\rho M', 'R', 't_0']
    units = ['10^8.5 cm/s', 'Msun', 'Msun', '10^13 cm', 'd']

    def __init__(self, lc=None, redshift=0.):
        super().__init__(lc, redshift=redshift)
        self.A, self.a, self.alpha = 0.9, 2., 0.5
        self.L_br_0, self.T_col_br_0 = 3.69e42, 8.19
        self.t_min_0, self.t_br_0, self.t_07eV_0, self.t_tr_0 = 0.012, 0.036, 6.86, 19.5

    def _consts(self):
        return [self.A, self.a, self.alpha, self.L_br_0, self.T_col_br_0, self.t_br_0, self.t_tr_0]

    def t_min(self, p, kappa=1.):
        t_exp = p[4] if len(p) > 4 else 0.
        return self.t_min_0 * p[3] + t_exp

    def t_max(self, p, kappa=1.):
        v_s, M_env, f_rho_M, R, t_exp, *_ = p
        t_07eV = self.t_07eV_0 * R ** 0.56 * v_s ** 0.16 * kappa ** -0.61 * f_rho_M ** -0.06
        t_tr = self.t_tr_0 ** np.sqrt(kappa * M_env / v_s)  # sic: ** as in models.py:656
        return np.minimum(t_07eV, t_tr / self.a) + t_exp


_SIFTO_COLUMNS = ('Epoch', 'U', 'B', 'V', 'g', 'r', 'i')


def sifto_template():
    """SiFTO SN Ia template without its first three (~0) rows (models.py:660-661): columns Epoch,U,B,V,g,r,i."""
    return _tables()['template/sifto'][3:]


class BaseCompanionShocking(Model):
    """Kasen (2010) companion-shocking component + SiFTO template scaled to the observed peak (models.py:665-845)."""
    _kasen_factor = {}
    _sifto_factor = {}
    _dt_param = {}

    def __init__(self, lc, redshift=0.):
        super().__init__(lc, redshift=redshift)
        if 'lum' not in getattr(lc, 'colnames', list(getattr(lc, 'keys', lambda: [])())):
            if hasattr(lc, 'calcAbsMag'):
                if 'absmag' not in lc.colnames:
                    lc.calcAbsMag()
                lc.calcLum()
        tab = sifto_template()
        self._knots = np.ascontiguousarray(tab[:, 0])
        filts = [as_filter(f) for f in _column(lc, 'filter')]
        lum = np.asarray(_column(lc, 'lum'), dtype=np.float64)
        have_dlt40 = filtdict['DLT40'] in filts
        self.sifto = {}
        for filt in dict.fromkeys(filts):  # models.py:701-717
            if filt.name == 'unfilt.' and have_dlt40:
                column, scale_by = 'r', filtdict['DLT40']
            elif filt.name == 'DLT40':
                column, scale_by = 'r', filt
            elif filt.char in _SIFTO_COLUMNS[1:]:
                column, scale_by = filt.char, filt
            else:
                raise Exception('No SiFTO template for filter ' + filt.name)
            col = tab[:, _SIFTO_COLUMNS.index(column)]
            peak = np.max(lum[[f == scale_by for f in filts]])
            self.sifto[filt] = not_a_knot_coefficients(self._knots, col * peak / np.max(col))

    def _companion_tables(self, uniq_filters):
        nk = len(self._knots)
        coef = np.zeros((len(uniq_filters), nk - 1, 4))
        kp, sp, dtp = [], [], []
        for i, f in enumerate(uniq_filters):
            if f not in self.sifto:
                raise Exception('No SiFTO template for filter ' + f.name)
            coef[i] = self.sifto[f]
            kp.append(self._kasen_factor.get(f.char, -1))
            sp.append(self._sifto_factor.get(f.char, -1))
            dtp.append(self._dt_param.get(f.name, -1))
        return kp, sp, dtp, self._knots, coef

    def _n_tr_params(self):
        return 3

    def companion_shocking(self, t_in, f, t_exp, a13, Mc_v9_7, kappa=1.):
        """The shock component alone at times ``t_in`` in filters ``f`` (models.py:757-784): ``temperature_radius``
        followed by ``blackbody_to_filters``.  An opacity ``kappa`` other than 1 enters as the separation ``a13 / kappa``
        and the product ``kappa * Mc_v9_7`` (models.py:753-754 depend on these two combinations only)."""
        a13 = np.asarray(a13, dtype=np.float64) / kappa
        Mc_v9_7 = np.asarray(Mc_v9_7, dtype=np.float64) * kappa
        if self.model_id == _eng.MODEL_COMPANION_SHOCKING3 and np.any(Mc_v9_7 != 1.):
            raise NotImplementedError('CompanionShocking3 fixes kappa * Mc_v9_7 = 1 (models.py:1040)')
        T, R = self.temperature_radius(t_in, t_exp, a13, Mc_v9_7)
        return blackbody_to_filters(f, T, R, self.z)

    @staticmethod
    def t_min(p):
        return p[3] + p[4] * sifto_template()[:, 0].min()

    @staticmethod
    def t_max(p):
        return p[3] + p[4] * sifto_template()[:, 0].max()


class CompanionShocking(BaseCompanionShocking):
    """Factors on the r and i templates and on the U shock component (models.py:848-918)."""
    model_id = _eng.MODEL_COMPANION_SHOCKING
    input_names = ['t_0', 'a', 'M v^7', 't_\\mathrm{max}', 's', 'r_r', 'r_i', 'r_U']
    units = ['d', '10^13 cm', 'M_Ch (10^9 cm/s)^7', 'd', '', '', '', '']
    _kasen_factor = {'U': 7}      # keyed on filt.char (models.py:913-916)
    _sifto_factor = {'r': 5, 'i': 6}


class CompanionShocking2(BaseCompanionShocking):
    """Time offsets for the U and i templates (models.py:921-980)."""
    model_id = _eng.MODEL_COMPANION_SHOCKING2
    input_names = ['t_0', 'a', 'M v^7', 't_\\mathrm{max}', 's', '\\Delta t_U', '\\Delta t_i']
    units = ['d', '10^13 cm', 'M_Ch (10^9 cm/s)^7', 'd', '', 'd', 'd']
    _dt_param = {'U': 5, 'i': 6}   # keyed on the filter itself (models.py:804-807)


class CompanionShocking3(BaseCompanionShocking):
    """Time offsets + Brown et al. (2012) viewing-angle dependence (models.py:983-1045)."""
    model_id = _eng.MODEL_COMPANION_SHOCKING3
    input_names = ['t_0', 'a', '\\theta', 't_\\mathrm{max}', 's', '\\Delta t_U', '\\Delta t_i']
    units = ['d', '10^13 cm', 'deg', 'd', '', 'd', 'd']
    _dt_param = {'U': 5, 'i': 6}


class Blackbody(Model):
    """Direct (T, R) blackbody -- the spectrum ``spectrum_mcmc`` fits per epoch (bolometric.py:154-164)."""
    model_id = _eng.MODEL_BLACKBODY
    input_names = ['T', 'R']
    units = ['kK', '1000 Rsun']

    def __init__(self, lc=None, redshift=0., cutoff_freq=np.inf):
        super().__init__(lc, redshift)
        self.cutoff_freq = cutoff_freq   # (the band tables of every engine this model makes)

    def _eval_engine(self, t_in, f, scalar_params=True):
        # not a reference Model: one (filter, time) point per entry even for arrays of candidates, result (npoints, n)
        return super()._eval_engine(t_in, f, True)


class CustomModel(Model):
    """A model the user writes: a photosphere ``T(t, p)``, ``R(t, p)`` in HIP device code, followed by
    ``blackbody_to_filters(f, T, R, z)`` -- the two steps of every shock-cooling class of the reference -- compiled at
    run time for the GPU and fitted like the built-in models.

    ``source`` defines exactly this function (see ``include/lcf.h``, "custom models")::

        __device__ void lcf_user_state(double t_in, const double* p, const double* consts, double z,
                                       double& T_kK, double& R_1000Rsun);

    ``t_in``: the observation time as stored in the light curve (subtract the explosion time and apply ``1 + z`` as the
    model requires); ``p``: the ``len(input_names)`` parameters, without a fitted sigma; ``consts``: up to 12 numbers
    given here; units as ``temperature_radius`` returns them.  ``lcf::pw`` is the reference's ``power()``.
    ``T <= 0`` or ``T >= 1e15`` gives a zero light curve, a NaN state a NaN likelihood.

    ``log_likelihood``, ``evaluate`` / ``__call__``, ``temperature_radius``, ``make_log_posterior`` and
    ``lightcurve_mcmc`` work as for every model; the fit runs through :class:`~lightcurve_fitting_amd.sampler.
    TemperedSampler` (one rung at ``beta = 1`` unless a ladder is asked for), since the resident sampler's kernels,
    ``posterior_predictive`` and ``thermal_predictive`` are compiled per built-in model and raise ``LcfError`` here;
    :func:`~lightcurve_fitting_amd.fitting.custom_predictive` gives the bands of its light curves, T, R and L over a chain.
    The source is compiled on first use (:meth:`compile`); an error in it raises ``LcfError`` with the compiler's log,
    which names the source's own lines as ``user_model:<line>``."""
    model_id = _eng.MODEL_CUSTOM

    def __init__(self, source, input_names, units=None, consts=(), lc=None, redshift=0., output_quantity='lum'):
        super().__init__(lc, redshift=redshift)
        self.source = str(source)
        self.input_names = list(input_names)
        self.units = [''] * len(self.input_names) if units is None else list(units)
        if len(self.units) != len(self.input_names):
            raise ValueError('units must have one entry per parameter')
        self._n_par = len(self.input_names)
        if not 1 <= self._n_par <= 15:
            raise ValueError('a custom model has 1 to 15 parameters')
        self._custom_consts = [float(c) for c in consts]
        if len(self._custom_consts) > _eng.N_CONSTS:
            raise ValueError(f'at most {_eng.N_CONSTS} consts')
        self.output_quantity = output_quantity
        self._programs = {}

    @property
    def n_model_params(self):
        return self._n_par

    def _consts(self):
        return self._custom_consts

    def compile(self, arch=None, device=None):
        """The :class:`~lightcurve_fitting_amd.engine.CustomProgram` of the source for ``arch`` (e.g. ``'gfx950'``:
        no GPU needed) or, by default, for the architecture of ``device`` (the model's)."""
        device = self.device if device is None else device
        key = arch or ('device', device)
        if key not in self._programs:
            self._programs[key] = _eng.CustomProgram(self.source, arch, device)
        return self._programs[key]

    def make_engine(self, t, filts, y, dy, use_sigma=False, sigma_type='relative', priors=None, device=None):
        eng = super().make_engine(t, filts, y, dy, use_sigma, sigma_type, priors, device)
        eng.set_custom(self.compile(device=eng.device), self.z)
        return eng


def _parse_template(template):
    """``(epochs, {column: values})`` of a template given in either form (see :class:`WithTemplate`), checked."""
    if isinstance(template, tuple) and len(template) == 2 and isinstance(template[1], dict):
        epochs = np.array(template[0], dtype=np.float64)
        cols = {str(k): np.array(v, dtype=np.float64) for k, v in template[1].items()}
    else:
        tab = np.asarray(template, dtype=np.float64)
        if tab.ndim != 2 or tab.shape[1] != len(_SIFTO_COLUMNS):
            raise ValueError('a template is (epochs, {column: values}) or a 2-D array with the columns of '
                             f'sifto_template(): {", ".join(_SIFTO_COLUMNS)}')
        epochs = tab[:, 0].copy()
        cols = {name: tab[:, k].copy() for k, name in enumerate(_SIFTO_COLUMNS) if k}
    if epochs.ndim != 1 or len(epochs) < 4:
        raise ValueError('a template needs at least 4 epochs (the smallest not-a-knot spline)')
    if not np.all(np.isfinite(epochs)) or not np.all(np.diff(epochs) > 0.):
        raise ValueError('the epochs of a template must be finite and strictly increasing')
    for name, v in cols.items():
        if v.shape != epochs.shape or not np.all(np.isfinite(v)):
            raise ValueError(f'template column {name!r} must have one finite value per epoch')
    return epochs, cols


class WithTemplate(Model):
    """A shock model plus a second peak from a template (extension): ``base`` -- a :class:`ShockCooling`,
    :class:`ShockCooling2`, :class:`ShockCooling3`, :class:`ShockCooling4` or :class:`CustomModel` instance -- and, per
    filter of ``lc``, a template light curve that the fit may shift, stretch and scale.  What
    :class:`BaseCompanionShocking` does with SiFTO (models.py:665-845), for any base model and any template: the
    double-peaked core-collapse light curves, a shock-cooling peak followed by the nickel-powered main peak.

    At a data point ``j`` of filter ``f``::

        m_j(p) = base_j(p_base) + r_f * S_f((t_j - t_max - dt_f) / s)

    ``S_f`` is the not-a-knot cubic spline through the template column of ``f``, 0 outside the template's epochs (and
    for a NaN argument); ``t`` is the observed time (the reference does not redshift it either); ``r_f`` is a parameter
    for the filters whose ``char`` is in ``factors`` and 1 for the others, ``dt_f`` one for those in ``offsets`` and 0
    for the others.  Parameters: ``base.input_names + ['t_\\\\mathrm{max}', 's'] + ['r_X' ...] + ['\\\\Delta t_X' ...]``
    (then ``\\\\sigma`` where ``use_sigma`` appends it).

    ``template``: ``(epochs, {column_name: values})``, or a 2-D array with the columns of :func:`sifto_template`
    (``Epoch, U, B, V, g, r, i``); at least 4 epochs, finite and strictly increasing (``ValueError``).  ``columns`` maps a
    filter of ``lc`` (object or name) to a template column, by default ``filter.char``; a filter of ``lc`` without a
    column raises as the reference does for SiFTO.  ``scale='peak'``: every filter's column is multiplied by
    ``max(lc[quantity] over the filter's rows) / max(column)`` (models.py:701-717); ``scale={filter: value}`` gives the
    peak values instead.

    ``log_likelihood``, ``make_log_posterior``, ``engine_for``, ``lightcurve_mcmc`` and ``model(t, f, *p)`` work as for
    every model; :meth:`components` gives the two terms, ``temperature_radius`` is the base's.  The fit runs through
    :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` (one rung at ``beta = 1`` unless a ladder or ``moves`` is
    asked for): the resident samplers, population runs and the other predictive functions compute the model in kernels of
    their own and raise ``LcfError`` for it.  :func:`~lightcurve_fitting_amd.fitting.template_predictive` gives the
    bands of the model and of its two terms over a whole chain, and per sample the two peaks, the hand-over and the dip
    between them (built-in bases); ``model(t, f, *p)`` on a thinned chain gives single curves.  Non-detections
    are measurements of zero, as in the reference: ``nondet='censored'`` raises ``ValueError`` (out of scope)."""

    def __init__(self, base, template, lc, columns=None, factors=(), offsets=(), scale='peak'):
        if not isinstance(base, (ShockCooling, ShockCooling2, ShockCooling3, ShockCooling4, CustomModel)):
            raise TypeError('the base of WithTemplate is a ShockCooling, ShockCooling2, ShockCooling3, ShockCooling4 or '
                            f'CustomModel instance, not {type(base).__name__}: companion-shocking models have a template '
                            'of their own, central-engine models have no filters')
        super().__init__(None, redshift=0.)
        self.base = base
        self.z = base.z
        self.output_quantity = base.output_quantity
        self.model_id = base.model_id
        self.device = base.device
        self.factors, self.offsets = tuple(factors), tuple(offsets)
        for what, chars in (('factors', self.factors), ('offsets', self.offsets)):
            if len(set(chars)) != len(chars) or not all(isinstance(x, str) for x in chars):
                raise ValueError(f'{what} must be distinct filter characters')
        n_base = base.n_model_params
        self.input_names = (list(base.input_names[:n_base]) + ['t_\\mathrm{max}', 's']
                            + ['r_' + x for x in self.factors] + ['\\Delta t_' + x for x in self.offsets])
        self.units = list(base.units[:n_base]) + ['d', ''] + [''] * len(self.factors) + ['d'] * len(self.offsets)
        self._n_par = len(self.input_names)
        self._n_base = n_base
        if self._n_par + 1 > 16:
            raise ValueError('the base model, t_max, s, the factors, the offsets and a fitted sigma take at most 16 columns')
        self._knots, cols = _parse_template(template)
        columns = {} if columns is None else {as_filter(k): str(v) for k, v in columns.items()}
        peaks = None if isinstance(scale, str) else {as_filter(k): float(v) for k, v in scale.items()}
        if peaks is None and scale != 'peak':
            raise ValueError("scale must be 'peak' or a dict {filter: peak value}")
        filts = [as_filter(f) for f in _column(lc, 'filter')]
        if peaks is None:
            names = getattr(lc, 'colnames', None)
            if hasattr(lc, 'calcAbsMag') and names is not None and self.output_quantity not in names:
                for method in {'flux': ('calcFlux',), 'lum': ('calcAbsMag', 'calcLum')}.get(self.output_quantity, ()):
                    getattr(lc, method)()
            y = np.asarray(_column(lc, self.output_quantity), dtype=np.float64)
        self.template = {}
        for filt in dict.fromkeys(filts):  # models.py:701-717
            column = columns.get(filt, filt.char)
            if column not in cols:
                raise Exception('No template for filter ' + filt.name)
            col = cols[column]
            if peaks is None:
                peak = np.max(y[[f == filt for f in filts]])
            elif filt in peaks:
                peak = peaks[filt]
            else:
                raise ValueError('scale has no peak value for filter ' + filt.name)
            self.template[filt] = not_a_knot_coefficients(self._knots, col * peak / np.max(col))

    @property
    def n_model_params(self):
        return self._n_par

    def __repr__(self):
        return f'<{self.__class__.__name__}: {self.base!r} + template of {len(self._knots)} epochs>'

    def _template_tables(self, uniq_filters):
        """What ``Engine.set_template`` takes for these filters: coefficients, factor and offset columns."""
        coef = np.zeros((len(uniq_filters), len(self._knots) - 1, 4))
        fac, off = [], []
        first = self._n_base + 2
        for i, f in enumerate(uniq_filters):
            if f not in self.template:
                raise Exception('No template for filter ' + f.name)
            coef[i] = self.template[f]
            fac.append(first + self.factors.index(f.char) if f.char in self.factors else -1)
            off.append(first + len(self.factors) + self.offsets.index(f.char) if f.char in self.offsets else -1)
        return coef, fac, off

    def make_engine(self, t, filts, y, dy, use_sigma=False, sigma_type='relative', priors=None, device=None):
        """The base model's engine on this photometry with the template attached (``Engine.set_template``)."""
        filts = [as_filter(f) for f in filts]
        uniq, _ = _index_filters(filts)
        coef, fac, off = self._template_tables(uniq)   # (raises before anything is built)
        pri = None if priors is None else [p.descriptor() for p in priors]
        if pri is not None and len(pri) != self._n_par + bool(use_sigma):
            raise ValueError(f'priors must have length {self._n_par + bool(use_sigma)}')
        eng = self.base.make_engine(t, filts, y, dy, use_sigma, sigma_type, None, device)
        eng.set_template(self._knots, coef, fac, off, self._n_base, self._n_base + 1, self._n_par - self._n_base, pri)
        return eng

    def engine_for(self, lc, use_sigma=False, sigma_type='relative', priors=None, nondet='gaussian'):
        """As :meth:`Model.engine_for`; ``nondet='censored'`` raises ``ValueError``: upper limits together with a template
        are out of scope."""
        _check_nondet_mode(nondet)
        if nondet == 'censored':
            raise ValueError("nondet='censored' is out of scope for a WithTemplate model: its non-detections enter as "
                             "measurements of zero ('gaussian'), as in the reference")
        return super().engine_for(lc, use_sigma, sigma_type, priors)

    def _component(self, component, t_in, f, *params):
        if len(params) != self.n_model_params:
            raise TypeError(f'{type(self).__name__} takes {self.n_model_params} parameters, got {len(params)}')
        cols = np.broadcast_arrays(*[np.asarray(x, dtype=np.float64) for x in params])
        scalar = cols[0].ndim == 0
        eng, shape = self._eval_engine(t_in, f, scalar)
        P = np.column_stack([np.atleast_1d(c).ravel() for c in cols])
        y = eng.evaluate_components(P, component)  # (n, npoints)
        y = y[0] if scalar else y.T
        if shape is not None:
            y = y.reshape(shape if scalar else shape + (len(P),))
        return y

    def evaluate(self, t_in, f, *params):
        """Model light curve(s), both components; shapes as :meth:`Model.evaluate`."""
        return self._component('total', t_in, f, *params)

    def components(self, t_in, f, *params):
        """``(base, template)``: the two terms of :meth:`evaluate`, in its shapes."""
        return self._component('base', t_in, f, *params), self._component('template', t_in, f, *params)

    def temperature_radius(self, t_in, *params):
        """The base model's photosphere (the template has none): ``params`` as the base's ``temperature_radius`` takes
        them; of a whole row of this model, the base's columns are passed on."""
        if len(params) == self._n_par:
            params = params[:self._n_base]
        return self.base.temperature_radius(t_in, *params)


class BaseCentralEngine(Model):
    """A bolometric light curve ``L(t)`` [W] -- one number per epoch, no filters -- from a power source ``P(s)`` at the
    centre of the ejecta, diffusing out as in Arnett (1982); fitted to what ``calculate_bolometric`` produces.

    With ``t = (MJD - t_0) / (1 + z)`` in days, ``L = 0`` for ``t <= 0`` and otherwise::

        L(t) = leak(t) * int_0^t P(s) (2 s / tau_m^2) exp(-(t - s)(t + s) / tau_m^2) ds
        leak(t) = 1,  or  1 - exp(-(t_gamma / t)^2)  with gamma_leakage=True

    The integral is one fixed 64-node quadrature that is part of the model's definition (``include/lcf.h``, "central-
    engine models"): within 1e-6 of the exact integral (measured: 4e-12) for ``2 <= tau_m <= 60`` d,
    ``0.01 <= t <= 400`` d and a magnetar spin-down time ``1 <= t_p <= 100`` d.  Below ``t_p = 1`` d the accuracy
    degrades (5e-6 at 0.1 d), so a prior should keep ``t_p`` above it.  A non-finite parameter, ``tau_m <= 0``,
    ``t_p <= 0`` or ``t_gamma <= 0`` gives NaN: the priors have to exclude them.

    ``lc`` needs the columns ``MJD``, ``ycol`` (default ``'L_bol'``) and ``dycol`` (default ``'d' + ycol``), in watts, and
    no ``filter`` column; rows with a non-finite or non-positive uncertainty raise ``ValueError`` (``calculate_bolometric``
    leaves NaN where a fit failed: drop those rows).  ``model(t, *p)`` evaluates ``L``; ``log_likelihood``,
    ``make_log_posterior`` and ``lightcurve_mcmc`` work as for every model, the fit running through
    :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` (one rung at ``beta = 1`` unless a ladder is asked for).
    :func:`~lightcurve_fitting_amd.fitting.luminosity_predictive` gives the percentile bands of ``L(t)`` over a whole
    chain, and every sample's peak luminosity and rise time.  The resident sampler, ``posterior_predictive``,
    ``thermal_predictive`` and ``temperature_radius`` are compiled per photometric model and raise ``LcfError`` here."""
    #: parameters of the source, in front of tau_m
    _source_names = []
    _source_units = []

    def __init__(self, lc=None, redshift=0., gamma_leakage=False, ycol='L_bol', dycol=None):
        super().__init__(lc, redshift=redshift)
        self.gamma_leakage = bool(gamma_leakage)
        self.output_quantity = ycol
        self.dycol = 'd' + ycol if dycol is None else dycol
        self.input_names = list(self._source_names) + ['\\tau_m'] + (['t_\\gamma'] if self.gamma_leakage else []) + ['t_0']
        self.units = list(self._source_units) + ['d'] + (['d'] if self.gamma_leakage else []) + ['d']
        self._n_par = len(self.input_names)

    def __repr__(self):
        return f'<{self.__class__.__name__}: z={self.z:.3f}, gamma_leakage={self.gamma_leakage}>'

    @property
    def n_model_params(self):
        return self._n_par

    def _consts(self):
        return [float(self.z), 1. if self.gamma_leakage else 0.]

    def make_engine(self, t, y, dy, use_sigma=False, sigma_type='relative', priors=None, device=None):
        """Build a device engine for an explicit bolometric light curve: epochs ``t`` (MJD), ``y`` and ``dy`` in W."""
        if sigma_type == 'relative':
            st = _eng.SIGMA_RELATIVE
        elif sigma_type == 'absolute':
            st = _eng.SIGMA_ABSOLUTE
        else:
            raise Exception('sigma_type must either be "relative" or "absolute"')
        dy = np.asarray(dy, dtype=np.float64)
        bad = np.nonzero(~(np.isfinite(dy) & (dy > 0.)))[0]
        if len(bad):
            raise ValueError(f'rows {bad.tolist()} of the light curve have a non-finite or non-positive {self.dycol}: '
                             'drop them (calculate_bolometric leaves NaN where a fit failed)')
        pri = None if priors is None else [p.descriptor() for p in priors]
        return _eng.Engine(self.model_id, self.n_model_params, self._consts(), t, y, dy, None, None, None, None,
                           use_sigma=use_sigma, sigma_type=st, priors=pri,
                           device=self.device if device is None else device)

    def engine_for(self, lc, use_sigma=False, sigma_type='relative', priors=None, nondet='gaussian'):
        """Engine bound to the columns ``MJD``, ``ycol`` and ``dycol`` as ``lc`` holds them NOW (cached by content, as
        :meth:`Model.engine_for`).  A bolometric table has no non-detections: ``nondet='censored'`` with a true ``nondet``
        row raises ``LcfError`` (status 5)."""
        if sigma_type not in ('relative', 'absolute'):
            raise Exception('sigma_type must either be "relative" or "absolute"')
        _check_nondet_mode(nondet)
        if nondet == 'censored' and _nondet_mask(lc) is not None:
            raise _eng.LcfError(5, 'a central-engine model (Arnett, Magnetar) fits a bolometric table, which has no '
                                   'non-detections: upper limits belong to photometric models')
        t = np.asarray(_column(lc, 'MJD'), dtype=np.float64)
        y = np.asarray(_column(lc, self.output_quantity), dtype=np.float64)
        dy = np.asarray(_column(lc, self.dycol), dtype=np.float64)
        none = np.empty(0, dtype=object)
        mode = (bool(use_sigma), sigma_type, None if priors is None else tuple(p.descriptor() for p in priors))
        for k, bound in enumerate(self._bound):
            if bound.mode == mode and bound.holds(t, none, y, dy):
                if k:  # most recently used first
                    self._bound.insert(0, self._bound.pop(k))
                return bound.engine
        eng = self.make_engine(t, y, dy, use_sigma, sigma_type, priors)
        self._bound.insert(0, _BoundEngine(eng, mode, t, none, y, dy))
        del self._bound[self.max_bound_engines:]
        return eng

    def _grid_engine(self, t_in):
        """The evaluation engine on the times ``t_in`` (1-D float64): dummy data, no sigma, no priors."""
        key = ('eval', t_in.tobytes())
        eng = self._engines.get(key)
        if eng is None:
            eng = self.make_engine(t_in, np.zeros(len(t_in)), np.ones(len(t_in)))
            self._engines = {key: eng}  # one evaluation grid at a time
        return eng

    def evaluate(self, t_in, *params):
        """``L(t)`` [W] at the times ``t_in`` (MJD).  Scalar parameters -> (ntimes,); array parameters of length n ->
        (ntimes, n)."""
        if len(params) != self.n_model_params:
            raise TypeError(f'{type(self).__name__} takes {self.n_model_params} parameters, got {len(params)}')
        t_in = np.atleast_1d(np.asarray(t_in, dtype=np.float64)).ravel()
        cols = np.broadcast_arrays(*[np.asarray(x, dtype=np.float64) for x in params])
        scalar = cols[0].ndim == 0
        eng = self._grid_engine(t_in)
        y = eng.evaluate(np.column_stack([np.atleast_1d(c).ravel() for c in cols]))  # (n, ntimes)
        return y[0] if scalar else y.T

    def temperature_radius(self, t_in, *params):
        """Not for this family: the model is a luminosity, it has no photosphere.  Raises ``LcfError`` (status 5)."""
        raise _eng.LcfError(5, 'temperature_radius is compiled per photometric model: a central-engine model (Arnett, '
                               'Magnetar) is a bolometric luminosity without a photosphere; model(t, *p) evaluates it, '
                               'and its fit runs through the tempered route (TemperedSampler)')

    @staticmethod
    def ejecta_mass(tau_m, v_ej, kappa=0.07, beta=13.8):
        """Ejecta mass [Msun] from the diffusion time: ``tau_m^2 beta c v_ej / (2 kappa)`` with ``tau_m`` [d], ``v_ej``
        [1000 km/s] and the opacity ``kappa`` [cm^2/g] (Arnett 1982; ``beta = 13.8``).  Vectorised."""
        tau = np.asarray(tau_m, dtype=np.float64) * 86400.
        v = np.asarray(v_ej, dtype=np.float64) * 1e8
        return tau ** 2 * beta * 2.99792458e10 * v / (2. * kappa) / 1.988409870698051e33

    @staticmethod
    def kinetic_energy(M_ej, v_ej):
        """Kinetic energy [1e51 erg] of homogeneous ejecta: ``0.3 M_ej v_ej^2`` with ``M_ej`` [Msun] and ``v_ej``
        [1000 km/s].  Vectorised."""
        v = np.asarray(v_ej, dtype=np.float64) * 1e8
        return 0.3 * np.asarray(M_ej, dtype=np.float64) * 1.988409870698051e33 * v ** 2 / 1e51


class Arnett(BaseCentralEngine):
    """Radioactive heating by 56Ni -> 56Co -> 56Fe (Arnett 1982; Valenti et al. 2008): parameters ``M_Ni`` [Msun],
    ``tau_m`` [d], (``t_gamma`` [d] with ``gamma_leakage=True``,) ``t_0`` [d];
    ``P(s) = M_Ni Msun [(e_Ni - e_Co) exp(-s / 8.8 d) + e_Co exp(-s / 111.3 d)]`` with ``e_Ni = 3.9e10`` and
    ``e_Co = 6.78e9`` erg/s/g."""
    model_id = _eng.MODEL_ARNETT
    _source_names = ['M_\\mathrm{Ni}']
    _source_units = ['Msun']


class Magnetar(BaseCentralEngine):
    """Magnetar spin-down (Kasen & Bildsten 2010): parameters ``E_p`` [1e51 erg], ``t_p`` [d], ``tau_m`` [d], (``t_gamma``
    [d] with ``gamma_leakage=True``,) ``t_0`` [d]; ``P(s) = E_p / t_p / (1 + s / t_p)^2``.  The quadrature holds its
    accuracy for ``t_p >= 1`` d."""
    model_id = _eng.MODEL_MAGNETAR
    _source_names = ['E_p', 't_p']
    _source_units = ['10^51 erg', 'd']


def blackbody_to_filters(filters, T, R, z=0., cutoff_freq=np.inf, ebv=0., variant=None):
    """Band-averaged L_nu of blackbodies through filters (models.py:1131-1165).

    Pointwise when ``T`` is 1-D with one entry per filter, else every filter for every (T, R): result shape
    ``(nfilters,) + T.shape``.  ``ebv``: one E(B-V) for the whole call (the reddening goes into the table weights at
    pack time); per-walker reddening inside a fit is ``ShockCooling3``'s job.  ``variant``: the band-sum level
    (``Engine.set_variant``; None = the engine's default, the interpolants of ln S(ln T))."""
    if np.ndim(ebv) != 0:
        raise NotImplementedError('blackbody_to_filters takes one scalar E(B-V) per call')
    T = np.array(T, dtype=np.float64)
    R = np.array(R, dtype=np.float64)
    if T.shape != R.shape:
        raise Exception('T & R must have the same shape')
    filts = [as_filter(f) for f in (filters if not isinstance(filters, (Filter, str)) else [filters])]
    uniq, idx = _index_filters(filts)
    if ebv:
        tabs = PackedTables(uniq, z=z, cutoff_freq=cutoff_freq, compress=False, reddening=True)
        tabs.w = tabs.w * 10. ** (-0.4 * float(ebv) * tabs.ext)
        ctab = None
    else:
        tabs = PackedTables(uniq, z=z, cutoff_freq=cutoff_freq)
        ctab = (tabs.coff, tabs.ca, tabs.cw, tabs.ctmin)
    itab = None if ebv else (tabs.icoef, tabs.itmin, tabs.iu0, tabs.ih)
    eng = _eng.Engine(_eng.MODEL_BLACKBODY, 2, [], np.zeros(1), np.zeros(1), np.ones(1), np.zeros(1, dtype=np.int32),
                      tabs.off, tabs.a, tabs.w, ctab=ctab, itab=itab)  # (pointwise kernel: interpolants + cool level)
    if variant is not None:
        eng.set_variant(variant)
    try:
        if T.ndim == 1 and len(T) == len(filts):
            return eng.blackbody_to_filters(idx, T, R)
        flat_T, flat_R = T.ravel(), R.ravel()
        out = eng.blackbody_to_filters(np.repeat(idx, flat_T.size), np.tile(flat_T, len(filts)),
                                       np.tile(flat_R, len(filts)))
        return out.reshape((len(filts),) + T.shape)
    finally:
        eng.close()
