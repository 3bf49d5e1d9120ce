"""Integrated autocorrelation time of MCMC chains: ``emcee.autocorr.integrated_time`` and its ``AutocorrError``.

The estimator runs on the GPU (``lcf_autocorr_time`` / ``lcf_samplers_autocorr_time`` in ``include/lcf.h``): per
parameter, the walkers' normalised autocorrelations are averaged, ``taus = 2 cumsum(f) - 1``, and Sokal's window is the
first lag ``k`` with ``k >= c taus[k]`` -- only the lags up to it are computed.  There is no CPU fallback.  The ``tol``
check, the exception and the warning follow emcee's text.
"""
import logging

import numpy as np

from . import engine as _engine

logger = logging.getLogger(__name__)


class AutocorrError(Exception):
    """Raised if the chain is too short to estimate an autocorrelation time.  ``tau`` holds the estimate."""

    def __init__(self, tau, *args, **kwargs):
        self.tau = tau
        super().__init__(*args, **kwargs)


def _as_3d(x, has_walkers=True):
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if x.ndim == 1:
        x = x[:, np.newaxis, np.newaxis]
    if x.ndim == 2:
        x = x[:, np.newaxis, :] if not has_walkers else x[:, :, np.newaxis]
    if x.ndim != 3:
        raise ValueError('invalid dimensions')
    return x


def convergence_message(tau, n_t, tol):
    """emcee's message for estimates with ``tol * tau > n_t`` (None if there are none)."""
    flag = tol * np.asarray(tau) > n_t
    if not np.any(flag):
        return None
    msg = ('The chain is shorter than {0} times the integrated autocorrelation time for {1} parameter(s). Use this '
           'estimate with caution and run a longer chain!\n').format(tol, np.sum(flag))
    return msg + 'N/{0} = {1:.0f};\ntau: {2}'.format(tol, n_t / tol, tau)


def check_convergence(tau, n_t, tol=50, quiet=False):
    """Raise :class:`AutocorrError` (or, with ``quiet``, log a warning) if the chain is shorter than ``tol * tau``."""
    msg = convergence_message(tau, n_t, tol)
    if msg is not None:
        if not quiet:
            raise AutocorrError(tau, msg)
        logger.warning(msg)
    return tau


def integrated_time(x, c=5, tol=50, quiet=False, has_walkers=True, device=0):
    """Estimate the integrated autocorrelation time of a time series (emcee's ``integrated_time``).

    ``x``: (n_t,), (n_t, n_w) if ``has_walkers`` else (n_t, n_d), or (n_t, n_w, n_d).  ``c``: window factor; ``tol``:
    minimum number of autocorrelation times the chain must span; ``quiet``: warn instead of raising
    :class:`AutocorrError`.  Returns ``tau`` of shape (n_d,)."""
    x = _as_3d(x, has_walkers)
    if x.shape[0] == 0 or x.shape[1] == 0 or x.shape[2] == 0:
        raise ValueError('the chain is empty')
    tau, _ = _engine.autocorr_time(x, c, device=device)
    return check_convergence(tau, x.shape[0], tol, quiet)
