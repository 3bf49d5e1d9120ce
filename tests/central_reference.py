"""NumPy restatement of the central-engine models ``Arnett`` and ``Magnetar`` (a helper, not a test): the fixed
quadrature rule that is part of their definition ("Central-engine models"), both power sources, the
light curve ``L(t)`` in watts and the Gaussian log-likelihood in the three sigma modes -- what the device kernel
``k_central_points`` is held to -- and ``truth``: the same integral by ``scipy.integrate.quad``.

Rest-frame time ``t = (MJD - t_0) / (1 + z)`` in days; ``L = 0`` for ``t <= 0``, else

    L(t) = leak(t) * int_0^t P(s) (2 s / tau_m^2) exp(-(t - s)(t + s) / tau_m^2) ds

The rule: cut the range to ``[s_lo, t]``, ``s_lo = sqrt(max(0, t^2 - 40 tau_m^2))``; split it at
``s_lo + (t - s_lo) / 8``; 32 Gauss-Legendre nodes on each piece.  Parameter rows: Arnett ``M_Ni, tau_m, [t_gamma,]
t_0``, Magnetar ``E_p, t_p, tau_m, [t_gamma,] t_0``, then sigma when it is fitted."""
import numpy as np

M_SUN = 1.988409870698051e33            # g
EPS_NI, EPS_CO = 3.9e10, 6.78e9         # erg / s / g
TAU_NI, TAU_CO = 8.8, 111.3             # d
CUT, SPLIT, NODES = 40., 0.125, 32
GL_X, GL_W = np.polynomial.legendre.leggauss(NODES)

#: the box the rule is held to 1e-6 in (days)
BOX = dict(tau_m=(2., 60.), t=(0.01, 400.), t_p=(1., 100.))

N_SOURCE = {'arnett': 1, 'magnetar': 2}   # source parameters in front of tau_m


def source(kind, s, src):
    """P(s) [W].  ``src``: (M_Ni,) [Msun] or (E_p [1e51 erg], t_p [d]); everything broadcasts."""
    if kind == 'arnett':
        return src[0] * M_SUN * ((EPS_NI - EPS_CO) * np.exp(-s / TAU_NI) + EPS_CO * np.exp(-s / TAU_CO)) * 1e-7
    if kind == 'magnetar':
        d = 1. + s / src[1]
        return src[0] * 1e51 / (src[1] * 86400.) / (d * d) * 1e-7
    raise ValueError(kind)


def integrand(kind, s, t, src, tau_m):
    return source(kind, s, src) * (2. * s / tau_m ** 2) * np.exp(-((t - s) * (t + s)) / tau_m ** 2)


def pieces(t, tau_m):
    """``(s_lo, s_mid)`` of the rule at rest-frame time ``t > 0``."""
    s_lo = np.sqrt(np.maximum(0., t * t - CUT * (tau_m * tau_m)))
    return s_lo, s_lo + (t - s_lo) * SPLIT


def rule(kind, t, src, tau_m):
    """The diffusion integral (no leakage) by the fixed rule at rest-frame times ``t > 0``; arguments broadcast."""
    t, tau_m = np.asarray(t, dtype=np.float64), np.asarray(tau_m, dtype=np.float64)
    src = [np.asarray(v, dtype=np.float64)[..., None] for v in src]
    s_lo, s_mid = pieces(t, tau_m)
    total = 0.
    for a, b in ((s_lo, s_mid), (s_mid, t)):
        h, c = 0.5 * (b - a), 0.5 * (a + b)
        s = c[..., None] + h[..., None] * GL_X
        inv_tau2 = (1. / (tau_m * tau_m))[..., None]
        g = source(kind, s, src) * (2. * s * inv_tau2) * np.exp(-((t[..., None] - s) * (t[..., None] + s)) * inv_tau2)
        total = total + np.sum(g * (h[..., None] * GL_W), axis=-1)
    return total


def leak_factor(t, t_gamma):
    """``1 - exp(-(t_gamma / t)^2)``, evaluated without cancellation."""
    return -np.expm1(-(t_gamma / t) ** 2)


def truth(kind, t, src, tau_m, t_gamma=None):
    """L(t) [W] at ONE rest-frame time by ``scipy.integrate.quad(epsrel=1e-13)`` over the whole of ``[0, t]`` (the
    rule's break points are handed over as ``points`` so that a narrow peak at ``s = t`` is not missed)."""
    from scipy.integrate import quad
    if not t > 0.:
        return 0.
    s_lo, s_mid = (float(v) for v in pieces(np.float64(t), np.float64(tau_m)))
    pts = sorted({p for p in (s_lo, s_mid, t - 6. * tau_m ** 2 / (2. * t)) if 0. < p < t})
    val, _ = quad(lambda s: float(integrand(kind, s, t, src, tau_m)), 0., t, epsrel=1e-13, epsabs=0., limit=400,
                  points=pts or None)
    return val * (1. if t_gamma is None else float(leak_factor(t, t_gamma)))


def split_rows(kind, P, leak, use_sigma=False):
    """Columns of parameter rows ``P`` (n, D): ``(src, tau_m, t_gamma or None, t_0, sigma or None)``."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    k = N_SOURCE[kind]
    src = [P[:, j] for j in range(k)]
    tau_m = P[:, k]
    t_gamma = P[:, k + 1] if leak else None
    t_0 = P[:, k + 1 + int(bool(leak))]
    want = k + 2 + int(bool(leak)) + int(bool(use_sigma))
    assert P.shape[1] == want, (P.shape, want)
    return src, tau_m, t_gamma, t_0, (P[:, -1] if use_sigma else None)


def luminosity(kind, mjd, P, z=0., leak=False, use_sigma=False):
    """L [W], shape (n, npoints), of rows ``P`` at the epochs ``mjd``: exactly 0 where ``t <= 0``; NaN in every epoch of
    a row with a non-finite parameter, ``tau_m <= 0``, ``t_p <= 0`` or ``t_gamma <= 0``."""
    src, tau_m, t_gamma, t_0, _ = split_rows(kind, P, leak, use_sigma)
    mjd = np.asarray(mjd, dtype=np.float64)
    with np.errstate(all='ignore'):
        t = (mjd[None, :] - t_0[:, None]) / (1. + z)
        late = t > 0.
        ts = np.where(late, t, 1.)
        L = rule(kind, ts, [v[:, None] for v in src], tau_m[:, None])
        if leak:
            L = L * leak_factor(ts, t_gamma[:, None])
        L = np.where(late, L, np.where(np.isnan(t), np.nan, 0.))
        bad = ~np.isfinite(tau_m) | ~(tau_m > 0.) | ~np.isfinite(t_0)
        for v in src:
            bad |= ~np.isfinite(v)
        if kind == 'magnetar':
            bad |= ~(src[1] > 0.)
        if leak:
            bad |= ~np.isfinite(t_gamma) | ~(t_gamma > 0.)
        L[bad] = np.nan
    return L


def gaussian_log_likelihood(L, y, dy, sigma=None, sigma_type='relative'):
    """``Model.log_likelihood`` for model values ``L`` (n, npoints); ``sigma`` (n,) or None."""
    y, dy = np.asarray(y, dtype=np.float64)[None, :], np.asarray(dy, dtype=np.float64)[None, :]
    with np.errstate(all='ignore'):
        if sigma is None:
            s = dy
        else:
            unit = dy if sigma_type == 'relative' else np.median(dy)
            s = np.sqrt(dy ** 2. + (unit * np.asarray(sigma)[:, None]) ** 2.)
        return -0.5 * np.sum(np.log(2. * np.pi * s ** 2.) + ((y - L) / s) ** 2., axis=1)


def log_likelihood(kind, mjd, y, dy, P, z=0., leak=False, use_sigma=False, sigma_type='relative'):
    """(n,) log-likelihoods of rows ``P`` (with sigma as the last column when ``use_sigma``)."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    L = luminosity(kind, mjd, P, z, leak, use_sigma)
    return gaussian_log_likelihood(L, y, dy, P[:, -1] if use_sigma else None, sigma_type)


def log_uniform(rng, lo, hi, size=None):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))
