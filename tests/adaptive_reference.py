"""NumPy restatement of the adaptive ladder and of the stepping-stone estimator (a helper, not a test): the definition
``lcf_tempered_run_adaptive`` / ``k_t_adapt`` and ``lcf_tempered_stepping_stones`` / ``k_t_stone`` are held to, on top of
``tempered_reference`` (same generators, likelihood, swap step and start).

The ladder rule (Vousden, Farr & Mandel 2016), after the swaps of an ODD step, if every pair was offered since the last
adaptation: ``A_k`` = accepted / offered swaps of pair ``k`` since then, ``kappa = lag / (t + lag) / time`` with ``t`` the
adapting steps made (this one included), ``dT_k = (1 / beta_{k+1} - 1 / beta_k) exp(kappa (A_k - A_{k+1}))`` for
``k = 0 .. K - 3``, then left to right ``T_0 = 1``, ``T_{k+1} = T_k + dT_k``, ``beta_{k+1} = 1 / T_{k+1}``.  ``beta_0 = 1``
and ``beta_{K-1} = 0`` never move.

``python tests/adaptive_reference.py`` prints the reference log-evidence of ``small_problem()`` by importance sampling
(see :func:`importance_log_evidence`); ``python tests/adaptive_reference.py restate SEED...`` prints what the restatement
of the end-to-end case of tests/test_gpu_adaptive.py gives for those seeds."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:        # (run as a script: only tests/ is on the path)
    sys.path.insert(0, ROOT)
import tempered_reference as R  # noqa: E402
from oracle import lcf_oracle as O  # noqa: E402


def adapt_ladder(betas, A, t, lag, time):
    """The ladder after one adaptation, from the pairs' swap fractions ``A`` (K - 1,).  A new array."""
    betas = np.array(betas, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    K = len(betas)
    if K < 3 or betas[-1] != 0.:
        raise ValueError('an adaptive ladder needs at least 3 rungs and a last rung at beta = 0')
    kappa = lag / (t + lag) / time
    dT = (1. / betas[1:K - 1] - 1. / betas[0:K - 2]) * np.exp(kappa * (A[:K - 2] - A[1:K - 1]))
    T = 1.
    for k in range(K - 2):          # (in this order: the device's one lane)
        T = T + dT[k]
        betas[k + 1] = 1. / T
    return betas


class Window:
    """The swap counts since the last adaptation."""

    def __init__(self, n_pairs):
        self.acc, self.prop = np.zeros(n_pairs, dtype=np.int64), np.zeros(n_pairs, dtype=np.int64)

    def clear(self):
        self.acc[:] = 0
        self.prop[:] = 0


def run(pb, x0, betas, nsteps, seed, lag=10000., time=100., t0=0, adapt=True, a=2., first_step=0, window=None,
        state=None):
    """``tempered_reference.run`` with a ladder that adapts (``adapt=False``: frozen, then the two agree).  ``t0``: the
    adapting steps made before; ``window``: the :class:`Window` of an adapting run this one continues (None: empty);
    ``state``: ``(x, lnL, lnpr)`` to go on from instead of evaluating ``x0``.  Returns the dict of
    ``tempered_reference.run`` plus ``betas`` (the ladder after the run), ``beta_history`` (n, K) (the ladder every step
    was sampled under), ``adaptations``, ``window`` and ``state``."""
    betas = np.array(betas, dtype=np.float64)
    K = len(betas)
    if adapt and (K < 3 or betas[-1] != 0.):
        raise ValueError('an adaptive ladder needs at least 3 rungs and a last rung at beta = 0')
    if state is None:
        x = np.array(x0, dtype=np.float64)
        W, D = x.shape[1:]
        ll = R.log_like(pb, x.reshape(-1, D)).reshape(K, W)
        lpr = R.log_prior(pb, x.reshape(-1, D)).reshape(K, W)
    else:
        x, ll, lpr = (np.array(v, dtype=np.float64) for v in state)
        W, D = x.shape[1:]
    assert np.all(np.isfinite(lpr)) and not np.any(np.isnan(ll))
    window = Window(K - 1) if window is None else window
    chain, lls, hist = np.empty((nsteps, K, W, D)), np.empty((nsteps, K, W)), np.empty((nsteps, K))
    nacc = np.zeros((K, W), dtype=np.int64)
    sw_acc, sw_prop = np.zeros(K - 1, dtype=np.int64), np.zeros(K - 1, dtype=np.int64)
    move_margin, swap_margin, nan_proposals, adaptations = np.inf, np.inf, 0, 0
    half_n = (W + 1) // 2
    for it in range(nsteps):
        s = first_step + it
        perms = [O.split_permutation(R.rung_seed(seed, k), s, W) for k in range(K)]
        for half in (0, 1):
            act, q, zl, ln_u = [], [], [], []
            for k in range(K):
                sets = (perms[k][:half_n], perms[k][half_n:])
                ak, oth = sets[half], sets[1 - half]
                z, j, lu = O.stretch_draws(R.rung_seed(seed, k), s, half, ak, len(oth), a)
                partner = x[k, oth[j]]
                act.append(ak)
                q.append(partner - (partner - x[k, ak]) * z[:, None])
                zl.append((D - 1.) * np.log(z))
                ln_u.append(lu)
            with np.errstate(all='ignore'):
                q_ll = R.log_like(pb, np.concatenate(q))
            q_lpr = R.log_prior(pb, np.concatenate(q))
            lo = 0
            for k in range(K):
                n = len(act[k])
                lq, pq, ak = q_ll[lo:lo + n], q_lpr[lo:lo + n], act[k]
                lo += n
                inside = np.isfinite(pq)
                if np.any(np.isnan(lq) & inside):
                    raise ValueError('Probability function returned NaN')
                nan_proposals += int(np.sum(np.isnan(lq)))
                test = inside & (lq > -np.inf)
                with np.errstate(invalid='ignore'):
                    dl = betas[k] * (lq - ll[k, ak]) if betas[k] > 0. else 0.
                    stat = zl[k] + dl + (pq - lpr[k, ak])
                    ok = test & (stat > ln_u[k])
                if test.any():
                    move_margin = min(move_margin, float(np.min(np.abs(stat[test] - ln_u[k][test]))))
                x[k, ak[ok]] = q[k][ok]
                ll[k, ak[ok]] = lq[ok]
                lpr[k, ak[ok]] = pq[ok]
                nacc[k, ak[ok]] += 1
        acc, prop, margin = R.swap_step(x, ll, lpr, betas, seed, s)
        sw_acc += acc
        sw_prop += prop
        swap_margin = min(swap_margin, margin)
        chain[it], lls[it], hist[it] = x, ll, betas
        if adapt:
            window.acc += acc
            window.prop += prop
            if (s & 1) and np.all(window.prop > 0):
                betas = adapt_ladder(betas, window.acc / window.prop, t0 + it + 1, lag, time)
                window.clear()
                adaptations += 1
    return dict(chain=chain, lnL=lls, nacc=nacc, swaps_accepted=sw_acc, swaps_proposed=sw_prop, move_margin=move_margin,
                swap_margin=swap_margin, nan_proposals=nan_proposals, betas=betas, beta_history=hist,
                adaptations=adaptations, window=window, state=(x, ll, lpr))


_runs = {}


def cached_run(nwalkers, betas, nsteps, seed, lag, time):
    """``(pb, x0, run(...))`` of a test case with ``t0 = 0``, computed once per process (callers leave it unchanged)."""
    key = (int(nwalkers), tuple(betas), int(nsteps), int(seed), float(lag), float(time))
    if key not in _runs:
        pb = R.problem(False)
        x0 = R.start(pb, len(betas), nwalkers, seed)
        _runs[key] = (pb, x0, run(pb, x0, betas, nsteps, seed, lag, time))
    return _runs[key]


# ---- stepping stones --------------------------------------------------------------------------------------------------
def batch_edges(n, batches):
    """The ``batches + 1`` edges ``(b * n) // batches`` of the contiguous batches of ``n`` steps."""
    return (np.arange(batches + 1) * n) // batches


def stone_partials(lnL, betas, batches, discard=0):
    """``(max, sum, count)``, each (K - 1, batches), of ``lnL`` (n, K, W): per pair ``k`` and batch over rung ``k + 1``,
    the maximum ``m``, ``sum exp((betas[k] - betas[k+1]) (ln L - m))`` (0 when ``m = -inf``) and the number of terms."""
    lnL = np.asarray(lnL, dtype=np.float64)[discard:]
    betas = np.asarray(betas, dtype=np.float64)
    n, K = lnL.shape[:2]
    if batches > n:
        raise ValueError('more batches than steps')
    edges = batch_edges(n, batches)
    m, total, count = (np.empty((K - 1, batches)) for _ in range(3))
    for k in range(K - 1):
        for b in range(batches):
            v = lnL[edges[b]:edges[b + 1], k + 1].ravel()
            m[k, b] = np.max(v)
            with np.errstate(invalid='ignore'):
                total[k, b] = np.sum(np.exp((betas[k] - betas[k + 1]) * (v - m[k, b]))) if m[k, b] > -np.inf else 0.
            count[k, b] = v.size
    return m, total, count


def log_ratios(betas, partials):
    """``ln r_kb = dbeta_k m + ln(sum / count)``, (K - 1, batches)."""
    betas = np.asarray(betas, dtype=np.float64)
    m, total, count = partials
    return (betas[:-1] - betas[1:])[:, None] * m + np.log(total / count)


def stepping_stone(lnL, betas, batches=8, discard=0):
    """``(lnZ, dlnZ)`` of ``lnL`` (n, K, W), restated directly: per pair the log of the average of ``L**dbeta`` over all
    kept samples of rung ``k + 1`` (by log-sum-exp), and the batch-means standard error of the batches' own logs."""
    lnL = np.asarray(lnL, dtype=np.float64)[discard:]
    betas = np.asarray(betas, dtype=np.float64)
    n, K = lnL.shape[:2]
    edges = batch_edges(n, batches)
    lnZ, var = 0., 0.
    for k in range(K - 1):
        d = betas[k] - betas[k + 1]

        def ln_mean(v):
            top = np.max(v)
            return d * top + np.log(np.mean(np.exp(d * (v - top))))
        lnZ += ln_mean(lnL[:, k + 1].ravel())
        var += np.var([ln_mean(lnL[edges[b]:edges[b + 1], k + 1].ravel()) for b in range(batches)], ddof=1)
    return float(lnZ), float(np.sqrt(var / batches))


# ---- the independent answer -------------------------------------------------------------------------------------------
PRIOR_LO = np.array([0., 0., 0., 0., -1.])      # the uniform priors of the GPU tests on small_problem()
PRIOR_HI = np.array([10., 10., 10., 10., .5])
LN_PRIOR_VOLUME = float(np.sum(np.log(PRIOR_HI - PRIOR_LO)))   # ln(10^4 * 1.5)


def importance_log_evidence(n=40000, nu=5, seed=3, walkers=24, burn=300, keep=200):
    """``(lnZ, standard error, effective sample size)`` of ``small_problem()`` under NORMALISED uniform priors, by
    importance sampling: a multivariate Student-t (``nu`` degrees of freedom) with the mean and covariance of a cold
    chain (one rung of ``tempered_reference.run``, ``keep`` steps after ``burn``), ``n`` draws, weights
    ``L * 1[inside the prior] / t``.  The engine's uniform priors are unnormalised (``ln prior = 0`` inside), so the mean
    weight estimates ``integral of L``; the ladder's estimators give ``ln(Z(1) / Z(0))`` with ``Z(0)`` the prior's
    volume, hence ``lnZ = ln(mean weight) - ln(10^4 * 1.5)``."""
    pb = R.problem(False)
    cold = R.run(pb, R.start(pb, 1, walkers, seed), (1.,), burn + keep, seed)['chain'][burn:, 0].reshape(-1, 5)
    mu, cov = cold.mean(axis=0), np.cov(cold.T)
    D = len(mu)
    rng = np.random.default_rng(seed)
    chol = np.linalg.cholesky(cov)
    g = rng.standard_normal((n, D)) @ chol.T
    x = mu + g / np.sqrt(rng.chisquare(nu, n) / nu)[:, None]
    from math import lgamma
    maha = np.sum(np.linalg.solve(chol, (x - mu).T) ** 2, axis=0)
    ln_q = (lgamma((nu + D) / 2.) - lgamma(nu / 2.) - .5 * D * np.log(nu * np.pi) - np.sum(np.log(np.diag(chol)))
            - .5 * (nu + D) * np.log1p(maha / nu))
    inside = np.all((x > PRIOR_LO) & (x < PRIOR_HI), axis=1)
    ln_w = np.full(n, -np.inf)
    with np.errstate(all='ignore'):
        ln_w[inside] = R.log_like(pb, x[inside]) - ln_q[inside]
    ln_w[np.isnan(ln_w)] = -np.inf
    top = np.max(ln_w)
    w = np.exp(ln_w - top)
    lnZ = top + np.log(np.mean(w)) - LN_PRIOR_VOLUME
    return float(lnZ), float(np.std(w, ddof=1) / np.sqrt(n) / np.mean(w)), float(np.sum(w) ** 2 / np.sum(w ** 2))


# the end-to-end case of tests/test_gpu_adaptive.py
E2E = dict(ntemps=12, walkers=24, burn=300, steps=400, lag=1000., time=10.)


def e2e_restated(seed, adapt=True):
    """The end-to-end case on the restatement: ``(lnZ stepping stones, its dlnZ, lnZ thermodynamic, ladder)``."""
    from lightcurve_fitting_amd.sampler import default_betas, thermodynamic_integration
    c = E2E
    pb = R.problem(False)
    betas = default_betas(5, c['ntemps'], np.inf)
    burn = run(pb, R.start(pb, c['ntemps'], c['walkers'], seed), betas, c['burn'], seed, c['lag'], c['time'], adapt=adapt)
    kept = run(pb, None, burn['betas'], c['steps'], seed, adapt=False, first_step=c['burn'], state=burn['state'])
    lnZ, dlnZ = stepping_stone(kept['lnL'], burn['betas'])
    ti = thermodynamic_integration(burn['betas'], kept['lnL'].mean(axis=(0, 2)))
    return lnZ, dlnZ, ti.lnZ, burn['betas']


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'restate':
        for seed in map(int, sys.argv[2:]):
            for adapt in ((True, False) if seed == 3 else (True,)):   # (the fixed ladder: the test's own seed only)
                lnZ, dlnZ, ti, ladder = e2e_restated(seed, adapt)
                print(f'seed {seed} adapt {adapt}: stepping stones {lnZ:.3f} +- {dlnZ:.3f}, thermodynamic {ti:.1f}',
                      flush=True)
    else:
        lnZ, err, ess = importance_log_evidence()
        print(f'lnZ = {lnZ:.3f} +- {err:.3f} (effective sample size {ess:.0f})')
