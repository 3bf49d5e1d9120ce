"""NumPy restatement of the moves of the parallel-tempered driver (a helper, not a test): the definition
``lcf_tempered_set_moves`` / ``k_t_propose_moves`` are held to, over the oracle's ``philox4x32``, ``u01`` and
``split_permutation``, with the swap step and the start of ``tempered_reference`` and the ladder rule of
``adaptive_reference``.

A step of rung ``k`` makes ONE kind of move in both half-steps: the first entry ``m`` of the mixture with
``um < cum[m]``, ``um = u01`` of words 0, 1 of ``philox(0, s, 4, 0)`` under the rung's key.  The colouring, the active
walker of every slot and ``ln u`` are the stretch move's (``split_permutation``, ``stretch_draws``).  The new numbers of
walker ``wid`` are ``P2 = philox(wid, s, half, 2)`` and ``P3 = philox(wid, s, half, 3)`` under the rung's key:
``ua = u01(P2[0], P2[1])``, ``ub = u01(P2[2], P2[3])``, ``uc = u01(P3[0], P3[1])``, ``ud = u01(P3[2], P3[3])``.
``c[0 .. n)`` is the complementary colour in permutation order.

* stretch: as ``tempered_reference.run``.
* DE: ``j1 = min(int(ua n), n - 1)``, ``j2 = min(int(ub (n - 1)), n - 2)``, ``j2 += (j2 >= j1)``;
  ``g = sqrt(-2 ln uc) cos(2 pi ud)``; ``q = x + gamma0 (1 + sigma g) (c[j1] - c[j2])``; log proposal factor 0.
* snooker: ``j0, j1`` as DE's pair; ``j2 = min(int(uc (n - 2)), n - 3)`` bumped past the smaller, then the larger of
  them; ``z = c[j0]``, ``d = x - z``, ``u = d / |d|``, ``q = x + u gammas (u.c[j1] - u.c[j2])``; log proposal factor
  ``(ndim - 1) (ln |q - z| - ln |d|)``; ``|d| = 0`` or ``|q - z| = 0``: the proposal is ``x`` with log-prior ``-inf``.

The accept test is ``factor + beta (ln L(q) - ln L(x)) + (ln pr(q) - ln pr(x)) > ln u``."""
import numpy as np

import adaptive_reference as A
import tempered_reference as R
from oracle import lcf_oracle as O

STRETCH, DE, SNOOKER = 0, 1, 2


def stretch(weight=1.):
    return (STRETCH, weight, 0., 0.)


def de(weight=1., sigma=1e-5, gamma0=None):
    """``gamma0=None``: ``2.38 / sqrt(2 ndim)``."""
    return (DE, weight, sigma, gamma0)


def snooker(weight=1., gammas=1.7):
    return (SNOOKER, weight, gammas, 0.)


def _key(seed):
    return (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def cumulative(moves):
    """The cumulative weights as the host hands them to the device: normalised, ``np.cumsum``, the last exactly 1."""
    w = np.array([m[1] for m in moves], dtype=np.float64)
    cum = np.cumsum(w / w.sum())
    cum[-1] = 1.
    return cum


def mixture_index(rseed, step, cum):
    """The entry of the mixture a rung (of seed ``rseed``) makes at ``step`` (scalars or arrays)."""
    s = np.asarray(step, dtype=np.uint64)
    r0, r1, _, _ = O.philox4x32((np.zeros_like(s), s, np.full_like(s, 4), np.zeros_like(s)), _key(rseed))
    return np.searchsorted(cum, O.u01(r0, r1), side='right')     # the first m with um < cum[m]


def uniforms(rseed, step, half, walker_ids):
    """``ua, ub, uc, ud`` of the listed active walkers in one half-step."""
    wid = np.asarray(walker_ids, dtype=np.uint64)
    s, h = np.full_like(wid, step), np.full_like(wid, half)
    a0, a1, a2, a3 = O.philox4x32((wid, s, h, np.full_like(wid, 2)), _key(rseed))
    b0, b1, b2, b3 = O.philox4x32((wid, s, h, np.full_like(wid, 3)), _key(rseed))
    return O.u01(a0, a1), O.u01(a2, a3), O.u01(b0, b1), O.u01(b2, b3)


def _pick(u, n):
    return np.minimum((u * n).astype(np.int64), n - 1)


def de_partners(ua, ub, n):
    """Two distinct indices into a complement of ``n``, every ordered pair equally likely."""
    j1 = _pick(ua, n)
    j2 = _pick(ub, n - 1)
    return j1, j2 + (j2 >= j1)


def snooker_partners(ua, ub, uc, n):
    """Three distinct indices into a complement of ``n``, every ordered triple equally likely."""
    j0, j1 = de_partners(ua, ub, n)
    j2 = _pick(uc, n - 2)
    j2 = j2 + (j2 >= np.minimum(j0, j1))
    return j0, j1, j2 + (j2 >= np.maximum(j0, j1))


def propose(move, x, act, oth, rseed, step, half, a=2., snooker_exponent=None, dtype=np.float64):
    """The proposals of one rung's half-step: ``x`` (W, D) its walkers, ``act`` / ``oth`` the active colour and its
    complement in permutation order.  Returns ``q`` (n, D) float64, the log proposal factors, ``ln u`` and ``dead``
    (proposals that are never accepted).  ``dtype``: the arithmetic of the DE and snooker proposals."""
    kind, _, p0, p1 = move
    D, n = x.shape[1], len(oth)
    z, j, ln_u = O.stretch_draws(rseed, step, half, act, n, a)
    if kind == STRETCH:
        partner = x[oth[j]]
        return partner - (partner - x[act]) * z[:, None], (D - 1.) * np.log(z), ln_u, np.zeros(len(act), dtype=bool)
    ua, ub, uc, ud = uniforms(rseed, step, half, act)
    xa, c = x[act].astype(dtype), x[oth].astype(dtype)
    if kind == DE:
        assert n >= 2
        j1, j2 = de_partners(ua, ub, n)
        g = np.sqrt(-2. * np.log(uc)) * np.cos(2. * np.pi * ud)
        gamma0 = 2.38 / np.sqrt(2. * D) if p1 is None else p1
        scale = gamma0 * (1. + p0 * g)
        q = xa + scale[:, None] * (c[j1] - c[j2])
        return q.astype(np.float64), np.zeros(len(act)), ln_u, np.zeros(len(act), dtype=bool)
    assert kind == SNOOKER and n >= 3
    exponent = D - 1. if snooker_exponent is None else snooker_exponent
    j0, j1, j2 = snooker_partners(ua, ub, uc, n)
    zc = c[j0]
    d = xa - zc
    norm = np.sqrt(np.sum(d * d, axis=1))
    with np.errstate(invalid='ignore', divide='ignore'):
        u = d / norm[:, None]
        proj = np.sum(u * c[j1], axis=1) - np.sum(u * c[j2], axis=1)
        q = (xa + u * p0 * proj[:, None]).astype(np.float64)
        t = q.astype(dtype) - zc
        qn = np.sqrt(np.sum(t * t, axis=1))
        dead = ~(norm > 0.) | ~(qn > 0.)
        factor = (exponent * (np.log(qn) - np.log(norm))).astype(np.float64)
    q[dead] = x[act][dead]
    factor[dead] = 0.
    return q, factor, ln_u, dead


def run(pb, x0, betas, nsteps, seed, moves=None, a=2., first_step=0, log_like=None, log_prior=None,
        snooker_exponent=None, adapt=None, dtype=np.float64):
    """``nsteps`` steps from ``x0`` (K, W, D) in the shape of ``tempered_reference.run``.  ``moves``: a list of
    :func:`stretch`, :func:`de`, :func:`snooker` entries (None: the stretch move alone).  ``log_like`` / ``log_prior``:
    (n, D) -> (n,) (default: ``tempered_reference``'s over ``pb``).  ``adapt``: ``dict(lag, time, t0=0)`` for a ladder
    that adapts by ``adaptive_reference.adapt_ladder``.  Returns the dict of ``tempered_reference.run`` plus ``kinds``
    (n, K) (the kind of move per step and rung), ``betas`` and ``beta_history`` (n, K)."""
    if log_like is None:
        log_like = lambda block: R.log_like(pb, block)
    if log_prior is None:
        log_prior = lambda block: R.log_prior(pb, block)
    moves = [stretch()] if moves is None else list(moves)
    cum = cumulative(moves)
    betas = np.array(betas, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    K, W, D = x.shape
    if adapt is not None and (K < 3 or betas[-1] != 0.):
        raise ValueError('an adaptive ladder needs at least 3 rungs and a last rung at beta = 0')
    ll = np.asarray(log_like(x.reshape(-1, D)), dtype=np.float64).reshape(K, W)
    lpr = np.asarray(log_prior(x.reshape(-1, D)), dtype=np.float64).reshape(K, W)
    assert np.all(np.isfinite(lpr)) and not np.any(np.isnan(ll))
    chain, lls, hist = np.empty((nsteps, K, W, D)), np.empty((nsteps, K, W)), np.empty((nsteps, K))
    kinds = np.empty((nsteps, K), dtype=np.int64)
    nacc = np.zeros((K, W), dtype=np.int64)
    sw_acc, sw_prop = np.zeros(K - 1, dtype=np.int64), np.zeros(K - 1, dtype=np.int64)
    window = A.Window(K - 1)
    move_margin, swap_margin, nan_proposals = np.inf, np.inf, 0
    half_n = (W + 1) // 2
    for it in range(nsteps):
        s = first_step + it
        rseeds = [R.rung_seed(seed, k) for k in range(K)]
        perms = [O.split_permutation(rseeds[k], s, W) for k in range(K)]
        step_moves = [moves[mixture_index(rseeds[k], s, cum)] for k in range(K)]   # ONE kind for both halves
        kinds[it] = [m[0] for m in step_moves]
        for half in (0, 1):
            act, q, fac, ln_u, dead = [], [], [], [], []
            for k in range(K):
                sets = (perms[k][:half_n], perms[k][half_n:])
                ak, oth = sets[half], sets[1 - half]
                qk, fk, lu, dk = propose(step_moves[k], x[k], ak, oth, rseeds[k], s, half, a, snooker_exponent, dtype)
                act.append(ak)
                q.append(qk)
                fac.append(fk)
                ln_u.append(lu)
                dead.append(dk)
            with np.errstate(all='ignore'):
                q_ll = np.asarray(log_like(np.concatenate(q)), dtype=np.float64)   # ONE evaluation for all rungs
            q_lpr = np.array(log_prior(np.concatenate(q)), dtype=np.float64)
            q_lpr[np.concatenate(dead)] = -np.inf
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
                    stat = fac[k] + dl + (pq - lpr[k, ak])
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
        if adapt is not None:
            window.acc += acc
            window.prop += prop
            if (s & 1) and np.all(window.prop > 0):
                betas = A.adapt_ladder(betas, window.acc / window.prop, adapt.get('t0', 0) + it + 1, adapt['lag'],
                                       adapt['time'])
                window.clear()
    return dict(chain=chain, lnL=lls, nacc=nacc, swaps_accepted=sw_acc, swaps_proposed=sw_prop,
                move_margin=move_margin, swap_margin=swap_margin, nan_proposals=nan_proposals, kinds=kinds, betas=betas,
                beta_history=hist)


_runs = {}


def cached_run(use_sigma, nwalkers, betas, nsteps, seed, moves, adapt=None):
    """``(pb, x0, run(...))`` of a case on ``small_problem()``, computed once per process and shared (callers leave it
    unchanged).  ``adapt``: ``(lag, time)`` or None."""
    key = (bool(use_sigma), int(nwalkers), tuple(betas), int(nsteps), int(seed), tuple(moves), adapt)
    if key not in _runs:
        pb = R.problem(use_sigma)
        x0 = R.start(pb, len(betas), nwalkers, seed)
        _runs[key] = (pb, x0, run(pb, x0, betas, nsteps, seed, moves,
                                  adapt=None if adapt is None else dict(lag=adapt[0], time=adapt[1])))
    return _runs[key]
