"""NumPy restatement of the parallel-tempered ensemble (a helper, not a test): the definition the device driver
``lcf_tempered_*`` is held to, over the oracle's generators and likelihood and ``helpers.small_problem()``.

Rungs ``k`` of inverse temperature ``betas[k]`` (1 first, descending, ``>= 0``), each an ensemble of ``W`` walkers with
``x``, ``lnL(x)`` and ``lnpr(x)`` per walker.  Rung ``k`` draws its colouring (``split_permutation``) and its moves
(``stretch_draws``) under ``seed + k * 0x9E3779B97F4A7C15 (mod 2^64)``.  Step ``s``: two half-steps of stretch moves
on ``prior * L**beta``, then the pairs ``(k, k + 1)`` with ``k = s (mod 2)`` swap slot by slot."""
import numpy as np

from helpers import small_problem
from oracle import lcf_oracle as O

GOLDEN_GAMMA = 0x9E3779B97F4A7C15
BOX_LO = np.array([1., .3, 2., 1.5, 0.])
BOX_HI = np.array([1.5, .7, 4., 2.5, .2])
SIGMA_PRIOR = (0, 0., 5., 0., 1.)       # the sigma parameter of the use_sigma problem: uniform on (0, 5) ...
SIGMA_BOX = (0.1, 1.)                   # ... started in this interval

_problems = {}


def problem(use_sigma=False):
    """``small_problem()`` (built once), with a fitted relative sigma as a sixth parameter if asked."""
    if use_sigma not in _problems:
        pb = dict(small_problem())
        if use_sigma:
            pb.update(use_sigma=True, sigma_type='relative', priors=list(pb['priors']) + [SIGMA_PRIOR])
        _problems[use_sigma] = pb
    return _problems[use_sigma]


def start(pb, ntemps, nwalkers, seed):
    """(K, W, D) uniform in the box, from ``default_rng(seed)``."""
    lo, hi = BOX_LO, BOX_HI
    if pb.get('use_sigma'):
        lo, hi = np.append(lo, SIGMA_BOX[0]), np.append(hi, SIGMA_BOX[1])
    return lo + (hi - lo) * np.random.default_rng(seed).random((ntemps, nwalkers, len(lo)))


def rung_seed(seed, k):
    return (seed + k * GOLDEN_GAMMA) & (2 ** 64 - 1)


def log_like(pb, block):
    """(n, D) -> (n,) log-likelihoods (no prior), whatever the prior says about the rows."""
    block = np.atleast_2d(block)
    args = (('ShockCooling', pb['orc']), pb['t'], pb['bands'], pb['y'], pb['dy'])
    kw = dict(use_sigma=pb.get('use_sigma', False), sigma_type=pb.get('sigma_type', 'relative'))
    if len(block) == 1:  # (a single column would be squeezed away inside the oracle)
        return np.array([O.log_likelihood(*args, block[0], **kw)])
    return np.asarray(O.log_likelihood(*args, block.T, **kw), dtype=np.float64)


def log_prior(pb, block):
    return np.array([O.log_prior(pb['priors'], p) for p in np.atleast_2d(block)])


def swap_step(x, ll, lpr, betas, seed, s):
    """The swaps after step ``s``, in place.  Returns ``(accepted, proposed)`` per pair (K - 1,) and the smallest
    ``|statistic - ln u|`` of the tests made (inf: none)."""
    K, W = ll.shape
    acc, prop = np.zeros(K - 1, dtype=np.int64), np.zeros(K - 1, dtype=np.int64)
    margin = np.inf
    i = np.arange(W, dtype=np.uint64)
    for k in range(s & 1, K - 1, 2):
        r0, r1, _, _ = O.philox4x32((i, np.full_like(i, s), np.full_like(i, 3), np.full_like(i, k)),
                                    (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        ln_u = np.log(O.u01(r0, r1))
        with np.errstate(invalid='ignore'):
            stat = (betas[k] - betas[k + 1]) * (ll[k + 1] - ll[k])
            ok = stat > ln_u
        margin = min(margin, float(np.min(np.abs(stat - ln_u))))
        for a in (x, ll, lpr):
            a[k, ok], a[k + 1, ok] = a[k + 1, ok].copy(), a[k, ok].copy()
        acc[k] += ok.sum()
        prop[k] += W
    return acc, prop, margin


def run(pb, x0, betas, nsteps, seed, a=2., first_step=0):
    """``nsteps`` steps from ``x0`` (K, W, D).  Returns a dict: ``chain`` (n, K, W, D), ``lnL`` (n, K, W), ``nacc``
    (K, W) accepted moves by slot, ``swaps_accepted`` / ``swaps_proposed`` (K - 1,), ``move_margin`` / ``swap_margin``
    (the smallest ``|statistic - ln u|`` over all move tests that reached the comparison / over all swap tests) and
    ``nan_proposals`` (NaN likelihoods of proposals the prior excluded; one inside the prior raises)."""
    betas = np.asarray(betas, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    K, W, D = x.shape
    ll = log_like(pb, x.reshape(-1, D)).reshape(K, W)
    lpr = log_prior(pb, x.reshape(-1, D)).reshape(K, W)
    assert np.all(np.isfinite(lpr)) and not np.any(np.isnan(ll))
    chain, lls = np.empty((nsteps, K, W, D)), np.empty((nsteps, K, W))
    nacc = np.zeros((K, W), dtype=np.int64)
    sw_acc, sw_prop = np.zeros(K - 1, dtype=np.int64), np.zeros(K - 1, dtype=np.int64)
    move_margin, swap_margin, nan_proposals = np.inf, np.inf, 0
    half_n = (W + 1) // 2
    for it in range(nsteps):
        s = first_step + it
        perms = [O.split_permutation(rung_seed(seed, k), s, W) for k in range(K)]
        for half in (0, 1):
            act, q, zl, ln_u = [], [], [], []
            for k in range(K):
                sets = (perms[k][:half_n], perms[k][half_n:])
                ak, oth = sets[half], sets[1 - half]
                z, j, lu = O.stretch_draws(rung_seed(seed, k), s, half, ak, len(oth), a)
                partner = x[k, oth[j]]
                act.append(ak)
                q.append(partner - (partner - x[k, ak]) * z[:, None])
                zl.append((D - 1.) * np.log(z))
                ln_u.append(lu)
            with np.errstate(all='ignore'):
                q_ll = log_like(pb, np.concatenate(q))          # ONE evaluation for all rungs
            q_lpr = log_prior(pb, np.concatenate(q))
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
        acc, prop, margin = swap_step(x, ll, lpr, betas, seed, s)
        sw_acc += acc
        sw_prop += prop
        swap_margin = min(swap_margin, margin)
        chain[it], lls[it] = x, ll
    return dict(chain=chain, lnL=lls, nacc=nacc, swaps_accepted=sw_acc, swaps_proposed=sw_prop,
                move_margin=move_margin, swap_margin=swap_margin, nan_proposals=nan_proposals)


_runs = {}


def cached_run(use_sigma, nwalkers, betas, nsteps, seed):
    """``(pb, x0, run(...))`` of a test case, computed once per process and shared (callers leave it unchanged)."""
    key = (bool(use_sigma), int(nwalkers), tuple(betas), int(nsteps), int(seed))
    if key not in _runs:
        pb = problem(use_sigma)
        x0 = start(pb, len(betas), nwalkers, seed)
        _runs[key] = (pb, x0, run(pb, x0, betas, nsteps, seed))
    return _runs[key]
