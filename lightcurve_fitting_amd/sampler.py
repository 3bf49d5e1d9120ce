"""Ensemble sampler driver with the surface of ``emcee.EnsembleSampler`` that ``lightcurve_mcmc`` and its
consumers use (reference fitting.py:130-148, 171-277): ``run_mcmc``, ``reset``, ``chain``, ``flatchain``,
``lnprobability``/``get_log_prob``, ``acceptance_fraction``.

The stretch move itself (Goodman & Weare 2010, red/blue halves, a = 2) runs on the GPU
(``lcf_sampler_*`` in ``include/lcf.h``):

* single GPU: the whole run is enqueued by one native call, no host round-trip per step;
* several GPUs (``torch.distributed`` initialised, one process per GPU): every rank holds the full ensemble,
  proposals and accept/reject are replicated from the same counter-based RNG, each rank evaluates the likelihood of
  its contiguous shard of the active half, and ONE all-gather of ``n_walkers/2`` float64 log-probabilities per
  half-step (RCCL over xGMI; latency-bound, <= 16 KiB) makes the ranks agree.  Chains are therefore identical for
  any number of GPUs.

The per-half-step protocol is factored into :class:`ShardedStretchDriver` over a small backend interface so that
the multi-rank logic can be exercised on CPU with ``gloo`` (tests inject a checker backend there).
"""
import numpy as np

from . import rng as _rng


class State(tuple):
    """``(coords, log_prob, random_state)`` -- unpacks like emcee's ``State`` (fitting.py:133)."""

    def __new__(cls, coords, log_prob, random_state=None):
        return super().__new__(cls, (coords, log_prob, random_state))

    coords = property(lambda self: self[0])
    log_prob = property(lambda self: self[1])
    random_state = property(lambda self: self[2])


def shard_bounds(n_items, world_size, rank):
    """Contiguous, balanced partition of ``range(n_items)``: returns ``(lo, hi, width)`` with ``width`` the padded
    per-rank slot size used by the all-gather."""
    width = -(-n_items // world_size)
    lo = min(rank * width, n_items)
    hi = min(lo + width, n_items)
    return lo, hi, width


class NativeBackend:
    """Backend over ``lcf_sampler``: device buffers live in the native library; the collective sees them as torch
    tensors through ``__cuda_array_interface__`` (no copy)."""

    def __init__(self, native_sampler, rows=False):
        self.ns = native_sampler
        self.n_half = (native_sampler.nwalkers + 1) // 2   # slots per half-step (an odd ensemble's larger colour)
        #: what the collective carries per proposal: its row of partial chi^2 sums + log-prior (no finalize launch;
        #: the protocol of the native ``lcf_sampler_run_sharded``), or its finished log-posterior
        self.rows = bool(rows)
        self._newlp = {}
        self._side = None

    def begin(self, first_step, nsteps, split, store):
        self.ns.begin(first_step, nsteps, split, store)

    def stream(self):
        """Raw handle of torch's current stream.  The native ABI reads handle 0 as "the engine's own stream", which
        is NOT ordered with torch's default stream: callers run under :meth:`stream_context` (a real side stream)."""
        import torch
        return torch.cuda.current_stream().cuda_stream

    def stream_context(self):
        """Context under which kernels enqueued through the ABI and torch collectives share one (non-default) stream."""
        import torch
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.ns.engine.device)
        self._side.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self._side)

    def stream_sync(self):
        if self._side is not None:
            self._side.synchronize()

    def propose(self, step, half):
        self.ns.propose(step, half, self.stream())

    def evaluate(self, lo, hi):
        self.ns.evaluate(lo, hi, self.stream())

    def half_step(self, step, half, lo, hi):
        if self.rows:
            self.ns.half_step_rows(step, half, lo, hi, self.stream())
        else:
            self.ns.half_step(step, half, lo, hi, self.stream())

    def accept(self, step, half):
        self.ns.accept(step, half, self.stream())

    def newlp(self):
        """float64 torch tensor aliasing the native buffer the collective works on, for the half-step drawn last:
        ``rows[n_half][row]`` or ``newlp[n_half]`` (first axis = proposal slot either way; the native side
        double-buffers it, so there are two aliases)."""
        if self.rows:
            ptr, row = self.ns.rows_ptr()
            shape = (self.n_half, row)
        else:
            ptr, shape = self.ns.newlp_ptr(), (self.n_half,)
        if ptr not in self._newlp:
            import torch

            class _Alias:
                __cuda_array_interface__ = {'shape': shape, 'typestr': '<f8', 'data': (ptr, False), 'version': 2,
                                            'strides': None}
            self._newlp[ptr] = torch.as_tensor(_Alias(), device=f'cuda:{self.ns.engine.device}')
        return self._newlp[ptr]

    def empty(self, n):
        """Staging buffer for ``n`` proposal slots, shaped like :meth:`newlp`."""
        import torch
        shape = (n, self.ns.rows_ptr()[1]) if self.rows else (n,)
        return torch.empty(shape, dtype=torch.float64, device=f'cuda:{self.ns.engine.device}')

    def finish(self):
        self.ns.check()


class ShardedStretchDriver:
    """Runs half-steps over a backend, sharding the likelihood evaluation over the ranks of a process group."""

    def __init__(self, backend, group=None, force_collective=False):
        import torch.distributed as dist
        self.backend = backend
        self.dist = dist
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.lo, self.hi, self.width = shard_bounds(backend.n_half, self.world, self.rank)
        self.collective = self.world > 1 or force_collective
        # equal shards: the all-gather runs IN PLACE on the native newlp buffer (rank r's input is the slice
        # [r*width, (r+1)*width) of the output) -- no staging copies, one collective per half-step
        self.in_place = backend.n_half == self.width * self.world
        if self.collective and not self.in_place:
            self._send = backend.empty(self.width)
            self._recv = backend.empty(self.width * self.world)

    def run(self, first_step, nsteps, split, store):
        """``split``: 'random' | 'identity' | int32 array (nsteps, nwalkers), see ``NativeSampler._split``."""
        b = self.backend
        b.begin(first_step, nsteps, split, store)
        if hasattr(b, 'stream_context'):
            with b.stream_context():
                self._loop(first_step, nsteps)
            b.stream_sync()
        else:
            self._loop(first_step, nsteps)
        b.finish()

    def _loop(self, first_step, nsteps):
        b = self.backend
        for k in range(nsteps):
            step = first_step + k
            for half in (0, 1):
                if hasattr(b, 'half_step'):
                    b.half_step(step, half, self.lo, self.hi)
                else:
                    b.propose(step, half)
                    b.evaluate(self.lo, self.hi)
                if self.collective and self.in_place:
                    newlp = b.newlp()
                    self.dist.all_gather_into_tensor(newlp, newlp[self.lo:self.hi], group=self.group)
                elif self.collective:
                    newlp = b.newlp()
                    n = self.hi - self.lo
                    if n:
                        self._send[:n].copy_(newlp[self.lo:self.hi])
                    self.dist.all_gather_into_tensor(self._recv, self._send, group=self.group)
                    for r in range(self.world):  # unpad: rank r owns [r*width, min((r+1)*width, n_half))
                        lo, hi, _ = shard_bounds(b.n_half, self.world, r)
                        if hi > lo and r != self.rank:
                            newlp[lo:hi].copy_(self._recv[r * self.width:r * self.width + (hi - lo)])
                b.accept(step, half)


def partition(n_items, world_size, rank):
    """Indices of the items (transients, epochs) owned by ``rank``: contiguous, balanced blocks."""
    lo, hi, _ = shard_bounds(n_items, world_size, rank)
    return range(lo, hi)


class PopulationSampler:
    """Population mode (BASELINE configs[4]): many independent transients, each with its own light curve, engine and
    walker ensemble.  Embarrassingly parallel: transients are partitioned over the ranks of a process group (no
    communication) and, on each GPU, all of a rank's ensembles are enqueued on their own HIP streams before any is
    waited for, so that small per-transient kernels overlap on the device.

    ``problems``: sequence of ``(model, lc, priors)``; every rank passes the full list and keeps
    ``self.indices`` (its share).  ``seed + index`` keys each transient's RNG, so results do not depend on the
    number of GPUs."""

    def __init__(self, problems, nwalkers, seed=0, a=2.0, group=None, device=None):
        world, rank = 1, 0
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                world, rank = dist.get_world_size(group), dist.get_rank(group)
        except ImportError:
            pass
        self.indices = list(partition(len(problems), world, rank))
        self.samplers = {}
        for k in self.indices:
            model, lc, priors, *extra = problems[k]  # optional 4th entry: engine keywords (use_sigma, sigma_type)
            if device is not None:
                model.device = device
            eng = model.engine_for(lc, priors=priors, **(extra[0] if extra else {}))
            self.samplers[k] = EnsembleSampler(nwalkers, eng.ndim, eng, seed=seed + k, a=a)
        self.nwalkers = nwalkers

    def run_mcmc(self, initial_states, nsteps, store=True, batched=True):
        """``initial_states``: mapping/sequence index -> (nwalkers, ndim) coordinates, or None to continue.

        ``batched`` (default): one native call runs all transients in lock step, every launch covering the whole
        population: resident workgroups for blocks of half-steps where the transients and the device allow them, else
        one launch per half-step, else one proposal launch and one likelihood launch per half-step; if the transients
        cannot share launches (mixed table placement etc.) or ``batched`` is false, every ensemble is enqueued on its
        own stream instead."""
        from .engine import LcfError, population_run
        samplers = list(self.samplers.values())
        for k, s in self.samplers.items():
            s._prepare(None if initial_states is None else initial_states[k])
        done = False
        if batched and samplers and len({s._steps_done for s in samplers}) == 1 and \
                len({s.randomize_split for s in samplers}) == 1:
            try:
                self.last_run_ms = population_run([s._native for s in samplers], samplers[0]._steps_done, nsteps,
                                                  'random' if samplers[0].randomize_split else 'identity', store)
                done = True
            except LcfError as exc:
                if exc.status == 6:
                    raise ValueError('Probability function returned NaN') from None
                if exc.status != 5:  # LCF_ERR_UNSUPPORTED -> per-transient streams
                    raise
        for s in samplers:
            if not done:
                s._launch(nsteps, store, asynchronous=True)
        for s in samplers:
            s._finish(nsteps, store)
        return {k: s._state for k, s in self.samplers.items()}

    def get_autocorr_time(self, discard=0, thin=1, c=5, tol=50, quiet=False, has_walkers=True):
        """``{index: tau}`` of this rank's transients, each as ``EnsembleSampler.get_autocorr_time`` gives it; the
        chains still on the device go through one native call together.  If any transient fails the ``tol`` test,
        ``quiet=False`` raises one :class:`~lightcurve_fitting_amd.autocorr.AutocorrError` whose ``.tau`` is the
        whole dict (``quiet=True`` logs one warning per such transient)."""
        from .autocorr import AutocorrError, convergence_message, logger
        from .engine import samplers_autocorr_time
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1:
            raise ValueError('need discard >= 0 and thin >= 1')
        resident = [k for k, s in self.samplers.items() if len(s._chain_host) == 0 and s._chain_on_device > 0]
        est = {}
        for k, s in self.samplers.items():
            if k not in resident:
                est[k] = s._autocorr(discard, thin, c)
            elif len(range(discard, s.iteration, thin)) == 0:
                raise ValueError(f'discard={discard} leaves no steps of the {s.iteration} stored (transient {k})')
        if resident:
            got = samplers_autocorr_time([self.samplers[k]._native for k in resident], discard, thin, c)
            for k, (tau, window) in zip(resident, got):
                est[k] = (tau, window, len(range(discard, self.samplers[k].iteration, thin)))
        taus, raw, msgs = {}, {}, []
        for k in self.samplers:
            tau, _, n_t = est[k]
            raw[k] = tau
            msg = convergence_message(tau, n_t, tol)
            if msg is not None:
                if quiet:
                    logger.warning(msg)
                msgs.append(f'transient {k}: {msg}')
            taus[k] = thin * tau
        if msgs and not quiet:
            raise AutocorrError(raw, '\n'.join(msgs))
        return taus

    def corner(self, models=None, bins=20, range=None, levels=None, t0_offset=None, discard=0, thin=1, use_sigma=None):
        """``{index: CornerData}`` of this rank's transients, each as :func:`~lightcurve_fitting_amd.fitting.
        posterior_corner` gives it; the chains still on the device go through one native call per pass together.
        ``models``: index -> the transient's model (mapping or sequence), or None (columns ``p0, p1, ...``).  ``range``,
        ``t0_offset`` and ``use_sigma`` hold for every transient, or are dicts index -> value; ``use_sigma=None``: a
        chain with one column more than its model has parameters carries sigma."""
        from .engine import chain_hist, chain_range
        from .fitting import _CornerPlan, posterior_corner
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1:
            raise ValueError('need discard >= 0 and thin >= 1')

        def pick(value, k):
            return value.get(k) if isinstance(value, dict) else value
        plans, n_samples = {}, {}
        for k, s in self.samplers.items():
            model = None if models is None else models[k]
            sigma = pick(use_sigma, k)
            if sigma is None:
                sigma = model is not None and s.ndim == model.n_model_params + 1
            plans[k] = (model, sigma, _CornerPlan(model, s.ndim, bins, pick(range, k), levels, pick(t0_offset, k), sigma))
            if s.iteration == 0:
                raise ValueError(f'no chain is stored (transient {k}): run the sampler with store=True first')
            if discard >= s.iteration:
                raise ValueError(f'discard={discard} leaves no steps of the {s.iteration} stored (transient {k})')
            n_samples[k] = (s.iteration - discard + thin - 1) // thin * s.nwalkers
        resident = [k for k, s in self.samplers.items() if len(s._chain_host) == 0 and s._chain_on_device > 0]
        out = {}
        for k, s in self.samplers.items():
            if k not in resident:
                model, sigma, _ = plans[k]
                out[k] = posterior_corner(model, s, bins=bins, range=pick(range, k), levels=levels,
                                          t0_offset=pick(t0_offset, k), discard=discard, thin=thin, use_sigma=sigma)
        if resident:
            natives = [self.samplers[k]._native for k in resident]
            extremes = chain_range(natives, discard, thin)
            settled = [plans[k][2].settle(lo, hi) for k, (lo, hi, _) in zip(resident, extremes)]
            counts = chain_hist(natives, [st[0] for st in settled], [st[2] for st in settled], discard, thin)
            for k, st, (_, _, n_nan), (hist1d, pairs) in zip(resident, settled, extremes, counts):
                out[k] = plans[k][2].data(*st, hist1d, pairs, n_samples[k], n_nan)
        return {k: out[k] for k in self.samplers}

    def history(self, models=None, percentiles=None, t_bins=None, v_bins=64, range=None, discard=0, thin=1,
                use_sigma=None):
        """``{index: ChainHistory}`` of this rank's transients, each as :func:`~lightcurve_fitting_amd.fitting.
        chain_history` gives it; the chains still on the device go through one native call per pass together.
        ``models``: index -> the transient's model (mapping or sequence), or None (columns ``p0, p1, ...``).  ``range``
        and ``use_sigma`` hold for every transient, or are dicts index -> value; ``t_bins=None``: ``min(n_keep, 512)``
        per transient, and the transients with the same number of step bins share a native call."""
        from .engine import chain_history as native_history, chain_range, chain_raster
        from .fitting import HISTORY_PERCENTILES, _HistoryPlan, chain_history
        percentiles = HISTORY_PERCENTILES if percentiles is None else percentiles

        def pick(value, k):
            return value.get(k) if isinstance(value, dict) else value
        plans = {}
        for k, s in self.samplers.items():
            if s.iteration == 0:
                raise ValueError(f'no chain is stored (transient {k}): run the sampler with store=True first')
            try:
                plans[k] = _HistoryPlan(None if models is None else models[k], s.iteration, s.nwalkers, s.ndim,
                                        percentiles, t_bins, v_bins, pick(range, k), discard, thin, pick(use_sigma, k))
            except ValueError as exc:
                raise ValueError(f'{exc} (transient {k})') from None
        resident = [k for k, s in self.samplers.items() if len(s._chain_host) == 0 and s._chain_on_device > 0]
        out = {}
        for k, s in self.samplers.items():
            if k not in resident:
                out[k] = chain_history(None if models is None else models[k], s, percentiles=percentiles, t_bins=t_bins,
                                       v_bins=v_bins, range=pick(range, k), discard=discard, thin=thin,
                                       use_sigma=pick(use_sigma, k))
        if resident:
            discard, thin = int(discard), int(thin)
            natives = [self.samplers[k]._native for k in resident]
            stats = native_history(natives, plans[resident[0]].percentiles, discard=discard, thin=thin)
            if any(plans[k].needs_extremes for k in resident):
                extremes = chain_range(natives, discard, thin)
            else:
                extremes = [(None, None, None)] * len(resident)
            settled = {k: plans[k].settle(lo, hi) for k, (lo, hi, _) in zip(resident, extremes)}
            for nb in sorted({plans[k].t_bins for k in resident}):
                group = [k for k in resident if plans[k].t_bins == nb]
                counts = chain_raster([self.samplers[k]._native for k in group], nb, [settled[k][1] for k in group],
                                      discard, thin)
                for k, c in zip(group, counts):
                    out[k] = plans[k].data(*stats[resident.index(k)], c, *settled[k])
        return {k: out[k] for k in self.samplers}

    def __getitem__(self, k):
        return self.samplers[k]


#: multi-rank drivers in the order they are probed (fastest expected first)
COLLECTIVES = ('rows', 'peers', 'allgather')
_probe_cache = {}   # (process group, world size) -> the driver the first probe in that group selected


def probe_collectives(make_sampler, dist, x0, probe_steps=20, group=None, modes=COLLECTIVES, device=None):
    """Which multi-rank driver runs an ensemble fastest on THIS node: every driver in ``modes`` gets a few untimed steps
    from ``x0`` on a sampler of its own (``make_sampler(mode)``); one that raises on any rank (its waits are bounded),
    that could not connect its peer memory, or that leaves the ranks with different replicas of the ensemble is out; of
    the rest the fastest (the slowest rank's time counts) wins.  Returns ``(sampler, report)``.

    Every rank takes the same path: success is AGREED (all-reduce of a flag) after the sampler is made, after its first
    short run and after the probe run, and a stage is skipped on every rank as soon as one rank failed the one before
    -- a rank that raised never sits in a different collective than the ranks that did not.

    ``device``: where the flags of those agreements live (``'cuda:<n>'`` of this rank's engine under RCCL; default: the
    current CUDA device under RCCL, the CPU otherwise)."""
    import time
    import torch
    dev = device if device is not None else ('cuda' if dist.get_backend(group) == 'nccl' else 'cpu')

    def agreed(ok):   # logical AND over the ranks
        flag = torch.tensor([1. if ok else 0.], dtype=torch.float64, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        return float(flag[0]) == 1.

    weights = np.cos(np.arange(x0.size, dtype=np.float64)).reshape(x0.shape)
    report, best = {}, None
    for mode in modes:
        seconds, checksum, why, s = float('inf'), 0., None, None
        try:
            s = make_sampler(mode)
        except Exception as exc:  # noqa: BLE001
            why = f'{type(exc).__name__}: {exc}'[:200]
        ok = agreed(why is None)
        if ok:
            try:
                s.run_mcmc(x0, 5, store=False)
                if (mode == 'peers' and not s._peers) or (mode == 'rows' and not s._boards):
                    why = 'the peer memory could not be connected'
            except Exception as exc:  # noqa: BLE001
                why = f'{type(exc).__name__}: {exc}'[:200]
            ok = agreed(why is None)
        if ok:
            try:
                t0 = time.perf_counter()
                state = s.run_mcmc(None, probe_steps, store=False)   # (returns after the device has finished)
                seconds = time.perf_counter() - t0
                checksum = float(np.sum(np.asarray(state[0]) * weights))
            except Exception as exc:  # noqa: BLE001
                seconds, why = float('inf'), f'{type(exc).__name__}: {exc}'[:200]
            ok = agreed(why is None)
        agg = torch.tensor([seconds if np.isfinite(seconds) else 1e30, checksum, -checksum], dtype=torch.float64, device=dev)
        dist.all_reduce(agg, op=dist.ReduceOp.MAX, group=group)
        worst, hi, lo = float(agg[0]), float(agg[1]), -float(agg[2])
        ok = ok and worst < 1e29 and hi == lo
        report[mode] = {'ok': ok, 'ms_per_step': 1e3 * worst / probe_steps if worst < 1e29 else None,
                        'replicas_agree': hi == lo, 'note': why}
        if ok and (best is None or worst < best[0]):
            best = (worst, mode, s)
    if best is None:
        raise RuntimeError(f'no multi-GPU driver completed its probe: {report}')
    report['selected'] = best[1]
    report['probe_steps'] = probe_steps
    return best[2], report


class EnsembleSampler:
    """Drop-in for the subset of ``emcee.EnsembleSampler`` the reference uses, bound to one engine.

    Parameters
    ----------
    nwalkers, ndim : int
    engine : lightcurve_fitting_amd.engine.Engine
        Device engine whose log-posterior is sampled (priors baked in at engine creation).
    seed : int
        Key of the counter-based RNG (emcee uses NumPy's global state instead; sampler parity is statistical).
    a : float
        Stretch scale (emcee default 2.0).
    randomize_split : bool
        Fresh random red/blue colouring every step, as emcee's ``RedBlueMove`` does.
    """

    def __init__(self, nwalkers, ndim, engine, seed=0, a=2.0, randomize_split=True, group=None,
                 force_sharded=False, native_collectives=True, collective=None):
        from .engine import NativeSampler
        if nwalkers < 2 * ndim:  # emcee's check; odd ensembles are fine (the red-blue split is then ceil / floor)
            raise ValueError('It is unadvisable to use a red-blue move with fewer walkers than twice the number of '
                             'dimensions.')
        if ndim != engine.ndim:
            raise ValueError(f'ndim = {ndim} but the engine has {engine.ndim} parameters')
        self.nwalkers, self.ndim = nwalkers, ndim
        self.engine = engine
        self.seed = int(seed)
        self.randomize_split = randomize_split
        self._native = NativeSampler(engine, nwalkers, seed, a)
        self._group = group
        self._force_sharded = force_sharded  # run the phase-by-phase collective path even with a single rank
        self.native_collectives = native_collectives
        #: how the ranks of a multi-GPU run work together: 'rows' (every rank moves its share of the walkers with k_solo
        #: and stores their new rows into every rank's board over IPC-mapped memory), 'peers' (every rank evaluates its
        #: share, stores partial sums into every mailbox, replicates the bookkeeping), 'allgather' (the same with one RCCL
        #: all-gather per half-step; the default -- the only driver whose wire protocol is RCCL's own), or 'auto'
        #: (``collective='auto'`` / LCF_COLLECTIVE=auto): the first run of the first sampler of a process group probes
        #: all of them for a few steps (probe_collectives) and the group keeps the fastest that works.  The peer-memory
        #: drivers stay opt-in until an 8-GPU run has timed them (bench.py --gpus N probes by default and says what it saw).
        import os
        self.collective = collective or os.environ.get('LCF_COLLECTIVE', 'allgather')
        if self.collective not in COLLECTIVES + ('auto',):
            raise ValueError("collective must be 'auto', 'allgather', 'peers' or 'rows'")
        self.collective_probe = None   # the report of the probe this sampler ran (None: named, cached or single rank)
        self._boards = None
        self._peers = None  # True once the mailboxes are connected, False if unavailable
        self._comm = None  # NativeComm once created, False if unavailable
        self._steps_done = 0   # RNG step counter: never reset, so burn-in and sampling use disjoint streams
        self._chain_host = np.empty((0, nwalkers, ndim))
        self._lp_host = np.empty((0, nwalkers))
        self._chain_on_device = 0   # steps of the last stored run whose chain is still in HBM only
        self._naccepted = np.zeros(nwalkers, dtype=np.int64)
        self._acc_seen = None   # the native acceptance counts as of the last finished run
        self._nsteps_counted = 0
        self._state = None

    def _native_comm(self):
        """RCCL communicator for the native sharded loop, or None (then the Python-driven loop over
        torch.distributed collectives is used): needs equal shards and a loadable RCCL.  Every rank takes the same
        decision: the outcome of the (collective) creation is agreed with an all-reduce."""
        if self._comm is False:
            return None
        if self._comm is None:
            import torch
            import torch.distributed as dist
            from .engine import NativeComm
            world = dist.get_world_size(self._group)
            dev = f'cuda:{self.engine.device}' if dist.get_backend(self._group) == 'nccl' else 'cpu'

            def agreed(ok):  # logical AND over the ranks
                flag = torch.tensor([1 if ok else 0], device=dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self._group)
                return int(flag.item()) == 1

            # 1. everything that can fail locally (options, shard shape, binding RCCL) BEFORE any collective RCCL call,
            #    so that no rank is left waiting in ncclCommInitRank for one that bailed out
            comm = None
            if agreed(self.native_collectives and ((self.nwalkers + 1) // 2) % world == 0 and NativeComm.probe()):
                try:
                    comm = NativeComm(self.engine.device, self._group)
                except Exception:  # noqa: BLE001 - then every rank falls back to the torch.distributed path
                    comm = None
                if not agreed(comm is not None):
                    if comm is not None:
                        comm.close()
                    comm = None
            self._comm = comm if comm is not None else False
        return self._comm or None

    def _peer_mailboxes(self):
        """Connect the ranks' mailboxes (once): every rank exports an IPC handle, the handles travel over
        torch.distributed, every rank maps them all.  All ranks take the same decision (all-reduce of the outcome)."""
        if self._peers is None:
            import torch
            import torch.distributed as dist
            world, rank = dist.get_world_size(self._group), dist.get_rank(self._group)
            dev = f'cuda:{self.engine.device}' if dist.get_backend(self._group) == 'nccl' else 'cpu'

            def agreed(ok):
                flag = torch.tensor([1 if ok else 0], device=dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self._group)
                return int(flag.item()) == 1

            handle = None
            try:
                if world <= 8 and ((self.nwalkers + 1) // 2) % world == 0 and self._native.one_launch:
                    handle, _ = self._native.mailbox_export()
            except Exception:  # noqa: BLE001 - then every rank falls back to the all-gather
                handle = None
            ok = agreed(handle is not None)
            if ok:
                handles = [None] * world
                dist.all_gather_object(handles, handle, group=self._group)
                try:
                    self._native.mailbox_connect(world, rank, handles=handles)
                except Exception:  # noqa: BLE001
                    ok = False
                ok = agreed(ok)
            self._peers = ok
        return self._peers

    def _peer_boards(self):
        """Connect the ranks' row boards (once), as :meth:`_peer_mailboxes` connects the mailboxes: for the sharded run
        in which every rank moves its share of the walkers itself (``lcf_sampler_run_rows``)."""
        if self._boards is None:
            import torch
            import torch.distributed as dist
            world, rank = dist.get_world_size(self._group), dist.get_rank(self._group)
            dev = f'cuda:{self.engine.device}' if dist.get_backend(self._group) == 'nccl' else 'cpu'

            def agreed(ok):
                flag = torch.tensor([1 if ok else 0], device=dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self._group)
                return int(flag.item()) == 1

            handle = None
            try:
                # (whether the engine can run one workgroup per proposal is checked by board_connect on every rank)
                if world <= 8 and ((self.nwalkers + 1) // 2) % world == 0:
                    handle, _ = self._native.board_export()
            except Exception:  # noqa: BLE001 - then every rank falls back to the all-gather
                handle = None
            ok = agreed(handle is not None)
            if ok:
                handles = [None] * world
                dist.all_gather_object(handles, handle, group=self._group)
                try:
                    self._native.board_connect(world, rank, handles=handles)
                except Exception:  # noqa: BLE001
                    ok = False
                ok = agreed(ok)
            self._boards = ok
        return self._boards

    def _resolve_collective(self):
        """'auto' -> the driver this process group runs fastest: probed once per group (on samplers of their own, a few
        steps from this sampler's present state), then remembered.  Every rank gets here at the same run."""
        import torch.distributed as dist
        # (the fastest driver depends on the shape of a half-step -- walkers, parameters, parts of the light curve --, not
        # only on the node: one probe per group AND shape)
        key = (id(self._group), dist.get_world_size(self._group), self.nwalkers, self.ndim, self._native.rows_ptr()[1])
        if key not in _probe_cache:
            x0 = self._native.get_state()[0]
            made = []

            def make(mode):
                made.append(EnsembleSampler(self.nwalkers, self.ndim, self.engine, seed=self.seed + 7919,
                                            randomize_split=self.randomize_split, group=self._group, collective=mode,
                                            native_collectives=self.native_collectives))
                return made[-1]
            dev = f'cuda:{self.engine.device}' if dist.get_backend(self._group) == 'nccl' else 'cpu'
            _, self.collective_probe = probe_collectives(make, dist, x0, group=self._group, device=dev)
            _probe_cache[key] = self.collective_probe['selected']
            # The probe samplers own peer-mapped memory (boards, mailboxes) that other ranks may still be writing into:
            # every rank has finished its probe runs before any rank unmaps anything, and the unmapping is explicit
            # (not left to the garbage collector's order).
            dist.barrier(group=self._group)
            for s in made:
                s.close()
            made.clear()
            dist.barrier(group=self._group)
        self.collective = _probe_cache[key]

    def close(self):
        """Release the native sampler (device buffers, peer mappings) now instead of at garbage collection."""
        if self._comm:
            self._comm.close()
        self._comm = False
        self._native.close()

    def _distributed(self):
        try:
            import torch.distributed as dist
        except ImportError:
            return False
        if not (dist.is_available() and dist.is_initialized()):
            return False
        return self._force_sharded or dist.get_world_size(self._group) > 1

    # --- emcee surface -------------------------------------------------------------------------------------------
    def reset(self):
        """Forget the stored chain (not the RNG position), like ``emcee.EnsembleSampler.reset``."""
        self._chain_host = np.empty((0, self.nwalkers, self.ndim))
        self._lp_host = np.empty((0, self.nwalkers))
        self._chain_on_device = 0
        self._naccepted[:] = 0
        self._nsteps_counted = 0

    def reserve_chain(self, nsteps):
        """Allocate the device memory of a stored run of ``nsteps`` steps ahead of it (a timed run then allocates
        nothing)."""
        self._collect_chain()
        self._native.reserve_chain(nsteps)

    def _collect_chain(self):
        """Bring the last stored run's chain to the host (once)."""
        if self._chain_on_device:
            chain, lp = self._native.get_chain()
            self._chain_host = np.concatenate([self._chain_host, chain])
            self._lp_host = np.concatenate([self._lp_host, lp])
            self._chain_on_device = 0

    @property
    def _chain(self):
        self._collect_chain()
        return self._chain_host

    @property
    def _lp(self):
        self._collect_chain()
        return self._lp_host

    def _prepare(self, initial_state, skip_initial_state_check=False):
        """Validate and upload the starting positions (or continue from the stored state)."""
        self._collect_chain()   # (the next run reuses the device's chain buffer)
        if initial_state is not None:
            coords = np.array(initial_state[0] if isinstance(initial_state, tuple) else initial_state,
                              dtype=np.float64)
            if coords.shape != (self.nwalkers, self.ndim):
                raise ValueError('incompatible input dimensions')
            if not np.all(np.isfinite(coords)):
                raise ValueError('At least one parameter value was infinite or NaN')
            if not skip_initial_state_check and np.linalg.matrix_rank(coords - coords.mean(0)) < self.ndim:
                raise ValueError('Initial state has a large condition number. '
                                 'Make sure that your walkers are linearly independent for the best performance')
            self._native.set_state(coords)
            self._acc0 = np.zeros(self.nwalkers, dtype=np.int64)
            self._acc_seen = None
        elif self._state is None:
            raise ValueError('Cannot have `initial_state=None` if run_mcmc has never been called.')
        else:
            # (the counts the last run left: remembered by _finish -- nothing but a run changes them)
            self._acc0 = self._acc_seen if self._acc_seen is not None else self._native.naccepted()
        if initial_state is not None and np.any(np.isnan(self._native.get_state()[1])):
            raise ValueError('Probability function returned NaN')
        self._in_flight = False

    def _launch(self, nsteps, store=True, asynchronous=True):
        split = 'random' if self.randomize_split else 'identity'
        if self.randomize_split and self.nwalkers > 16384:  # beyond the device sort: host-generated colouring
            split = _rng.split_permutations(self.seed, self._steps_done, nsteps, self.nwalkers)
        self._in_flight = False
        distributed = self._distributed()      # (asked once: every question below used to ask torch.distributed again)
        if self.collective == 'auto' and distributed:
            self._resolve_collective()
        try:
            if distributed and self.collective == 'rows' and self._peer_boards():
                import torch.distributed as dist
                dist.barrier(group=self._group)  # every rank has returned from its previous run (see lcf_sampler_run_rows)
                self._native.run_rows(self._steps_done, nsteps, split, store)
            elif distributed and self.collective == 'peers' and self._peer_mailboxes():
                import torch.distributed as dist
                dist.barrier(group=self._group)  # every rank has returned from its previous run (see lcf_sampler_run_peers)
                self._native.run_peers(self._steps_done, nsteps, split, store)
            elif distributed and self._native_comm() is not None:
                self._native.run_sharded(self._comm, self._steps_done, nsteps, split, store)
            elif distributed:
                ShardedStretchDriver(NativeBackend(self._native, rows=True), self._group,
                                     force_collective=self._force_sharded).run(self._steps_done, nsteps, split, store)
            elif asynchronous:
                self._native.run_async(self._steps_done, nsteps, split, store)
                self._in_flight = True
            else:
                self._native.run(self._steps_done, nsteps, split, store)
        except Exception as exc:
            self._acc_seen = None   # (see _finish)
            if getattr(exc, 'status', None) == 6:
                raise ValueError('Probability function returned NaN') from None
            raise

    def _finish(self, nsteps, store=True):
        try:
            if self._in_flight:
                self._native.wait()
        except Exception as exc:
            self._acc_seen = None   # (a run that ended midway: the counts on the device are not what the last run left)
            if getattr(exc, 'status', None) == 6:
                raise ValueError('Probability function returned NaN') from None
            raise
        finally:
            self._in_flight = False
        self._steps_done += nsteps
        if store and nsteps:
            # The chain of a run stays in HBM until somebody reads it (or the next run needs the buffer): a run returns
            # when the device has finished, not when 80 bytes per walker and step have crossed PCIe.
            self._chain_on_device = nsteps
        x, lp, self._acc_seen = self._native.snapshot()     # (state and counts: one trip through the binding)
        self._naccepted += self._acc_seen - self._acc0
        self._nsteps_counted += nsteps
        self._state = State(x, lp, None)
        return self._state

    def run_mcmc(self, initial_state, nsteps, progress=False, progress_kwargs=None, skip_initial_state_check=False,
                 store=True, **kwargs):
        self._prepare(initial_state, skip_initial_state_check)
        self._launch(nsteps, store, asynchronous=False)
        return self._finish(nsteps, store)

    def get_chain(self, flat=False, thin=1, discard=0):
        c = self._chain[discard::thin]
        return c.reshape(-1, self.ndim) if flat else c

    def _autocorr(self, discard, thin, c):
        """``(tau, window, n_t)`` of the stored chain's rows ``discard::thin``, without the ``tol`` check: on the
        device chain in place when the whole stored chain is the last run's, else on ``get_chain`` (host entry)."""
        from .engine import autocorr_time, samplers_autocorr_time
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1:
            raise ValueError('need discard >= 0 and thin >= 1')
        if self.iteration == 0:
            raise ValueError('no chain is stored: run the sampler with store=True first')
        n_t = len(range(discard, self.iteration, thin))
        if n_t == 0:
            raise ValueError(f'discard={discard} leaves no steps of the {self.iteration} stored')
        if len(self._chain_host) == 0 and self._chain_on_device > 0:
            tau, window = samplers_autocorr_time([self._native], discard, thin, c)[0]
        else:
            tau, window = autocorr_time(self.get_chain(discard=discard, thin=thin), c, device=self.engine.device)
        return tau, window, n_t

    def get_autocorr_time(self, discard=0, thin=1, c=5, tol=50, quiet=False, has_walkers=True):
        """``thin * integrated_time(self.get_chain(discard=discard, thin=thin), c, tol, quiet)``, emcee's definition
        (``lightcurve_fitting_amd.autocorr``).  The chain of the last run is read where it lies in device memory."""
        from .autocorr import check_convergence
        tau, _, n_t = self._autocorr(discard, thin, c)
        return thin * check_convergence(tau, n_t, tol, quiet)

    def get_log_prob(self, flat=False, thin=1, discard=0):
        lp = self._lp[discard::thin]
        return lp.reshape(-1) if flat else lp

    @property
    def chain(self):
        """(nwalkers, nsteps, ndim), as emcee's deprecated-but-used ``.chain`` (fitting.py:139, 152)."""
        return np.swapaxes(self._chain, 0, 1)

    @property
    def flatchain(self):
        """(nwalkers * nsteps, ndim), walker-major like emcee's ``.flatchain`` (fitting.py:147, 203)."""
        s = self.chain.shape
        return self.chain.reshape(s[0] * s[1], s[2])

    @property
    def lnprobability(self):
        return self._lp.T

    @property
    def flatlnprobability(self):
        return self.lnprobability.reshape(-1)

    @property
    def iteration(self):
        return len(self._chain_host) + self._chain_on_device

    @property
    def acceptance_fraction(self):
        """Accepted proposals per walker and step since the last reset (steps run with ``store=False`` count)."""
        return self._naccepted / max(1, self._nsteps_counted)

    @property
    def last_run_ms(self):
        return self._native.last_run_ms()


# ---------------------------------------------------------------------------------------------------------------
# parallel-tempered ensembles (what emcee 2 had as PTSampler): degenerate posteriors and the log-evidence
# ---------------------------------------------------------------------------------------------------------------
MAX_TEMPS = 64   # rungs the native driver takes (include/lcf.h)


def default_betas(ndim, ntemps, Tmax=None):
    """The ladder of inverse temperatures, ``betas[0] = 1`` descending.  ``Tmax=None``: ``betas[k] = c**-k`` with
    ``c = 1 + 2 sqrt(ln 4) / sqrt(ndim)`` (neighbouring rungs of a Gaussian posterior then swap about every fourth
    time); a finite ``Tmax``: ``betas[k] = Tmax**(-k / (ntemps - 1))``; ``Tmax=inf``: ``c**-k`` below a last rung at
    ``beta = 0``, which samples the prior."""
    ndim, ntemps = int(ndim), int(ntemps)
    if ndim < 1 or ntemps < 1:
        raise ValueError('need ndim >= 1 and ntemps >= 1')
    k = np.arange(ntemps, dtype=np.float64)
    c = 1. + 2. * np.sqrt(np.log(4.)) / np.sqrt(ndim)
    if Tmax is None:
        return c ** -k
    if np.isinf(Tmax):
        betas = c ** -k
        if ntemps > 1:
            betas[-1] = 0.
        return betas
    if not Tmax > 1.:
        raise ValueError('Tmax must be greater than 1')
    return np.ones(1) if ntemps == 1 else Tmax ** (-k / (ntemps - 1))


def check_betas(betas):
    """``betas`` as a float64 vector, or ``ValueError``: it starts at 1, descends strictly and stays ``>= 0``."""
    betas = np.array(betas, dtype=np.float64)
    if betas.ndim != 1 or not 1 <= len(betas) <= MAX_TEMPS:
        raise ValueError(f'betas must be a vector of 1 to {MAX_TEMPS} inverse temperatures')
    if betas[0] != 1.:
        raise ValueError('betas must start at 1 (the posterior itself)')
    if not np.all(betas >= 0.) or not np.all(np.diff(betas) < 0.):    # (a NaN fails both)
        raise ValueError('betas must descend strictly and stay >= 0')
    return betas


def check_proper_priors(priors, names=None):
    """A rung at ``beta = 0`` samples the prior itself, so every prior must be proper: Uniform needs finite bounds,
    LogUniform finite bounds with ``p_min > 0``, Gaussian always is.  ``priors``: descriptors ``(kind, p_min, p_max,
    mean, stddev)`` (``Prior.descriptor()``) or None (no priors: improper).  ``ValueError`` names the parameter."""
    from .engine import PRIOR_GAUSSIAN, PRIOR_LOG_UNIFORM
    if priors is None:
        raise ValueError('a rung at beta = 0 samples the prior, and the engine has no priors: they are improper')
    for i, (kind, lo, hi, *_) in enumerate(priors):
        name = names[i] if names is not None and i < len(names) else f'p{i}'
        if kind == PRIOR_GAUSSIAN:
            continue
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f'a rung at beta = 0 samples the prior, and the prior of {name} is improper: its bounds '
                             f'({lo}, {hi}) are not finite')
        if kind == PRIOR_LOG_UNIFORM and not lo > 0.:
            raise ValueError(f'a rung at beta = 0 samples the prior, and the log-uniform prior of {name} is improper: '
                             f'p_min = {lo} is not positive')


class LogEvidence(tuple):
    """``(lnZ, dlnZ)`` of :func:`thermodynamic_integration` or :func:`stepping_stone`; ``reaches_prior`` says whether
    the ladder ended at ``beta = 0`` (otherwise thermodynamic integration continued the integrand flat from the last
    rung, as emcee 2 did, and the stepping stones stop at the last rung)."""

    def __new__(cls, lnZ, dlnZ, reaches_prior):
        self = super().__new__(cls, (float(lnZ), float(dlnZ)))
        self.reaches_prior = bool(reaches_prior)
        return self

    lnZ = property(lambda self: self[0])
    dlnZ = property(lambda self: self[1])


def _trapezoid(betas, mean):
    return float(np.sum(0.5 * (mean[:-1] + mean[1:]) * (betas[:-1] - betas[1:])))


def thermodynamic_integration(betas, mean_lnL):
    """``ln Z = integral over beta in [0, 1] of <ln L>_beta`` by the trapezoid rule over the ladder:
    ``lnZ = sum_k (m_k + m_{k+1}) / 2 * (betas[k] - betas[k+1])``.  A ladder that stops at ``betas[-1] > 0`` is first
    continued by the pair ``(0, m_{K-1})`` (emcee 2's convention; the result then has ``reaches_prior = False`` and
    is an upper bound in spirit only: ``<ln L>`` falls towards the prior).  ``dlnZ = |lnZ - lnZ_coarse|``, the
    coarse ladder being the rungs 0, 2, 4, ... plus the last one if it was skipped.

    ``dlnZ`` measures the discretisation only, and a coarse ladder near ``beta = 0`` dominates it: ``<ln L>`` there
    changes by orders of magnitude between neighbouring rungs (on the small test problem of this repository the
    prior rung's mean ``ln L`` is about -1e7 against -2.7e3 at ``beta = 1/16``), so the last trapezoid carries
    nearly all of the error.  Returns a :class:`LogEvidence`."""
    betas = np.array(betas, dtype=np.float64)
    mean = np.array(mean_lnL, dtype=np.float64)
    if betas.ndim != 1 or betas.shape != mean.shape or len(betas) < 1:
        raise ValueError('betas and mean_lnL must be vectors of one length')
    reaches = bool(betas[-1] == 0.)
    if not reaches:
        betas, mean = np.append(betas, 0.), np.append(mean, mean[-1])
    lnZ = _trapezoid(betas, mean)
    keep = np.arange(0, len(betas), 2)
    if keep[-1] != len(betas) - 1:
        keep = np.append(keep, len(betas) - 1)
    return LogEvidence(lnZ, abs(lnZ - _trapezoid(betas[keep], mean[keep])), reaches)


def stepping_stone(betas, partials):
    """``ln Z`` by the stepping-stone estimator (Xie et al. 2011): ``Z = prod_k r_k`` with
    ``r_k = Z(betas[k]) / Z(betas[k+1]) = < L**(betas[k] - betas[k+1]) >`` over the samples of rung ``k + 1``.

    ``partials = (max, sum, count)``, each (K - 1, B): per pair ``k`` and batch ``b`` of the stored steps the maximum
    ``m`` of rung ``k + 1``'s ``ln L``, ``sum exp((betas[k] - betas[k+1]) (ln L - m))`` and the number of terms
    (``TemperedSampler.log_evidence`` gets them from the device).  ``ln r_kb = dbeta_k m + ln(sum / count)``;
    ``ln r_k`` combines the batches' partials by log-sum-exp (the average over all samples, not the mean of the
    batches' logarithms); ``lnZ = sum_k ln r_k``; ``dlnZ = sqrt(sum_k var_b(ln r_kb, ddof=1) / B)``, the batch-means
    standard error.  ``reaches_prior = (betas[-1] == 0)``: otherwise the sum is ``ln(Z / Z(betas[-1]))``, the
    evidence relative to the hottest rung's, not the evidence.

    What ``dlnZ`` cannot see: a stone whose average is carried by samples its hot rung never drew.  ``L**dbeta`` is
    then dominated by a tail no batch has visited, every batch agrees on too small a value, and the estimate is biased
    low with a small ``dlnZ``.  Close rungs near ``beta = 0`` (an adapted ladder) are the remedy, not more steps.
    Batches are taken as independent; steps correlated over more than a batch make ``dlnZ`` too small as well."""
    betas = np.array(betas, dtype=np.float64)
    if betas.ndim != 1 or len(betas) < 2:
        raise ValueError('betas must be a vector of at least 2 inverse temperatures')
    try:
        m, total, count = (np.array(p, dtype=np.float64) for p in partials)
    except (TypeError, ValueError):
        raise ValueError('partials must be (max, sum, count)') from None
    if not (m.shape == total.shape == count.shape and m.ndim == 2 and m.shape[0] == len(betas) - 1):
        raise ValueError('max, sum and count must each have shape (len(betas) - 1, batches)')
    B = m.shape[1]
    if B < 2:
        raise ValueError('the batch-means error needs batches >= 2')
    dbeta = (betas[:-1] - betas[1:])[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        ln_rkb = dbeta * m + np.log(total / count)
        top = np.max(m, axis=1, keepdims=True)
        scaled = np.where(total > 0., total * np.exp(dbeta * (m - top)), 0.)
        ln_rk = dbeta[:, 0] * top[:, 0] + np.log(np.sum(scaled, axis=1) / np.sum(count, axis=1))
        dlnZ = np.sqrt(np.sum(np.var(ln_rkb, axis=1, ddof=1)) / B)
    return LogEvidence(np.sum(ln_rk), dlnZ, betas[-1] == 0.)


def check_adaptive(betas):
    """``ValueError`` unless the ladder can adapt: at least 3 rungs, the last one at ``beta = 0`` (with a finite
    hottest rung the last gap is no free variable, and the rungs could cross)."""
    if len(betas) < 3 or betas[-1] != 0.:
        raise ValueError('an adaptive ladder needs at least 3 rungs and a last rung at beta = 0 (Tmax=inf)')


MAX_MOVES = 8    # entries of a mixture of moves the native driver takes (include/lcf.h)


class StretchMove:
    """The stretch move (Goodman & Weare 2010), what the sampler makes without ``moves``; its scale is the sampler's
    ``a``."""
    kind, needs = 0, 1    # LCF_MOVE_STRETCH; partners the move draws from the complementary colour

    def native_params(self, ndim):
        return (0., 0.)

    def __repr__(self):
        return 'StretchMove()'


class DEMove:
    """The differential-evolution move (ter Braak 2006; emcee's ``DEMove``, its names and defaults): the proposal is
    ``x + gamma0 (1 + sigma g) (c1 - c2)`` with two distinct walkers of the complementary colour and ``g`` standard
    normal.  ``gamma0=None``: ``2.38 / sqrt(2 ndim)``."""
    kind, needs = 1, 2    # LCF_MOVE_DE

    def __init__(self, sigma=1.0e-5, gamma0=None):
        if not (np.isfinite(sigma) and sigma >= 0.):
            raise ValueError('sigma must be finite and >= 0')
        if gamma0 is not None and not (np.isfinite(gamma0) and gamma0 > 0.):
            raise ValueError('gamma0 must be finite and > 0')
        self.sigma, self.gamma0 = float(sigma), None if gamma0 is None else float(gamma0)

    def native_params(self, ndim):
        return (self.sigma, 2.38 / np.sqrt(2. * ndim) if self.gamma0 is None else self.gamma0)

    def __repr__(self):
        return f'DEMove(sigma={self.sigma!r}, gamma0={self.gamma0!r})'


class DESnookerMove:
    """The snooker move (ter Braak & Vrugt 2008; emcee's ``DESnookerMove``): the walker moves along its line to a walker
    ``z`` of the complementary colour, by ``gammas`` times the distance between the projections of two more walkers
    onto that line."""
    kind, needs = 2, 3    # LCF_MOVE_SNOOKER

    def __init__(self, gammas=1.7):
        if not (np.isfinite(gammas) and gammas > 0.):
            raise ValueError('gammas must be finite and > 0')
        self.gammas = float(gammas)

    def native_params(self, ndim):
        return (self.gammas, 0.)

    def __repr__(self):
        return f'DESnookerMove(gammas={self.gammas!r})'


def check_moves(moves, nwalkers):
    """``moves`` as emcee takes it -- one move, or a list of moves or ``(move, weight)`` pairs -- as the list of
    ``(move, weight)`` with the weights normalised, or ``ValueError``: unknown objects, weights that are not positive and
    finite, more than ``MAX_MOVES`` entries, or fewer walkers than a move needs (either colour of the split must hold the
    partners it draws: 4 walkers for ``DEMove``, 6 for ``DESnookerMove``)."""
    kinds = (StretchMove, DEMove, DESnookerMove)
    if isinstance(moves, kinds):
        moves = [moves]
    try:
        entries = [m if isinstance(m, (tuple, list)) else (m, 1.) for m in moves]
    except TypeError:
        raise ValueError(f'moves must be a move or a list of moves or (move, weight) pairs, not {moves!r}') from None
    if not 1 <= len(entries) <= MAX_MOVES:
        raise ValueError(f'moves must have 1 to {MAX_MOVES} entries, not {len(entries)}')
    for entry in entries:
        if len(entry) != 2 or not isinstance(entry[0], kinds):
            raise ValueError(f'not a move or a (move, weight) pair: {entry!r} (StretchMove, DEMove and DESnookerMove '
                             f'are the moves there are)')
    try:
        w = np.array([float(weight) for _, weight in entries])
    except (TypeError, ValueError):
        raise ValueError('the weights of moves must be numbers') from None
    if not (np.all(np.isfinite(w)) and np.all(w > 0.)):
        raise ValueError(f'the weights of moves must be positive and finite, not {w.tolist()}')
    smaller = int(nwalkers) - (int(nwalkers) + 1) // 2
    for move, _ in entries:
        if smaller < move.needs:
            raise ValueError(f'{move!r} draws {move.needs} distinct partners from either colour of the split: it needs '
                             f'at least {2 * move.needs} walkers, not {nwalkers}')
    return [(move, float(x)) for (move, _), x in zip(entries, w / w.sum())]


def native_moves(moves, ndim):
    """``(kinds, cum_weights, params)`` of ``NativeTempered.set_moves`` for a list from :func:`check_moves`: the
    cumulative weights by ``np.cumsum``, the last set to exactly 1."""
    cum = np.cumsum([w for _, w in moves])
    cum[-1] = 1.
    return ([m.kind for m, _ in moves], cum, np.array([m.native_params(ndim) for m, _ in moves], dtype=np.float64))


class TemperedSampler:
    """A parallel-tempered ensemble on one engine: ``ntemps`` rungs of inverse temperature ``betas`` (1 first), each
    an ensemble of ``nwalkers`` walkers that makes the stretch move on ``prior * L**beta``; after every step
    neighbouring rungs offer each other their walkers slot by slot.  The cold rung (``temp=0``) samples the posterior
    and is what ``chain`` / ``flatchain`` give, in the shapes of :class:`EnsembleSampler`; the hot rungs cross between
    modes and along degeneracies and hand what they find down the ladder, and the rungs' mean log-likelihoods
    integrate to the log-evidence (:meth:`log_evidence`).

    ``betas`` wins over ``ntemps`` / ``Tmax`` (:func:`default_betas`; ``ntemps=None`` with ``Tmax`` given is not
    guessed).  A rung at ``beta = 0`` needs proper priors (:func:`check_proper_priors`).  Rung ``k`` draws under
    ``seed + k * 0x9E3779B97F4A7C15``, so rung 0 of a sampler is the :class:`EnsembleSampler` of the same seed until
    the first accepted swap.  ``names``: the parameters' names, for the message that refuses an improper prior
    (default ``p0, p1, ...``).

    ``run_mcmc(..., adapt=True)`` moves the rungs while it runs, on the device, until neighbouring pairs swap equally
    often (Vousden, Farr & Mandel 2016, as ``ptemcee``; ``adaptation_lag`` and ``adaptation_time`` are its names and
    defaults): after every second step, from the swaps since the last adaptation, the gaps ``1 / beta_{k+1} -
    1 / beta_k`` are scaled by ``exp(kappa (A_k - A_{k+1}))`` with ``kappa = lag / (t + lag) / time`` and ``t`` the
    adapting steps made so far (``adaptation_steps``, never reset).  Needs ``ntemps >= 3`` and a last rung at
    ``beta = 0``.  A moving ladder samples no fixed distribution: adapt during burn-in, then run frozen.

    ``moves`` (as emcee's): a move, or a list of moves or ``(move, weight)`` pairs of :class:`StretchMove`,
    :class:`DEMove` and :class:`DESnookerMove` (:func:`check_moves`); None: the stretch move, as ever.  Every step, each
    rung draws ONE kind of move by the weights and makes it in both half-steps; the colouring, the order of the walkers
    and the accept test's ``ln u`` are the same whatever the moves.  ``moves`` holds the normalised list,
    :meth:`set_moves` changes it between runs, :meth:`get_move_kinds` says what the stored steps made."""

    def __init__(self, nwalkers, ndim, engine, ntemps=None, betas=None, Tmax=None, seed=0, a=2.0, names=None,
                 adaptation_lag=10000, adaptation_time=100, moves=None):
        from .engine import NativeTempered
        if nwalkers < 2 * ndim:
            raise ValueError('It is unadvisable to use a red-blue move with fewer walkers than twice the number of '
                             'dimensions.')
        if ndim != engine.ndim:
            raise ValueError(f'ndim = {ndim} but the engine has {engine.ndim} parameters')
        if betas is None:
            if ntemps is None:
                raise ValueError('give ntemps or betas')
            betas = default_betas(ndim, ntemps, Tmax)
        self.betas = check_betas(betas)        # the ladder now: read back after every run
        if self.betas[-1] == 0.:
            check_proper_priors(getattr(engine, 'priors', None), names)
        if not (0. < adaptation_lag < np.inf and 0. < adaptation_time < np.inf):
            raise ValueError('adaptation_lag and adaptation_time must be positive and finite')
        self.adaptation_lag, self.adaptation_time = float(adaptation_lag), float(adaptation_time)
        self.adaptation_steps = 0   # adapting steps made: never reset
        self.ntemps, self.nwalkers, self.ndim = len(self.betas), int(nwalkers), int(ndim)
        self.engine = engine
        self.seed = int(seed)
        self.moves = [(StretchMove(), 1.)] if moves is None else check_moves(moves, nwalkers)
        self._tempered = NativeTempered(engine, self.betas, nwalkers, seed, a)
        if moves is not None:
            self._tempered.set_moves(*native_moves(self.moves, self.ndim))
        self._steps_done = 0      # RNG step counter: never reset
        self._stored = 0          # steps of the stored chain (on the device)
        self._host = None         # (chain, lnL) once read, until the next stored run
        self._host_betas = None   # (stored, K) ladder per stored step, likewise
        self._nacc = np.zeros((self.ntemps, self.nwalkers), dtype=np.int64)
        self._swaps = np.zeros((2, self.ntemps - 1), dtype=np.int64)   # accepted, proposed
        self._nsteps_counted = 0
        self._state = None

    def close(self):
        self._tempered.close()

    def set_moves(self, moves):
        """The moves of the steps from the next run on (None: the stretch move, through the kernels of a sampler that
        never had moves).  The state, the counts and the stored chain stay."""
        if moves is None:
            self._tempered.set_moves([], [], np.empty((0, 2)))
            self.moves = [(StretchMove(), 1.)]
        else:
            new = check_moves(moves, self.nwalkers)
            self._tempered.set_moves(*native_moves(new, self.ndim))
            self.moves = new

    def get_move_kinds(self, discard=0, thin=1):
        """(nsteps, ntemps) integers: the kind of move every rung made in every stored step (the ``kind`` of the move
        classes: 0 stretch, 1 differential evolution, 2 snooker), as the device recorded it."""
        return self._tempered.get_move_history(self._stored)[discard::thin]

    def reset(self):
        """Forget the stored chain and the counts (not the RNG position)."""
        self._stored, self._host, self._host_betas = 0, None, None
        self._nacc[:] = 0
        self._swaps[:] = 0
        self._nsteps_counted = 0

    def run_mcmc(self, initial_state, nsteps, store=True, adapt=False, **kwargs):
        """``initial_state``: (ntemps, nwalkers, ndim) coordinates (or a state tuple whose first entry they are), or
        None to continue.  ``adapt``: the ladder moves during this run (see the class).  Returns
        ``State(coords, lnL, None)`` of all rungs."""
        nt = self._tempered
        if adapt:
            check_adaptive(self.betas)
        if initial_state is not None:
            coords = np.array(initial_state[0] if isinstance(initial_state, tuple) else initial_state, dtype=np.float64)
            if coords.shape != (self.ntemps, self.nwalkers, self.ndim):
                raise ValueError('incompatible input dimensions')
            if not np.all(np.isfinite(coords)):
                raise ValueError('At least one parameter value was infinite or NaN')
            try:
                nt.set_state(coords)
            except Exception as exc:
                if getattr(exc, 'status', None) == 6:
                    raise ValueError('Probability function returned NaN') from None
                if getattr(exc, 'status', None) == 7:
                    raise ValueError(f'Initial state outside the prior: {exc}') from None
                raise
            before = (0, 0, 0)
        elif self._state is None:
            raise ValueError('Cannot have `initial_state=None` if run_mcmc has never been called.')
        else:
            before = nt.counts()
        mode = ('append' if self._stored else True) if store else False
        try:
            if adapt:
                nt.run_adaptive(self._steps_done, nsteps, mode, self.adaptation_lag, self.adaptation_time,
                                self.adaptation_steps)
            else:
                nt.run(self._steps_done, nsteps, mode)
        except Exception as exc:
            if store and not self._stored:   # (a run that replaces the chain and fails leaves none; an appending one, the old)
                self._host = self._host_betas = None
            if getattr(exc, 'status', None) == 6:
                raise ValueError('Probability function returned NaN') from None
            raise
        self._steps_done += nsteps
        if adapt:
            self.adaptation_steps += nsteps
        self.betas = nt.get_betas()
        if store and nsteps:
            self._stored += nsteps
            self._host = self._host_betas = None
        acc, sa, sp = nt.counts()
        self._nacc += acc - before[0]
        self._swaps += np.stack([sa - before[1], sp - before[2]])
        self._nsteps_counted += nsteps
        x, ll, _ = nt.get_state()
        self._state = State(x, ll, None)
        return self._state

    def _collect(self):
        if self._host is None:
            self._host = self._tempered.get_chain(self._stored)
        return self._host

    @property
    def iteration(self):
        return self._stored

    def get_chain(self, temp=0, flat=False, thin=1, discard=0):
        """(nsteps, nwalkers, ndim) of rung ``temp``; ``temp=None``: (nsteps, ntemps, nwalkers, ndim)."""
        c = self._collect()[0][discard::thin]
        if temp is None:
            return c.reshape(-1, self.ndim) if flat else c
        c = c[:, temp]
        return c.reshape(-1, self.ndim) if flat else c

    def get_log_like(self, temp=None, flat=False, thin=1, discard=0):
        """Log-LIKELIHOODS (no prior): (nsteps, ntemps, nwalkers), or (nsteps, nwalkers) of rung ``temp``."""
        ll = self._collect()[1][discard::thin]
        if temp is not None:
            ll = ll[:, temp]
        return ll.reshape(-1) if flat else ll

    def get_betas(self, discard=0, thin=1):
        """(nsteps, ntemps): the ladder every stored step was sampled under (before any adaptation that follows the
        step).  All rows are equal unless the chain was stored while adapting."""
        if self._host_betas is None:
            self._host_betas = self._tempered.get_beta_history(self._stored)
        return self._host_betas[discard::thin]

    @property
    def chain(self):
        """The cold rung, (nwalkers, nsteps, ndim) as ``EnsembleSampler.chain``."""
        return np.swapaxes(self.get_chain(0), 0, 1)

    @property
    def flatchain(self):
        """The cold rung, (nwalkers * nsteps, ndim), walker-major as ``EnsembleSampler.flatchain``."""
        c = self.chain
        return c.reshape(c.shape[0] * c.shape[1], c.shape[2])

    @property
    def acceptance_fraction(self):
        """(ntemps, nwalkers): accepted moves per slot and step since the last reset."""
        return self._nacc / max(1, self._nsteps_counted)

    @property
    def swap_acceptance_fraction(self):
        """(ntemps - 1,): accepted / proposed swaps of the pairs (k, k + 1) since the last reset (NaN: none proposed)."""
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(self._swaps[1] > 0, self._swaps[0] / self._swaps[1], np.nan)

    def get_autocorr_time(self, discard=0, thin=1, c=5, tol=50, quiet=False):
        """``thin * integrated_time`` of the cold chain (``lightcurve_fitting_amd.autocorr``)."""
        from .autocorr import integrated_time
        if self._stored == 0:
            raise ValueError('no chain is stored: run the sampler with store=True first')
        return thin * integrated_time(self.get_chain(0, discard=discard, thin=thin), c=c, tol=tol, quiet=quiet,
                                      device=self.engine.device)

    def mean_log_like(self, discard=0):
        """(ntemps,): every rung's mean log-likelihood over the stored steps ``discard:`` and all walkers, reduced on
        the device in a fixed order."""
        if self._stored == 0:
            raise ValueError('no chain is stored: run the sampler with store=True first')
        if not 0 <= int(discard) < self._stored:
            raise ValueError(f'discard={discard} leaves no steps of the {self._stored} stored')
        return self._tempered.mean_loglike(discard)

    def log_evidence(self, discard=0, method='thermodynamic', batches=8):
        """``(lnZ, dlnZ)`` with ``reaches_prior``, from the stored steps ``discard:``.  ``method='thermodynamic'``:
        :func:`thermodynamic_integration` of the rungs' mean log-likelihoods, only as good as the ladder is fine where
        ``<ln L>`` is steep.  ``method='stepping_stone'``: :func:`stepping_stone` over ``batches`` contiguous batches
        of the steps, reduced on the device; right to a few tenths on ladders where the trapezoids are off by
        thousands.  Both need a chain sampled under ONE ladder (``ValueError`` otherwise): adapt during burn-in, store
        the frozen run."""
        if method not in ('thermodynamic', 'stepping_stone'):
            raise ValueError(f"method must be 'thermodynamic' or 'stepping_stone', not {method!r}")
        if method == 'stepping_stone' and (batches != int(batches) or int(batches) < 2):
            raise ValueError('the batch-means error needs an integer batches >= 2')
        if self._stored == 0:
            raise ValueError('no chain is stored: run the sampler with store=True first')
        if not 0 <= int(discard) < self._stored:
            raise ValueError(f'discard={discard} leaves no steps of the {self._stored} stored')
        if method == 'stepping_stone':
            if self.ntemps < 2:
                raise ValueError('stepping stones need at least 2 rungs')
            if int(batches) > self._stored - int(discard):
                raise ValueError(f'batches={batches} is more than the {self._stored - int(discard)} stored steps kept')
        ladder = self.get_betas(discard=int(discard))
        if np.any(ladder != ladder[0]):
            raise ValueError('the ladder moved while these steps were stored (they were sampled with adapt=True): '
                             'adapt during burn-in, then store a frozen run, or discard the adapting steps')
        if method == 'stepping_stone':
            return stepping_stone(ladder[0], self._tempered.stepping_stones(int(discard), int(batches)))
        return thermodynamic_integration(ladder[0], self.mean_log_like(discard))
