"""The resident half-step kernel (k_solo_run) reads what no half-step of a launch changes -- dimensions, priors, model
constants, the interpolants' grid, the columns of each group of threads, the strides of the row board, the state and
chain pointers -- from a block in LDS that the launch fills once.  Every case here compares a resident run with the
'phases' path (k_step + k_points: none of the changed code) bit for bit -- chain, log-probabilities, final state and
acceptance counts -- at the smallest shapes at which such a block can go wrong: left over from another launch, filled
once but used by several slots, skipped by an empty first slot, wrong for the excluded / general / generic / inter-rank
paths."""
import numpy as np
import pytest

from helpers import lc_dict, oracle_log_posterior
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.engine import NativeSampler
from oracle import lcf_oracle as O

pytestmark = pytest.mark.gpu

FILTERS = list('UBVgri')


def _shock(n_epochs, seed, r_max=10., z=0.004):
    """ShockCooling, six filters at `n_epochs` shared epochs (one column per epoch: up to 64 columns are one part, more
    are two), uniform priors; `r_max`: the upper edge of the prior on R (truth 2.0)."""
    rng = np.random.default_rng(seed)
    epochs = np.sort(rng.uniform(0.4, 9., n_epochs))
    t, names = np.repeat(epochs, 6), list(np.tile(FILTERS, n_epochs))
    bands = [O.band(n) for n in names]
    truth = np.array([1.2, 0.5, 3.0, 2.0, 0.1])
    om = ('ShockCooling', O.ShockCoolingOracle(z))
    ytrue = O.evaluate(om, t, bands, truth)
    y, dy = ytrue * (1 + 0.05 * rng.standard_normal(len(t))), 0.05 * ytrue
    priors = [M.UniformPrior(0., 10.)] * 3 + [M.UniformPrior(0., r_max)] + [M.UniformPrior(-1., 0.5)]
    pb = dict(model=om, orc=None, t=t, bands=bands, y=y, dy=dy, priors=[p.descriptor() for p in priors], truth=truth,
              lc=lc_dict(t, names, y, dy), prior_objects=priors, z=z)
    return pb, M.ShockCooling(redshift=z).engine_for(pb['lc'], priors=priors)


def _start(truth, nwalkers, seed, scatter=0.05):
    return truth * (1 + scatter * np.random.default_rng(seed).standard_normal((nwalkers, len(truth))))


def _sampler(eng, nwalkers, seed, x0, kernel):
    s = NativeSampler(eng, nwalkers, seed)
    s.set_half_step_kernel(kernel)
    s.set_state(x0)
    return s


def _results(s):
    chain, lp = s.get_chain()
    x, lp_end = s.get_state()
    return chain, lp, x, lp_end, s.naccepted()


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def _against_phases(eng, nwalkers, seed, x0, runs):
    """`runs`: (first step, steps) one after the other; the resident sampler against the 'phases' one after each."""
    res, ref = _sampler(eng, nwalkers, seed, x0, 'auto'), _sampler(eng, nwalkers, seed, x0, 'phases')
    for first, n in runs:
        res.run(first, n, 'random', True)
        ref.run(first, n, 'random', True)
        assert res.last_run_kernel() == 'run' and ref.last_run_kernel() == 'phases'
        _same(_results(res), _results(ref))
    return res, ref


def test_two_samplers_with_different_invariants_alternate():
    """ShockCooling, 6 filters x 20 shared epochs (ONE part), uniform priors, 40 walkers, and ShockCooling2 (another
    kernel, four parameters) at 65 epochs (the fewest that make TWO parts), no priors, 41 walkers: 7 steps each, in turn,
    twice.  A block that survived from the other sampler's launch -- dimension, priors, constants, columns, board -- gives
    a wrong chain.  (The engine does not expose its part count: an epoch-major engine makes one part of up to 64
    columns and two of 65 to 512 -- `n_cols > 64 ? 2 : 1` where the engine is created -- and shared epochs in every
    filter are one column each.)"""
    pb_a, eng_a = _shock(20, 5)
    rng = np.random.default_rng(6)
    epochs = np.sort(rng.uniform(0.4, 20., 65))
    t, names = np.repeat(epochs, 6), list(np.tile(FILTERS, 65))
    model_b = M.ShockCooling2(redshift=0.01)
    truth_b = np.array([30., 3., 30., 0.2])
    y = model_b(t, names, *truth_b) * (1 + 0.05 * rng.standard_normal(len(t)))
    eng_b = model_b.engine_for(lc_dict(t, names, y, 0.05 * np.abs(y)))
    xa, xb = _start(pb_a['truth'], 40, 1), _start(truth_b, 41, 2, 0.03)
    pairs = [(_sampler(e, n, sd, x, 'auto'), _sampler(e, n, sd, x, 'phases'))
             for e, n, sd, x in ((eng_a, 40, 11, xa), (eng_b, 41, 12, xb))]
    for first in (0, 7):
        for res, ref in pairs:
            res.run(first, 7, 'random', True)
            ref.run(first, 7, 'random', True)
            assert res.last_run_kernel() == 'run' and ref.last_run_kernel() == 'phases'
            _same(_results(res), _results(ref))
    for res, _ in pairs:
        assert 0 < res.naccepted().sum() < 14 * len(res.naccepted())


def test_block_filled_once_serves_every_slot_and_is_refilled_per_launch(monkeypatch):
    """40 walkers on 7 resident workgroups (three slots of a half-step each), draw records in blocks of 5 steps: 23 steps
    are five launches, each of which fills its block again."""
    monkeypatch.setenv('LCF_RUN_GRID', '7')
    monkeypatch.setenv('LCF_DRAW_BLOCK', '5')
    pb, eng = _shock(110, 77, r_max=2.2)
    res, _ = _against_phases(eng, 40, 31, _start(pb['truth'], 40, 4), [(0, 23)])
    assert res.last_run_launches() >= 5


@pytest.mark.parametrize('grid', ['7', '21'])
def test_odd_ensemble_with_an_empty_slot(grid, monkeypatch):
    """41 walkers: the colour of 20 leaves slot 20 of its half-steps empty.  On 7 workgroups it is the last of workgroup
    6's three slots; on 21 it is the ONLY slot of workgroup 20, whose launch therefore starts with an empty slot: what
    the first executed half-step sets up (tables, first columns) must wait for the next one."""
    monkeypatch.setenv('LCF_RUN_GRID', grid)
    pb, eng = _shock(110, 77, r_max=2.2)
    _against_phases(eng, 41, 32, _start(pb['truth'], 41, 5), [(0, 6), (6, 3)])


def test_priors_that_exclude_part_of_the_proposals():
    """A prior on R whose upper edge lies just above the truth: within 10 steps some proposals are excluded (log-prior
    -inf: the likelihood is skipped, stale wave sums must not enter the accept test) and others are not -- counted with
    the oracle-driven run of the same draws, which the chain also equals."""
    pb, eng = _shock(30, 9, r_max=2.05)
    x0 = _start(pb['truth'], 40, 8, 0.02)
    x0[:, 3] = np.minimum(x0[:, 3], 2.04)
    res, _ = _against_phases(eng, 40, 33, x0, [(0, 10)])
    seen = {'excluded': 0, 'scored': 0}
    log_post = oracle_log_posterior(pb)

    def counting(block):
        out = log_post(block)
        seen['excluded'] += int(np.sum(out == -np.inf))
        seen['scored'] += int(np.sum(np.isfinite(out)))
        return out
    ref, ref_lp, ref_acc = O.stretch_move_run(counting, x0, 10, 33)
    assert seen['excluded'] > 0 and seen['scored'] > 0
    chain = res.get_chain()[0]
    assert np.max(np.abs(chain - ref) / np.abs(ref)) < 1e-9 and np.array_equal(res.naccepted(), ref_acc)


def test_waves_outside_the_interpolants_take_the_cold_path():
    """Half of the walkers start with an explosion time behind the first epochs (negative phases: no log-space state):
    lean_column gives up for their waves and the out-of-line general column runs, beside the block."""
    pb, eng = _shock(110, 77, r_max=2.2)
    rng = np.random.default_rng(11)
    x0 = pb['truth'] * (1 + 0.05 * rng.standard_normal((64, 5)))
    x0[::2, 4] = rng.uniform(0.405, 0.49, 32)      # epochs start at 0.4 d; the prior allows up to 0.5
    assert np.any(pb['t'].min() < x0[:, 4])
    res, _ = _against_phases(eng, 64, 5, x0, [(0, 6)])
    assert np.any(res.get_chain()[0][-1][:, 4] > pb['t'].min())   # (walkers behind the first epoch survive to the end)


def test_generic_resident_kernel_with_a_fitted_sigma():
    """A fitted sigma: the generic kernel, walker dimension at run time (6 = 5 + sigma), no lean columns."""
    pb, _ = _shock(30, 13)
    priors = pb['prior_objects'] + [M.UniformPrior(0., 5.)]
    eng = M.ShockCooling(redshift=pb['z']).engine_for(pb['lc'], use_sigma=True, priors=priors)
    x0 = _start(np.append(pb['truth'], 0.5), 24, 14, 0.03)
    _against_phases(eng, 24, 34, x0, [(0, 7)])


def test_two_emulated_ranks_against_the_single_process_chain():
    """k_solo_run<..., RANKS>: two samplers on engines (streams) of their own move their shares of 40 walkers for 9 steps
    (two runs that continue each other) and post every row on both boards; each rank's chain, state and counts are the
    single-process 'phases' run's."""
    pb, eng = _shock(110, 77, r_max=2.2)
    nwalkers, nsteps, ranks = 40, 9, 2
    x0 = _start(pb['truth'], nwalkers, 4)
    ref = _sampler(eng, nwalkers, 321, x0, 'phases')
    ref.run(0, nsteps, 'random', True)
    assert ref.last_run_kernel() == 'phases'
    want_chain, want_lp, want_x, want_lp_end, want_acc = _results(ref)
    engines = [M.ShockCooling(redshift=pb['z']).engine_for(pb['lc'], priors=pb['prior_objects']) for _ in range(ranks)]
    samplers = [NativeSampler(e, nwalkers, 321) for e in engines]
    ptrs = [s.board_export()[1] for s in samplers]
    for r, s in enumerate(samplers):
        s.board_connect(ranks, r, local_ptrs=ptrs)
        s.set_state(x0)                       # (every buffer sized before any rank waits for another)
        s.run(100, nsteps, 'random', True)
        s.set_state(x0)
        s.set_half_step_kernel('auto')
    for first, n in ((0, 4), (4, nsteps - 4)):
        for s in samplers:
            s.run_rows(first, n, 'random', True, asynchronous=True)
        for s in samplers:
            s.wait()
            assert s.last_run_kernel() == 'run'
    for s in samplers:
        chain, lp, x, lp_end, acc = _results(s)
        assert np.array_equal(chain, want_chain[4:]) and np.array_equal(lp, want_lp[4:])
        assert np.array_equal(x, want_x) and np.array_equal(lp_end, want_lp_end) and np.array_equal(acc, want_acc)
