"""The resident half-step kernel (k_solo_run) takes the logarithm of its columns' phases in front of barrier 1: wave 0
passes a barrier of its own right behind the store of the proposal, the other waves compute tlog(t - t_0) from the
proposal's t_0 while wave 0 finishes the head (wave 0 takes its own behind barrier 1), and lean_column starts from the
value.  Every case compares a resident run ('auto', which must report 'run')
with the 'phases' path (k_step + k_points: none of the changed code) bit for bit -- chain, log-probabilities, final state,
acceptance counts, after a run and after its continuation -- at the shapes at which the split can go wrong.

A column takes the lean path -- the only one that uses the early value -- where the interpolants are staged in LDS: a light
curve of at least 1024 points per part, at most 256 columns in a part (lcf_engine_create).  The shapes below that (1 to 130
epochs) pass the new barrier and take no early logarithm; 256 epochs in one part, 400, 500 and 512 epochs use it; 520
epochs have a part beyond the limit.  (So no lean shape has a partly filled wave 0: a part of at least 1024 points in
six filters has at least 171 columns.)  Every ShockCooling / ShockCooling2 case asserts that the model's own kernel
instance ran: the generic kernels have no early phase."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import sampler_cases as S  # noqa: E402
from helpers import lc_dict, oracle_log_posterior  # noqa: E402
from lightcurve_fitting_amd import models as M  # noqa: E402
from lightcurve_fitting_amd.engine import NativeSampler  # noqa: E402
from oracle import lcf_oracle as O  # noqa: E402
from test_gpu_lane_head import (FILTERS, TRUTH, Z, engine, non_positive_case, rejected_case, shock_problem,  # noqa: E402
                                start, uniform_priors)

pytestmark = pytest.mark.gpu

RUNS = [(0, 12), (12, 10)]     # 22 steps: a run and its continuation
LEAN = 400                     # epochs of the cases that need lean columns in both parts (2400 points, 200 columns each)
SC, SC2 = S.SC, S.SC2          # the model of the kernel instance a run reports (last_run_instance()[2]; 0: generic)


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


def _run(s, first, n):
    """The error a run ends with (None: none), as text: whatever a run reports, both samplers must report."""
    try:
        s.run(first, n, 'random', True)
    except Exception as e:   # noqa: BLE001
        return f'{type(e).__name__}: {e}'
    return None


def _against_phases(eng, nwalkers, seed, x0, runs, model=SC):
    """`runs`: (first step, steps) one after the other; the resident sampler -- the kernel of `model`, the only one with
    the early phase -- against the 'phases' one after each.  -> the two samplers, the resident one's chain of all runs."""
    res, ref, chain = _sampler(eng, nwalkers, seed, x0, 'auto'), _sampler(eng, nwalkers, seed, x0, 'phases'), []
    for first, n in runs:
        assert _run(res, first, n) == _run(ref, first, n)
        assert res.last_run_kernel() == 'run' and ref.last_run_kernel() == 'phases'
        assert res.last_run_instance()[2] == model, res.last_run_instance()
        _same(_results(res), _results(ref))
        chain.append(np.array(res.get_chain()[0]))
    return res, ref, np.concatenate(chain)


def _moves(res, nsteps):
    """Walkers that moved / stayed, summed over the steps of all runs (`nsteps` of them)."""
    acc = int(res.naccepted().sum())
    return acc, nsteps * len(res.naccepted()) - acc


@pytest.mark.parametrize('n_epochs', [1, 64, 65, 130, 500, 512, 520])
def test_shapes(n_epochs, monkeypatch):
    """1 / 64: one part, every column on wave 0 (one live lane / all); 65: two parts, waves 0 and 4 partly filled; 130: a
    wave that is neither wave 0 nor a part's last; 500: the benchmark's layout; 512: 256 columns per part, the lean
    limit; 520: parts of 260 columns, the general path behind the same barriers (in two parts, LCF_PARTS=2 when the
    engine is created: the three parts it would get by itself are not run by resident workgroups at this size)."""
    if n_epochs == 520:
        monkeypatch.setenv('LCF_PARTS', '2')
    pb = shock_problem(uniform_priors(), n_epochs=n_epochs)
    res, _, _ = _against_phases(engine(pb), 12, 41, start(TRUTH, 12, 4), RUNS)
    moved, stayed = _moves(res, 22)
    assert moved > 0 and stayed > 0


def test_one_lean_part_beside_an_empty_group(monkeypatch):
    """256 epochs in ONE part (LCF_PARTS=1, read when the engine is created): waves 0-3 lean, all full; the second group
    of 256 threads has no part and takes the general path's empty branch behind the same barriers."""
    monkeypatch.setenv('LCF_PARTS', '1')
    pb = shock_problem(uniform_priors(), n_epochs=256)
    _against_phases(engine(pb), 12, 42, start(TRUTH, 12, 4), RUNS)


def early_epoch_case():
    """Epochs from 0.05 d, data of an explosion at 0.02 d, a prior that allows t_0 up to 8 d and a start spread from
    -0.2 to 6 d: proposals whose t_0 lies behind the first epochs -- the phase of those columns is not positive, their
    waves (wave 0 with its own logarithm, the others with the early one) leave lean_column for cold_column_with_state -- beside
    proposals with every phase positive."""
    rng = np.random.default_rng(51)
    epochs = np.sort(rng.uniform(0.6, 9., LEAN))
    epochs[0] = 0.05
    truth = np.append(TRUTH[:4], 0.02)
    t, names = np.repeat(epochs, 6), list(np.tile(FILTERS, LEAN))
    bands = [O.band(n) for n in names]
    om = ('ShockCooling', O.ShockCoolingOracle(Z))
    ytrue = O.evaluate(om, t, bands, truth)
    assert np.all(ytrue > 0.)
    y, dy = ytrue * (1 + 0.05 * rng.standard_normal(len(t))), 0.05 * ytrue
    priors = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 8.)]
    pb = dict(model=om, orc=None, t=t, bands=bands, y=y, dy=dy, priors=[p.descriptor() for p in priors], truth=truth,
              lc=lc_dict(t, names, y, dy), prior_objects=priors)
    x0 = start(truth, 14, 52, 0.03)
    x0[:, 4] = np.concatenate([np.linspace(-0.2, 0.12, 8), np.linspace(0.5, 6., 6)])
    return pb, x0, 53


def test_phases_that_are_not_positive():
    """The case above against the 'phases' path, and the 22 steps of the two runs (a sampler stores the chain of its
    last run: each run's is kept here) against the oracle-driven run of the same draws, which counts the proposals."""
    pb, x0, seed = early_epoch_case()
    res, _, chain = _against_phases(engine(pb), 14, seed, x0, RUNS)
    first_epoch, seen = pb['t'].min(), {'behind': 0, 'in front': 0, 'deep': 0}
    log_post = oracle_log_posterior(pb)

    def counting(block):
        out = log_post(block)
        scored = out != -np.inf      # (an excluded proposal has no columns)
        seen['behind'] += int(np.sum(scored & (block[:, 4] >= first_epoch)))
        seen['in front'] += int(np.sum(scored & (block[:, 4] < first_epoch)))
        seen['deep'] += int(np.sum(scored & (block[:, 4] > 2.)))    # (columns of more waves than wave 0)
        return out
    ref, _, ref_acc = O.stretch_move_run(counting, x0, 22, seed)
    print(seen)
    assert seen['behind'] > 0 and seen['in front'] > 0 and seen['deep'] > 0
    assert np.array_equal(res.naccepted(), ref_acc)
    assert chain.shape == ref.shape
    assert np.max(np.abs(chain - ref) / np.maximum(np.abs(ref), 1e-3)) < 1e-9


@pytest.mark.parametrize('n_epochs', [40, LEAN])
def test_prior_edge(n_epochs):
    """test_gpu_lane_head's rejected_case(): excluded proposals beside scored ones -- an early logarithm that nobody
    reads.  (40 epochs: that case as it stands; LEAN: the same walkers where the scored ones do read theirs.)"""
    pb, x0, seed = rejected_case()
    if n_epochs != 40:
        pb = shock_problem(uniform_priors(r_max=2.02), n_epochs=n_epochs)
    res, _, _ = _against_phases(engine(pb), 12, seed, x0, RUNS)
    moved, stayed = _moves(res, 22)
    assert moved > 0 and stayed > 0


@pytest.mark.parametrize('n_epochs', [40, LEAN])
def test_non_positive_parameters(n_epochs):
    """test_gpu_lane_head's non_positive_case(): cold_coefficients stores the coefficients itself (c_stored), t_0 among
    them, behind an early hand-off of the same number."""
    pb, x0, seed = non_positive_case()
    if n_epochs != 40:
        pb = shock_problem(uniform_priors(lo=-1.), n_epochs=n_epochs)
    _against_phases(engine(pb), 12, seed, x0, RUNS)


def shock2_problem(n_epochs=LEAN, seed=61):
    """ShockCooling2 (four parameters, t_0 the last), six filters at shared epochs."""
    rng = np.random.default_rng(seed)
    truth = np.array([30., 3., 30., 0.2])
    epochs = np.sort(rng.uniform(0.6, 9., n_epochs))
    t, names = np.repeat(epochs, 6), list(np.tile(FILTERS, n_epochs))
    bands = [O.band(n) for n in names]
    ytrue = O.evaluate(('ShockCooling2', O.ShockCoolingOracle(Z)), t, bands, truth)
    y, dy = ytrue * (1 + 0.05 * rng.standard_normal(len(t))), 0.05 * ytrue
    priors = [M.UniformPrior(0., 100.)] * 3 + [M.UniformPrior(-1., 0.5)]
    return truth, lc_dict(t, names, y, dy), priors


def test_shock_cooling2():
    """The other specialised model: t_0 is coordinate 3 of the proposal."""
    truth, lc, priors = shock2_problem()
    eng = M.ShockCooling2(redshift=Z).engine_for(lc, priors=priors)
    res, _, _ = _against_phases(eng, 12, 62, start(truth, 12, 6, 0.03), RUNS, model=SC2)
    moved, stayed = _moves(res, 22)
    assert moved > 0 and stayed > 0


def test_generic_kernel_keeps_its_two_barriers():
    """CompanionShocking at the smallest shape of tests/sampler_cases.py (case 5): a generic kernel, which has no early
    phase."""
    case = S.CASES[5]
    eng = S.make_engine(case)
    auto, phases = S.run_single(case, 'auto', eng), S.run_single(case, 'phases', eng)
    assert auto['kernel'] == 'run' and phases['kernel'] == 'phases'
    for key in ('chain', 'lp', 'nacc', 'x', 'lp_end', 'mid_x', 'mid_lp', 'mid_nacc'):
        assert np.array_equal(auto[key], phases[key]), key


def _digest(results):
    m = hashlib.sha256()
    for a in results:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def _grid_run(kernel):
    """16 walkers at the benchmark's layout, a run and its continuation -> (kernel reported, digest after each run)."""
    pb = shock_problem(uniform_priors(), n_epochs=500)
    s = _sampler(engine(pb), 16, 71, start(TRUTH, 16, 7), kernel)
    out = []
    for first, n in RUNS:
        s.run(first, n, 'random', True)
        out.append(_digest(_results(s)))
    return s.last_run_kernel(), out


def test_several_slots_per_workgroup():
    """LCF_RUN_GRID=3 in a child process: 8 slots of a half-step on 3 resident workgroups, the early value taken
    slot after slot."""
    env = dict(os.environ, LCF_RUN_GRID='3')
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    line = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{')][-1]
    assert line['kernel'] == 'run'
    kernel, want = _grid_run('phases')
    assert kernel == 'phases' and line['digests'] == want


def test_two_emulated_ranks():
    """k_solo_run<..., RANKS> (BOARD = 3) with lean columns: two samplers on engines of their own move their shares of 12
    walkers in a run and its continuation; after each, every rank's chain, state and counts are the 'phases' run's."""
    pb = shock_problem(uniform_priors(), n_epochs=LEAN)
    nwalkers, ranks = 12, 2
    x0 = start(TRUTH, nwalkers, 4)
    ref = _sampler(engine(pb), nwalkers, 321, x0, 'phases')
    engines = [engine(pb) for _ in range(ranks)]
    samplers = [NativeSampler(e, nwalkers, 321) for e in engines]
    ptrs = [s.board_export()[1] for s in samplers]
    for r, s in enumerate(samplers):
        s.board_connect(ranks, r, local_ptrs=ptrs)
        s.set_state(x0)                       # (every buffer sized before any rank waits for another)
        s.run(100, max(n for _, n in RUNS), 'random', True)
        s.set_state(x0)
        s.set_half_step_kernel('auto')
    for first, n in RUNS:
        ref.run(first, n, 'random', True)
        assert ref.last_run_kernel() == 'phases'
        want = _results(ref)
        for s in samplers:
            s.run_rows(first, n, 'random', True, asynchronous=True)
        for s in samplers:
            s.wait()
            assert s.last_run_kernel() == 'run' and s.last_run_instance()[2:] == (SC, 1), s.last_run_instance()
        for s in samplers:
            _same(_results(s), want)


if __name__ == '__main__':
    kernel_, digests_ = _grid_run('auto')
    print(json.dumps(dict(kernel=kernel_, digests=digests_)), flush=True)
