"""The resident half-step kernel (k_solo_run) runs the columns of a LATE item at a raised issue priority: wave 0 stores,
directly behind its poll, whether every polling lane found its rows at the first look -- a 4-byte word above the abort
word, the upper half of the double beside the log-prior in this item's copy of the scratch words -- and every wave takes
the bit out of the 16-byte read it makes behind barrier 1 anyway, raises its priority for the column section and drops it
in front of barrier 2.  No value and no operation changes, so every case compares a resident run ('auto', which must
report 'run' and its kernel instance) with the 'phases' path (k_step + k_points: none of the changed code) bit for bit --
chain, log-posteriors, acceptance counts, returned state, snapshot -- after a run of 9 steps and after a continuation of
7 (the helpers of tests/test_gpu_commit_wave.py).

What can go wrong, and what would show it: a store wider than four bytes over the abort word (the launch gives up: the
run is no longer 'run') or over the log-prior (the chain differs; with priors that exclude proposals, so does the set of
scored ones); a store into the other copy of the scratch words, which the committing wave is reading (several slots per
workgroup, an empty slot, an odd number of items per launch, runs of several launches); a wave that no longer passes every
barrier on some path (excluded proposals, the general columns, the four-part and the rank kernel)."""
import gc
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import sampler_cases as S  # noqa: E402
from lightcurve_fitting_amd import models as M  # noqa: E402
from test_gpu_commit_wave import (FOUR_PARTS, RUNS, _against_phases, _moves, _results, _two_ranks,  # noqa: E402
                                  half_excluded_case)
from test_gpu_early_phase_log import LEAN, SC, SC2, _digest, _sampler, shock2_problem  # noqa: E402
from test_gpu_lane_head import TRUTH, Z, engine, shock_problem, start, uniform_priors  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n_epochs', [LEAN, 40])
def test_lean_and_general_columns(n_epochs):
    """12 walkers, six workgroups.  LEAN epochs in six filters: lean columns in both parts; 40 epochs: the general
    columns, behind the same raise and in front of the same drop."""
    pb = shock_problem(uniform_priors(), n_epochs=n_epochs)
    res = _against_phases(engine(pb), 12, 191, start(TRUTH, 12, 14))
    moved, stayed = _moves(res)
    assert moved > 0 and stayed > 0


@pytest.mark.parametrize('n_epochs', [LEAN, 40])
def test_excluded_proposals(n_epochs):
    """Priors that exclude about half of the proposals: an excluded item has no columns and goes from barrier 1 straight
    to barrier 2 -- wave 0 arrives earliest at the next poll -- and must not carry a raised priority into the next item;
    a log-prior changed by the flag's store would change which proposals are excluded."""
    pb, x0, seed = half_excluded_case(n_epochs)
    res = _against_phases(engine(pb), 12, seed + 100, x0)
    moved, stayed = _moves(res)
    assert moved > 0 and stayed > 0


@pytest.mark.parametrize('n_epochs', [LEAN, 40])
def test_a_run_of_several_launches(n_epochs, monkeypatch):
    """Blocks of three steps of draw records: every launch starts with copy 0 of the scratch words again."""
    monkeypatch.setenv('LCF_DRAW_BLOCK', '3')
    pb = shock_problem(uniform_priors(), n_epochs=n_epochs)
    res = _against_phases(engine(pb), 12, 192, start(TRUTH, 12, 15))
    assert res.last_run_launches() >= 3


def test_shock_cooling2():
    """ND = 4: lanes 0 .. 5 poll, the ballot is over six lanes."""
    truth, lc, priors = shock2_problem(seed=161)
    eng = M.ShockCooling2(redshift=Z).engine_for(lc, priors=priors)
    res = _against_phases(eng, 12, 195, start(truth, 12, 16, 0.03), model=SC2)
    moved, stayed = _moves(res)
    assert moved > 0 and stayed > 0


def test_two_emulated_ranks():
    """k_solo_run<..., RANKS> (BOARD = 3) shares the body.  (Collected and with the collector off for the reason
    test_gpu_commit_wave.test_two_emulated_ranks gives.)"""
    gc.collect()
    gc.disable()
    try:
        _two_ranks()
    finally:
        gc.enable()


# ---- several slots per workgroup, and the four-part kernel: switches that need a child process ------------------------
def _grid_run(kernel, block=None):
    """13 walkers with lean columns on three workgroups (LCF_RUN_GRID=3, the child process): seven slots of a half-step,
    the smaller colour's last one empty, five items per workgroup and step at most -- an odd number of items in a launch
    of three steps (`block`: LCF_DRAW_BLOCK).  -> (kernel, instance, launches of the last run, digest after each run)."""
    with S.environment(LCF_DRAW_BLOCK=block):
        pb = shock_problem(uniform_priors(), n_epochs=LEAN)
        s = _sampler(engine(pb), 13, 193, start(TRUTH, 13, 17), kernel)
        out = []
        for first, n in RUNS:
            s.run(first, n, 'random', True)
            out.append(_digest(_results(s, True)))
    return s.last_run_kernel(), list(s.last_run_instance()), s.last_run_launches(), out


@pytest.fixture(scope='module')
def child_lines():
    """One child process with LCF_RUN_GRID=3 and LCF_RUN_ANY_SIZE=1: this file's main below."""
    env = dict(os.environ, LCF_RUN_GRID='3', LCF_RUN_ANY_SIZE='1')
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    return {ln['what']: ln for ln in (json.loads(t) for t in out.stdout.splitlines() if t.startswith('{'))}


@pytest.mark.parametrize('block', [None, '3'])
def test_several_slots_per_workgroup(block, child_lines):
    line = child_lines[f'grid-{block}']
    assert line['kernel'] == 'run' and line['instance'] == [5, 2, SC, 0]
    kernel, _, _, want = _grid_run('phases', block)
    assert kernel == 'phases' and line['digests'] == want
    if block:
        assert line['launches'] >= 3


def test_four_parts(child_lines):
    """k_solo_run<5, 1, true, 4, ShockCooling>: no barrier 0 and no lean columns; the flag is stored and read all the same."""
    line = child_lines['four-parts']
    case = S.CASES[FOUR_PARTS]
    assert line['kernel'] == 'run' and line['instance'] == [5, 4, SC, 0]
    assert line['digest'] == S.digest(S.run_single(case, 'phases'))


if __name__ == '__main__':
    for block_ in (None, '3'):
        kernel_, instance_, launches_, digests_ = _grid_run('auto', block_)
        print(json.dumps(dict(what=f'grid-{block_}', kernel=kernel_, instance=instance_, launches=launches_, digests=digests_)),
              flush=True)
    run_ = S.run_single(S.CASES[FOUR_PARTS], 'grid')
    print(json.dumps(dict(what='four-parts', kernel=run_['kernel'], instance=list(run_['instance']), digest=S.digest(run_))),
          flush=True)
