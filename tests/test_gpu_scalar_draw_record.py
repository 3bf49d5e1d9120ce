"""The resident half-step kernel (k_solo_run) reads its draw records through the scalar cache -- the whole 48-byte record
by scalar loads at the top of the half-step, the accept test's words ((n_dim - 1) ln z, ln u, the walker) again behind
barrier 2 -- requests the head's words of the launch's block in front of the poll, and the commit's LDS operands in one
batch with that reload.
No value and no operation changes, so every case compares a resident run ('auto', which must report 'run' and the
ShockCooling instance) with the 'phases' path (k_step + k_points: none of the changed code) bit for bit -- chain,
log-probabilities, final state, acceptance counts -- after a run and after its continuation.

What can go wrong, and the case that would show it: a record served stale from the scalar cache after k_draws has
rewritten its buffer (tiny blocks of records: every buffer is rewritten between the launches that read it); a record
that straddles two cache lines, or the empty slot of an odd ensemble (13 walkers: seven slots, at all four offsets a
48-byte record can have in a 64-byte line, the smaller colour's last one empty); the accept test reading the record of
another slot (several slots per workgroup); a commit whose batch posts the row of an excluded proposal again
unchanged, or follows the out-of-line coefficients; the same between two ranks (BOARD = 3)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lightcurve_fitting_amd.engine import NativeSampler  # noqa: E402
from test_gpu_early_phase_log import (LEAN, RUNS, SC, _against_phases, _digest, _moves, _results, _same,  # noqa: E402
                                      _sampler)
from test_gpu_lane_head import (TRUTH, engine, non_positive_case, rejected_case, shock_problem, start,  # noqa: E402
                                uniform_priors)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n_epochs', [40, LEAN])
def test_recycled_record_buffers(n_epochs, monkeypatch):
    """Blocks of three steps: the 22 steps of the two runs take eight blocks, which alternate over the sampler's two
    record buffers -- every launch reads records that k_draws has written over those of the launch before the previous
    one, at the same addresses.  (40 epochs: general columns; LEAN: lean ones.)"""
    monkeypatch.setenv('LCF_DRAW_BLOCK', '3')
    pb = shock_problem(uniform_priors(), n_epochs=n_epochs)
    res, _, _ = _against_phases(engine(pb), 12, 81, start(TRUTH, 12, 4), RUNS)
    assert res.last_run_launches() >= 4   # (a launch never crosses a block of records)
    moved, stayed = _moves(res, 22)
    assert moved > 0 and stayed > 0


def test_every_alignment_of_a_record_and_an_empty_slot():
    """13 walkers: seven slots per half-step, records at offsets 0, 48, 32 and 16 of a 64-byte line (two of them across
    a line's end), and the colour of six leaves its seventh slot empty (wid < 0: the workgroup skips the half-step)."""
    pb = shock_problem(uniform_priors(), n_epochs=LEAN)
    res, _, _ = _against_phases(engine(pb), 13, 82, start(TRUTH, 13, 5), RUNS)
    moved, stayed = _moves(res, 22)
    assert moved > 0 and stayed > 0


def _grid_run(kernel):
    """The 13 walkers of the case above, a run and its continuation -> (kernel, instance's model, digest after each run)."""
    pb = shock_problem(uniform_priors(), n_epochs=LEAN)
    s = _sampler(engine(pb), 13, 82, start(TRUTH, 13, 5), kernel)
    out = []
    for first, n in RUNS:
        s.run(first, n, 'random', True)
        out.append(_digest(_results(s)))
    return s.last_run_kernel(), s.last_run_instance()[2], out


def test_several_slots_per_workgroup():
    """LCF_RUN_GRID=3 in a child process: seven slots of a half-step on three resident workgroups.  The record hinted at
    is then the one of the workgroup's NEXT SLOT of the same half-step, and the accept test's reload must name the
    slot the head read, not a neighbour."""
    env = dict(os.environ, LCF_RUN_GRID='3')
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    line = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{')][-1]
    assert line['kernel'] == 'run' and line['model'] == SC
    kernel, _, want = _grid_run('phases')
    assert kernel == 'phases' and line['digests'] == want


def test_benchmark_layout():
    """500 epochs x 6 filters, 12 walkers.  The continuation's first block of records is the one the sampler generated
    speculatively behind the first run."""
    pb = shock_problem(uniform_priors(), n_epochs=500)
    res, _, _ = _against_phases(engine(pb), 12, 83, start(TRUTH, 12, 6), RUNS)
    moved, stayed = _moves(res, 22)
    assert moved > 0 and stayed > 0


def test_excluded_proposals_post_the_row_unchanged():
    """test_gpu_lane_head's rejected_case() at LEAN epochs: an excluded proposal takes no column, and its row is posted
    again unchanged from the commit's batch (wave sums nobody has written in this half-step are read and dropped)."""
    _, x0, seed = rejected_case()
    pb = shock_problem(uniform_priors(r_max=2.02), n_epochs=LEAN)
    res, _, _ = _against_phases(engine(pb), 12, seed, x0, RUNS)
    moved, stayed = _moves(res, 22)
    assert moved > 0 and stayed > 0


def test_non_positive_parameters():
    """test_gpu_lane_head's non_positive_case() at LEAN epochs: the coefficients come from the out-of-line branch, and
    columns leave the lean path for the cold one between the head's reads and the commit's batch."""
    _, x0, seed = non_positive_case()
    pb = shock_problem(uniform_priors(lo=-1.), n_epochs=LEAN)
    _against_phases(engine(pb), 12, seed, x0, RUNS)


def test_two_emulated_ranks():
    """k_solo_run<..., RANKS> (BOARD = 3): two samplers on engines of their own move their shares of 12 walkers in a run
    and its continuation; after each, every rank's chain, state and counts are the 'phases' run's."""
    pb = shock_problem(uniform_priors(), n_epochs=LEAN)
    nwalkers, ranks = 12, 2
    x0 = start(TRUTH, nwalkers, 4)
    ref = _sampler(engine(pb), nwalkers, 84, x0, 'phases')
    samplers = [NativeSampler(engine(pb), nwalkers, 84) for _ in range(ranks)]
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
    kernel_, model_, digests_ = _grid_run('auto')
    print(json.dumps(dict(kernel=kernel_, model=model_, digests=digests_)), flush=True)
