"""The serial head of the resident half-step kernel (k_solo_run) is computed lane-parallel: lane d polls for coordinate d
of the partner AND of the walker, computes its own coordinate of the proposal, its logarithm and its prior's term, and
writes its own words of the LDS hand-off; the coefficients' branch for non-positive parameters and the poll's time-out
handling are out of line.  Every case compares a resident run ('auto', which must report 'run') with the 'phases' path
(k_step + k_points: none of the changed code) bit for bit -- chain, log-probabilities, final state, acceptance counts
-- at the smallest shapes at which such a head can go wrong."""
import numpy as np
import pytest

from helpers import lc_dict, oracle_log_posterior
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.engine import NativeSampler
from oracle import lcf_oracle as O

pytestmark = pytest.mark.gpu

FILTERS = list('UBVgri')
TRUTH = np.array([1.2, 0.5, 3.0, 2.0, 0.1])
Z = 0.004


def uniform_priors(r_max=10., lo=0.):
    """Uniform priors of the ShockCooling parameters; `r_max`: the upper edge for R (truth 2.0), `lo`: the lower edge
    for v, M, f and R."""
    return [M.UniformPrior(lo, 10.)] * 3 + [M.UniformPrior(lo, r_max)] + [M.UniformPrior(-1., 0.5)]


def shock_problem(priors, n_epochs=40, seed=21):
    """ShockCooling, six filters at `n_epochs` shared epochs (one column per epoch), data from the oracle."""
    rng = np.random.default_rng(seed)
    epochs = np.sort(rng.uniform(0.6, 9., n_epochs))
    t, names = np.repeat(epochs, 6), list(np.tile(FILTERS, n_epochs))
    bands = [O.band(n) for n in names]
    om = ('ShockCooling', O.ShockCoolingOracle(Z))
    ytrue = O.evaluate(om, t, bands, TRUTH)
    y, dy = ytrue * (1 + 0.05 * rng.standard_normal(len(t))), 0.05 * ytrue
    return dict(model=om, orc=None, t=t, bands=bands, y=y, dy=dy, priors=[p.descriptor() for p in priors], truth=TRUTH,
                lc=lc_dict(t, names, y, dy), prior_objects=priors)


def rejected_case():
    """A prior on R whose upper edge lies just above the truth, the walkers at distances 0.05 / 2^k below it: a proposal
    that moves a walker towards the edge mostly crosses it (an upper edge can exclude at most the half of the proposals
    that move upwards; here 29 of 108, counted with the oracle)."""
    r_max = 2.02
    pb = shock_problem(uniform_priors(r_max=r_max))
    x0 = start(TRUTH, 12, 8, 0.02)
    x0[:, 3] = r_max - 0.05 * 0.5 ** np.random.default_rng(80).permutation(12)
    return pb, x0, 33


def non_positive_case():
    """Priors that allow negative v, M, f, R, and a start in which a third of the walkers have a negative v and another
    third a negative f: their proposals, and those of their partners, take the coefficients' general branch."""
    pb = shock_problem(uniform_priors(lo=-1.))
    x0 = start(TRUTH, 12, 9, 0.05)
    x0[0::3, 0] = -0.05 - 0.01 * np.arange(4)
    x0[1::3, 2] = -0.1 - 0.02 * np.arange(4)
    return pb, x0, 34


def start(truth, nwalkers, seed, scatter=0.05):
    return truth * (1 + scatter * np.random.default_rng(seed).standard_normal((nwalkers, len(truth))))


def engine(pb, **kw):
    return M.ShockCooling(redshift=Z).engine_for(pb['lc'], priors=pb['prior_objects'], **kw)


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
    """The error a run ends with (None: none), as text."""
    try:
        s.run(first, n, 'random', True)
    except Exception as e:   # noqa: BLE001 (whatever the run reports must be reported by both samplers)
        return f'{type(e).__name__}: {e}'
    return None


def _against_phases(eng, nwalkers, seed, x0, runs):
    """`runs`: (first step, steps) one after the other; the resident sampler against the 'phases' one after each."""
    res, ref = _sampler(eng, nwalkers, seed, x0, 'auto'), _sampler(eng, nwalkers, seed, x0, 'phases')
    for first, n in runs:
        assert _run(res, first, n) == _run(ref, first, n)
        assert res.last_run_kernel() == 'run' and ref.last_run_kernel() == 'phases'
        _same(_results(res), _results(ref))
    return res, ref


def _moves(res, nsteps):
    """Walkers that moved / stayed, summed over the steps of the stored chain (`nsteps` of them)."""
    acc = int(res.naccepted().sum())
    return acc, nsteps * len(res.naccepted()) - acc


def test_specialised_kernel_in_two_runs_that_continue_each_other():
    """ShockCooling, 6 filters x 40 epochs, 12 walkers: 5 steps, then 4 more."""
    pb = shock_problem(uniform_priors())
    res, _ = _against_phases(engine(pb), 12, 31, start(TRUTH, 12, 4), [(0, 5), (5, 4)])
    moved, stayed = _moves(res, 9)
    assert moved > 0 and stayed > 0


def test_odd_ensemble():
    """11 walkers: the colour of 5 leaves the last slot of its half-steps empty; nd + 1 = 6 lanes of rows."""
    pb = shock_problem(uniform_priors())
    _against_phases(engine(pb), 11, 32, start(TRUTH, 11, 5), [(0, 5), (5, 4)])


def test_rejected_proposals_leave_the_row_unchanged():
    """Excluded proposals (log-prior -inf: no columns, the walker's row posted again unchanged) beside scored ones, and
    both accepted and rejected moves -- counted with the oracle-driven run of the same draws, which the chain equals."""
    pb, x0, seed = rejected_case()
    res, _ = _against_phases(engine(pb), 12, seed, x0, [(0, 9)])
    seen = {'excluded': 0, 'scored': 0}
    log_post = oracle_log_posterior(pb)

    def counting(block):
        out = log_post(block)
        seen['excluded'] += int(np.sum(out == -np.inf))
        seen['scored'] += int(np.sum(np.isfinite(out)))
        return out
    ref, _, ref_acc = O.stretch_move_run(counting, x0, 9, seed)
    assert seen['excluded'] > 20 and seen['scored'] > 20
    assert 0 < ref_acc.sum() < 9 * 12 and np.array_equal(res.naccepted(), ref_acc)
    assert np.max(np.abs(res.get_chain()[0] - ref) / np.abs(ref)) < 1e-9


def test_log_uniform_and_gaussian_priors_among_the_five():
    """Each lane's own prior meets its own coordinate of the proposal, and the terms are summed in parameter order."""
    priors = [M.UniformPrior(0., 10.), M.LogUniformPrior(0.01, 10.), M.GaussianPrior(0., 10., 3., 0.2), M.UniformPrior(0., 10.),
              M.UniformPrior(-1., 0.5)]
    pb = shock_problem(priors)
    res, _ = _against_phases(engine(pb), 12, 35, start(TRUTH, 12, 6), [(0, 9)])
    moved, stayed = _moves(res, 9)
    assert moved > 0 and stayed > 0


def test_non_positive_parameters_take_the_out_of_line_coefficients():
    """Walkers with a negative v or f inside priors that allow them: the coefficients' general branch (out of line in the
    resident kernel) for them and for proposals between them and the others; whatever a run reports -- a NaN
    log-probability included -- both samplers report."""
    pb, x0, seed = non_positive_case()
    res, _ = _against_phases(engine(pb), 12, seed, x0, [(0, 9)])
    chain = res.get_chain()[0]
    assert np.any(chain[:, :, [0, 2]] <= 0.)
    moved, stayed = _moves(res, 9)
    assert moved > 0 and stayed > 0


def test_several_slots_per_workgroup(monkeypatch):
    """41 walkers on 7 resident workgroups: three slots of a half-step each, the lanes' registers reused slot after slot
    (the last slot of the smaller colour is empty)."""
    monkeypatch.setenv('LCF_RUN_GRID', '7')
    pb = shock_problem(uniform_priors(r_max=2.2))
    _against_phases(engine(pb), 41, 36, start(TRUTH, 41, 7), [(0, 4)])


def test_generic_kernel_with_a_fitted_sigma():
    """Six parameters (5 + sigma): the generic kernel, dimension at run time, n_par = 5 logarithms on 6 lanes."""
    pb = shock_problem(uniform_priors() + [M.UniformPrior(0., 5.)])
    eng = engine(pb, use_sigma=True)
    _against_phases(eng, 12, 37, start(np.append(TRUTH, 0.5), 12, 8, 0.03), [(0, 5)])


def test_generic_kernel_with_eight_parameters():
    """CompanionShocking: 8 parameters, nd + 2 = 10 lanes of rows, fewer logarithms than parameters; 16 walkers, 3 steps."""
    rng = np.random.default_rng(1011)
    truth = np.array([57001., 0.5, 1.2, 57018., 1.05, 0.95, 0.9, 0.6])
    priors = [M.UniformPrior(56999., 57001.4), M.UniformPrior(0., 10.), M.UniformPrior(0., 10.), M.UniformPrior(57008., 57028.),
              M.UniformPrior(0.5, 2.), M.UniformPrior(0., 5.), M.UniformPrior(0., 5.), M.UniformPrior(0., 5.)]
    filts = list('UBri')
    epochs = 57001.5 + np.sort(rng.uniform(0., 40., 20))
    t, names = np.repeat(epochs, len(filts)), list(np.tile(filts, len(epochs)))
    bands = [O.band(n) for n in names]
    guess = 2e20 * np.exp(-0.5 * ((t - 57018.) / 12.) ** 2)   # (the template is scaled to the observed peak)
    ytrue = O.evaluate(('CompanionShocking', O.CompanionShockingOracle(bands, guess, 0.003, 1)), t, bands, truth)
    y, dy = ytrue * (1 + 0.05 * rng.standard_normal(len(t))), 0.05 * np.abs(ytrue)
    lc = lc_dict(t, names, y, dy)
    eng = M.CompanionShocking(lc, redshift=0.003).engine_for(lc, priors=priors)
    x0 = truth + np.array([0.05, 0.02, 0.05, 0.2, 0.01, 0.02, 0.02, 0.02]) * rng.standard_normal((16, 8))
    _against_phases(eng, 16, 38, x0, [(0, 3)])


def test_two_emulated_ranks():
    """k_solo_run<..., RANKS> (rows from the rank's own board, commits posted on both): two samplers on engines of their
    own move their shares of 12 walkers for 5 steps; each rank's chain, state and counts are the 'phases' run's."""
    pb = shock_problem(uniform_priors())
    nwalkers, nsteps, ranks = 12, 5, 2
    x0 = start(TRUTH, nwalkers, 4)
    ref = _sampler(engine(pb), nwalkers, 321, x0, 'phases')
    ref.run(0, nsteps, 'random', True)
    assert ref.last_run_kernel() == 'phases'
    want = _results(ref)
    engines = [engine(pb) for _ in range(ranks)]
    samplers = [NativeSampler(e, nwalkers, 321) for e in engines]
    ptrs = [s.board_export()[1] for s in samplers]
    for r, s in enumerate(samplers):
        s.board_connect(ranks, r, local_ptrs=ptrs)
        s.set_state(x0)                       # (every buffer sized before any rank waits for another)
        s.run(100, nsteps, 'random', True)
        s.set_state(x0)
        s.set_half_step_kernel('auto')
    for s in samplers:
        s.run_rows(0, nsteps, 'random', True, asynchronous=True)
    for s in samplers:
        s.wait()
        assert s.last_run_kernel() == 'run'
    for s in samplers:
        _same(_results(s), want)
