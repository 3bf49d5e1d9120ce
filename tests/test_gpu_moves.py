"""The moves of the parallel-tempered driver (``lcf_tempered_set_moves``, ``k_t_propose_moves``, ``TemperedSampler(moves=)``)
against their NumPy restatement (tests/moves_reference.py), held as tests/test_gpu_tempered.py holds the stretch move: the
same counter-based draws, so the same decisions, the same swap counts, the same kind of move per (rung, step) and -- up to
rounding -- the same chains.  Every comparison first checks, on the restatement alone, that no accept test of the case is
closer to its threshold than 1e-6.

Tolerances.  Chain 1e-12 and ln L 1e-11 relative, as tests/test_gpu_tempered.py.  The snooker move needs more: it divides
by |x - z| and takes the difference of two projections, and a restatement of the same run with the proposals formed in
``np.longdouble`` already differs from the float64 one by more than 1e-12 after 12 steps.  For a case with snooker moves
the bound is therefore 8 x that difference (never below 1e-12 / 1e-11), computed here on the CPU for the case's own run;
the margin of 8 covers FMA contraction and the order of the sums.  Measured on the CPU (chain / ln L, float64 against
long double), and on the device (chain / ln L against the float64 restatement):
  snooker  6.6e-13 / 6.0e-15    device 2.5e-12 / 3.4e-14   (the chain's bound: 5.3e-12)
  mixture  5.7e-13 / 6.2e-15    device 4.5e-14 / 1.2e-14
  one rung 1.2e-14 / 4.4e-16    device 9.4e-15 / 3.8e-15
  snooker after DE (the second leg of the run whose moves change)  1.9e-13 / 1.4e-15
  snooker in one dimension (W = 6)  5.0e-15 / 3.9e-15    device 5.0e-15 / 9.6e-15
DE alone and the adapting DE run differ from the restatement by 1.4e-13 / 1.8e-14 and 7.1e-14 / 3.2e-14.

Margins measured on the CPU (smallest |statistic - ln u| over the move tests / over the swap tests):
  DE       (W = 11, betas 1, .5, 0, 12 steps, seed 7):                  2.1e-2 / 0.27
  snooker  (W = 10, betas 1, .6, .3, 0, 12 steps, seed 7):              2.6e-3 / 0.12
  mixture  (D = 6, W = 13, betas 1, .5, 0, 16 steps, seed 7):           1.5e-2 / 0.17; every rung makes every kind
  one rung (W = 11, 12 steps, seed 7, mixture):                         8.1e-2 / none
  adapting (W = 11, betas 1, .5, .1, 0, 16 steps, seed 7, DE, lag 10, time 2): 5.3e-3 / 7.2e-2
  Arnett   (W = 6, 10 steps, seed 7): DE 52.7 / none, snooker 3.15 / none;  (W = 16, 20 steps, mixture): 0.44 / none

The smallest ensembles run on an engine of ONE parameter (a ``CustomModel``: a blackbody of fixed temperature whose
radius is fitted), since a handle takes no fewer walkers than twice the parameters: DE with complements of exactly 2
(W = 4; 12 steps, seed 7: margin 5.42 / none), the snooker move with complements of exactly 3 (W = 6: 2.44 / none), and
DE at W = 5 (complements 2 and 3: 1.06 / none).  In one dimension the snooker's factor is 0 and its direction +-1."""
import gc

import numpy as np
import pytest

import central_reference as C
import moves_reference as MR
import tempered_reference as R
from helpers import lc_dict
from lightcurve_fitting_amd import models as M
from lightcurve_fitting_amd.engine import LcfError, NativeTempered
from lightcurve_fitting_amd.fitting import lightcurve_mcmc
from lightcurve_fitting_amd.sampler import DEMove, DESnookerMove, StretchMove, TemperedSampler
from oracle import lcf_oracle as O

pytestmark = pytest.mark.gpu

_cache = {}

DE, SNOOKER = ([(DEMove(), 1.)], [MR.de()]), ([(DESnookerMove(), 1.)], [MR.snooker()])
MIXTURE = ([(DEMove(), .5), (DESnookerMove(), .3), (StretchMove(), .2)], [MR.de(.5), MR.snooker(.3), MR.stretch(.2)])


def _priors(use_sigma=False):
    priors = [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., 0.5)]
    return priors + [M.UniformPrior(*R.SIGMA_PRIOR[1:3])] if use_sigma else priors


def _engine(use_sigma=False):
    """The engine of ``small_problem()`` (tests/test_gpu_tempered.py's set-up), built once."""
    if use_sigma not in _cache:
        pb = R.problem(use_sigma)
        lc = lc_dict(pb['t'], pb['names'], pb['y'], pb['dy'])
        _cache[use_sigma] = M.ShockCooling(redshift=0.).engine_for(lc, use_sigma=use_sigma, priors=_priors(use_sigma))
    return _cache[use_sigma]


@pytest.fixture(scope='module', autouse=True)
def _release_the_engines():
    """The engines -- each a stream of its own -- go with this module, as those of tests/test_gpu_adaptive.py do."""
    yield
    _cache.clear()
    gc.collect()


def _bounds(snooker, ref, again):
    """(chain, ln L) relative bounds: see the module docstring.  ``again``: the long-double run of a case with snooker
    moves."""
    if not snooker:
        return 1e-12, 1e-11
    assert np.array_equal(again['nacc'], ref['nacc'])
    dc, dl = np.max(np.abs(again['chain'] / ref['chain'] - 1.)), np.max(np.abs(again['lnL'] / ref['lnL'] - 1.))
    print(f'float64 against long double on the CPU: chain {dc:.2e}, lnL {dl:.2e}')
    return max(1e-12, 8. * dc), max(1e-11, 8. * dl)


def _compare(s, ref, nsteps, bounds):
    acc, sw_acc, sw_prop = s._tempered.counts()
    print(f'moves accepted per rung: {acc.sum(1)} (restatement {ref["nacc"].sum(1)}); swaps {sw_acc} of {sw_prop}')
    assert np.array_equal(acc, ref['nacc'])                              # identical decisions
    assert np.array_equal(sw_acc, ref['swaps_accepted']) and np.array_equal(sw_prop, ref['swaps_proposed'])
    assert np.array_equal(s.get_move_kinds(), ref['kinds'])              # the kind of every (step, rung), as recorded
    chain, ll = s.get_chain(temp=None), s.get_log_like()
    print(f'largest relative difference: chain {np.max(np.abs(chain / ref["chain"] - 1.)):.2e}, '
          f'lnL {np.max(np.abs(ll / ref["lnL"] - 1.)):.2e}; bounds {bounds[0]:.2e}, {bounds[1]:.2e}')
    np.testing.assert_allclose(chain, ref['chain'], rtol=bounds[0], atol=0.)
    np.testing.assert_allclose(ll, ref['lnL'], rtol=bounds[1], atol=0.)
    assert np.array_equal(s.acceptance_fraction, ref['nacc'] / nsteps)   # accepted moves of any kind


def _against_restatement(use_sigma, nwalkers, betas, nsteps, seed, moves, adapt=None):
    pb, x0, ref = MR.cached_run(use_sigma, nwalkers, betas, nsteps, seed, moves[1], adapt)
    print(f'margins: moves {ref["move_margin"]:.3g}, swaps {ref["swap_margin"]:.3g}; NaN proposals outside the prior: '
          f'{ref["nan_proposals"]}')
    assert ref['move_margin'] > 1e-6 and ref['swap_margin'] > 1e-6       # the precondition, on the restatement alone
    snooker = any(m[0] == MR.SNOOKER for m in moves[1])
    again = MR.run(pb, x0, betas, nsteps, seed, moves[1], dtype=np.longdouble) if snooker else None
    eng = _engine(use_sigma)
    kw = dict(adaptation_lag=adapt[0], adaptation_time=adapt[1]) if adapt else {}
    s = TemperedSampler(nwalkers, eng.ndim, eng, betas=betas, seed=seed, moves=moves[0], **kw)
    state = s.run_mcmc(x0, nsteps, adapt=bool(adapt))
    _compare(s, ref, nsteps, _bounds(snooker, ref, again))
    assert np.array_equal(state.coords, s.get_chain(temp=None)[-1])
    return s, ref


def test_de_with_odd_halves_and_a_prior_rung():
    """Complements of 5 (first half) and 6 (second half)."""
    s, ref = _against_restatement(False, 11, (1, .5, 0), 12, 7, DE)
    assert np.all(ref['kinds'] == MR.DE) and [type(m) for m, _ in s.moves] == [DEMove]


def test_snooker_on_four_rungs():
    _against_restatement(False, 10, (1, .6, .3, 0), 12, 7, SNOOKER)


def test_mixture_with_a_fitted_sigma():
    s, ref = _against_restatement(True, 13, (1, .5, 0), 16, 7, MIXTURE)
    for k in range(3):                                                   # every rung makes every kind at least once
        assert set(ref['kinds'][:, k]) == {MR.DE, MR.SNOOKER, MR.STRETCH}
    assert any(len(set(row)) > 1 for row in ref['kinds'])                # rungs of one step differ in kind


def test_mixture_on_one_rung():
    _against_restatement(False, 11, (1.,), 12, 7, MIXTURE)


def test_adapting_ladder_with_de():
    s, ref = _against_restatement(False, 11, (1, .5, .1, 0), 16, 7, DE, adapt=(10., 2.))
    assert not np.array_equal(ref['betas'], [1., .5, .1, 0.])            # the ladder moved
    np.testing.assert_allclose(s.get_betas(), ref['beta_history'], rtol=1e-12, atol=0.)
    np.testing.assert_allclose(s.betas, ref['betas'], rtol=1e-12, atol=0.)


# ---- another model: Arnett, three parameters ---------------------------------------------------------------------------
TRUTH = np.array([0.07, 12., -5.])
BOX_LO, BOX_HI = np.array([0.05, 9., -7.]), np.array([0.09, 15., -3.])


def _arnett():
    """(light curve, problem of the restatement, engine): the curve of tests/test_gpu_central.py."""
    if 'arnett' not in _cache:
        mjd = np.linspace(0., 90., 40)
        exact = np.array([C.truth('arnett', t - TRUTH[2], TRUTH[:1], TRUTH[1]) for t in mjd])
        lc = {'MJD': mjd, 'L_bol': exact * (1. + .02 * np.random.default_rng(11).standard_normal(40)), 'dL_bol': .02 * exact}
        priors = [M.UniformPrior(0.001, 1.), M.UniformPrior(2., 60.), M.UniformPrior(-30., -0.01)]
        pb = dict(t=lc['MJD'], y=lc['L_bol'], dy=lc['dL_bol'], priors=[p.descriptor() for p in priors])
        _cache['arnett'] = (lc, pb, priors, M.Arnett().engine_for(lc, priors=priors))
    return _cache['arnett']


def _arnett_restated(nwalkers, nsteps, seed, moves):
    key = ('arnett', nwalkers, nsteps, seed, tuple(moves))
    if key not in _cache:
        pb = _arnett()[1]
        x0 = BOX_LO + (BOX_HI - BOX_LO) * np.random.default_rng(seed).random((1, nwalkers, 3))
        _cache[key] = (x0, MR.run(pb, x0, (1.,), nsteps, seed, moves,
                                  log_like=lambda b: C.log_likelihood('arnett', pb['t'], pb['y'], pb['dy'], np.atleast_2d(b))))
    return _cache[key]


def _arnett_against_restatement(nwalkers, nsteps, seed, moves):
    """Under the tolerance tests/test_gpu_central.py takes for its own chain comparison (1e-9)."""
    x0, ref = _arnett_restated(nwalkers, nsteps, seed, moves[1])
    print(f'smallest accept margin of the restatement: {ref["move_margin"]:.3g}; moves accepted: {ref["nacc"].sum()}')
    assert ref['move_margin'] > 1e-6
    s = TemperedSampler(nwalkers, 3, _arnett()[3], betas=(1.,), seed=seed, moves=moves[0])
    s.run_mcmc(x0, nsteps)
    _compare(s, ref, nsteps, (1e-9, 1e-9))
    return ref


def test_model_independence_arnett_mixture():
    ref = _arnett_against_restatement(16, 20, 7, MIXTURE)
    assert set(ref['kinds'][:, 0]) == {MR.DE, MR.SNOOKER, MR.STRETCH}


@pytest.mark.parametrize('moves', [DE, SNOOKER], ids=['de', 'snooker'])
def test_smallest_ensemble_of_three_parameters(moves):
    """Six walkers: either colour holds exactly the three partners a snooker move draws."""
    ref = _arnett_against_restatement(6, 10, 7, moves)
    assert ref['nacc'].sum() > 0


# ---- the smallest legal ensembles: an engine of ONE parameter -----------------------------------------------------------
# A blackbody of fixed temperature consts[0] [kK] whose radius [1000 Rsun] is the parameter.
ONE_SOURCE = r'''
__device__ void lcf_user_state(double t_in, const double* p, const double* consts, double z,
                               double& T_kK, double& R_1000Rsun) {
    T_kK = consts[0];
    R_1000Rsun = p[0];
}
'''
ONE_T, ONE_R, ONE_BOX = 12., 2., (1.5, 2.5)


def one_parameter_problem():
    """The epochs and filters of ``small_problem()`` under that blackbody with 5 % noise, the radius uniform on (0.1, 10);
    ``log_like``: its restatement over the oracle's blackbody (models.py:116-136 for the Gaussian)."""
    if 'one_pb' not in _cache:
        sp = R.problem(False)
        npts = len(sp['t'])
        fit = lambda radii: O.blackbody_to_filters_batch(sp['bands'], np.full((npts, len(radii)), ONE_T),
                                                         np.tile(radii, (npts, 1)), 0.)
        ytrue = fit(np.array([ONE_R]))[:, 0]
        y, dy = ytrue * (1. + .05 * np.random.default_rng(21).standard_normal(npts)), .05 * ytrue

        def log_like(block):
            with np.errstate(all='ignore'):
                f = fit(np.atleast_2d(block)[:, 0])
                return -.5 * np.sum(np.log(2 * np.pi * dy[:, None] ** 2.) + ((y[:, None] - f) / dy[:, None]) ** 2., axis=0)
        _cache['one_pb'] = dict(t=sp['t'], names=sp['names'], y=y, dy=dy, priors=[(0, .1, 10., 0., 1.)], log_like=log_like)
    return _cache['one_pb']


def one_parameter_restated(nwalkers, nsteps, seed, moves):
    key = ('one', nwalkers, nsteps, seed, tuple(moves))
    if key not in _cache:
        pb = one_parameter_problem()
        x0 = ONE_BOX[0] + (ONE_BOX[1] - ONE_BOX[0]) * np.random.default_rng(seed).random((1, nwalkers, 1))
        _cache[key] = (x0, MR.run(pb, x0, (1.,), nsteps, seed, moves, log_like=pb['log_like']),
                       MR.run(pb, x0, (1.,), nsteps, seed, moves, log_like=pb['log_like'], dtype=np.longdouble))
    return _cache[key]


def _one_parameter_engine():
    if 'one_engine' not in _cache:
        pb = one_parameter_problem()
        model = M.CustomModel(ONE_SOURCE, ['R'], consts=[ONE_T], redshift=0.)
        _cache['one_engine'] = model.engine_for(lc_dict(pb['t'], pb['names'], pb['y'], pb['dy']), priors=[M.UniformPrior(.1, 10.)])
    return _cache['one_engine']


@pytest.mark.parametrize('nwalkers,moves', [(4, DE), (6, SNOOKER), (5, DE)], ids=['de-4', 'snooker-6', 'de-5'])
def test_smallest_legal_ensembles(nwalkers, moves):
    """DE with a complement of exactly 2 (and of 2 and 3), the snooker move with one of exactly 3."""
    x0, ref, again = one_parameter_restated(nwalkers, 12, 7, moves[1])
    print(f'smallest accept margin of the restatement: {ref["move_margin"]:.3g}; moves accepted: {ref["nacc"].sum()}')
    assert ref['move_margin'] > 1e-6 and ref['nacc'].sum() > 0
    s = TemperedSampler(nwalkers, 1, _one_parameter_engine(), betas=(1.,), seed=7, moves=moves[0])
    s.run_mcmc(x0, 12)
    _compare(s, ref, 12, _bounds(moves is SNOOKER, ref, again))


def test_one_walker_fewer_is_refused():
    eng = _one_parameter_engine()
    for nwalkers, move, needs in ((3, DEMove(), 4), (5, DESnookerMove(), 6)):
        with pytest.raises(ValueError, match=f'at least {needs} walkers'):
            TemperedSampler(nwalkers, 1, eng, betas=(1.,), moves=move)
        nt = NativeTempered(eng, (1.,), nwalkers)                           # (the handle itself is legal: stretch moves)
        with pytest.raises(LcfError, match=f'at least {needs} walkers') as exc:
            nt.set_moves([move.kind], [1.], [move.native_params(1)])
        assert exc.value.status == 1
        nt.set_moves([0], [1.], [[0., 0.]])
        nt.close()


# ---- the handle ---------------------------------------------------------------------------------------------------------
def test_argument_errors_of_set_moves_are_status_1_with_a_reason():
    nt = NativeTempered(_engine(), (1., .5), 10)
    ok = ([1, 2], [.8, 1.], [[1e-5, .75], [1.7, 0.]])
    nt.set_moves(*ok)
    for what, args in (('unknown kind', ([1, 3], ok[1], ok[2])), ('unknown kind', ([-1], [1.], [[0., 0.]])),
                       ('end at exactly 1', ([1, 2], [.8, .99], ok[2])), ('ascend', ([1, 2], [.8, .5], ok[2])),
                       ('ascend', ([1, 2], [0., 1.], ok[2])), ('ascend', ([1, 2], [np.nan, 1.], ok[2])),
                       ('ascend', ([1, 2], [.5, 1.5], ok[2])),
                       ('sigma', ([1], [1.], [[-1e-5, .75]])), ('sigma', ([1], [1.], [[np.inf, .75]])),
                       ('gamma0', ([1], [1.], [[1e-5, 0.]])), ('gamma0', ([1], [1.], [[1e-5, np.nan]])),
                       ('gammas', ([2], [1.], [[0., 0.]])), ('gammas', ([2], [1.], [[np.inf, 0.]])),
                       ('n_moves', ([0] * 9, list(np.linspace(.1, 1., 9)), [[0., 0.]] * 9))):
        with pytest.raises(LcfError, match=what) as exc:
            nt.set_moves(*args)
        assert exc.value.status == 1, what
    lib = nt._lib
    assert lib.lcf_tempered_set_moves(nt._h, 1, None, None, None) == 1 and b'null' in lib.lcf_last_error()
    assert lib.lcf_tempered_set_moves(None, 0, None, None, None) == 1
    assert lib.lcf_tempered_set_moves(nt._h, 0, None, None, None) == 0        # the default again: no pointers needed


def test_stretch_move_through_set_moves_is_the_default_sampler_bit_for_bit():
    pb, x0, _ = MR.cached_run(False, 11, (1, .5, 0), 12, 7, DE[1])
    eng = _engine()
    a = TemperedSampler(11, 5, eng, betas=(1, .5, 0), seed=7)
    b = TemperedSampler(11, 5, eng, betas=(1, .5, 0), seed=7, moves=StretchMove())
    a.run_mcmc(x0, 12)
    b.run_mcmc(x0, 12)
    assert np.array_equal(a.get_chain(temp=None), b.get_chain(temp=None)) and np.array_equal(a.get_log_like(), b.get_log_like())
    assert all(np.array_equal(p, q) for p, q in zip(a._tempered.counts(), b._tempered.counts()))
    assert np.all(a.get_move_kinds() == 0) and np.all(b.get_move_kinds() == 0) and a.get_move_kinds().shape == (12, 3)


def _all(s):
    return (s.get_chain(temp=None), s.get_log_like(), s.get_move_kinds()) + tuple(s._tempered.counts())


def test_continuation_is_bitwise():
    pb, x0, _ = MR.cached_run(True, 13, (1, .5, 0), 16, 7, MIXTURE[1])
    eng = _engine(True)
    a = TemperedSampler(13, 6, eng, betas=(1, .5, 0), seed=7, moves=MIXTURE[0])
    b = TemperedSampler(13, 6, eng, betas=(1, .5, 0), seed=7, moves=MIXTURE[0])
    sa = a.run_mcmc(x0, 16)
    b.run_mcmc(x0, 7)
    sb = b.run_mcmc(None, 9)
    assert b.iteration == 16
    for got, want in zip(_all(b), _all(a)):
        assert np.array_equal(got, want)
    assert np.array_equal(sa.coords, sb.coords) and np.array_equal(sa.log_prob, sb.log_prob)


def test_a_run_across_a_draw_block_is_bitwise():
    """300 steps against 200 + 100: the draws come in blocks of 256 steps at this size."""
    x0 = R.start(R.problem(False), 1, 11, 7)
    eng = _engine()
    a = TemperedSampler(11, 5, eng, betas=(1.,), seed=7, moves=MIXTURE[0])
    b = TemperedSampler(11, 5, eng, betas=(1.,), seed=7, moves=MIXTURE[0])
    a.run_mcmc(x0, 300)
    b.run_mcmc(x0, 200)
    b.run_mcmc(None, 100)
    for got, want in zip(_all(b), _all(a)):
        assert np.array_equal(got, want)
    kinds = a.get_move_kinds()[:, 0]
    cum = MR.cumulative(MIXTURE[1])
    want = np.array([m[0] for m in MIXTURE[1]])[MR.mixture_index(R.rung_seed(7, 0), np.arange(300), cum)]
    assert np.array_equal(kinds, want) and len(set(kinds[256:])) == 3       # ... beyond the block's edge too


def test_moves_changed_between_runs():
    """``set_moves`` changes the proposals from the next step on and nothing else: the first six steps are the DE run's,
    the next six are snooker moves from the state and the step number the DE steps left."""
    pb, x0, ref = MR.cached_run(False, 11, (1, .5, 0), 12, 7, DE[1])
    eng = _engine()
    s = TemperedSampler(11, 5, eng, betas=(1, .5, 0), seed=7, moves=DE[0])
    mid = s.run_mcmc(x0, 6)
    before = _all(s)
    state = s._tempered.get_state()
    s.set_moves(SNOOKER[0])
    assert [type(m) for m, _ in s.moves] == [DESnookerMove]
    for got, want in zip(_all(s), before):                                  # the chain and the counts stay
        assert np.array_equal(got, want)
    assert all(np.array_equal(p, q) for p, q in zip(s._tempered.get_state(), state))
    np.testing.assert_allclose(before[0], ref['chain'][:6], rtol=1e-12, atol=0.)
    assert np.array_equal(before[3], MR.run(pb, x0, (1, .5, 0), 6, 7, DE[1])['nacc'])
    s.run_mcmc(None, 6)
    assert s.iteration == 12 and np.array_equal(s.get_chain(temp=None)[:6], before[0])
    assert np.array_equal(s.get_move_kinds(), np.repeat([[MR.DE] * 3, [MR.SNOOKER] * 3], 6, axis=0))
    rest = MR.run(pb, mid.coords, (1, .5, 0), 6, 7, SNOOKER[1], first_step=6)
    again = MR.run(pb, mid.coords, (1, .5, 0), 6, 7, SNOOKER[1], first_step=6, dtype=np.longdouble)
    print(f'margins of the second leg: moves {rest["move_margin"]:.3g}, swaps {rest["swap_margin"]:.3g}')
    assert rest['move_margin'] > 1e-6 and rest['swap_margin'] > 1e-6
    bounds = _bounds(True, rest, again)
    assert np.array_equal(s._tempered.counts()[0] - before[3], rest['nacc'])
    np.testing.assert_allclose(s.get_chain(temp=None)[6:], rest['chain'], rtol=bounds[0], atol=0.)
    np.testing.assert_allclose(s.get_log_like()[6:], rest['lnL'], rtol=bounds[1], atol=0.)
    assert not np.array_equal(s.get_chain(temp=None)[6:], ref['chain'][6:])
    # back to the default: the kernels of a sampler that never had moves, and stretch moves in the record
    s.set_moves(None)
    s.run_mcmc(None, 2)
    assert np.all(s.get_move_kinds()[12:] == 0) and np.array_equal(s.get_move_kinds()[:12], np.repeat([[1] * 3, [2] * 3], 6, axis=0))
    s.reset()
    s.run_mcmc(None, 3)                                                     # a run that REPLACES rows moves once wrote
    assert s.get_move_kinds().shape == (3, 3) and np.all(s.get_move_kinds() == 0)


def test_lightcurve_mcmc_routes_moves_through_the_tempered_sampler():
    pb = R.problem(False)
    lc = lc_dict(pb['t'], pb['names'], pb['y'], pb['dy'])
    np.random.seed(4)
    s = lightcurve_mcmc(lc, M.ShockCooling(redshift=0.), priors=_priors(), p_lo=R.BOX_LO, p_up=R.BOX_HI, moves=DEMove(),
                        nwalkers=12, nsteps=5, nsteps_burnin=5, seed=11)
    assert isinstance(s, TemperedSampler) and s.ntemps == 1 and np.array_equal(s.betas, [1.])
    assert s.chain.shape == (12, 5, 5) and s.flatchain.shape == (60, 5) and np.all(np.isfinite(s.chain))
    assert [type(m) for m, _ in s.moves] == [DEMove] and np.all(s.get_move_kinds() == 1)
    assert s.acceptance_fraction.shape == (1, 12)
    t = lightcurve_mcmc(lc, M.ShockCooling(redshift=0.), priors=_priors(), p_lo=R.BOX_LO, p_up=R.BOX_HI, nwalkers=12, nsteps=5,
                        nsteps_burnin=5, seed=11, ntemps=3, Tmax=np.inf, moves=[(DEMove(), .8), (DESnookerMove(), .2)])
    assert t.ntemps == 3 and [w for _, w in t.moves] == [.8, .2] and set(np.unique(t.get_move_kinds())) <= {1, 2}
    s.close()
    t.close()
