"""Host side of the moves of ``TemperedSampler`` (``moves=``, ``lcf_tempered_set_moves``): the entry points are declared,
bound and exported; every ``ValueError`` of the interface is raised before the device is reached; the draw rules of the
NumPy restatement (tests/moves_reference.py) give what they promise; and the restated moves leave an analytic Gaussian
invariant -- while the same snooker move with a wrong exponent of its proposal factor does not.  No GPU.

Detailed balance, measured with the Philox draws (W = 12, one rung, 4000 steps, first fifth dropped, 20 batch means of
the per-step second moments of a 3-D correlated Gaussian; z = (mean - covariance diagonal) / batch-means standard error,
per dimension, seed 3):
  DE                               z = +0.58, +0.09, +0.16   (acceptance 0.32)
  snooker                          z = -2.04, +0.53, +1.48   (0.34)
  mixture 0.5 / 0.3 / 0.2          z = -0.31, -1.01, -1.56   (0.39)
  snooker, exponent ndim           z = +9.27, +9.86, +11.3   (0.30; must miss: some |z| > 5)
  snooker, exponent ndim - 2       z = -19.3, -27.4, -14.0   (0.41; must miss)
The correct rules stay within |z| = 2.1, the wrong exponents miss by 9 to 27: a wrong Jacobian is told from noise."""
import os
import re

import numpy as np
import pytest

import moves_reference as MR
import tempered_reference as R
from lightcurve_fitting_amd import engine as E, fitting as Fit, models as M, sampler as S
from lightcurve_fitting_amd.sampler import DEMove, DESnookerMove, StretchMove, TemperedSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# upper 1e-6 quantiles of chi-square (scipy.stats.chi2.isf(1e-6, df)) for df = 2, 11 and 23
CHI2_1E6 = {2: 27.631021115928547, 11: 48.86564276320364, 23: 70.54955713688595}


def test_symbols_are_declared_and_bound_and_the_abi_is_8():
    header = open(os.path.join(ROOT, 'include', 'lcf.h')).read()
    declared = set(re.findall(r'\b(lcf_[a-z_0-9]+)\s*\(', header))
    bound = {name: (res, args) for name, res, args in E.SIGNATURES}
    lib = E.load_library()
    for name in ('lcf_tempered_set_moves', 'lcf_tempered_get_move_history'):
        assert name in declared and name in bound and hasattr(lib, name)
    assert re.search(r'lcf_status lcf_tempered_set_moves\(lcf_tempered\* t, int32_t n_moves, const int32_t\* kinds, '
                     r'const double\* cum_weights,\s+const double\* params', header)
    assert len(bound['lcf_tempered_set_moves'][1]) == 5
    assert callable(E.NativeTempered.set_moves) and callable(E.NativeTempered.get_move_history)
    assert E.LCF_ABI_VERSION == 8 and lib.lcf_abi_version() == 8
    assert re.search(r'#define LCF_ABI_VERSION 8\b', header)
    assert len(dict(re.findall(r'(LCF_MODEL_\w+) = (\d+)', header))) == 11
    for name, value in (('LCF_MOVE_STRETCH', StretchMove.kind), ('LCF_MOVE_DE', DEMove.kind),
                        ('LCF_MOVE_SNOOKER', DESnookerMove.kind), ('LCF_MAX_MOVES', S.MAX_MOVES)):
        assert int(re.search(rf'#define {name} (\d+)', header).group(1)) == value
    assert (E.MOVE_STRETCH, E.MOVE_DE, E.MOVE_SNOOKER, E.MAX_MOVES) == (0, 1, 2, 8)


# ---- errors before the device ------------------------------------------------------------------------------------------
class _Engine:
    ndim, device = 5, 0
    priors = [p.descriptor() for p in [M.UniformPrior(0., 10.)] * 4 + [M.UniformPrior(-1., .5)]]


class _NoDevice:
    """Stands in for ``NativeTempered``: anything that would reach the device fails the test; ``set_moves`` among it
    unless the test allows it, and then it only records what it was given."""
    allow_set_moves = False

    def __init__(self, engine, betas, nwalkers, seed=0, a=2.):
        self.betas, self.given = np.array(betas, dtype=np.float64), []

    def _reached(self, *a, **k):
        raise AssertionError('the device was reached')

    set_state = run = run_adaptive = get_chain = mean_loglike = stepping_stones = get_state = counts = _reached
    get_move_history = _reached

    def set_moves(self, kinds, cum_weights, params):
        if not self.allow_set_moves:
            self._reached()
        self.given.append((list(kinds), np.array(cum_weights), np.array(params)))

    def get_betas(self):
        return self.betas.copy()

    def close(self):
        pass


class _NoMoves:
    """The stand-in of tests/test_adaptive_host.py: the constructor of ``NativeTempered`` and NO ``set_moves``."""

    def __init__(self, engine, betas, nwalkers, seed=0, a=2.):
        self.args = (engine, tuple(betas), nwalkers, seed, a)

    def close(self):
        pass


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(E, 'NativeTempered', _NoDevice)
    monkeypatch.setattr(E, 'load_library', _NoDevice._reached)
    monkeypatch.setattr(_NoDevice, 'allow_set_moves', False)


BAD_MOVES = [
    ('weights', [(DEMove(), 0.), (StretchMove(), 1.)]),
    ('weights', [(DEMove(), -1.), (StretchMove(), 2.)]),
    ('weights', [(DEMove(), np.nan)]),
    ('weights', [(DEMove(), np.inf), (StretchMove(), 1.)]),
    ('weights', [(DEMove(), 'much')]),
    ('not a move', ['DEMove']),
    ('not a move', [(DEMove, 1.)]),                       # the class, not a move
    ('not a move', [(DEMove(), 1., 2.)]),
    ('not a move', [None]),
    ('moves must be', 7),
    ('1 to 8 entries', []),
    ('1 to 8 entries', [DEMove()] * 9),
]


@pytest.mark.parametrize('what,moves', BAD_MOVES, ids=[f'{i}-{w.replace(" ", "_")}' for i, (w, _) in enumerate(BAD_MOVES)])
def test_bad_moves_are_refused_before_the_device(no_device, what, moves):
    with pytest.raises(ValueError, match=what):
        TemperedSampler(12, 5, _Engine(), betas=(1., .5), moves=moves)


def test_too_few_walkers_for_a_move_are_refused_before_the_device(no_device):
    class Small(_Engine):
        ndim, priors = 1, _Engine.priors[:1]
    for nwalkers, moves, ok in ((3, DEMove(), False), (4, DEMove(), True), (5, DESnookerMove(), False),
                                (6, DESnookerMove(), True), (5, [(StretchMove(), .5), (DESnookerMove(), .5)], False),
                                (5, [StretchMove(), DEMove()], True), (2, StretchMove(), True)):
        _NoDevice.allow_set_moves = ok
        if ok:
            TemperedSampler(nwalkers, 1, Small(), betas=(1.,), moves=moves)
        else:
            with pytest.raises(ValueError, match=f'at least {4 if isinstance(moves, DEMove) else 6} walkers'):
                TemperedSampler(nwalkers, 1, Small(), betas=(1.,), moves=moves)


def test_move_parameters_are_validated():
    for bad in (dict(sigma=-1e-5), dict(sigma=np.nan), dict(sigma=np.inf), dict(gamma0=0.), dict(gamma0=-1.),
                dict(gamma0=np.inf), dict(gamma0=np.nan)):
        with pytest.raises(ValueError, match='sigma|gamma0'):
            DEMove(**bad)
    for bad in (0., -1.7, np.inf, np.nan):
        with pytest.raises(ValueError, match='gammas'):
            DESnookerMove(gammas=bad)
    d, s = DEMove(), DESnookerMove()
    assert (d.sigma, d.gamma0, s.gammas) == (1e-5, None, 1.7)                 # emcee's defaults
    assert d.native_params(5) == (1e-5, 2.38 / np.sqrt(10.)) and DEMove(0., .5).native_params(5) == (0., .5)
    assert DEMove(sigma=0.).sigma == 0.


def test_moves_are_normalised_and_handed_to_the_native_handle(no_device):
    _NoDevice.allow_set_moves = True
    s = TemperedSampler(12, 5, _Engine(), betas=(1., .5), moves=[(DEMove(), 4.), (DESnookerMove(), 1.)])
    assert [type(m) for m, _ in s.moves] == [DEMove, DESnookerMove] and [w for _, w in s.moves] == [.8, .2]
    (kinds, cum, params), = s._tempered.given
    assert kinds == [1, 2] and np.array_equal(cum, [.8, 1.])
    assert np.array_equal(params, [[1e-5, 2.38 / np.sqrt(10.)], [1.7, 0.]])
    # thirds do not sum to one in floating point: the last cumulative weight is set, not computed
    s = TemperedSampler(12, 5, _Engine(), betas=(1.,), moves=[StretchMove(), DEMove(gamma0=1.), DESnookerMove(2.)])
    (kinds, cum, params), = s._tempered.given
    assert kinds == [0, 1, 2] and cum[-1] == 1. and np.allclose(cum, [1 / 3, 2 / 3, 1.], rtol=1e-15)
    assert np.array_equal(params, [[0., 0.], [1e-5, 1.], [2., 0.]])
    one = TemperedSampler(12, 5, _Engine(), betas=(1.,), moves=DEMove())                  # a single move
    assert one._tempered.given[0][0] == [1] and np.array_equal(one._tempered.given[0][1], [1.])
    one.set_moves([(StretchMove(), 1.), (DEMove(), 3.)])
    assert [w for _, w in one.moves] == [.25, .75] and one._tempered.given[1][0] == [0, 1]
    with pytest.raises(ValueError, match='weights'):
        one.set_moves([(DEMove(), -1.)])
    assert [w for _, w in one.moves] == [.25, .75] and len(one._tempered.given) == 2     # a refused list changes nothing
    one.set_moves(None)
    assert one._tempered.given[2][0] == [] and isinstance(one.moves[0][0], StretchMove)


def test_without_moves_the_native_handle_is_made_as_ever_and_set_moves_is_never_called(monkeypatch):
    monkeypatch.setattr(E, 'NativeTempered', _NoMoves)
    s = TemperedSampler(12, 5, _Engine(), betas=(1., .5), seed=3, a=2.5)
    assert s._tempered.args[1:] == ((1., .5), 12, 3, 2.5) and not hasattr(s._tempered, 'set_moves')
    assert len(s.moves) == 1 and isinstance(s.moves[0][0], StretchMove) and s.moves[0][1] == 1.
    monkeypatch.setattr(E, 'NativeTempered', _NoDevice)
    monkeypatch.setattr(_NoDevice, 'allow_set_moves', False)
    TemperedSampler(12, 5, _Engine(), betas=(1., .5), moves=None)


def test_lightcurve_mcmc_passes_moves_on_only_when_given(monkeypatch):
    seen = []

    class Stop(Exception):
        pass

    def sampler(*a, **k):
        seen.append(k)
        raise Stop
    monkeypatch.setattr(Fit, '_prepare_photometry', lambda lc, model: None)
    monkeypatch.setattr(M.ShockCooling, 'engine_for', lambda self, lc, **k: _Engine())
    monkeypatch.setattr(S, 'TemperedSampler', sampler)
    monkeypatch.setattr(Fit, 'EnsembleSampler', sampler)
    kw = dict(p_lo=np.zeros(5), p_up=np.ones(5), nwalkers=12, seed=1)
    move = DEMove()
    with pytest.raises(Stop):
        Fit.lightcurve_mcmc({}, M.ShockCooling(redshift=0.), moves=move, **kw)
    assert seen[-1]['moves'] is move and seen[-1]['betas'] == [1.] and seen[-1]['ntemps'] is None   # one rung at beta = 1
    with pytest.raises(Stop):
        Fit.lightcurve_mcmc({}, M.ShockCooling(redshift=0.), moves=move, ntemps=3, **kw)
    assert seen[-1]['moves'] is move and seen[-1]['betas'] is None and seen[-1]['ntemps'] == 3
    with pytest.raises(Stop):
        Fit.lightcurve_mcmc({}, M.ShockCooling(redshift=0.), ntemps=3, **kw)
    assert 'moves' not in seen[-1] and seen[-1]['ntemps'] == 3
    with pytest.raises(Stop):
        Fit.lightcurve_mcmc({}, M.ShockCooling(redshift=0.), **kw)                 # the ensemble sampler, as ever
    assert 'moves' not in seen[-1] and 'ntemps' not in seen[-1]
    import inspect
    assert 'moves' not in inspect.signature(S.EnsembleSampler.__init__).parameters
    assert 'moves' not in inspect.signature(S.PopulationSampler.__init__).parameters
    assert 'moves' in Fit.lightcurve_mcmc.__doc__


# ---- the draw rules of the restatement ---------------------------------------------------------------------------------
SEED = 20260


def _chi2(counts, expected):
    return float(np.sum((counts - expected) ** 2 / expected))


def test_de_partners_are_distinct_and_every_ordered_pair_is_drawn_evenly():
    n, wid = 4, np.arange(8)
    counts = np.zeros((n, n))
    for step in range(1500):
        for half in (0, 1):
            ua, ub, _, _ = MR.uniforms(SEED, step, half, wid)
            j1, j2 = MR.de_partners(ua, ub, n)
            assert np.all(j1 != j2) and np.all((0 <= j1) & (j1 < n) & (0 <= j2) & (j2 < n))
            np.add.at(counts, (j1, j2), 1)
    off = ~np.eye(n, dtype=bool)
    assert np.all(counts[off] > 0) and np.all(counts[~off] == 0)
    stat = _chi2(counts[off], counts.sum() / 12.)
    print(f'ordered pairs: chi-square {stat:.1f} on 11 degrees of freedom (bound {CHI2_1E6[11]:.1f})')
    assert stat < CHI2_1E6[11]
    for n in (2, 3, 5, 6):                                 # the complements of the GPU cases, and the smallest
        ua, ub, _, _ = MR.uniforms(SEED + 1, 0, 0, np.arange(400))
        j1, j2 = MR.de_partners(ua, ub, n)
        assert np.all(j1 != j2) and j1.min() == 0 and j2.min() == 0 and j1.max() == n - 1 and j2.max() == n - 1
    edge = np.array([np.nextafter(1., 0.)])                # the largest uniform stays inside the complement
    assert MR.de_partners(edge, edge, 5) == (4, 3) and MR.snooker_partners(edge, edge, edge, 5)[2] == 2


def test_snooker_partners_are_distinct_and_every_ordered_triple_is_drawn_evenly():
    n, wid = 4, np.arange(8)
    counts = np.zeros((n, n, n))
    for step in range(1500):
        for half in (0, 1):
            ua, ub, uc, _ = MR.uniforms(SEED, step, half, wid)
            j0, j1, j2 = MR.snooker_partners(ua, ub, uc, n)
            assert np.all((j0 != j1) & (j0 != j2) & (j1 != j2)) and np.all((0 <= j2) & (j2 < n))
            np.add.at(counts, (j0, j1, j2), 1)
    i, j, k = np.indices((n, n, n))
    distinct = (i != j) & (i != k) & (j != k)
    assert distinct.sum() == 24 and np.all(counts[distinct] > 0) and np.all(counts[~distinct] == 0)
    stat = _chi2(counts[distinct], counts.sum() / 24.)
    print(f'ordered triples: chi-square {stat:.1f} on 23 degrees of freedom (bound {CHI2_1E6[23]:.1f})')
    assert stat < CHI2_1E6[23]
    ua, ub, uc, _ = MR.uniforms(SEED + 1, 0, 0, np.arange(400))
    j0, j1, j2 = MR.snooker_partners(ua, ub, uc, 3)        # the smallest complement: a permutation of (0, 1, 2)
    assert np.all(np.sort(np.stack([j0, j1, j2]), axis=0) == np.arange(3)[:, None])


def test_mixture_frequencies_follow_the_weights_and_a_step_has_one_kind_per_rung():
    moves = [MR.de(.5), MR.snooker(.3), MR.stretch(.2)]
    cum = MR.cumulative(moves)
    assert np.allclose(cum, [.5, .8, 1.]) and cum[-1] == 1.
    steps, K = np.arange(6000), 3
    idx = np.stack([MR.mixture_index(R.rung_seed(SEED, k), steps, cum) for k in range(K)], axis=1)
    counts = np.bincount(idx.ravel(), minlength=3)
    stat = _chi2(counts, np.array([.5, .3, .2]) * idx.size)
    print(f'mixture: counts {counts} of {idx.size}; chi-square {stat:.2f} on 2 degrees of freedom')
    assert stat < CHI2_1E6[2]
    assert np.any(idx[:, 0] != idx[:, 1]) and np.any(idx[:, 1] != idx[:, 2])       # rungs of one step may differ
    assert MR.mixture_index(R.rung_seed(SEED, 1), 17, cum) == idx[17, 1]           # (scalars as arrays)
    # ... and both halves of a step never do: a run's proposals of either half are the recorded kind's
    pb = R.problem(False)
    x0 = R.start(pb, 2, 12, 5)
    ref = MR.run(pb, x0, (1., .5), 6, 5, moves)
    assert ref['kinds'].shape == (6, 2)
    table = np.array([m[0] for m in moves])
    want = np.stack([table[MR.mixture_index(R.rung_seed(5, k), np.arange(6), cum)] for k in range(2)], axis=1)
    assert np.array_equal(ref['kinds'], want)
    seen = []
    real = MR.propose

    def spy(move, x, act, oth, rseed, step, half, *a, **k):
        seen.append((rseed, step, half, move[0]))
        return real(move, x, act, oth, rseed, step, half, *a, **k)
    MR.propose = spy
    try:
        MR.run(pb, x0, (1., .5), 6, 5, moves)
    finally:
        MR.propose = real
    kinds = {(r, s): set() for r, s, _, _ in seen}
    for r, s, h, kind in seen:
        kinds[(r, s)].add(kind)
    assert len(seen) == 6 * 2 * 2 and all(len(v) == 1 for v in kinds.values())


def test_stretch_steps_are_the_tempered_restatement_bit_for_bit():
    pb = R.problem(False)
    x0 = R.start(pb, 3, 11, 7)
    want = R.run(pb, x0, (1, .5, 0), 8, 7)
    for moves in (None, [MR.stretch()], [MR.stretch(.4), MR.stretch(.6)]):
        got = MR.run(pb, x0, (1, .5, 0), 8, 7, moves)
        for key, value in want.items():
            assert np.array_equal(got[key], value), key
        assert np.all(got['kinds'] == MR.STRETCH)


def test_a_snooker_proposal_from_its_own_partner_is_never_accepted():
    x = np.array([[0., 0.], [1., 0.], [0., 1.], [1., 1.], [0., 0.], [2., 2.], [3., 1.], [1., 3.]])   # walker 4 = walker 0
    act, oth = np.array([4, 5, 6, 7]), np.array([0, 1, 2, 3])
    dead_seen = 0
    for step in range(40):
        q, fac, _, dead = MR.propose(MR.snooker(), x, act, oth, SEED, step, 1)
        ua, ub, uc, _ = MR.uniforms(SEED, step, 1, act)
        j0 = MR.snooker_partners(ua, ub, uc, 4)[0]
        assert np.array_equal(dead, (act == 4) & (j0 == 0))
        assert np.array_equal(q[dead], x[act][dead]) and np.all(fac[dead] == 0.) and np.all(np.isfinite(fac))
        dead_seen += int(dead.sum())
    assert dead_seen > 0


# ---- detailed balance --------------------------------------------------------------------------------------------------
COV = np.array([[1., .9, -.3], [.9, 1.5, .2], [-.3, .2, .7]])
_PREC = np.linalg.inv(COV)


def _gauss_z(moves, snooker_exponent=None, seed=3, nwalkers=12, nsteps=4000, batches=20):
    """z-scores of the chain's second moments against the covariance diagonal (see the module docstring)."""
    rng = np.random.default_rng(seed)
    x0 = rng.multivariate_normal(np.zeros(3), COV, size=(1, nwalkers))
    run = MR.run(None, x0, (1.,), nsteps, seed, moves, snooker_exponent=snooker_exponent,
                 log_like=lambda b: -.5 * np.einsum('ni,ij,nj->n', b, _PREC, b), log_prior=lambda b: np.zeros(len(b)))
    m2 = np.mean(run['chain'][nsteps // 5:, 0] ** 2, axis=1)           # (steps kept, 3)
    means = m2.reshape(batches, -1, 3).mean(axis=1)
    z = (means.mean(axis=0) - np.diag(COV)) / (means.std(axis=0, ddof=1) / np.sqrt(batches))
    print(f'acceptance {run["nacc"].sum() / (nsteps * nwalkers):.2f}; z = {np.array2string(z, precision=3)}')
    return z


MIXTURE = [MR.de(.5), MR.snooker(.3), MR.stretch(.2)]


@pytest.mark.parametrize('name,moves', [('de', [MR.de()]), ('snooker', [MR.snooker()]), ('mixture', MIXTURE)])
def test_the_moves_leave_a_gaussian_invariant(name, moves):
    assert np.all(np.abs(_gauss_z(moves)) < 5.)


@pytest.mark.parametrize('exponent', [3., 1.], ids=['ndim', 'ndim-2'])
def test_a_wrong_snooker_exponent_is_found_out(exponent):
    assert np.max(np.abs(_gauss_z([MR.snooker()], snooker_exponent=exponent))) > 5.
