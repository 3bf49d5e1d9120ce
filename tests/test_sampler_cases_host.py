"""The case table of the sampler sweep (tests/sampler_cases.py), checked on the reference alone -- no GPU: the oracle
chain of every case is free of NaN and +inf, decides in both directions, excludes proposals where the case says so; the
light curve has the shape its name says; and every kernel instance the tables expect is what the dispatch rules of
csrc/lcf_hip.hip, restated in ``sampler_cases.dispatch``, give for that shape."""
import numpy as np
import pytest

import sampler_cases as S
from lightcurve_fitting_amd.filters import PackedTables

CASE_IDS = sorted(S.CASES)


def _check_chain(case, nwalkers=None, seed=None):
    chain, lp, acc, proposals, _ = S.oracle_chain(case, nwalkers, seed)
    nw, n = nwalkers or case.nwalkers, sum(S.STEPS)
    assert chain.shape == (n, nw, case.ndim) and np.all(np.isfinite(chain))
    assert np.all(np.isfinite(lp)), 'a walker without a finite log-probability'
    assert not np.any(np.isnan(proposals)) and not np.any(proposals == np.inf)
    # the accept test decides in both directions, so a wrong (n_dim - 1) ln z or z would move the chain
    assert 0.1 * nw * n < acc.sum() < 0.9 * nw * n, (case, acc.sum(), nw * n)
    return proposals


@pytest.mark.parametrize('cid', CASE_IDS)
def test_oracle_chain_of_the_case(cid):
    case = S.CASES[cid]
    h = S.host(case)
    assert np.all(np.isfinite(S.oracle_log_posterior(h['pb'])(h['x0'])))   # a finite start for every walker
    t_exp = 0 if case.companion else (3 if case.kind == 'ShockCooling2' else 6 if case.kind == 'ShockCooling3' else 4)
    assert case.priors[t_exp].p_max < h['t'].min()            # the explosion stays in front of the first epoch
    proposals = _check_chain(case)
    if case.excluded:
        assert np.any(proposals == -np.inf), 'no proposal of the run was excluded by the prior'


def test_the_table_has_odd_and_even_ensembles_and_the_issue_sizes():
    sizes = [c.nwalkers for c in S.CASES.values()]
    assert any(n % 2 for n in sizes) and any(n % 2 == 0 for n in sizes)
    for c in S.CASES.values():
        sh = S.engine_shape(c)
        assert 3 <= sh['n_filters'] <= 7 and (c.shape == 'single' or 12 <= c.n_epochs <= 40), c


@pytest.mark.parametrize('cid', CASE_IDS)
def test_shape_is_what_its_name_says(cid):
    case = S.CASES[cid]
    sh = S.engine_shape(case)
    counts, names, t = sh['counts'], np.array(sh['names']), sh['t']
    if case.shape == 'ragged':
        per_epoch = [list(names[t == te]) for te in np.unique(t)]
        assert any(len(set(ep)) < len(ep) for ep in per_epoch), 'no epoch with a repeated filter'
        assert counts.max() > 2 * counts.mean() and counts.max() > sh['em_k'], 'no epoch of several columns'
        assert any(len(set(ep)) < sh['n_filters'] for ep in per_epoch) and not sh['em_dense']
        assert sh['n_cols'] > sh['n_epochs']
    elif case.shape == 'single':
        assert sh['n_epochs'] == 1 and sh['n_points'] == 4 and sh['n_cols'] == 1 and sh['n_parts'] == 1
    elif case.shape == 'unshared':
        assert sh['n_epochs'] == sh['n_points'] and not sh['em_dense']
    else:
        assert case.shape == 'dense' and sh['em_dense'] and sh['n_points'] == sh['n_epochs'] * sh['n_filters']
    if case.parts is not None:
        assert sh['n_parts'] == case.parts, 'LCF_PARTS does not give that many parts for this light curve'
    else:
        assert sh['n_parts'] == 1     # (at most 64 columns)
    if 'white' in case.filters:
        for z in (0., 0.3, 0.7, case.z):
            tmin = PackedTables(sh['filters'], z).interpolants()[1]
            assert [f for f, tm in zip(sh['filters'], tmin) if np.isinf(tm)] == ['white']
        assert not sh['itab_uniform']
    else:
        assert sh['itab_uniform'] == (case.kind != 'ShockCooling3')
    assert sh['tab_in_lds']


@pytest.mark.parametrize('cid', CASE_IDS)
def test_expected_instances_follow_the_dispatch_rules(cid):
    case = S.CASES[cid]
    kernel, nd, np_, m = case.expect
    assert S.dispatch(case, 'auto') == S.dispatch(case, 'grid') == (kernel, (nd, np_, m, 0 if nd >= 0 else -1))
    if kernel in ('run', 'solo'):
        assert S.dispatch(case, 'solo') == ('solo', (nd, np_, m, 0))
        assert S.dispatch(case, 'fused') == ('fused', S.NONE)
    else:
        assert case.variant == 0 and S.dispatch(case, 'solo') == S.dispatch(case, 'fused') == ('fused', S.NONE)
    assert S.dispatch(case, 'phases') == ('phases', S.NONE)


def test_rank_switch_and_population_expectations_follow_the_dispatch_rules():
    for cid, (env, resident, per_half_step) in S.RANK_CASES.items():
        case = S.CASES[cid]
        assert ((case.nwalkers + 1) // 2) % 2 == 0, 'the slots of a half-step must divide over two ranks'
        assert S.dispatch(case, 'auto', switches=tuple(env), ranks=2) == ('run', resident), cid
        assert S.dispatch(case, 'solo', switches=tuple(env), ranks=2) == ('solo', per_half_step), cid
    for name, (env, runs) in S.SWITCHES.items():
        for cid, form, want in runs:
            assert S.dispatch(S.CASES[cid], form, switches=tuple(env)) == want, (name, cid)
    for pop_id, (nw, cases, (run, pop)) in S.POPULATIONS.items():
        assert S.population_dispatch(cases, 'population-run') == ('population-run', run), pop_id
        assert S.population_dispatch(cases, 'population') == ('population', pop), pop_id
        assert S.population_dispatch(cases, 'population-phases') == ('population-phases', S.NONE), pop_id
        assert nw >= 2 * max(S.CASES[c].ndim for c in cases)


def test_every_required_instance_is_expected_somewhere():
    """The rows the sweep's last test asks for are rows some run of the tables is expected to launch."""
    seen = set()
    for case in S.CASES.values():
        for form in S.FORMS:
            seen.add(S.dispatch(case, form))
    for cid, (env, resident, per_half_step) in S.RANK_CASES.items():
        seen |= {('run', resident), ('solo', per_half_step)}
    for env, runs in S.SWITCHES.values():
        seen |= {want for _, _, want in runs}
    assert not [r for r in S.REQUIRED if r not in seen]


@pytest.mark.parametrize('pop_id', sorted(S.POPULATIONS))
def test_oracle_chains_of_the_populations(pop_id):
    nw, cases, _ = S.POPULATIONS[pop_id]
    for k, cid in enumerate(cases):
        _check_chain(S.CASES[cid], nw, S.POP_SEED + k)
