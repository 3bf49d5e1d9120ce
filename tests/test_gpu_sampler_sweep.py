"""Every model and light-curve shape through every sampler kernel: the cases of tests/sampler_cases.py -- the companion
models with time shifts and viewing angle, n = 3 / RW constants, absolute sigma, log-uniform and Gaussian priors, ragged
shared epochs, one epoch, 1-8 parts, the Swift white filter, the band-sum levels -- through k_solo_run, k_solo, k_fused
and the separate launches, through the population kernels, between two emulated ranks, and under the process-wide
switches the README documents.  The bounds are the sampler tests' two: relative 1e-9 against the oracle-driven chain with
equal acceptance counts, and bit-for-bit equality between the kernel forms of one run.  Every run also says which
template instance it was launched with (``last_run_instance``), held against the table; the last test of the module asks
that every row of the instantiation table was executed by the tests before it (it needs the whole module)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sampler_cases as S
from conftest import relerr
from lightcurve_fitting_amd.sampler import EnsembleSampler, PopulationSampler

pytestmark = pytest.mark.gpu

ENV = ('LCF_PARTS', 'LCF_RUN_GRID', 'LCF_RUN_ANY_SIZE', 'LCF_NO_POP_RUN', 'LCF_NO_POP', 'LCF_DRAW_BLOCK', 'LCF_NO_RUN_KERNEL',
       'LCF_ROWS_PER_HALF_STEP', 'LCF_POP_ITAB_LDS', 'LCF_SHARED_EPOCHS_ONLY')
STATE = ('chain', 'lp', 'nacc', 'x', 'lp_end')

_SEEN = set()     # (kernel, instance) of every run of the module
_AUTO = {}        # case -> its 'auto' run on one GPU: the chain every other form of the case must reproduce


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _auto(case):
    if case.id not in _AUTO:
        _AUTO[case.id] = S.run_single(case, 'auto')
    return _AUTO[case.id]


def _saw(run):
    _SEEN.add((run['kernel'], tuple(run['instance'])))
    return run['kernel'], tuple(run['instance'])


@pytest.mark.parametrize('cid', sorted(S.CASES))
def test_single_gpu_forms_are_one_chain_and_the_oracles(cid):
    case = S.CASES[cid]
    eng = S.make_engine(case)
    runs = {'auto': _auto(case)}
    runs.update({form: S.run_single(case, form, eng) for form in S.FORMS if form != 'auto'})
    kernel, nd, np_, m = case.expect
    for form, run in runs.items():
        assert _saw(run) == S.dispatch(case, form), (case, form)
    assert _saw(runs['auto']) == (kernel, (nd, np_, m, 0 if nd >= 0 else -1)), case
    for form, run in runs.items():     # after the first run and after the continuation
        for key in STATE + ('mid_x', 'mid_lp', 'mid_nacc'):
            assert np.array_equal(run[key], runs['auto'][key]), (case, form, key)
    ref, ref_lp, ref_acc, _, ref_acc_first = S.oracle_chain(case)
    got = runs['auto']
    print(f'case {cid}: chain {relerr(got["chain"], ref):.2e}, log-prob {relerr(got["lp"], ref_lp):.2e} of the oracle\'s; '
          f'{ref_acc.sum()} of {case.nwalkers * sum(S.STEPS)} moves accepted')
    assert relerr(got['chain'], ref) < 1e-9 and relerr(got['lp'], ref_lp) < 1e-9, case
    assert np.array_equal(got['nacc'], ref_acc) and np.array_equal(got['mid_nacc'], ref_acc_first), case
    assert np.array_equal(got['x'], got['chain'][-1]) and np.array_equal(got['lp_end'], got['lp'][-1])
    assert np.array_equal(got['mid_x'], got['chain'][S.STEPS[0] - 1])


_POP_REFS = {}


def _population_references(pop_id):
    """Per transient: its solo run and its oracle chain (once per population)."""
    if pop_id not in _POP_REFS:
        nw, cases, _ = S.POPULATIONS[pop_id]
        refs = []
        for k, cid in enumerate(cases):
            case = S.CASES[cid]
            solo = EnsembleSampler(nw, case.ndim, S.make_engine(case, nw), seed=S.POP_SEED + k)
            solo.run_mcmc(S.host(case, nw)['x0'], S.STEPS[0])
            solo.run_mcmc(None, S.STEPS[1])
            refs.append(((solo.get_chain(), solo.get_log_prob(), solo.acceptance_fraction),
                         S.oracle_chain(case, nw, S.POP_SEED + k)))
        _POP_REFS[pop_id] = refs
    return _POP_REFS[pop_id]


@pytest.mark.parametrize('form', list(S.POP_FORMS))
@pytest.mark.parametrize('pop_id', sorted(S.POPULATIONS))
def test_populations_equal_solo_runs_and_the_oracle(pop_id, form, monkeypatch):
    nw, cases, (run_instance, pop_instance) = S.POPULATIONS[pop_id]
    refs = _population_references(pop_id)
    for name, value in S.POP_FORMS[form].items():
        monkeypatch.setenv(name, value)
    problems, x0 = [], {}
    for k, cid in enumerate(cases):
        case = S.CASES[cid]
        h = S.host(case, nw)
        model, lc = S.make_model(case, h)
        problems.append((model, lc, case.priors) + ((S.engine_keywords(case),) if case.sigma else ()))
        x0[k] = h['x0']
    pop = PopulationSampler(problems, nw, seed=S.POP_SEED)
    pop.run_mcmc(x0, S.STEPS[0])
    pop.run_mcmc(None, S.STEPS[1])
    got = (pop[0]._native.last_run_kernel(), pop[0]._native.last_run_instance())
    _SEEN.add(got)
    want = {'population-run': run_instance, 'population': pop_instance, 'population-phases': S.NONE}[form]
    assert got == (form, want) == S.population_dispatch(cases, form), (pop_id, form)
    n = sum(S.STEPS)
    for k, ((chain, lp, acc), (ref, ref_lp, ref_acc, _, _)) in enumerate(refs):
        got = (pop[k].get_chain(), pop[k].get_log_prob(), pop[k].acceptance_fraction)
        assert got[0].shape == (n, nw, S.CASES[cases[k]].ndim)
        assert np.array_equal(got[0], chain), (pop_id, form, k)
        np.testing.assert_allclose(got[1], lp, rtol=1e-12, atol=1e-9, err_msg=f'{pop_id} {form} {k}')
        assert np.array_equal(got[2], acc), (pop_id, form, k)
        assert relerr(got[0], ref) < 1e-9 and relerr(got[1], ref_lp) < 1e-9, (pop_id, form, k)
        assert np.array_equal(np.round(got[2] * n).astype(int), ref_acc), (pop_id, form, k)
        assert 0.1 * nw * n < ref_acc.sum() < 0.9 * nw * n, (pop_id, k, ref_acc.sum())


@pytest.mark.parametrize('form', ['resident', 'per half-step'])
@pytest.mark.parametrize('cid', list(S.RANK_CASES))
def test_row_boards_two_emulated_ranks(cid, form):
    """Two emulated ranks of a row-board run on one GPU, resident and per half-step: every rank's chain, counts and state
    equal the single-GPU run bit for bit (waits between ranks are bounded by LCF_PEER_WAIT_S: a stuck rank is an
    LcfError)."""
    case = S.CASES[cid]
    env, resident, per_half_step = S.RANK_CASES[cid]
    want = _auto(case)     # (first: the single-GPU run of the case, with nothing of `env` set)
    runs = S.run_ranks(case, form, env)
    for run in runs:
        assert _saw(run) == (('run', resident) if form == 'resident' else ('solo', per_half_step)), (case, form)
        for key in STATE:
            assert np.array_equal(run[key], want[key]), (case, form, key)


@pytest.mark.parametrize('switch', list(S.SWITCHES))
def test_process_wide_switches(switch):
    """The switches that are read once per process, each in a child process of its own: the chains' digests are the
    parent's, the kernels and instances what the switch asks for."""
    env, runs = S.SWITCHES[switch]
    want = {cid: S.digest(_auto(S.CASES[cid])) for cid, _, _ in runs}
    child_env = {k: v for k, v in os.environ.items() if k not in ENV}
    child_env.update(env)
    out = subprocess.run([sys.executable, os.path.abspath(S.__file__)] + [f'{cid}:{form}' for cid, form, _ in runs],
                         env=child_env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert [(ln['case'], ln['form']) for ln in lines] == [(cid, form) for cid, form, _ in runs]
    _SEEN.update((ln['kernel'], tuple(ln['instance'])) for ln in lines)
    for ln, (cid, form, (kernel, instance)) in zip(lines, runs):
        assert (ln['kernel'], tuple(ln['instance'])) == (kernel, instance), (switch, cid, form)
        assert ln['digest'] == want[cid], (switch, cid, form)


def test_every_instance_ran():
    """Every row of SpecialisedModels x {NP 2, 4} (k_solo and k_solo_run), of WideRuns and of RanksRuns, the generic rank
    kernel at NP 2 and 4 and k_solo's board form at the generic dimensions 5, 6 and 7 were executed by the tests above."""
    missing = [row for row in S.REQUIRED if row not in _SEEN]
    assert not missing, (missing, sorted(_SEEN))
