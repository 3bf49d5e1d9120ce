"""The layout ``lcf_engine_create`` plans -- point order, columns, parts, table placement -- read back from the library
without a device (``lcf_debug_engine_layout``: the plan of csrc/lcf_plan.h as the engine would upload it), held against
the restatement of the rules in ``sampler_cases.engine_shape`` for every case of the sweep and against shapes written
out here.  (tools/native/plan_check.cpp checks the layout's invariants over a few hundred generated problems.)"""
import numpy as np
import pytest

import sampler_cases as S
from lightcurve_fitting_amd import engine as E, models as M


@pytest.mark.parametrize('cid', sorted(S.CASES))
def test_case_layout_is_the_restated_shape(cid):
    case = S.CASES[cid]
    shape, real = S.engine_shape(case), S.engine_layout(case)
    assert real['use_therm'] == 1                    # (every case of the sweep is epoch-major: engine_shape assumes it)
    # (the filters are no integer of the layout: the descriptors staged with the tables count them, four entries each)
    n_filters, rest = divmod(real['stage_d2'] - real['n_lds_tab'] - real['n_itab_lds'] // 2 - real['n_spl_lds'] // 2, 4)
    assert rest == 0
    got = dict(n_points=real['n_points'], n_filters=n_filters, n_epochs=real['n_epochs'], em_k=real['em_k'],
               n_cols=real['em_cols'], em_dense=bool(real['em_dense']), n_parts=real['n_parts'],
               tab_in_lds=bool(real['tab_in_lds']), itab_uniform=bool(real['itab_uniform']))
    assert got == {k: shape[k] for k in got}
    n = real['n_parts']
    assert real['part_start'][:n] == shape['start'] and real['part_start'][n:] == [shape['n_points']] * (9 - n)
    assert real['part_col0'][0] == 0 and real['part_col0'][n:] == [shape['n_cols']] * (9 - n)


def _layout(t, names, **env):
    """The layout of a ShockCooling engine on these times and filters."""
    t = np.asarray(t, dtype=float)
    with S.planned_engines() as layouts, S.environment(**env):
        M.ShockCooling(redshift=0.).make_engine(t, list(names), np.full(len(t), 1e20), np.full(len(t), 1e18))
    return layouts[0]


def _scalars(layout, *names):
    return tuple(layout[n] for n in names)


def test_benchmark_shape():
    """500 epochs in 6 filters, dense: a column an epoch, two parts of 250 columns."""
    lo = _layout(np.repeat(1. + 0.05 * np.arange(500), 6), list('UBVgri') * 500)
    assert _scalars(lo, 'n_points', 'n_epochs', 'use_therm', 'em_k', 'em_cols', 'em_dense', 'n_parts') == \
        (3000, 500, 1, 6, 500, 1, 2)
    assert lo['part_start'] == [0, 1500] + [3000] * 7
    assert lo['part_col0'] == [0, 250] + [500] * 7
    assert lo['part_ep0'] == [0, 250] + [500] * 7
    assert _scalars(lo, 'n_chunks', 'cpb', 'tab_in_lds') == (12, 6, 1)


SINGLE_T, SINGLE_NAMES = 1. + 0.01 * np.arange(3000), list('UBVgri') * 500


def test_single_point_epochs_take_two_rounds():
    """3000 epochs of one point: 3000 columns are more than 8 x 256, so a part's lanes make two rounds -- 6 parts of 500."""
    lo = _layout(SINGLE_T, SINGLE_NAMES)
    assert _scalars(lo, 'n_points', 'n_epochs', 'use_therm', 'em_k', 'em_cols', 'em_dense', 'n_parts') == \
        (3000, 3000, 1, 1, 3000, 0, 6)
    bounds = [0, 500, 1000, 1500, 2000, 2500, 3000, 3000, 3000]
    assert lo['part_start'] == bounds and lo['part_col0'] == bounds and lo['part_ep0'] == bounds


def test_shared_epochs_only_puts_single_point_epochs_on_the_points_path():
    lo = _layout(SINGLE_T, SINGLE_NAMES, LCF_SHARED_EPOCHS_ONLY='1')
    assert _scalars(lo, 'n_points', 'n_epochs', 'use_therm', 'em_cols', 'n_parts', 'n_chunks', 'cpb', 'use_itab') == \
        (3000, 3000, 0, 0, 2, 12, 6, 0)
    assert lo['part_start'] == [0, 1500] + [3000] * 7
    assert lo['part_col0'] == [0] * 9
    assert lo['part_ep0'] == [0, 1500] + [3000] * 7


def test_a_nan_time_makes_every_point_its_own_epoch():
    """No order to sort by: the epochs are the points in the caller's order, nothing is epoch-major, no part names a first
    epoch."""
    t = np.repeat(1. + 0.05 * np.arange(100), 6)
    t[77] = np.nan
    lo = _layout(t, list('UBVgri') * 100)
    assert _scalars(lo, 'n_points', 'n_epochs', 'use_therm', 'em_cols', 'em_dense', 'n_parts') == (600, 600, 0, 0, 0, 2)
    assert lo['part_start'] == [0, 300] + [600] * 7 and lo['part_ep0'] == [600] * 9
    other = np.array(t)
    other[[0, 599]] = other[[599, 0]]          # (the caller's order is what is uploaded)
    assert _layout(other, list('UBVgri') * 100)['hash'] != lo['hash']


def test_no_points():
    pr, _keep = E.make_problem(E.MODEL_SHOCK_COOLING, 5, [], [], [], [], [], [0, 2], [1., 2.], [1., 1.])
    lo = S.problem_layout(pr)
    assert _scalars(lo, 'n_points', 'n_epochs', 'use_therm', 'em_k', 'em_cols', 'em_dense', 'n_parts', 'n_chunks', 'cpb') == \
        (0, 0, 0, 1, 0, 0, 1, 0, 1)
    assert lo['part_start'] == [0] * 9 and lo['part_col0'] == [0] * 9 and lo['part_ep0'] == [0] * 9
    assert _scalars(lo, 'n_tab', 'n_lds_tab', 'tab_in_lds', 'stage_d2', 'stage_n16') == (4, 4, 1, 8, 152)


def test_lds_tab_max_zero_stages_no_table():
    t, names = np.repeat(1. + 0.05 * np.arange(20), 3), list('gri') * 20
    staged, none = _layout(t, names), _layout(t, names, LCF_LDS_TAB_MAX='0')
    assert _scalars(staged, 'tab_in_lds', 'stage_n16') == (1, 144 + staged['stage_d2'])
    assert staged['n_lds_tab'] == staged['n_tab']
    assert _scalars(none, 'tab_in_lds', 'n_lds_tab', 'n_itab_lds', 'stage_n16') == (0, 0, 0, 144)
    assert none['n_tab'] == staged['n_tab']


def test_the_layout_is_a_function_of_the_problem():
    """Two plans of one problem hash alike; another observation does not."""
    t, names = np.repeat(1. + 0.05 * np.arange(20), 3), list('gri') * 20
    assert _layout(t, names) == _layout(t, names)
    assert _layout(t + 1e-9, names)['hash'] != _layout(t, names)['hash']
