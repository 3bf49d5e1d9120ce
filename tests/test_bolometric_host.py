"""Host side of the bolometric light curve (no GPU): binning, epoch grouping, direct integration, colours and the
interval statistics against the reference's own numbers (tests/golden/bolometric.npz), and the output table's layout."""
import numpy as np
import pytest

from conftest import golden
from lightcurve_fitting_amd import bolometric as B
from lightcurve_fitting_amd.filters import filtdict
from lightcurve_fitting_amd.lightcurve import LC, binflux


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape
    same_nan = np.isnan(a) == np.isnan(b)
    assert same_nan.all()
    ok = ~np.isnan(a)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300), initial=0.))


def _config1_flux():
    c, g = golden('config1'), golden('bolometric')
    return LC({'MJD': c['cfg1/MJD'], 'filter': c['cfg1/filter'], 'source': c['cfg1/source'],
               'flux': g['bin/flux'], 'dflux': g['bin/dflux']}), g


@pytest.mark.parametrize('delta', [0.3, np.inf])
def test_binflux_and_bin_match_reference(delta):
    lc, g = _config1_flux()
    want = g[f'bin/delta_{delta:g}']
    keys = list(zip(g['bin/key_filter'], g['bin/key_source']))
    for j, (fn, src) in enumerate(keys):
        sel = (np.array([f.name for f in lc['filter']]) == filtdict[fn].name) & (lc['source'] == src)
        got = np.column_stack(binflux(lc['MJD'][sel], lc['flux'][sel], lc['dflux'][sel], delta))
        assert _rel(got, want[want[:, 0] == j, 1:]) < 1e-12
    binned = lc.bin(delta=delta)
    assert binned.colnames == ['MJD', 'flux', 'dflux', 'filter', 'source']
    assert len(binned) == len(want)
    for j, (fn, src) in enumerate(keys):
        sel = np.array([f is filtdict[fn] for f in binned['filter']]) & (binned['source'] == src)
        got = np.column_stack([binned['MJD'][sel], binned['flux'][sel], binned['dflux'][sel]])
        assert _rel(got, want[want[:, 0] == j, 1:]) < 1e-12


def test_bin_groups_only_by_present_columns():
    lc = LC({'MJD': [1., 1.1, 1.2, 5.], 'filter': ['g', 'g', 'r', 'g'], 'flux': [1., 3., 2., 4.],
             'dflux': [1., 1., 1., 2.]})
    b = lc.bin(delta=0.5)
    assert b.colnames == ['MJD', 'flux', 'dflux', 'filter']
    assert sorted(f.name for f in b['filter']) == ['g', 'g', 'r']
    g = np.array([f is filtdict['g'] for f in b['filter']])
    np.testing.assert_allclose(np.sort(b['flux'][g]), [2., 4.])
    assert b.meta is lc.meta


def test_findNondet_and_calcMag():
    lc = LC({'MJD': [1., 2.], 'filter': ['g', 'g'], 'flux': [10., 1.], 'dflux': [1., 1.]})
    lc.calcMag()
    assert list(lc['nondet']) == [False, True]
    zp = filtdict['g'].m0
    np.testing.assert_allclose(lc['mag'], [zp - 2.5, zp - 2.5 * np.log10(3.)], rtol=1e-14)
    assert np.isfinite(lc['dmag'][0]) and np.isnan(lc['dmag'][1])


def _host_epochs(g):
    off = g['host/ep_off']
    for e in range(len(off) - 1):
        s = slice(off[e], off[e + 1])
        names = [str(n) for n in g['host/filter'][s]]
        yield e, LC({'filter': names, 'freq': [filtdict[n].freq_eff for n in names],
                     'dfreq': [filtdict[n].dfreq for n in names], 'lum': g['host/lum'][s],
                     'absmag': g['host/absmag'][s], 'dmag': g['host/dmag'][s], 'nondet': g['host/nondet'][s]})


def test_integrate_sed_and_calc_colors_match_reference():
    g = golden('bolometric')
    colors = [str(c) for c in g['host/colors']]
    for e, ep in _host_epochs(g):
        assert abs(B.integrate_sed(ep) / g['host/L_int'][e] - 1.) < 1e-12
        m, dm, lo, up = B.calc_colors(ep, colors)
        assert _rel(m, g['host/color_mags'][e]) < 1e-12
        assert _rel(dm, g['host/color_dmags'][e]) < 1e-12
        assert list(lo) == list(g['host/color_lolims'][e]) and list(up) == list(g['host/color_uplims'][e])


@pytest.mark.parametrize('perc', [68., 95., 100.])
def test_median_and_unc_matches_reference(perc):
    g = golden('bolometric')
    assert _rel(np.array(B.median_and_unc(g['host/samples'], perc)), g[f'host/median_and_unc_{perc:g}']) < 1e-12


def test_group_by_epoch():
    # res rounding (bolometric.py:401-404): x = MJD / res, frac = median(x - trunc(x)), round(x - frac + round(frac))
    mjd = np.array([10.9, 11.1, 11.2, 14.8, 15.3, 12.0])
    lc = LC({'MJD': mjd, 'filter': ['g', 'r', 'i', 'g', 'r', 'g'], 'epoch': [np.nan] * 5 + [100.]})
    groups = B.group_by_epoch(lc, res=2.)
    x = mjd[:5] / 2.
    frac = np.median(x - np.trunc(x))
    want = np.round(x - frac + np.round(frac)) * 2.
    np.testing.assert_array_equal(lc['epoch'][:5], want)
    assert lc['epoch'][5] == 100.   # a manual epoch is kept
    meds = [np.median(gr['MJD']) for gr in groups]
    assert meds == sorted(meds)
    assert sorted(len(gr) for gr in groups) == sorted(np.unique(lc['epoch'], return_counts=True)[1])
    assert any(list(gr['MJD']) == [12.0] for gr in groups)
    # also_group_by splits an epoch
    lc = LC({'MJD': [1., 1.1, 1.2, 1.3], 'filter': ['g', 'r', 'g', 'r'], 'source': ['a', 'a', 'b', 'b']})
    assert len(B.group_by_epoch(lc)) == 1
    split = B.group_by_epoch(lc, also_group_by=['source'])
    assert sorted(tuple(gr['source']) for gr in split) == [('a', 'a'), ('b', 'b')]
    assert [list(gr['MJD']) for gr in split] == [[1., 1.1], [1.2, 1.3]]


def test_output_columns_are_the_references():
    want = ['MJD', 'dMJD0', 'dMJD1', 'temp', 'radius', 'dtemp', 'dradius', 'L_bol', 'dL_bol', 'L', 'temp_mcmc',
            'radius_mcmc', 'dtemp_mcmc0', 'dtemp_mcmc1', 'dradius_mcmc0', 'dradius_mcmc1', 'L_bol_mcmc',
            'dL_bol_mcmc0', 'dL_bol_mcmc1', 'L_mcmc', 'dL_mcmc0', 'dL_mcmc1', 'L_int', 'npoints', 'B-V', 'g-r',
            'd(B-V)', 'd(g-r)', 'lolims(B-V)', 'lolims(g-r)', 'uplims(B-V)', 'uplims(g-r)', 'filts', 'source',
            'L_opt', 'lum', 'dlum', 'dtemp0', 'dtemp1', 'dradius0', 'dradius1']
    assert B.output_colnames(['B-V', 'g-r'], use_src=True) == want
    assert B.output_colnames([], use_src=False) == [c for c in want if c not in
                                                    ('B-V', 'g-r', 'd(B-V)', 'd(g-r)', 'lolims(B-V)', 'lolims(g-r)',
                                                     'uplims(B-V)', 'uplims(g-r)', 'source')]


def test_lstsq_rejects_p0_outside_the_box_before_device_use():
    with pytest.raises(ValueError, match='infeasible'):
        B.blackbody_lstsq_epochs([(np.array([500., 600., 700.]), np.ones(3))], 0., p0=(200., 10.))
