"""Bolometric light curves on the MI355X: k_bb_lstsq against the reference's curve_fit (tests/golden/bolometric.npz)
and against optimality itself, k_bb_lum against the host's pseudo / stefan_boltzmann, and calculate_bolometric end to
end on SN 2016bkv (the usage guide's example) and on a synthetic light curve with a known answer."""
import os
import re

import numpy as np
import pytest

from bolometric_reference import projected_gradient as _projected_gradient
from conftest import golden
from lightcurve_fitting_amd import bolometric as B
from lightcurve_fitting_amd import engine as E
from lightcurve_fitting_amd.filters import c1, c2, filtdict
from lightcurve_fitting_amd.lightcurve import LC

pytestmark = pytest.mark.gpu


def _planck(nu, T, R, cut):
    with np.errstate(over='ignore'):
        return c2 * R ** 2 * nu ** 3 * np.minimum(1., cut / nu) / np.expm1(c1 * nu / T)


def _golden_fit():
    g = golden('bolometric')
    off, setup = g['ls/ep_off'], g['ls/setup']
    out = []
    # one launch per (z, cutoff, box) setting: the batched form takes one box for all its epochs
    for key in sorted({tuple(r[[0, 1, 4, 5, 6, 7]]) for r in setup}):
        idx = [e for e in range(len(setup)) if tuple(setup[e][[0, 1, 4, 5, 6, 7]]) == key]
        z, cut, Tlo, Rlo, Thi, Rhi = key
        eps = [(g['ls/freq'][off[e]:off[e + 1]], g['ls/lum'][off[e]:off[e + 1]]) for e in idx]
        r = B.blackbody_lstsq_epochs(eps, z, setup[idx][:, 2:4], (Tlo, Thi), (Rlo, Rhi), cut)
        out += [(e, eps[k], setup[e], {n: v[k] for n, v in r.items()}) for k, e in enumerate(idx)]
    return g, sorted(out, key=lambda t: t[0])


def test_lstsq_matches_reference_curve_fit():
    """T, R within 1e-4 of the reference's uncertainty or 1e-5 relative; dT, dR, cov_TR, L_bol, dL_bol, L within 1e-4
    relative; m <= 2 -> infinite uncertainties.  Where scipy's tolerances stopped its fit early (the device cost is
    lower than the reference's by more than 1e-10 relative), the device optimum must instead be stationary, and
    those epochs must stay rare."""
    g, fits = _golden_fit()
    early = 0
    for e, (f, y), setup, r in fits:
        ref = g['ls/result'][e]
        assert r['status'] > 0, (e, r)
        rT, rR, rdT, rdR, rL, rdL, rLo, rcov, rcost = ref
        m = len(f)
        floor = 1e-24 * np.sum(y ** 2)   # (m = 2: an exact fit, both costs are rounding)
        assert r['cost'] <= rcost * (1 + 1e-9) + floor, (e, r['cost'], rcost)
        if m <= 2:
            assert np.isinf(r['dtemp']) and np.isinf(r['dradius']) and np.isinf(r['dL_bol'])
            assert abs(r['temp'] - rT) <= 1e-5 * rT and abs(r['radius'] - rR) <= 1e-5 * rR
            continue
        derived = (('dtemp', rdT), ('dradius', rdR), ('covTR', rcov), ('L_bol', rL), ('dL_bol', rdL), ('L', rLo))
        close = (abs(r['temp'] - rT) <= max(1e-4 * rdT, 1e-5 * rT) and abs(r['radius'] - rR) <= max(1e-4 * rdR, 1e-5 * rR)
                 and all(abs(r[k] / want - 1.) <= 1e-4 for k, want in derived))
        if not close:   # then scipy stopped early: the device optimum is better and stationary
            early += 1
            assert r['cost'] < rcost * (1 - 1e-10), (e, r, ref)
            lo, hi = setup[[4, 5]], setup[[6, 7]]
            assert np.all(np.abs(_projected_gradient(f, y, setup[0], setup[1], r['temp'], r['radius'], lo, hi)) < 1e-6)
            for k, want in derived:
                assert abs(r[k] / want - 1.) <= 1e-3, (e, k, r[k], want)
    assert early <= 10, early
    # the bound cases: T on T_hi
    on_bound = [(s[6], r['temp']) for _, _, s, r in fits if s[6] < 100.]
    assert on_bound and all(T == hi for hi, T in on_bound), on_bound


def test_lstsq_device_optimum_is_stationary():
    """Without scipy: the projected gradient at every device optimum is zero to rounding."""
    g, fits = _golden_fit()
    for e, (f, y), s, r in fits:
        if len(f) <= 2:
            continue
        pg = _projected_gradient(f, y, s[0], s[1], r['temp'], r['radius'], s[[4, 5]], s[[6, 7]])
        assert np.all(np.abs(pg) < 1e-6), (e, pg, r['niter'], r['status'])


def test_lstsq_single_epoch_form_and_errors():
    f = np.array([filtdict[n].freq_eff for n in 'UBVgri'])
    y = _planck(f, 12., 3., np.inf)
    T, R, dT, dR, L, dL, Lo = B.blackbody_lstsq({'freq': f, 'lum': y}, 0.)
    assert abs(T / 12. - 1) < 1e-9 and abs(R / 3. - 1) < 1e-9
    with pytest.raises(ValueError):
        B.blackbody_lstsq({'freq': f, 'lum': y}, 0., p0=(0.5, 10.))
    with pytest.raises(E.LcfError, match='INVALID_ARGUMENT'):
        E.bb_lstsq([0, 6], f, y, (10., 10.), (1., 0.01), (100., 1000.), z=-2.)


def test_luminosity_kernel_matches_host_pseudo():
    rng = np.random.default_rng(5)
    n = 100000
    T = np.concatenate([[0.3, 300., 0.05, 0.065, 0.], np.exp(rng.uniform(np.log(0.3), np.log(300.), n - 5))])
    R = np.exp(rng.uniform(np.log(0.01), np.log(100.), n))
    for z, cut in ((0., np.inf), (0.03, 700.), (0.1, 500.)):
        Lp, Lb = B.luminosity_samples(T, R, z, cut)
        want_p = B.pseudo(T, R, z, cutoff_freq=cut)
        want_b = B.stefan_boltzmann(T, R)
        pos = want_p > 0
        assert np.all(Lp[~pos] == 0.)
        assert np.max(np.abs(Lp[pos] / want_p[pos] - 1.)) < 1e-12
        hot = want_b > 0
        assert np.max(np.abs(Lb[hot] / want_b[hot] - 1.)) < 1e-12 and np.all(Lb[~hot] == 0.)


def _sn2016bkv():
    c = golden('config1')
    return LC({'MJD': c['cfg1/MJD'], 'mag': c['cfg1/mag'], 'dmag': c['cfg1/dmag'], 'filter': c['cfg1/filter'],
               'nondet': c['cfg1/nondet'], 'source': c['cfg1/source']}, meta={'dm': 30.79, 'redshift': 0.002})


COLORS = ['B-V', 'g-r', 'r-i']
MC_COLS = ['temp_mcmc', 'radius_mcmc', 'dtemp_mcmc0', 'dtemp_mcmc1', 'dradius_mcmc0', 'dradius_mcmc1', 'L_bol_mcmc',
           'dL_bol_mcmc0', 'dL_bol_mcmc1', 'L_mcmc', 'dL_mcmc0', 'dL_mcmc1']


@pytest.fixture(scope='module')
def sn_tables(tmp_path_factory):
    out = tmp_path_factory.mktemp('bolo')
    kw = dict(colors=COLORS, burnin_steps=100, steps=50, outpath=str(out))
    with pytest.warns(UserWarning):
        t_mc = B.calculate_bolometric(_sn2016bkv(), do_mcmc=True, seed=11, save_table_as=str(out / 't.txt'),
                                      save_chains=True, **kw)
        t_mc2 = B.calculate_bolometric(_sn2016bkv(), do_mcmc=True, seed=11, **kw)
        t_ls = B.calculate_bolometric(_sn2016bkv(), do_mcmc=False, **kw)
    return t_mc, t_mc2, t_ls, out


def test_calculate_bolometric_sn2016bkv_columns(sn_tables):
    t_mc, t_mc2, t_ls, out = sn_tables
    assert t_mc.colnames == B.output_colnames(COLORS, use_src=True)
    assert len(t_mc) > 20 and len(t_mc) == len(t_ls)
    # per-epoch functions on the same epochs
    lc = _sn2016bkv()
    lc = lc[np.isfinite(lc['dmag']) & (lc['dmag'] > 0)]
    k = 0
    for ep in B.group_by_epoch(lc):
        ep = B._prepare_epoch(ep)
        filts = set(ep.where(nondet=False)['filter'])
        if len(filts) < 3:
            continue
        for t in (t_mc, t_ls):
            np.testing.assert_allclose([t['MJD'][k], t['dMJD0'][k], t['dMJD1'][k]], B.median_and_unc(ep['MJD'], 100.),
                                       rtol=1e-15)
            assert t['npoints'][k] == len(filts)
            assert t['filts'][k] == ''.join(f.char for f in sorted(filts))
            ref = B.blackbody_lstsq(ep, 0.002)
            np.testing.assert_allclose([t[c][k] for c in ('temp', 'radius', 'dtemp', 'dradius', 'L_bol', 'dL_bol', 'L')],
                                       ref, rtol=1e-12)
            assert abs(t['L_int'][k] / B.integrate_sed(ep) - 1) < 1e-14
            m, dm, lo, up = B.calc_colors(ep[np.argsort(ep['freq'], kind='stable')], COLORS)
            for j, c in enumerate(COLORS):
                np.testing.assert_equal([t[c][k], t[f'd({c})'][k]], [m[j], dm[j]])
                assert (t[f'lolims({c})'][k], t[f'uplims({c})'][k]) == (lo[j], up[j])
        k += 1
    assert k == len(t_mc)
    for t in (t_mc, t_ls):
        for old, new in B.DEPRECATED_BOLOMETRIC_COLNAMES:
            np.testing.assert_array_equal(t[old], t[new])
    # MCMC columns are NaN exactly when do_mcmc=False
    for c in MC_COLS:
        assert np.all(np.isnan(t_ls[c])) and np.all(np.isfinite(t_mc[c])), c
    # the same seed -> the same table, bit for bit
    for c in t_mc.colnames:
        a, b = np.asarray(t_mc[c]), np.asarray(t_mc2[c])
        assert a.dtype == b.dtype and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == 'f'
                                       else np.array_equal(a, b)), c
    assert len([p for p in os.listdir(out) if p.endswith('.npy')]) == len(t_mc)


def test_calculate_bolometric_table_round_trip(sn_tables):
    t_mc, _, _, out = sn_tables
    lines = open(out / 't.txt').read().splitlines()
    header = lines[0].split()
    assert header == t_mc.colnames and set(lines[1].replace(' ', '')) == {'-'}
    rows = [ln.split() for ln in lines[2:]]
    assert len(rows) == len(t_mc)
    for j, c in enumerate(header):
        col = t_mc[c]
        for i, cell in enumerate(r[j] for r in rows):
            v = col[i]
            if isinstance(v, (bool, np.bool_)):
                assert cell == str(bool(v))
            elif isinstance(v, (float, np.floating)):
                assert (cell == '--' and np.isnan(v)) or float(cell) == v, (c, cell, v)
            else:
                assert cell == str(v)


def test_calculate_bolometric_recovers_a_known_light_curve():
    """40 epochs of UBVgri from known T(t), R(t), 2 % noise, plus one epoch with two filters (below min_nfilt)."""
    rng = np.random.default_rng(3)
    names = ['U', 'B', 'V', 'g', 'r', 'i']
    days = np.arange(40) * 2. + 100.
    T_true = 12. * np.exp(-(days - 100.) / 40.) + 5.
    R_true = 1. + 0.2 * (days - 100.)
    rows = []
    for d, T, R in zip(days, T_true, R_true):
        for n in names:
            rows.append((d + rng.uniform(-0.1, 0.1), n, T, R))
    rows += [(300., 'g', 10., 5.), (300.05, 'r', 10., 5.)]
    mjd = np.array([r[0] for r in rows])
    filt = [r[1] for r in rows]
    lum = np.array([_planck(filtdict[r[1]].freq_eff, r[2], r[3], np.inf) for r in rows])
    lum *= 1 + 0.02 * rng.standard_normal(len(rows))
    zp = np.array([filtdict[n].m0 for n in filt])
    mag = zp + 90.19 - 2.5 * np.log10(lum)       # absolute = apparent with dm = 0
    lc = LC({'MJD': mjd, 'mag': mag, 'dmag': np.full(len(rows), 0.02 * 2.5 / np.log(10)), 'filter': filt},
            meta={'dm': 0.})
    with pytest.warns(UserWarning):
        t = B.calculate_bolometric(lc, seed=1)
    assert len(t) == 40
    assert np.all(np.abs(t['temp_mcmc'] - T_true) <= 4 * 0.5 * (t['dtemp_mcmc0'] + t['dtemp_mcmc1']))
    assert np.all(np.abs(t['radius_mcmc'] - R_true) <= 4 * 0.5 * (t['dradius_mcmc0'] + t['dradius_mcmc1']))
    L_true = B.stefan_boltzmann(T_true, R_true)
    assert np.all(np.abs(t['L_bol_mcmc'] / L_true - 1) < 0.2)


def test_bolometric_kernels_neither_spill_nor_use_scratch():
    path = os.path.join(os.path.dirname(E.__file__), 'csrc', 'liblcf_hip.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no resource report next to the library (built without the Makefile)')
    text = open(path).read()
    blocks = {m.group(1): dict(re.findall(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)', m.group(2)))
              for m in re.finditer(r'Function Name: (\S+)(.*?)(?=Function Name:|\Z)', text, re.S)}
    for name in ('10k_bb_lstsq', '8k_bb_lum'):
        hits = [k for k in blocks if name + 'E' in k]
        assert len(hits) == 1, (name, hits)
        f = blocks[hits[0]]
        assert int(f['ScratchSize']) == 0 and int(f['VGPRs Spill']) == 0 and int(f['SGPRs Spill']) == 0, f
