"""``k_bb_lstsq`` and ``k_bb_lum`` (csrc/lcf_bolo.hip) at their edges, against the extended-precision reference of
tests/bolometric_reference.py (which tests/test_bolometric_reference_host.py checks without a GPU, together with the
inputs used here).  Everything goes through ``engine.bb_lstsq`` / ``engine.bb_luminosity`` unless stated.

Branches of ``k_bb_lstsq`` and the test that reaches each:

* optimum on T_lo, T_hi, R_lo, R_hi, in the T_hi,R_lo and T_lo,R_hi corners, interior -- test_fit_is_optimal_on_every_
  active_set, test_fit_equals_the_reference_optimum;
* ``free0`` / ``free1`` at iteration 0 (p0 on a bound or in a corner) -- the ``p0@...`` cases of the same two tests, and
  test_iteration_cap (started in the box's corner);
* a box per epoch (``box + 6 e``) -- the same (every epoch has its own) and test_per_epoch_boxes_equal_single_launches;
* the rank-one pseudo-inverse -- test_rank_one_covariance;
* ``s1 == 0`` -- test_zero_jacobian, test_singular_free_block;
* the singular free block that damps harder and the ``lambda >= 1e300`` exit -- test_singular_free_block;
* ``status == 0`` -- test_iteration_cap; ``status == -1``, ``m`` of 0, 1 and 2 inside a batch -- test_mixed_wave;
* 63, 64, 65 and 130 epochs, lanes 0, 63, 64 -- test_batch_position.

Largest relative deviations measured on an MI355X (MEASURED below; each bound held is 100 times its measurement and
never looser than test_gpu_bolometric.py's 1e-5 / 1e-4):

* the 354 epochs of ``fit_cases()`` against ``lstsq_ref``: T, R 3.0e-9, covariance 1.5e-8 (both on a ``p0@R_lo`` epoch);
* ``rank_one_cases()``: cost 2.9e-16, covariance 3.5e-15 against ``curve_fit_cov`` at the device's own optimum;
* ``k_bb_lum`` against ``pseudo_ref`` over T = 0.05-1e5 kK: 1.01e-13, at T = 0.05 kK; 2.0e-14 from 0.3 kK up."""
import ctypes as C

import numpy as np
import pytest

import bolometric_reference as BR
from lightcurve_fitting_amd import bolometric as B
from lightcurve_fitting_amd import engine as E

pytestmark = pytest.mark.gpu

#: largest relative deviations measured on an MI355X (see the tests' docstrings)
MEASURED = dict(fit=3.0e-9, cov=1.5e-8, rank_one_cost=2.9e-16, rank_one_cov=3.5e-15, lum=1.01e-13, lum_warm=2.0e-14)
FIT_TOL = min(100. * MEASURED['fit'], 1e-5)
COV_TOL = min(100. * MEASURED['cov'], 1e-4)
RANK_ONE_COST_TOL = min(100. * MEASURED['rank_one_cost'], 1e-5)
RANK_ONE_COV_TOL = min(100. * MEASURED['rank_one_cov'], 1e-4)
LUM_TOL = 1e-12


def _launch(cases, **kw):
    return E.bb_lstsq(*BR.pack(cases), z=cases[0].z, cutoff_freq=cases[0].cut, **kw)


def _alone(c, **kw):
    out, st = _launch([c], **kw)
    return out[0], st[0]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _rel(got, want):
    return float(np.max(np.abs((np.asarray(got, dtype=BR.F) - want) / want)))


def _cov3(cov):
    return np.array([cov[0, 0], cov[0, 1], cov[1, 1]])


def _floor(c):
    return 1e-24 * np.sum(c.lum ** 2)


@pytest.fixture(scope='module')
def fits():
    """``fit_cases()`` through the device, one launch per (z, cut): ``(cases, out, status)``."""
    cases = BR.fit_cases()
    out, st = np.empty((len(cases), 8)), np.empty(len(cases), dtype=np.int32)
    for idx in BR.by_setting(cases).values():
        out[idx], st[idx] = _launch([cases[k] for k in idx])
    return cases, out, st


def test_fit_is_optimal_on_every_active_set(fits):
    """Every epoch: converged, a cost not above the reference's, the bound variables EXACTLY on the bounds of the
    claimed active set (and no other), and a zero projected gradient (extended precision, the project's 1e-6)."""
    cases, out, st = fits
    for k, (c, o) in enumerate(zip(cases, out)):
        T, R, cost, _ = c.reference()
        assert st[k] > 0, (k, c.kind, st[k])
        assert o[2] <= float(cost) * (1 + 1e-9) + _floor(c), (k, c.kind, o[2], float(cost))
        assert BR.active_set(o[0], o[1], c.lo, c.hi) == c.active, (k, c.kind, o[:2], c.lo, c.hi)
        pg = BR.projected_gradient(c.freq, c.lum, c.z, c.cut, o[0], o[1], c.lo, c.hi)
        assert np.all(np.abs(pg) < 1e-6), (k, c.kind, pg)


def test_fit_equals_the_reference_optimum(fits):
    """T, R and the covariance against ``lstsq_ref`` and ``curve_fit_cov`` at its optimum, every epoch.

    Measured: T, R within 3.0e-9, the three covariance entries within 1.5e-8 (relative; the size expected of
    xtol = 1e-12 times the conditioning of a two-parameter fit to 3 % noise).  Held: 3.0e-7 and 1.5e-6."""
    cases, out, st = fits
    worst = dict(fit=(0., None), cov=(0., None))
    for k, (c, o) in enumerate(zip(cases, out)):
        T, R, cost, _ = c.reference()
        cov = _cov3(BR.curve_fit_cov(c.freq, c.z, c.cut, T, R, cost, c.m))
        worst['fit'] = max(worst['fit'], (max(_rel(o[0], T), _rel(o[1], R)), (k, c.kind)))
        worst['cov'] = max(worst['cov'], (_rel(o[3:6], cov), (k, c.kind)))
    print('fit_cases: largest relative deviation', worst)
    assert worst['fit'][0] <= FIT_TOL and worst['cov'][0] <= COV_TOL, worst


def test_noiseless_epochs_recover_the_truth():
    cases = BR.noiseless_cases()
    for idx in BR.by_setting(cases).values():
        out, st = _launch([cases[k] for k in idx])
        for k, o, s in zip(idx, out, st):
            T, R = cases[k].truth
            assert s > 0 and abs(o[0] / T - 1) < 1e-9 and abs(o[1] / R - 1) < 1e-9, (k, o, T, R)


def test_per_epoch_boxes_equal_single_launches():
    """100 epochs, each with its own lo, hi and p0, in one launch: every row is the row of that epoch alone."""
    cases = BR.box_cases()
    assert len({tuple(np.concatenate([c.lo, c.hi, c.p0])) for c in cases}) == len(cases) == 100
    out, st = _launch(cases)
    assert np.all(st > 0)
    for k, c in enumerate(cases):
        o1, s1 = _alone(c)
        assert s1 == st[k] and _same_bits(o1, out[k]), (k, c.kind, o1, out[k])
        assert c.lo[0] <= out[k, 0] <= c.hi[0] and c.lo[1] <= out[k, 1] <= c.hi[1]


def test_batch_position():
    """One epoch alone, at lanes 0, 63 and 64 of a batch, and last in batches of 63, 64, 65 and 130: the same bits."""
    c = BR.fit_cases()[3]
    fill = [BR.FitCase(f.kind, f.freq, f.lum, c.z, c.cut, f.p0, f.lo, f.hi) for f in BR.filler_cases(130)]
    o1, s1 = _alone(c)
    assert s1 > 0
    for n, lane in ((130, 0), (130, 63), (130, 64), (63, 62), (64, 63), (65, 64), (130, 129)):
        batch = fill[:lane] + [c] + fill[lane + 1:n]
        out, st = _launch(batch)
        assert len(out) == n and np.all(st > 0)
        assert st[lane] == s1 and _same_bits(out[lane], o1), (n, lane, out[lane], o1)


def test_mixed_wave():
    """Good epochs interleaved with epochs of 0, 1 and 2 points and epochs holding NaN / inf in lum or freq."""
    cases = BR.mixed_cases()
    out, st = _launch(cases)
    for k, (c, o) in enumerate(zip(cases, out)):
        if c.kind in ('good', 'm1', 'm2'):
            o1, s1 = _alone(c)
            assert st[k] > 0 and s1 == st[k] and _same_bits(o1, o), (k, c.kind, o1, o)
            assert c.lo[0] <= o[0] <= c.hi[0] and c.lo[1] <= o[1] <= c.hi[1]
            assert np.all(np.isinf(o[3:6])) == (c.m <= 2) and np.all(np.isfinite(o[3:6])) == (c.m > 2), (k, o)
            T, R, cost, _ = c.reference()
            assert o[2] <= float(cost) * (1 + 1e-9) + _floor(c), (k, c.kind, o[2], float(cost))
        else:
            assert st[k] == -1 and o[6] == 0, (k, c.kind, st[k], o)
    r = B.blackbody_lstsq_epochs([(c.freq, c.lum) for c in cases], 0.)
    bad = r['status'] <= 0
    assert np.array_equal(r['status'], st) and np.array_equal(bad, [c.kind not in ('good', 'm1', 'm2') for c in cases])
    for name in ('temp', 'radius', 'dtemp', 'dradius', 'covTR', 'L_bol', 'dL_bol', 'L'):
        assert np.array_equal(np.isnan(r[name]), bad), name
    assert np.all(np.isfinite(r['cost'][~bad])) and np.all(r['niter'][~bad] > 0)
    assert _same_bits(r['temp'][~bad], out[~bad, 0]) and _same_bits(r['radius'][~bad], out[~bad, 1])


def test_iteration_cap():
    """``status == 0``: epochs started in the far corner of a wide box, with ``max_iter`` of 1, 2, 5 and 500."""
    cases = BR.hard_cases()
    prev = None
    for max_iter in (1, 2, 5, 500):
        out, st = _launch(cases, max_iter=max_iter)
        assert np.all(st >= 0) and np.all(out[st == 0, 6] == max_iter) and np.all(out[:, 6] <= max_iter)
        assert np.all(np.isnan(out[st == 0, 3:6]))
        if max_iter <= 5:
            assert np.all(st == 0)
        if prev is not None:
            assert np.all(out[:, 2] <= prev)
        prev = out[:, 2]
    assert np.all(st > 0) and np.all(out[:, 6] > 5)
    for c, o in zip(cases, out):
        T, R, cost, _ = c.reference()
        assert o[2] <= float(cost) * (1 + 1e-9) + _floor(c)
        assert max(_rel(o[0], T), _rel(o[1], R)) <= FIT_TOL
    # the public function does not expose the cap: an epoch that cannot converge is one with a non-finite point
    c = cases[0]
    lum = c.lum.copy()
    lum[1] = np.nan
    with pytest.raises(RuntimeError, match='Optimal parameters not found'):
        B.blackbody_lstsq({'freq': c.freq, 'lum': lum}, 0.)
    assert len(B.blackbody_lstsq({'freq': c.freq, 'lum': c.lum}, 0., T_range=(1.5, 1000.))) == 7


def test_rank_one_covariance():
    """3-6 points at one frequency: J has rank one exactly and the optimum is a curve, so T and R are not compared.
    The cost is the reference's (measured: 2.9e-16; held: 2.9e-14) and the covariance is ``curve_fit_cov`` -- the
    pseudo-inverse, of rank one -- at the device's own T, R and cost (measured: 3.5e-15; held: 3.5e-13)."""
    cases = BR.rank_one_cases()
    worst = dict(cost=0., cov=0.)
    for idx in BR.by_setting(cases).values():
        out, st = _launch([cases[k] for k in idx])
        for k, o, s in zip(idx, out, st):
            c = cases[k]
            _, _, cost, _ = c.reference()
            cov = BR.curve_fit_cov(c.freq, c.z, c.cut, o[0], o[1], o[2], c.m)
            assert s > 0 and np.linalg.matrix_rank(cov) == 1
            assert o[3] > 0 and o[5] > 0 and abs(o[4] * o[4] / (o[3] * o[5]) - 1.) < 1e-12   # (rank one itself)
            worst['cost'] = max(worst['cost'], _rel(o[2], cost))
            worst['cov'] = max(worst['cov'], _rel(o[3:6], _cov3(cov).astype(BR.F)))
    print('rank_one_cases: largest relative deviation', worst)
    assert worst['cost'] <= RANK_ONE_COST_TOL and worst['cov'] <= RANK_ONE_COV_TOL, worst


def test_zero_jacobian():
    """``expm1`` overflows over the whole box: the projected gradient is exactly 0 at the start."""
    cases = BR.zero_jacobian_cases()
    out, st = _launch(cases)
    for c, o, s in zip(cases, out, st):
        assert s == 2 and o[6] == 0 and np.all(o[3:6] == 0.), (s, o)
        assert o[0] == c.p0[0] and o[1] == c.p0[1] and abs(o[2] / (0.5 * np.sum(c.lum ** 2)) - 1) < 1e-14


def test_singular_free_block():
    """J^T J underflows to 0 under a J^T r that does not: the free block is singular whatever the damping.  The epoch
    ends through the ``lambda >= 1e300`` exit (harder damping doubles its factor each time: 44 iterations) where it
    started, with the cost of a zero model and a zero covariance -- like its neighbours of test_zero_jacobian, and not
    at the iteration cap, where it ended before the exit covered this path."""
    cases = BR.singular_cases()
    out, st = _launch(cases)
    for c, o, s in zip(cases, out, st):
        assert s == 1 and 40 <= o[6] <= 50, (s, o)
        assert o[0] == c.p0[0] and o[1] == c.p0[1] and np.all(o[3:6] == 0.), o
        assert abs(o[2] / (0.5 * np.sum(c.lum ** 2)) - 1) < 1e-14
    out2, st2 = _launch(cases, max_iter=20)
    assert np.all(st2 == 0) and np.all(out2[:, 6] == 20)
    assert len(B.blackbody_lstsq({'freq': cases[0].freq, 'lum': cases[0].lum}, 0., p0=cases[0].p0)) == 7


def test_zero_and_negative_luminosities():
    cases = BR.zero_and_negative_cases()
    out, st = _launch(cases)
    for k, (c, o, s) in enumerate(zip(cases, out, st)):
        T, R, cost, _ = c.reference()
        assert s > 0, (k, c.kind, s)
        if c.kind == 'zero':
            assert o[1] == c.lo[1] and o[2] > 0
        assert o[2] <= float(cost) * (1 + 1e-9) + _floor(c), (k, c.kind, o[2], float(cost))
        assert o[2] >= float(cost) * (1 - 1e-9), (k, c.kind, o[2], float(cost))
        pg = BR.projected_gradient(c.freq, c.lum, c.z, c.cut, o[0], o[1], c.lo, c.hi)
        assert np.all(np.abs(pg) < 1e-6), (k, c.kind, pg)


# --- the ABI's argument checks ---------------------------------------------------------------------------------------
def _raw_lstsq(off, p0=(10., 10.), lo=BR.DEFAULT_LO, hi=BR.DEFAULT_HI, z=0., cut=np.inf, max_iter=500, xtol=1e-12):
    """``lcf_bb_lstsq`` itself on 6-point epochs -> (status code, whether an output was written)."""
    lib = E.load_library()
    off = np.ascontiguousarray(off, dtype=np.int32)
    n = len(off) - 1
    c = BR.noiseless_cases()[3]
    f, y = np.resize(c.freq, max(off.max(), 1)), np.resize(c.lum, max(off.max(), 1))
    p0, lo, hi = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n, 2))) for a in (p0, lo, hi))
    out, st = np.full((n, 8), -7.), np.full(n, -7, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    p = lambda a, t=dp: a.ctypes.data_as(t)
    rc = lib.lcf_bb_lstsq(0, n, p(off, ip), p(f), p(y), p(p0), p(lo), p(hi), float(z), float(cut), int(max_iter),
                          float(xtol), p(out), p(st, ip))
    return rc, bool(np.any(out != -7.) or np.any(st != -7))


@pytest.mark.parametrize('kw', [
    dict(off=[0, 6, 4, 12]), dict(off=[1, 6, 12]), dict(p0=(0.5, 10.)), dict(p0=(10., 1001.)), dict(p0=(np.nan, 10.)),
    dict(p0=(10., np.inf)), dict(lo=(100., 0.01)), dict(lo=(1., 1000.)), dict(hi=(1., 1000.)),
    dict(hi=(np.nan, 1000.)), dict(z=-1.),
    dict(z=np.nan), dict(z=np.inf), dict(cut=0.), dict(cut=np.nan), dict(max_iter=0), dict(xtol=0.),
    dict(xtol=np.nan)], ids=str)
def test_lstsq_rejects_bad_arguments_before_any_launch(kw):
    kw = dict(kw)
    rc, written = _raw_lstsq(kw.pop('off', [0, 6, 12]), **kw)
    assert E.STATUS_NAMES[rc] == 'LCF_ERR_INVALID_ARGUMENT' and not written


def test_lstsq_accepts_the_same_call_and_no_epochs():
    rc, written = _raw_lstsq([0, 6, 12])
    assert rc == 0 and written
    out, st = E.bb_lstsq([0], np.zeros(0), np.zeros(0), np.zeros((0, 2)), np.zeros((0, 2)), np.ones((0, 2)))
    assert out.shape == (0, 8) and st.shape == (0,)
    with pytest.raises(E.LcfError, match='INVALID_ARGUMENT'):   # (the checks that need no epoch still hold)
        E.bb_lstsq([0], np.zeros(0), np.zeros(0), np.zeros((0, 2)), np.zeros((0, 2)), np.ones((0, 2)), z=-1.)


@pytest.mark.parametrize('kw', [dict(n_grid=-1), dict(freq0=np.nan), dict(freq0=np.inf), dict(z=-1.), dict(z=np.nan),
                                dict(cutoff_freq=0.), dict(cutoff_freq=np.nan)], ids=str)
def test_luminosity_rejects_bad_arguments(kw):
    args = dict(z=0., freq0=300.5, n_grid=8, cutoff_freq=np.inf)
    args.update(kw)
    with pytest.raises(E.LcfError, match='INVALID_ARGUMENT'):
        E.bb_luminosity(np.array([10.]), np.array([1.]), **args)
    with pytest.raises(E.LcfError, match='INVALID_ARGUMENT'):   # (before the n == 0 return)
        E.bb_luminosity(np.zeros(0), np.zeros(0), **args)


def test_luminosity_of_no_samples():
    Lp, Lb = E.bb_luminosity(np.zeros(0), np.zeros(0), 0., 300.5, 8)
    assert Lp.shape == Lb.shape == (0,)


# --- k_bb_lum --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('z,cut', BR.LUM_SETTINGS)
def test_luminosities_equal_the_reference(z, cut):
    """4096 samples over T = 0.05-1e5 kK (and 0, negative, inf, NaN), R of both signs and 0, on five grids.
    ``L_pseudo`` is exactly 0 where the reference is, else within 1e-12; ``L_bol`` is NumPy's ``stefan_boltzmann``.

    Measured maximum over all settings and grids: 1.01e-13, at T = 0.05 kK, z = 0.1 -- the cold end, where c1 nu / T is
    350-450 and carries its float64 roundings (1 / T, the product, c1) into the exponential: the one-point grid, which
    has no recurrence, measures 7.5e-14 there.  From 0.06 kK up it is 7.3e-14, from 0.3 kK up 2.0e-14 (what the
    recurrence was stated to give), on the 64-point grid at 0.5 THz 1.9e-15.  The project's 1e-12 holds over the whole
    of 0.05-1e5 kK."""
    T, R = BR.lum_samples()
    with np.errstate(all='ignore'):
        want_b = B.stefan_boltzmann(T, R)
    for freq0, n_grid in BR.lum_grids():
        ref = BR.lum_reference(z, cut, freq0, n_grid)
        Lp, Lb = E.bb_luminosity(T, R, z, freq0, n_grid, cut)
        zero = ref == 0
        assert np.all(zero[~(T > 0) | np.isinf(T) | (R == 0)]) and (n_grid == 0) == bool(zero.all())
        assert np.all(Lp[zero] == 0.), (freq0, n_grid, T[zero][Lp[zero] != 0.])
        if not zero.all():
            rel = np.abs((Lp[~zero].astype(BR.F) - ref[~zero]) / ref[~zero]).astype(np.float64)
            warm = rel[T[~zero] >= 0.3].max()
            print(f'k_bb_lum z={z} cut={cut} freq0={freq0:.2f} n_grid={n_grid}: max rel {rel.max():.2e} at '
                  f'T={T[~zero][rel.argmax()]:.3g}; T >= 0.3: {warm:.2e}')
            assert rel.max() < LUM_TOL
            assert warm < 10. * MEASURED['lum_warm']   # (DESIGN.md states the figure)
        nan, inf = np.isnan(want_b), np.isinf(want_b)
        assert np.array_equal(np.isnan(Lb), nan) and np.array_equal(Lb[inf], want_b[inf])
        ok = ~nan & ~inf & (want_b != 0)
        assert np.max(np.abs(Lb[ok] / want_b[ok] - 1.)) < 1e-12 and np.all(Lb[~nan & (want_b == 0)] == 0.)


def test_luminosity_grid_stride_second_trip():
    """2 097 152 + 257 samples: the first size at which a lane of the capped grid (256 * 32 blocks of 256) handles two.
    The result is the tiling of the 4096-sample result; so are 255, 256 and 257 samples."""
    T, R = BR.lum_samples()
    z, cut = BR.LUM_SETTINGS[1]
    freq0, n_grid = BR.lum_grids()[0]
    Lp, Lb = E.bb_luminosity(T, R, z, freq0, n_grid, cut)
    for n in (255, 256, 257, 256 * 32 * 256 + 257):
        Lp_n, Lb_n = E.bb_luminosity(np.resize(T, n), np.resize(R, n), z, freq0, n_grid, cut)
        assert _same_bits(Lp_n, np.resize(Lp, n)) and _same_bits(Lb_n, np.resize(Lb, n)), n
