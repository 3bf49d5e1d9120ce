"""The case table of the sampler sweep (tests/test_gpu_sampler_sweep.py; tests/test_sampler_cases_host.py checks the
table itself without a GPU): every model, light-curve shape, sigma mode, prior kind and band-sum level that reaches a
code path of its own in the one-workgroup-per-proposal kernels -- k_solo, k_solo_run, their rank forms, k_pop, k_pop_run,
k_fused -- at the smallest size at which that path exists.

A case names model and constructor arguments, light-curve shape, filters, redshift, sigma mode, priors, walkers,
LCF_PARTS, band-sum level and seed -- and the template instance ``(kernel, ND, NP, M)`` its run must be launched with,
written down from the rules of the host dispatch (``specialised_model``, ``solo_eligible``, ``run_eligible``, the
instantiation table in csrc/lcf_hip.hip).  :func:`dispatch` restates those rules in Python; the host test holds every
expectation written in the tables of this file and of the sweep against it.

The reference of every case is ``O.stretch_move_run(oracle_log_posterior(pb), ...)``: NumPy around the float64 oracle.

Run as a program (a fresh process per process-wide switch: ``LCF_NO_SOLO=1 python tests/sampler_cases.py 6:auto ...``)
it prints one JSON line per ``case:form`` with the SHA-256 of the chain, log-probabilities, counts and state."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import lc_dict, oracle_log_posterior  # noqa: E402
from lightcurve_fitting_amd import engine as E, models as M  # noqa: E402
from oracle import lcf_oracle as O  # noqa: E402

STEPS = (5, 3)     # run(0, 5) and its continuation run(5, 3): first_step > 0
NONE = (-1, -1, -1, -1)
SC, SC2 = E.MODEL_SHOCK_COOLING, E.MODEL_SHOCK_COOLING2
U, LU, G = M.UniformPrior, M.LogUniformPrior, M.GaussianPrior

# kind -> (truth, walker spread, priors); every explosion-time prior ends in front of the first epoch (0.4 d / 57001.5)
_SC_PRIORS = [U(0., 10.)] * 4 + [U(-1., 0.29)]
_CS_HEAD = [U(56999., 57001.4), U(0., 10.)]
_CS_SPREAD = [0.05, 0.02, 0.05, 0.2, 0.01]
KINDS = {
    'ShockCooling': ([1.2, 0.5, 3.0, 2.0, 0.1], None, _SC_PRIORS),
    'ShockCooling4': ([1.2, 0.5, 3.0, 2.0, 0.1], None, _SC_PRIORS),
    'ShockCooling2': ([30., 3., 30., 0.2], None, [U(0., 100.)] * 3 + [U(-1., 0.29)]),
    'ShockCooling3': ([1.1, 0.6, 2.5, 1.8, 25., 0.15, 0.05], None,
                      [U(0., 10.)] * 4 + [U(1., 100.), U(0., 0.6), U(-1., 0.29)]),
    'CompanionShocking': ([57001., 0.5, 1.2, 57018., 1.05, 0.95, 0.9, 0.6], _CS_SPREAD + [0.02] * 3,
                          _CS_HEAD + [U(0., 10.), U(57008., 57028.), U(0.5, 2.)] + [U(0., 5.)] * 3),
    'CompanionShocking2': ([57001., 0.5, 1.2, 57018., 1.05, 1.0, -1.5], _CS_SPREAD + [0.2] * 2,
                           _CS_HEAD + [U(0., 10.), U(57008., 57028.), U(0.5, 2.)] + [U(-4., 4.)] * 2),
    'CompanionShocking3': ([57001., 0.5, 40., 57018., 1.05, 1.0, -1.5], _CS_SPREAD[:2] + [2., 0.2, 0.01] + [0.2] * 2,
                           _CS_HEAD + [U(0., 180.), U(57008., 57028.), U(0.5, 2.)] + [U(-4., 4.)] * 2),
}
SIGMA = (0.5, 0.05, U(0., 5.))   # a fitted sigma: truth, spread, prior (the last parameter)


class Case:
    """One row of the table.  ``expect``: ``(kernel, ND, NP, M)`` of an 'auto' run; the 'solo' form launches the same
    instance with a launch per half-step, 'fused' and 'phases' launch no such kernel."""

    def __init__(self, cid, kind, shape, filters, nwalkers, seed, expect, kw=None, n_epochs=16, z=0.01, sigma=None,
                 priors=None, parts=None, variant=3, excluded=False, note=''):
        self.id, self.kind, self.shape, self.filters, self.nwalkers, self.seed = cid, kind, shape, list(filters), nwalkers, seed
        self.expect, self.kw, self.n_epochs, self.z, self.sigma = expect, dict(kw or {}), n_epochs, z, sigma
        self.parts, self.variant, self.excluded, self.note = parts, variant, excluded, note
        self.priors = list(priors if priors is not None else KINDS[kind][2]) + ([SIGMA[2]] if sigma and priors is None else [])
        self.ndim = len(KINDS[kind][0]) + (1 if sigma else 0)
        self.companion = kind.startswith('Companion')
        assert len(self.priors) == self.ndim and 2 * self.ndim + 1 <= nwalkers <= 2 * self.ndim + 6, cid

    def __repr__(self):
        return f'<case {self.id}: {self.kind} {self.shape}>'


_CS2_MIXED = _CS_HEAD[:1] + [LU(0.01, 10.), U(0., 10.), G(57008., 57028., 57018., 2.), U(0.5, 2.)] + [U(-4., 4.)] * 2
_SC_MIXED = [U(0., 10.), LU(0.01, 10.), G(0., 10., 3., 1.), U(0., 10.), U(-1., 0.29), LU(0.01, 5.)]
_SC_EDGE = [U(0., 10.)] * 3 + [U(0., 2.05), U(-1., 0.29)]    # R = 2.0: its upper edge one walker spread above the truth
_CS7 = list('UBgri') + ['DLT40', 'unfilt.']

_TABLE = [
    # -- CompanionShocking2 / 3: seven parameters, the dtU / dti shifts, theta with Mv = 1 ----------------------------
    Case(1, 'CompanionShocking2', 'dense', 'UBgri', 16, 101, ('run', 7, 2, 0), n_epochs=18),
    Case(2, 'CompanionShocking2', 'ragged', _CS7, 17, 102, ('run', 7, 2, 0), n_epochs=20, priors=_CS2_MIXED),
    Case(3, 'CompanionShocking3', 'ragged', 'UBVgri', 19, 103, ('run', 7, 2, 0), n_epochs=18),
    Case(4, 'CompanionShocking3', 'dense', 'UBgri', 20, 104, ('run', 8, 8, 0), n_epochs=24, sigma='absolute', parts=4,
         note='four parts, 10 proposals: the 1024-thread row of WideRuns'),
    Case(5, 'CompanionShocking', 'ragged', 'UBVgri', 21, 105, ('run', 9, 2, 0), n_epochs=18, sigma='relative'),
    # -- the specialised kernels with other constants (read from the RunUniforms copy in LDS) ---------------------------
    Case(6, 'ShockCooling', 'dense', 'BVgr', 13, 106, ('run', 5, 2, SC), kw=dict(n=3., RW=True), n_epochs=20),
    Case(7, 'ShockCooling2', 'dense', 'Bgr', 12, 107, ('run', 4, 2, SC2), kw=dict(RW=True), n_epochs=20),
    # -- ragged shared epochs: em_dense = 0, the generic kernels ------------------------------------------------------
    Case(8, 'ShockCooling', 'ragged', 'UBVgri', 16, 108, ('run', 5, 2, 0), n_epochs=24, priors=_SC_EDGE, excluded=True),
    Case(9, 'ShockCooling', 'ragged', 'BVgri', 15, 109, ('run', 6, 2, 0), kw=dict(n=3., RW=True), n_epochs=30,
         sigma='absolute', priors=_SC_MIXED),
    Case(10, 'ShockCooling2', 'ragged', 'BVgr', 14, 110, ('run', 5, 2, 0), n_epochs=22, sigma='relative'),
    Case(11, 'ShockCooling4', 'ragged', 'UBVgri', 11, 111, ('run', 5, 2, 0), n_epochs=20),
    Case(12, 'ShockCooling3', 'ragged', 'BVgr', 18, 112, ('run', 7, 2, 0), n_epochs=16,
         note="reddened tables short enough for LDS: k_solo's generic kernel; a population takes the two launches"),
    # -- one epoch: one column, one part ---------------------------------------------------------------------------
    Case(13, 'ShockCooling', 'single', 'BVgr', 12, 113, ('run', 5, 2, SC)),
    Case(14, 'ShockCooling2', 'single', 'BVgr', 15, 114, ('run', 5, 2, 0), sigma='relative'),
    # -- Swift white: no interpolant, itab_uniform = 0 ----------------------------------------------------------------
    Case(15, 'ShockCooling', 'dense', ['white', 'B', 'V', 'r'], 14, 115, ('run', 5, 2, 0), n_epochs=16),
    Case(16, 'ShockCooling4', 'ragged', ['B', 'white', 'g', 'r', 'i'], 13, 116, ('run', 5, 2, 0), n_epochs=18),
    # -- small light curves in 1 / 3 / 4 / 8 parts: more than two parts and a proposal per CU at the most take k_solo's
    #    1024-thread form, which no model has a kernel of its own for, and no resident workgroups below dimension 8 ------
    Case(17, 'ShockCooling', 'dense', 'BVgr', 11, 117, ('run', 5, 2, SC), n_epochs=24, parts=1),
    Case(18, 'ShockCooling2', 'dense', 'BVg', 10, 118, ('solo', 4, 8, 0), n_epochs=28, parts=3),
    Case(19, 'ShockCooling', 'dense', 'UBVgri', 16, 119, ('solo', 5, 8, 0), n_epochs=32, parts=4),
    Case(20, 'ShockCooling2', 'dense', 'BVgr', 13, 120, ('solo', 4, 8, 0), n_epochs=40, parts=8),
    Case(21, 'ShockCooling', 'dense', 'BVgr', 16, 121, ('solo', 6, 8, 0), n_epochs=30, sigma='absolute', parts=3),
    # -- the other band-sum levels through the one-workgroup kernels; level 0 keeps k_fused ----------------------------
    Case(22, 'CompanionShocking2', 'ragged', _CS7, 17, 102, ('run', 7, 2, 0), n_epochs=20, priors=_CS2_MIXED, variant=2),
    Case(23, 'ShockCooling', 'ragged', 'UBVgri', 16, 108, ('run', 5, 2, 0), n_epochs=24, priors=_SC_EDGE, excluded=True,
         variant=1),
    Case(24, 'ShockCooling', 'dense', ['white', 'B', 'V', 'r'], 14, 115, ('fused',) + NONE[:3], n_epochs=16, variant=0),
    # -- beyond the issue's rows: other reachable rows of the instantiation table ----------------------------------------
    Case(25, 'ShockCooling2', 'unshared', 'UBVgri', 9, 125, ('run', 4, 2, 0), n_epochs=30,
         note='no two points at one time: columns of one point, em_dense = 0'),
    Case(26, 'CompanionShocking3', 'dense', 'UBgri', 19, 126, ('run', 8, 2, 0), n_epochs=16, sigma='absolute',
         note='dimension 8 in one part: RunRow<8, 2, 0> between ranks'),
    Case(27, 'ShockCooling', 'dense', 'BVgr', 12, 127, ('run', 5, 2, 0), n_epochs=20, variant=2,
         note='dense ShockCooling without interpolants: not the specialised kernel'),
]
CASES = {c.id: c for c in _TABLE}

FORMS = ('auto', 'solo', 'fused', 'phases', 'grid')   # 'grid': 'auto' with LCF_RUN_GRID=3, several slots per workgroup
GRID_ENV = {'LCF_RUN_GRID': '3'}

# populations: (walkers, cases with transient 0 first, (k_pop_run instance, k_pop instance))
POPULATIONS = {
    'A': (17, (2, 8, 7), ((0, 0, 0, 0), (0, 0, 0, 0))),     # dimensions 7, 5 generic, 4 specialised
    'B': (19, (3, 9, 13), ((0, 0, 0, 0), (0, 0, 0, 0))),    # 7, 6, 5 specialised (one epoch)
    'C': (16, (15, 10, 6), ((0, 0, 0, 0), (5, 0, 0, 0))),   # all 5: white (generic), ShockCooling2 + sigma, specialised
    'D': (20, (1, 2, 3), ((0, 0, 0, 0), (0, 0, 0, 0))),     # all 7: no entry in PopDims, the dimension at run time
}
POP_SEED = 61    # PopulationSampler(seed=...): transient k is keyed by POP_SEED + k
POP_FORMS = {'population-run': {}, 'population': {'LCF_NO_POP_RUN': '1'}, 'population-phases': {'LCF_NO_POP': '1'}}

# row boards, two emulated ranks: case -> (environment of the rank runs, instance resident, instance per half-step)
RANK_CASES = {
    7: ({}, (4, 2, SC2, 1), (4, 2, SC2, 1)),
    8: ({}, (0, 2, 0, 1), (5, 2, 0, 1)),
    9: ({}, (0, 2, 0, 1), (6, 2, 0, 1)),
    1: ({}, (0, 2, 0, 1), (7, 2, 0, 1)),
    # three parts below dimension 8: resident only with LCF_RUN_ANY_SIZE (read when a run is planned), 512 threads
    21: ({'LCF_RUN_ANY_SIZE': '1'}, (0, 4, 0, 1), (6, 8, 0, 1)),
    17: ({}, (5, 2, SC, 1), (5, 2, SC, 1)),
    26: ({}, (8, 2, 0, 1), (8, 2, 0, 1)),
    4: ({}, (8, 8, 0, 1), (8, 8, 0, 1)),
}

# process-wide switches (read when a run is planned; set here for a whole process): environment -> [(case, form, (kernel, instance))]
SWITCHES = {
    'LCF_NO_SPECIALISED': ({'LCF_NO_SPECIALISED': '1'},
                           [(6, 'auto', ('run', (5, 2, 0, 0))), (7, 'auto', ('run', (4, 2, 0, 0))),
                            (17, 'auto', ('run', (5, 2, 0, 0)))]),
    # (512-thread workgroups: here the specialised kernels exist, NP = 4)
    'LCF_NO_WIDE_SOLO': ({'LCF_NO_WIDE_SOLO': '1'},
                         [(4, 'auto', ('run', (8, 4, 0, 0))), (20, 'auto', ('solo', (4, 4, SC2, 0))),
                          (21, 'auto', ('solo', (6, 4, 0, 0))), (19, 'auto', ('solo', (5, 4, SC, 0))),
                          (4, 'ranks-resident', ('run', (8, 4, 0, 1)))]),
    'LCF_NO_SOLO': ({'LCF_NO_SOLO': '1'},
                    [(6, 'auto', ('fused', NONE)), (1, 'auto', ('fused', NONE)), (8, 'auto', ('fused', NONE))]),
    'LCF_NO_FUSED': ({'LCF_NO_FUSED': '1'},
                     [(6, 'auto', ('phases', NONE)), (1, 'auto', ('phases', NONE)), (8, 'auto', ('phases', NONE))]),
    # LCF_RUN_ANY_SIZE, here for the single-GPU runs of a process: resident workgroups for light curves of more than
    # two parts below a proposal per CU, two or three slots per workgroup; 512 threads where the table has no wide row
    'LCF_RUN_ANY_SIZE': ({'LCF_RUN_ANY_SIZE': '1'},
                         [(18, 'grid', ('run', (4, 4, SC2, 0))), (19, 'grid', ('run', (5, 4, SC, 0))),
                          (21, 'grid', ('run', (6, 4, 0, 0))), (4, 'grid', ('run', (8, 8, 0, 0)))]),
}

# every row of the instantiation table the sweep must have executed (test_every_instance_ran)
REQUIRED = (
    [(k, (nd, np_, m, 0)) for k in ('run', 'solo') for nd, m in ((5, SC), (4, SC2)) for np_ in (2, 4)]   # SpecialisedModels
    + [('run', (8, 8, 0, 0))]                                                                              # WideRuns
    + [('run', r + (1,)) for r in ((5, 2, SC), (4, 2, SC2), (8, 2, 0), (8, 8, 0), (8, 4, 0))]           # RanksRuns
    + [('run', (0, 2, 0, 1)), ('run', (0, 4, 0, 1))]                                                    # generic rank kernel
    + [('solo', (nd, 2, 0, 1)) for nd in (5, 6, 7)]                                                     # k_solo<..., board>
)


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
def light_curve(case):
    """``(t, names)`` of the case's shape from its seed."""
    rng = np.random.default_rng(7000 + case.seed)
    filts, n = case.filters, case.n_epochs
    epochs = (57001.5 + np.sort(rng.uniform(0., 40., n))) if case.companion else np.sort(rng.uniform(0.4, 16., n))
    if case.shape == 'dense':
        return np.repeat(epochs, len(filts)), list(np.tile(filts, n))
    if case.shape == 'single':
        return np.repeat(epochs[:1], len(filts)), list(filts)
    if case.shape == 'unshared':
        return epochs, [str(f) for f in rng.choice(filts, n)]
    assert case.shape == 'ragged'
    t, names = [], []
    twice, thrice = rng.choice(n, 2, replace=False)
    for e, te in enumerate(epochs):
        seen = [f for f in filts if rng.random() < 0.6] or [filts[int(rng.integers(len(filts)))]]
        if e == twice:
            seen = seen[:1] + seen         # its first filter twice at one time
        if e == thrice:
            seen = list(filts) * 3         # more points than em_k (twice the mean at the most): several columns
        t += [te] * len(seen)
        names += seen
    return np.array(t), names


_HOST = {}


def host(case, nwalkers=None):
    """Everything of a case that needs no GPU (built once): photometry from the oracle at the truth with 5 % noise, the
    oracle's problem ``pb``, the walkers' start ``x0``."""
    nw = nwalkers or case.nwalkers
    if (case.id, nw) in _HOST:
        return _HOST[case.id, nw]
    rng = np.random.default_rng(9000 + case.seed)
    t, names = light_curve(case)
    bands = [O.band(n) for n in names]
    truth = np.array(KINDS[case.kind][0])
    spread = np.array(KINDS[case.kind][1]) if case.companion else 0.03 * np.abs(truth)
    if case.companion:   # (the template is scaled to the observed peak: data from a smooth stand-in first)
        v = {'CompanionShocking': 1, 'CompanionShocking2': 2, 'CompanionShocking3': 3}[case.kind]
        guess = 2e20 * np.exp(-0.5 * ((t - 57018.) / 12.) ** 2)
        ytrue = O.evaluate(('CompanionShocking', O.CompanionShockingOracle(bands, guess, case.z, v)), t, bands, truth)
    elif case.kind == 'ShockCooling4':
        om = (case.kind, O.ShockCooling4Oracle(case.z))
        ytrue = O.evaluate(om, t, bands, truth)
    else:
        om = (case.kind, O.ShockCoolingOracle(case.z, **case.kw))
        ytrue = O.evaluate(om, t, bands, truth)
    y = ytrue * (1 + 0.05 * rng.standard_normal(len(t)))
    dy = 0.05 * np.abs(ytrue)
    if case.companion:
        om = ('CompanionShocking', O.CompanionShockingOracle(bands, y, case.z, v))
    if case.sigma:
        truth, spread = np.append(truth, SIGMA[0]), np.append(spread, SIGMA[1])
    x0 = truth + spread * rng.standard_normal((nw, len(truth)))
    for d, p in enumerate(case.priors):      # a start outside a prior's bounds is mirrored back inside
        lo, hi = p.p_min + 0.02 * spread[d], p.p_max - 0.02 * spread[d]
        x0[:, d] = np.where(x0[:, d] > hi, 2 * hi - x0[:, d], np.where(x0[:, d] < lo, 2 * lo - x0[:, d], x0[:, d]))
    pb = dict(model=om, t=t, bands=bands, y=y, dy=dy, priors=[p.descriptor() for p in case.priors],
              use_sigma=bool(case.sigma), sigma_type=case.sigma or 'relative')
    h = dict(t=t, names=names, y=y, dy=dy, bands=bands, pb=pb, x0=x0, nwalkers=nw)
    _HOST[case.id, nw] = h
    return h


_ORACLE = {}


def oracle_chain(case, nwalkers=None, seed=None):
    """The oracle-driven chain of the case's two runs: ``(chain, log_prob, accepted, log-posteriors of every proposal,
    accepted after the first run)``."""
    nw, seed = nwalkers or case.nwalkers, case.seed if seed is None else seed
    if (case.id, nw, seed) not in _ORACLE:
        h = host(case, nw)
        fn, seen = oracle_log_posterior(h['pb']), []

        def log_prob(block):
            out = fn(block)
            seen.append(np.array(out))
            return out
        a, a_lp, a_acc = O.stretch_move_run(log_prob, h['x0'], STEPS[0], seed)
        b, b_lp, b_acc = O.stretch_move_run(log_prob, a[-1], STEPS[1], seed, log_prob0=a_lp[-1], first_step=STEPS[0])
        _ORACLE[case.id, nw, seed] = (np.concatenate([a, b]), np.concatenate([a_lp, b_lp]), a_acc + b_acc,
                                      np.concatenate(seen[1:]), a_acc)    # (seen[0]: the start)
    return _ORACLE[case.id, nw, seed]


@contextlib.contextmanager
def environment(**env):
    """The environment with these variables set (None: unset), put back afterwards."""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def make_model(case, h):
    """``(model, light curve)``: a model object of its own per call (a model keeps one engine per light curve)."""
    lc = lc_dict(h['t'], h['names'], h['y'], h['dy'])
    if case.companion:
        return getattr(M, case.kind)(lc, redshift=case.z), lc
    if case.kind == 'ShockCooling3':   # (fits 'flux')
        lc = {'MJD': lc['MJD'], 'filter': lc['filter'], 'flux': h['y'], 'dflux': h['dy']}
    return getattr(M, case.kind)(redshift=case.z, **case.kw), lc


def engine_keywords(case):
    return dict(use_sigma=True, sigma_type=case.sigma) if case.sigma else {}


def _create_engine(case, nwalkers=None):
    """``(engine, model)`` of the case as it is created: LCF_PARTS is read then."""
    h = host(case, nwalkers)
    model, lc = make_model(case, h)
    with environment(LCF_PARTS=None if case.parts is None else str(case.parts)):
        return model.engine_for(lc, priors=case.priors, **engine_keywords(case)), model


def make_engine(case, nwalkers=None):
    """A new engine of the case, the band-sum level set on it."""
    eng, model = _create_engine(case, nwalkers)
    if case.variant != 3:
        eng.set_variant(case.variant)
    eng.model = model    # (keeps the model, and with it its cache of engines, alive as long as the engine)
    return eng


# the integers of lcf_debug_engine_layout (csrc/lcf_engine.hip), in its order; part_start, part_col0, part_ep0 follow
LAYOUT_FIELDS = ('n_points', 'n_epochs', 'use_therm', 'em_k', 'em_cols', 'em_dense', 'n_parts', 'n_chunks', 'cpb',
                 'n_tab', 'n_lds_tab', 'tab_in_lds', 'redden_slow', 'use_ctab', 'use_itab', 'itab_uniform',
                 'n_itab_lds', 'n_spl_lds', 'stage_d2', 'stage_n16')


def problem_layout(pr):
    """The layout ``lcf_engine_create`` plans for an ``LcfProblem``, computed without a device: the fields above, the
    three arrays of the parts (nine entries each) and ``hash``, FNV-1a over every array the engine would upload."""
    fn = E.load_library().lcf_debug_engine_layout
    fn.restype, fn.argtypes = C.c_int32, [C.POINTER(E.LcfProblem), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_uint64)]
    n = len(LAYOUT_FIELDS)
    out, h = (C.c_int32 * (n + 27))(), C.c_uint64()
    E._check(fn(C.byref(pr), out, len(out), C.byref(h)))
    return dict(zip(LAYOUT_FIELDS, out[:n]), part_start=out[n:n + 9], part_col0=out[n + 9:n + 18],
                part_ep0=out[n + 18:n + 27], hash=h.value)


@contextlib.contextmanager
def planned_engines():
    """Inside, ``E.Engine`` asks for no device: every engine's problem is planned only, and its layout appended to the
    list this yields.  (Such an engine has no native handle: nothing can be evaluated with it.)"""
    layouts = []

    def plan(self, pr):
        layouts.append(problem_layout(pr))
        self._h = None
    create, E.Engine._create = E.Engine._create, plan
    try:
        yield layouts
    finally:
        E.Engine._create = create


def engine_layout(case):
    """The layout of the case's engine as the library plans it (:func:`engine_shape` restates the rules)."""
    with planned_engines() as layouts:
        _create_engine(case)
    assert len(layouts) == 1
    return layouts[0]


def run_single(case, form, engine=None):
    """The case's two runs with the half-step kernels of ``form`` -> dict(chain, lp, nacc, x, lp_end, kernel, instance)."""
    h = host(case)
    eng = engine or make_engine(case)
    s = E.NativeSampler(eng, case.nwalkers, case.seed)
    s.set_half_step_kernel('auto' if form == 'grid' else form)
    s.set_state(h['x0'])
    chains, lps, seen = [], [], set()
    with environment(**({'LCF_RUN_GRID': None} if form != 'grid' else GRID_ENV)):
        for first, n in ((0, STEPS[0]), (STEPS[0], STEPS[1])):
            s.run(first, n, 'random', True)
            c, lp = s.get_chain()
            chains.append(c)
            lps.append(lp)
            seen.add((s.last_run_kernel(), s.last_run_instance()))
            if first == 0:
                mid = s.get_state() + (s.naccepted(),)
    x, lp_end = s.get_state()
    assert len(seen) == 1, seen    # the continuation takes the kernel the first run took
    kernel, instance = seen.pop()
    return dict(chain=np.concatenate(chains), lp=np.concatenate(lps), nacc=s.naccepted(), x=x, lp_end=lp_end,
                mid_x=mid[0], mid_lp=mid[1], mid_nacc=mid[2], kernel=kernel, instance=instance)


def run_ranks(case, form, env=None, ranks=2):
    """The case's two runs as a row-board run of ``ranks`` emulated ranks on one GPU, ``form`` 'resident' or 'per
    half-step' -> one dict as :func:`run_single` gives it per rank.  Engines (= streams) of their own; every buffer is
    sized by a run before the boards are used (ranks of ONE process share its host thread: an allocation made while
    another rank's launch waits for this rank would hold the launches back); both ranks are enqueued before either is
    waited for.  ``env``: set for the board calls only -- never while a single-GPU run is enqueued."""
    h = host(case)
    engines = [make_engine(case) for _ in range(ranks)]
    assert len({id(e) for e in engines}) == ranks
    samplers = [E.NativeSampler(e, case.nwalkers, case.seed) for e in engines]
    ptrs = [s.board_export()[1] for s in samplers]
    for r, s in enumerate(samplers):
        with environment(**(env or {})):
            s.board_connect(ranks, r, local_ptrs=ptrs)
        s.set_state(h['x0'])
        s.run(100, max(STEPS), 'random', True)
        s.set_state(h['x0'])
        s.set_half_step_kernel('auto' if form == 'resident' else 'solo')
    out = [dict(chain=[], lp=[], seen=set()) for _ in samplers]
    with environment(**(env or {})):
        for first, n in ((0, STEPS[0]), (STEPS[0], STEPS[1])):
            for s in samplers:
                s.run_rows(first, n, 'random', True, asynchronous=True)
            for s in samplers:
                s.wait()
            for s, o in zip(samplers, out):
                c, lp = s.get_chain()
                o['chain'].append(c)
                o['lp'].append(lp)
                o['seen'].add((s.last_run_kernel(), s.last_run_instance()))
    runs = []
    for s, o in zip(samplers, out):
        assert len(o['seen']) == 1, o['seen']
        kernel, instance = o['seen'].pop()
        x, lp_end = s.get_state()
        runs.append(dict(chain=np.concatenate(o['chain']), lp=np.concatenate(o['lp']), nacc=s.naccepted(), x=x,
                         lp_end=lp_end, kernel=kernel, instance=instance))
    return runs


def digest(run):
    """SHA-256 of a run's chain, log-probabilities, acceptance counts and final state."""
    m = hashlib.sha256()
    for key in ('chain', 'lp', 'nacc', 'x', 'lp_end'):
        m.update(np.ascontiguousarray(run[key]).tobytes())
    return m.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch rules of csrc/lcf_hip.hip, restated (an MI355X: 256 compute units)
# ---------------------------------------------------------------------------------------------------------------------
N_CUS, K_MAX_PARTS, K_LDS_TAB_MAX = 256, 8, 3700
SOLO_DIMS, POP_DIMS = (4, 5, 6, 7, 8, 9), (4, 5, 6, 8)
SPECIALISED = {(SC, 5), (SC2, 4)}                                  # Models<Model<M, ND>...>
WIDE_RUNS = {(8, 8, 0)}                                            # RunRow<ND, NP, M>
RANKS_RUNS = {(5, 2, SC), (4, 2, SC2), (8, 2, 0), (8, 8, 0), (8, 4, 0)}
MODEL_IDS = {'ShockCooling': SC, 'ShockCooling2': SC2, 'ShockCooling3': E.MODEL_SHOCK_COOLING3,
             'ShockCooling4': E.MODEL_SHOCK_COOLING4, 'CompanionShocking': E.MODEL_COMPANION_SHOCKING,
             'CompanionShocking2': E.MODEL_COMPANION_SHOCKING2, 'CompanionShocking3': E.MODEL_COMPANION_SHOCKING3}


def engine_shape(case):
    """What ``lcf_engine_create`` derives from the case's light curve and tables: columns, parts, em_dense, table
    placement, whether every filter's interpolant holds from the table's first interval."""
    from lightcurve_fitting_amd.filters import PackedTables
    h = host(case)
    t, names = h['t'], h['names']
    uniq = list(dict.fromkeys(names))
    fidx = np.array([uniq.index(n) for n in names])
    n_pts, nf = len(t), len(uniq)
    epochs, ep_of = np.unique(t, return_inverse=True)
    cnt = np.bincount(ep_of, minlength=len(epochs))
    em_k = int(min(cnt.max(), max(2, -(-2 * n_pts // len(epochs)))))
    col_epoch, col_first, at = [], [], 0
    for e, c in enumerate(cnt):
        for k in range(0, c, em_k):
            col_epoch.append(e)
            col_first.append(at + k)
        at += c
    n_cols = len(col_epoch)
    order = np.lexsort((np.arange(n_pts), fidx, ep_of))
    dense = em_k == nf and len(epochs) * nf == n_pts and all(fidx[order[i]] == i % nf for i in range(n_pts))
    n_parts = max(2 if n_cols > 64 else 1, -(-n_cols // 256))
    assert n_cols <= 256 * K_MAX_PARTS
    if case.parts is not None:
        n_parts = max(1, min(n_cols, K_MAX_PARTS, case.parts))
    start = [0]
    for j in range(1, n_parts):    # boundary j: the first epoch change at or after the equal split of the columns
        cb = n_cols * j // n_parts
        while 0 < cb < n_cols and col_epoch[cb] == col_epoch[cb - 1]:
            cb += 1
        b = col_first[cb] if cb < n_cols else n_pts
        if start[-1] < b < n_pts:
            start.append(b)
    reddened = case.kind == 'ShockCooling3'
    tabs = PackedTables(uniq, z=case.z, compress=not reddened, reddening=reddened)
    pad = lambda off: sum((int(b - a) + 3) // 4 * 4 for a, b in zip(off[:-1], off[1:]))   # noqa: E731
    n_comp = 0 if reddened else pad(tabs.coff) + pad(tabs.hoff)
    n_tab = n_comp + pad(tabs.off)
    n_lds = n_tab if n_tab <= K_LDS_TAB_MAX else n_comp if 0 < n_comp <= K_LDS_TAB_MAX else 0
    if reddened and n_lds != n_tab:
        n_lds = 0
    itmin = tabs.interpolants()[1]
    return dict(n_points=n_pts, n_filters=nf, n_epochs=len(epochs), em_k=em_k, n_cols=n_cols, em_dense=bool(dense),
                n_parts=len(start), start=start, tab_in_lds=n_lds > 0, have_itab=not reddened, filters=uniq, itab_tmin=itmin,
                itab_uniform=bool(not reddened and np.all(itmin <= np.exp(tabs.iu0) * (1. + 1e-12))), counts=cnt,
                names=names, t=t)


def dispatch(case, form='auto', switches=(), ranks=0, n_half=None):
    """``(kernel, (ND, NP, M, ranks))`` a run of the case is launched with: ``form`` as FORMS (between ranks: 'auto' =
    resident, 'solo' = a launch per half-step), ``switches`` the process-wide environment switches that are set,
    ``ranks`` the ranks of a row-board run (0: one GPU)."""
    if form.startswith('ranks-'):
        form, ranks = {'ranks-resident': 'auto', 'ranks-solo': 'solo'}[form], ranks or 2
    sh = engine_shape(case)
    n_dim, n_parts = case.ndim, sh['n_parts']
    variant = 0 if case.variant == 0 else 1
    use_itab = case.variant == 3 and sh['have_itab']
    one_wg = (form in ('auto', 'grid', 'solo') and 'LCF_NO_SOLO' not in switches and 'LCF_NO_FUSED' not in switches and
              variant != 0 and sh['tab_in_lds'] and n_parts <= K_MAX_PARTS)                         # solo_eligible
    if not one_wg:
        assert not ranks
        fused = form != 'phases' and 'LCF_NO_FUSED' not in switches and sh['tab_in_lds']          # fused_eligible
        return ('fused' if fused else 'phases'), NONE
    spec = 0                                                                                       # specialised_model
    if 'LCF_NO_SPECIALISED' not in switches and use_itab and sh['em_dense'] and sh['itab_uniform'] and not case.sigma:
        spec = MODEL_IDS[case.kind] if (MODEL_IDS[case.kind], n_dim) in SPECIALISED else 0
    width = (n_half or (case.nwalkers + 1) // 2) // max(ranks, 1)
    no_wide = 'LCF_NO_WIDE_SOLO' in switches
    wide_size = n_parts > 2 and width <= N_CUS and any(nd == n_dim for nd, _, _ in WIDE_RUNS)     # run_wide_size
    resident = width <= 4 * 512 if n_parts <= 2 else ((width > N_CUS or wide_size) and width <= (1024 if ranks else 512))
    resident = form in ('auto', 'grid') and (resident or 'LCF_RUN_ANY_SIZE' in switches)
    nd = n_dim if n_dim in SOLO_DIMS else 0
    if not resident:                                                                               # launch_solo
        np_ = 2 if n_parts <= 2 else 8 if (not no_wide and width <= N_CUS) else 4
        m = spec if np_ != 8 and (spec, nd) in SPECIALISED else 0
        return 'solo', (nd, np_, m, 1 if ranks else 0)
    np_ = 2 if n_parts <= 2 else 8 if (wide_size and not no_wide) else 4                           # launch_run
    if ranks:
        return 'run', ((n_dim, np_, spec, 1) if (n_dim, np_, spec) in RANKS_RUNS else (0, np_, 0, 1))
    if (n_dim, np_, spec) in WIDE_RUNS:
        return 'run', (n_dim, np_, spec, 0)
    return 'run', (nd, np_, spec if (spec, nd) in SPECIALISED else 0, 0)


def population_dispatch(case_ids, form):
    """``(kernel, instance)`` of a population of these cases (all at band-sum level 3, tables in LDS)."""
    cases = [CASES[c] for c in case_ids]
    dims = {c.ndim for c in cases}
    same = dims.pop() if len(dims) == 1 else 0
    specs = {dispatch(c, 'solo')[1][2] for c in cases}   # (one part each: k_solo's M is specialised_model)
    spec = specs.pop() if len(specs) == 1 else 0
    one_launch = form != 'population-phases' and all(c.kind != 'ShockCooling3' and c.variant != 0 for c in cases)
    if not one_launch:
        return 'population-phases', NONE
    if form == 'population':
        nd = same if same in POP_DIMS else 0
        return 'population', (nd, 0, spec if (spec, nd) in SPECIALISED else 0, 0)
    return 'population-run', ((same, 0, spec, 0) if (spec, same) in SPECIALISED else (0, 0, 0, 0))


def main(argv):
    out = []
    for arg in argv:
        cid, form = arg.split(':')
        if form.startswith('ranks-'):   # (after the single-GPU runs of this process: see run_ranks)
            runs = run_ranks(CASES[int(cid)], form[6:])
            assert len({(digest(r), r['kernel'], r['instance']) for r in runs}) == 1, 'the ranks differ'
            run = runs[0]
        else:
            run = run_single(CASES[int(cid)], form)
        out.append(dict(case=int(cid), form=form, digest=digest(run), kernel=run['kernel'], instance=list(run['instance'])))
        print(json.dumps(out[-1]), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
