"""ctypes binding of the C ABI in ``include/lcf.h`` (``csrc/liblcf_hip.so``, built for gfx950).

There is NO CPU fallback: if the shared library is missing or no MI355X is visible, constructing an
:class:`Engine` raises.  Host-side work here is limited to marshalling (contiguous float64 blocks in, arrays out).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('LCF_HIP_LIB') or os.path.join(_HERE, 'csrc', 'liblcf_hip.so')

LCF_ABI_VERSION = 8
N_CONSTS = 12

MODEL_SHOCK_COOLING = 1
MODEL_SHOCK_COOLING2 = 2
MODEL_SHOCK_COOLING3 = 3
MODEL_SHOCK_COOLING4 = 4
MODEL_COMPANION_SHOCKING = 5
MODEL_COMPANION_SHOCKING2 = 6
MODEL_COMPANION_SHOCKING3 = 7
MODEL_BLACKBODY = 8
MODEL_CUSTOM = 9
MODEL_ARNETT = 10
MODEL_MAGNETAR = 11

PRIOR_UNIFORM, PRIOR_LOG_UNIFORM, PRIOR_GAUSSIAN = 0, 1, 2
SIGMA_RELATIVE, SIGMA_ABSOLUTE = 0, 1
SPLIT_IDENTITY, SPLIT_RANDOM, SPLIT_HOST = 0, 1, 2
MOVE_STRETCH, MOVE_DE, MOVE_SNOOKER, MAX_MOVES = 0, 1, 2, 8   # lcf_tempered_set_moves (include/lcf.h)

STATUS_NAMES = {0: 'LCF_OK', 1: 'LCF_ERR_INVALID_ARGUMENT', 2: 'LCF_ERR_HIP', 3: 'LCF_ERR_NO_DEVICE',
                4: 'LCF_ERR_OUT_OF_MEMORY', 5: 'LCF_ERR_UNSUPPORTED', 6: 'LCF_ERR_NAN_LOGPROB', 7: 'LCF_ERR_STATE'}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class LcfPrior(C.Structure):
    _fields_ = [('kind', C.c_int32), ('reserved', C.c_int32), ('p_min', C.c_double), ('p_max', C.c_double),
                ('mean', C.c_double), ('stddev', C.c_double)]


class LcfProblem(C.Structure):
    _fields_ = [('abi_version', C.c_int32), ('model', C.c_int32), ('n_par', C.c_int32), ('use_sigma', C.c_int32),
                ('sigma_type', C.c_int32), ('n_filters', C.c_int32), ('n_points', C.c_int64),
                ('consts', C.c_double * N_CONSTS),
                ('t', _dp), ('y', _dp), ('dy', _dp), ('filt_idx', _ip), ('tab_off', _ip), ('tab_a', _dp),
                ('tab_w', _dp), ('tab_ext', _dp), ('ctab_off', _ip), ('ctab_a', _dp), ('ctab_w', _dp), ('ctab_tmin', _dp),
                ('htab_off', _ip), ('htab_a', _dp), ('htab_w', _dp), ('htab_tmin', _dp),
                ('itab_coef', _dp), ('itab_tmin', _dp), ('itab_m', C.c_int32), ('reserved2', C.c_int32),
                ('itab_u0', C.c_double), ('itab_h', C.c_double),
                ('filt_kasen_par', _ip), ('filt_sifto_par', _ip), ('filt_dt_par', _ip),
                ('n_knots', C.c_int32), ('reserved', C.c_int32), ('spline_knots', _dp), ('spline_coef', _dp),
                ('priors', C.POINTER(LcfPrior))]


class LcfError(RuntimeError):
    """A non-zero ``lcf_status`` from the native library."""

    def __init__(self, status, message):
        self.status = status
        super().__init__(f'{STATUS_NAMES.get(status, status)}: {message}')


_lib = None

#: every symbol include/lcf.h declares: (name, restype, argtypes)
SIGNATURES = [
    ('lcf_abi_version', C.c_int32, []),
    ('lcf_last_error', C.c_char_p, []),
    ('lcf_device_count', C.c_int32, []),
    ('lcf_engine_create', C.c_int, [C.POINTER(LcfProblem), C.c_int32, C.POINTER(C.c_void_p)]),
    ('lcf_engine_destroy', None, [C.c_void_p]),
    ('lcf_engine_ndim', C.c_int32, [C.c_void_p]),
    ('lcf_engine_npoints', C.c_int64, [C.c_void_p]),
    ('lcf_engine_samples_per_eval', C.c_int64, [C.c_void_p]),
    ('lcf_engine_set_variant', C.c_int, [C.c_void_p, C.c_int32]),
    ('lcf_log_likelihood', C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    ('lcf_log_posterior', C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    ('lcf_log_likelihood_dev', C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('lcf_log_posterior_dev', C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('lcf_model_evaluate', C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    ('lcf_temperature_radius', C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp]),
    ('lcf_blackbody_to_filters', C.c_int, [C.c_void_p, C.c_int64, _ip, _dp, _dp, _dp]),
    ('lcf_profile_loglike_kernel', C.c_int, [C.c_void_p, C.c_int64, _dp, C.c_int32, _dp]),
    ('lcf_sampler_create', C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_double, C.POINTER(C.c_void_p)]),
    ('lcf_sampler_destroy', None, [C.c_void_p]),
    ('lcf_sampler_set_state', C.c_int, [C.c_void_p, _dp]),
    ('lcf_sampler_get_state', C.c_int, [C.c_void_p, _dp, _dp]),
    ('lcf_sampler_run', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _ip, C.c_int32]),
    ('lcf_sampler_run_async', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _ip, C.c_int32]),
    ('lcf_sampler_wait', C.c_int, [C.c_void_p]),
    ('lcf_population_run', C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                     _dp]),
    ('lcf_sampler_get_chain', C.c_int, [C.c_void_p, _dp, _dp]),
    ('lcf_sampler_reserve_chain', C.c_int, [C.c_void_p, C.c_int64]),
    ('lcf_sampler_get_naccepted', C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ('lcf_sampler_get_snapshot', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('lcf_sampler_last_run_ms', C.c_double, [C.c_void_p]),
    ('lcf_sampler_begin', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _ip, C.c_int32]),
    ('lcf_sampler_propose', C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    ('lcf_sampler_evaluate', C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ('lcf_sampler_accept', C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    ('lcf_sampler_half_step', C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ('lcf_sampler_newlp_ptr', C.c_void_p, [C.c_void_p]),
    ('lcf_sampler_one_launch', C.c_int32, [C.c_void_p]),
    ('lcf_sampler_set_half_step_kernel', C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    ('lcf_sampler_last_run_kernel', C.c_int32, [C.c_void_p]),
    ('lcf_sampler_last_run_launches', C.c_int64, [C.c_void_p]),
    ('lcf_sampler_last_run_instance', None, [C.c_void_p, C.POINTER(C.c_int32)]),
    ('lcf_sampler_half_step_rows', C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ('lcf_sampler_rows_ptr', C.c_void_p, [C.c_void_p, C.POINTER(C.c_int32)]),
    ('lcf_sampler_check', C.c_int, [C.c_void_p]),
    ('lcf_comm_probe', C.c_int, [C.c_char_p]),
    ('lcf_comm_unique_id', C.c_int, [C.c_char_p, C.c_void_p]),
    ('lcf_comm_create', C.c_int, [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ('lcf_comm_destroy', None, [C.c_void_p]),
    ('lcf_comm_count', C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ('lcf_comm_time_allgather', C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _dp]),
    ('lcf_sampler_run_sharded', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _ip, C.c_int32]),
    ('lcf_sampler_mailbox_export', C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    ('lcf_sampler_mailbox_connect', C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    ('lcf_sampler_run_peers', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _ip, C.c_int32]),
    ('lcf_sampler_run_peers_async', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _ip, C.c_int32]),
    ('lcf_sampler_board_export', C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    ('lcf_sampler_board_connect', C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    ('lcf_sampler_run_rows', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _ip, C.c_int32]),
    ('lcf_sampler_run_rows_async', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _ip, C.c_int32]),
    ('lcf_sed_create', C.c_int, [C.c_int32, _ip, _dp, _dp, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int32, C.c_double,
                                 C.c_double, C.c_int32, C.POINTER(C.c_void_p)]),
    ('lcf_sed_destroy', None, [C.c_void_p]),
    ('lcf_sed_set_observations', C.c_int, [C.c_void_p, C.c_int64, _ip, _ip, _dp, _dp]),
    ('lcf_sed_log_likelihood', C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _dp, C.c_int32, C.c_int32, _dp,
                                         _dp]),
    ('lcf_bb_lstsq', C.c_int, [C.c_int32, C.c_int64, _ip, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int32,
                               C.c_double, _dp, _ip]),
    ('lcf_bb_luminosity', C.c_int, [C.c_int32, C.c_int64, _dp, _dp, C.c_double, C.c_double, C.c_int32, C.c_double, _dp,
                                    _dp]),
    ('lcf_autocorr_time', C.c_int, [C.c_int32, _dp, C.c_int64, C.c_int32, C.c_int32, C.c_double, _dp,
                                    C.POINTER(C.c_int64)]),
    ('lcf_samplers_autocorr_time', C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int64, C.c_double, _dp,
                                             C.POINTER(C.c_int64)]),
    ('lcf_predict_quantiles', C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, C.c_int32, _dp, C.c_int32, C.c_int64,
                                        _dp, C.POINTER(C.c_int64)]),
    ('lcf_sampler_predict_quantiles', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _dp,
                                                C.c_int32, C.c_int64, _dp, C.POINTER(C.c_int64)]),
    ('lcf_predict_colors', C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, C.c_int32, _ip, _dp, _dp, C.c_int32,
                                     C.c_int64, _dp, C.POINTER(C.c_int64), _dp, _ip]),
    ('lcf_sampler_predict_colors', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _ip, _dp, _dp,
                                             C.c_int32, C.c_int64, _dp, C.POINTER(C.c_int64), _dp, _ip]),
    ('lcf_predict_thermal', C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, _dp, C.c_int32, C.c_double, C.c_int64, _dp,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ('lcf_sampler_predict_thermal', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, _dp, C.c_int32, C.c_double,
                                              C.c_int64, _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64)]),
    ('lcf_predict_luminosity', C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, _dp, C.c_int32, C.c_int64, _dp,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), _dp, _ip]),
    ('lcf_predict_custom', C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, _dp, C.c_int32, C.c_double, C.c_int64, _dp,
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ('lcf_chain_range', C.c_int, [C.c_int32, _dp, C.c_int64, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(C.c_int64)]),
    ('lcf_chain_hist', C.c_int, [C.c_int32, _dp, C.c_int64, C.c_int32, C.c_int32, _dp, _dp, C.c_int32,
                                 C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ('lcf_samplers_chain_range', C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int64, _dp, _dp,
                                           C.POINTER(C.c_int64)]),
    ('lcf_samplers_chain_hist', C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int64, _dp, _dp, C.c_int32,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ('lcf_chain_history', C.c_int, [C.c_int32, _dp, _dp, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _dp,
                                    C.c_int32, _dp, _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ('lcf_chain_raster', C.c_int, [C.c_int32, _dp, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _dp,
                                   C.c_int32, C.POINTER(C.c_int64)]),
    ('lcf_samplers_chain_history', C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int64, _dp, C.c_int32, _dp,
                                             _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ('lcf_samplers_chain_raster', C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int64, C.c_int32, _dp,
                                            C.c_int32, C.POINTER(C.c_int64)]),
    ('lcf_tempered_create', C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, C.c_uint64, C.c_double,
                                      C.POINTER(C.c_void_p)]),
    ('lcf_tempered_destroy', None, [C.c_void_p]),
    ('lcf_tempered_set_state', C.c_int, [C.c_void_p, _dp]),
    ('lcf_tempered_get_state', C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    ('lcf_tempered_run', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32]),
    ('lcf_tempered_get_chain', C.c_int, [C.c_void_p, _dp, _dp]),
    ('lcf_tempered_get_counts', C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64)]),
    ('lcf_tempered_mean_loglike', C.c_int, [C.c_void_p, C.c_int64, _dp]),
    ('lcf_tempered_run_adaptive', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                            C.c_int64]),
    ('lcf_tempered_get_betas', C.c_int, [C.c_void_p, _dp]),
    ('lcf_tempered_get_beta_history', C.c_int, [C.c_void_p, _dp]),
    ('lcf_tempered_stepping_stones', C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp, _dp]),
    ('lcf_tempered_set_moves', C.c_int, [C.c_void_p, C.c_int32, _ip, _dp, _dp]),
    ('lcf_tempered_get_move_history', C.c_int, [C.c_void_p, _ip]),
    ('lcf_custom_compile', C.c_int, [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(C.c_void_p)]),
    ('lcf_custom_log', C.c_char_p, [C.c_void_p]),
    ('lcf_custom_code', C.c_void_p, [C.c_void_p, C.POINTER(C.c_int64)]),
    ('lcf_custom_destroy', None, [C.c_void_p]),
    ('lcf_engine_set_custom', C.c_int, [C.c_void_p, C.c_void_p]),
    ('lcf_engine_set_custom_redshift', C.c_int, [C.c_void_p, C.c_double]),
    ('lcf_engine_set_limits', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _dp, _dp]),
    ('lcf_limit_terms', C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    ('lcf_engine_set_template', C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, _ip, _ip, C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(LcfPrior)]),
    ('lcf_template_evaluate', C.c_int, [C.c_void_p, C.c_int64, _dp, C.c_int32, _dp]),
    ('lcf_predict_template', C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, C.c_int32, _dp, C.c_int32, C.c_int64, _dp,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ('lcf_template_features', C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, _dp, _ip]),
]

#: `component` of `lcf_template_evaluate` (include/lcf.h: LCF_TEMPLATE_*)
TEMPLATE_COMPONENTS = {'total': 1, 'base': 2, 'template': 3}
#: `components` of `lcf_predict_template` (include/lcf.h: LCF_TEMPLATE_MASK_*), in the order the results come out
TEMPLATE_MASK = {'total': 1, 'base': 2, 'template': 4}


def load_library(path=None):
    """dlopen the native library and attach prototypes.  Raises ``OSError`` with build instructions if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    try:
        # PyTorch ships its own HIP/HSA runtime.  Two runtimes in one process do not coexist, so when torch is
        # installed it is loaded FIRST and this library binds to the runtime already in the process (same soname).
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise OSError(f'{path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` or '
                      f'`make -C {os.path.dirname(path)}` (hipcc --offload-arch=gfx950). There is no CPU fallback.')
    lib = C.CDLL(path)
    for name, restype, argtypes in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.lcf_abi_version() != LCF_ABI_VERSION:
        raise OSError(f'{path}: ABI version {lib.lcf_abi_version()} != {LCF_ABI_VERSION}')
    _lib = lib
    return lib


def _check(status):
    if status != 0:
        raise LcfError(status, load_library().lcf_last_error().decode())


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a, typ=_dp):
    return a.ctypes.data_as(typ)


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _handles(native_samplers):
    """The ``lcf_sampler**`` of a call that takes several :class:`NativeSampler` objects."""
    return (C.c_void_p * len(native_samplers))(*[s._h for s in native_samplers])


def make_problem(model_id, n_par, consts, t, y, dy, filt_idx, tab_off, tab_a, tab_w, use_sigma=False,
                 sigma_type=SIGMA_RELATIVE, priors=None, companion=None, ctab=None, tab_ext=None, htab=None, itab=None):
    """``(problem, keep)``: the ``lcf_problem`` of :class:`Engine`'s arguments and the arrays its pointers point into
    (``keep`` must live as long as the problem is used)."""
    no_filters = tab_off is None
    if no_filters:
        filt_idx, tab_off, tab_a, tab_w = np.zeros(len(_f64(t)), dtype=np.int32), [0], [], []
    keep = [_f64(t), _f64(y), _f64(dy), _i32(filt_idx), _i32(tab_off), _f64(tab_a), _f64(tab_w)]
    pr = LcfProblem()
    pr.abi_version = LCF_ABI_VERSION
    pr.model = int(model_id)
    pr.n_par = int(n_par)
    pr.use_sigma = int(bool(use_sigma))
    pr.sigma_type = int(sigma_type)
    pr.n_filters = len(keep[4]) - 1
    pr.n_points = len(keep[0])
    if not (len(keep[1]) == len(keep[2]) == len(keep[3]) == pr.n_points):
        raise ValueError('t, y, dy, filt_idx must have the same length')
    cs = list(consts) + [0.] * (N_CONSTS - len(consts))
    pr.consts = (C.c_double * N_CONSTS)(*cs)
    pr.t, pr.y, pr.dy = _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2])
    if not no_filters:
        pr.filt_idx, pr.tab_off = _ptr(keep[3], _ip), _ptr(keep[4], _ip)
        pr.tab_a, pr.tab_w = _ptr(keep[5]), _ptr(keep[6])
    if tab_ext is not None:  # A_lambda / E(B-V) per table sample (ShockCooling3)
        ext = _f64(tab_ext)
        if len(ext) != len(keep[5]):
            raise ValueError('tab_ext must have one entry per table sample')
        keep.append(ext)
        pr.tab_ext = _ptr(ext)
    if ctab is not None:  # (coff, ca, cw, ctmin): Gauss-compressed companions of the band tables
        cx = [_i32(ctab[0]), _f64(ctab[1]), _f64(ctab[2]), _f64(ctab[3])]
        if len(cx[0]) != pr.n_filters + 1 or len(cx[3]) != pr.n_filters or len(cx[1]) != len(cx[2]):
            raise ValueError('inconsistent compressed tables')
        keep += cx
        pr.ctab_off, pr.ctab_a, pr.ctab_w, pr.ctab_tmin = _ptr(cx[0], _ip), _ptr(cx[1]), _ptr(cx[2]), _ptr(cx[3])
    if htab is not None:  # (hoff, ha, hw, htmin): the shorter "hot" level (needs ctab)
        hx = [_i32(htab[0]), _f64(htab[1]), _f64(htab[2]), _f64(htab[3])]
        if len(hx[0]) != pr.n_filters + 1 or len(hx[3]) != pr.n_filters or len(hx[1]) != len(hx[2]):
            raise ValueError('inconsistent hot-level tables')
        keep += hx
        pr.htab_off, pr.htab_a, pr.htab_w, pr.htab_tmin = _ptr(hx[0], _ip), _ptr(hx[1]), _ptr(hx[2]), _ptr(hx[3])
    if itab is not None:  # (coef[n_filters, m, 8], tmin[n_filters], u0, h): interpolants of ln S(ln T)
        ic, it = _f64(itab[0]), _f64(itab[1])
        if ic.ndim != 3 or ic.shape[0] != pr.n_filters or ic.shape[2] != 8 or it.shape != (pr.n_filters,):
            raise ValueError('inconsistent interpolant tables')
        keep += [ic, it]
        pr.itab_coef, pr.itab_tmin, pr.itab_m = _ptr(ic), _ptr(it), ic.shape[1]
        pr.itab_u0, pr.itab_h = float(itab[2]), float(itab[3])
    if companion is not None:
        kp, sp, dtp, knots, coef = companion
        extra = [_i32(kp), _i32(sp), _i32(dtp), _f64(knots), _f64(coef)]
        if extra[4].shape != (pr.n_filters, len(extra[3]) - 1, 4):
            raise ValueError('spline_coef must have shape (n_filters, n_knots - 1, 4)')
        keep += extra
        pr.filt_kasen_par, pr.filt_sifto_par, pr.filt_dt_par = (_ptr(x, _ip) for x in extra[:3])
        pr.n_knots = len(extra[3])
        pr.spline_knots, pr.spline_coef = _ptr(extra[3]), _ptr(extra[4])
    n_dim = pr.n_par + pr.use_sigma
    if priors is not None:
        if len(priors) != n_dim:
            raise ValueError(f'priors must have length {n_dim}')
        arr = (LcfPrior * n_dim)()
        for i, (kind, lo, hi, mean, std) in enumerate(priors):
            arr[i].kind, arr[i].p_min, arr[i].p_max, arr[i].mean, arr[i].stddev = int(kind), lo, hi, mean, std
        keep.append(arr)
        pr.priors = arr
    return pr, keep


class Engine:
    """One light curve + one model instance resident on one MI355X.

    Parameters are the fields of ``lcf_problem`` (see ``include/lcf.h``): ``priors`` is a sequence of
    ``(kind, p_min, p_max, mean, stddev)`` or ``None``.  ``filt_idx`` and ``tab_off`` None: the filter-less problem of
    the central-engine models (``n_filters = 0``, the table pointers NULL)."""

    def __init__(self, model_id, n_par, consts, t, y, dy, filt_idx, tab_off, tab_a, tab_w, use_sigma=False,
                 sigma_type=SIGMA_RELATIVE, priors=None, companion=None, device=0, ctab=None, tab_ext=None,
                 htab=None, itab=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        pr, _keep = make_problem(model_id, n_par, consts, t, y, dy, filt_idx, tab_off, tab_a, tab_w, use_sigma,
                                 sigma_type, priors, companion, ctab, tab_ext, htab, itab)
        self.ndim = pr.n_par + pr.use_sigma
        self.npoints = pr.n_points
        self.nfilters = pr.n_filters
        #: the prior descriptors the engine was created with (None: none)
        self.priors = None if priors is None else [tuple(p) for p in priors]
        self.device = int(device)
        self._create(pr)

    def _create(self, pr):
        """The native engine of ``pr`` on ``self.device`` (the engine copies what it keeps of the problem)."""
        _check(self._lib.lcf_engine_create(C.byref(pr), self.device, C.byref(self._h)))
        self.samples_per_eval = self._lib.lcf_engine_samples_per_eval(self._h)

    def close(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self._h = None   # (no module global is touched here: this also runs at interpreter shutdown)
            self._lib.lcf_engine_destroy(h)

    __del__ = close

    @property
    def handle(self):
        return self._h

    def set_variant(self, variant):
        _check(self._lib.lcf_engine_set_variant(self._h, int(variant)))

    def set_custom(self, program, redshift=0.):
        """Attach a :class:`CustomProgram` (engines created with ``MODEL_CUSTOM``) and the redshift its state function
        is handed."""
        _check(self._lib.lcf_engine_set_custom(self._h, program.handle))
        _check(self._lib.lcf_engine_set_custom_redshift(self._h, float(redshift)))
        self.program = program   # (kept alive with the engine)

    def set_limits(self, at, L_lim, dy):
        """Attach upper limits (``lcf_engine_set_limits``): ``at`` is an engine of the same model, constants and sigma
        mode on the limits' (t, filter); ``L_lim`` and ``dy`` have one entry per limit.  ``at=None`` detaches.  The
        log-likelihood then carries ``sum_j ln Phi((L_lim[j] - model_j) / sigma_j)``; the resident samplers refuse such
        an engine (``LcfError``, status 5), :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` takes it."""
        if at is None:
            _check(self._lib.lcf_engine_set_limits(self._h, None, 0, None, None))
            self.limits, self.nlimits = None, 0
            return
        L_lim, dy = _f64(L_lim), _f64(dy)
        if L_lim.ndim != 1 or L_lim.shape != dy.shape:
            raise ValueError('L_lim and dy must be 1-D and of equal length')
        _check(self._lib.lcf_engine_set_limits(self._h, at.handle, len(L_lim), _ptr(L_lim), _ptr(dy)))
        self.limits, self.nlimits = at, len(L_lim)   # (the limits' engine is kept alive with this one)

    def limit_terms(self, P):
        """``(n, n_limits)``: the ``ln Phi`` term of every (row, limit) of an engine with limits attached."""
        P = self._block(P)
        out = np.empty((len(P), getattr(self, 'nlimits', 0)))
        _check(self._lib.lcf_limit_terms(self._h, len(P), _ptr(P), _ptr(out)))
        return out

    def set_template(self, knots, coef, factor_par, offset_par, tmax_par, s_par, n_extra, priors=None):
        """Attach a second component (``lcf_engine_set_template``): a template per filter, the cubic coefficients ``coef``
        ``(n_filters, n_knots - 1, 4)`` on ``knots``, added to the model as ``r_f S_f((t - t_max - dt_f) / s)``.  The rows
        gain ``n_extra`` columns behind the model's own (in front of sigma): ``tmax_par`` and ``s_par`` are the columns of
        ``t_max`` and ``s``, ``factor_par`` / ``offset_par`` per filter those of its ``r_f`` / ``dt_f`` (-1: none).
        ``priors``: descriptors of ALL columns of the grown row, or None.  ``knots=None`` detaches.  ``ndim`` follows the
        engine's; the resident samplers refuse such an engine (``LcfError``, status 5),
        :class:`~lightcurve_fitting_amd.sampler.TemperedSampler` takes it."""
        if knots is None:
            _check(self._lib.lcf_engine_set_template(self._h, 0, None, None, None, None, -1, -1, 0, None))
            self.template = None
            self.priors = getattr(self, '_created_priors', self.priors)
        else:
            if not getattr(self, '_template_extra', 0):
                self._created_priors = self.priors
            knots, coef = _f64(knots), _f64(coef)
            fp, op = _i32(factor_par), _i32(offset_par)
            if knots.ndim != 1 or coef.shape != (self.nfilters, max(len(knots), 1) - 1, 4):
                raise ValueError('coef must have shape (n_filters, n_knots - 1, 4)')
            if fp.shape != (self.nfilters,) or op.shape != (self.nfilters,):
                raise ValueError('factor_par and offset_par must have one entry per filter')
            arr = None
            if priors is not None:
                arr = (LcfPrior * len(priors))()
                for i, (kind, lo, hi, mean, std) in enumerate(priors):
                    arr[i].kind, arr[i].p_min, arr[i].p_max, arr[i].mean, arr[i].stddev = int(kind), lo, hi, mean, std
                want = self._lib.lcf_engine_ndim(self._h) - getattr(self, '_template_extra', 0) + int(n_extra)
                if len(priors) != want:
                    raise ValueError(f'priors must have length {want}')
            _check(self._lib.lcf_engine_set_template(self._h, len(knots), _ptr(knots), _ptr(coef), _ptr(fp, _ip),
                                                     _ptr(op, _ip), int(tmax_par), int(s_par), int(n_extra), arr))
            self.template = (knots, coef)
            self.priors = None if priors is None else [tuple(p) for p in priors]
        self._template_extra = 0 if knots is None else int(n_extra)
        self.ndim = int(self._lib.lcf_engine_ndim(self._h))

    def evaluate_components(self, P, component='total'):
        """``(n, npoints)``: the model (``'total'``), the base model alone (``'base'``) or the template term alone
        (``'template'``) of an engine with a second component attached (``lcf_template_evaluate``)."""
        P = self._block(P)
        out = np.empty((len(P), self.npoints))
        _check(self._lib.lcf_template_evaluate(self._h, len(P), _ptr(P), TEMPLATE_COMPONENTS[component], _ptr(out)))
        return out

    def _block(self, P):
        P = _f64(P)
        if P.ndim == 1:
            P = P[None, :]
        if P.ndim != 2 or P.shape[1] != self.ndim:
            raise ValueError(f'parameter block must have shape (n, {self.ndim}), got {P.shape}')
        return P

    def log_likelihood(self, P):
        P = self._block(P)
        out = np.empty(len(P))
        _check(self._lib.lcf_log_likelihood(self._h, len(P), _ptr(P), _ptr(out)))
        return out

    def log_posterior(self, P):
        P = self._block(P)
        out = np.empty(len(P))
        _check(self._lib.lcf_log_posterior(self._h, len(P), _ptr(P), _ptr(out)))
        return out

    def log_likelihood_dev(self, n, dP, dout, stream=0, posterior=False):
        """Device pointers (ints), enqueue only."""
        fn = self._lib.lcf_log_posterior_dev if posterior else self._lib.lcf_log_likelihood_dev
        _check(fn(self._h, int(n), C.c_void_p(dP), C.c_void_p(dout), C.c_void_p(stream)))

    def evaluate(self, P):
        P = self._block(P)
        out = np.empty((len(P), self.npoints))
        _check(self._lib.lcf_model_evaluate(self._h, len(P), _ptr(P), _ptr(out)))
        return out

    def temperature_radius(self, P):
        P = self._block(P)
        T = np.empty((len(P), self.npoints))
        R = np.empty((len(P), self.npoints))
        _check(self._lib.lcf_temperature_radius(self._h, len(P), _ptr(P), _ptr(T), _ptr(R)))
        return T, R

    def profile_loglike_kernel(self, P, reps=20):
        """Average duration [ms] of the per-point likelihood kernel alone (HIP events, engine stream)."""
        P = self._block(P)
        ms = C.c_double()
        _check(self._lib.lcf_profile_loglike_kernel(self._h, len(P), _ptr(P), int(reps), C.byref(ms)))
        return ms.value

    def blackbody_to_filters(self, filt_idx, T, R):
        f, T, R = _i32(filt_idx), _f64(T), _f64(R)
        if not (f.shape == T.shape == R.shape and f.ndim == 1):
            raise ValueError('filt_idx, T and R must be 1-D and of equal length')
        out = np.empty(len(f))
        _check(self._lib.lcf_blackbody_to_filters(self._h, len(f), _ptr(f, _ip), _ptr(T), _ptr(R), _ptr(out)))
        return out


class CustomProgram:
    """A custom model's source compiled for one GPU architecture (``lcf_custom_compile``): ``arch`` such as
    ``'gfx950'``, or None for the architecture of ``device``.  A source that does not compile raises
    :class:`LcfError` carrying the compiler's log, in which the source's own lines are ``user_model:<line>``.  The
    library caches programs per process by (source, architecture): the same pair gives the same ``handle.value``."""

    def __init__(self, source, arch=None, device=0):
        self._lib = load_library()
        self.handle = C.c_void_p()
        self.source, self.arch = str(source), arch
        _check(self._lib.lcf_custom_compile(self.source.encode(), arch.encode() if arch else None, int(device),
                                            C.byref(self.handle)))

    @property
    def log(self):
        """The compiler's log (warnings; '' if none)."""
        return self._lib.lcf_custom_log(self.handle).decode()

    @property
    def code(self):
        """The code object, as bytes."""
        n = C.c_int64()
        ptr = self._lib.lcf_custom_code(self.handle, C.byref(n))
        return C.string_at(ptr, n.value) if ptr else b''


#: `lcf_sampler_last_run_kernel` values (include/lcf.h: LCF_KERNEL_*) -> the names `last_run_kernel()` returns
KERNEL_NAMES = {0: 'phases', 1: 'fused', 2: 'solo', 3: 'population', 4: 'population-phases', 5: 'run', 6: 'population-run'}


class NativeSampler:
    """Thin handle on ``lcf_sampler`` (device-resident stretch move)."""

    def __init__(self, engine, nwalkers, seed=0, a=2.0):
        self._lib = engine._lib
        self.engine = engine
        self.nwalkers = int(nwalkers)
        self.ndim = engine.ndim
        self._h = C.c_void_p()
        _check(self._lib.lcf_sampler_create(engine.handle, self.nwalkers, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                            float(a), C.byref(self._h)))

    def close(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self._h = None   # (no module global is touched here: this also runs at interpreter shutdown)
            self._lib.lcf_sampler_destroy(h)

    __del__ = close

    def set_state(self, coords):
        coords = _f64(coords)
        if coords.shape != (self.nwalkers, self.ndim):
            raise ValueError(f'coords must have shape ({self.nwalkers}, {self.ndim})')
        _check(self._lib.lcf_sampler_set_state(self._h, _ptr(coords)))

    def get_state(self):
        x = np.empty((self.nwalkers, self.ndim))
        lp = np.empty(self.nwalkers)
        _check(self._lib.lcf_sampler_get_state(self._h, _ptr(x), _ptr(lp)))
        return x, lp

    @staticmethod
    def _split(split, nsteps, nwalkers):
        """``split``: 'random' (device-generated, emcee's randomize_split), 'identity', or an int32 array
        (nsteps, nwalkers) of host-provided permutations."""
        if isinstance(split, str):
            return {'identity': SPLIT_IDENTITY, 'random': SPLIT_RANDOM}[split], None, None
        perm = _i32(split)
        if perm.shape != (nsteps, nwalkers):
            raise ValueError(f'perm must have shape ({nsteps}, {nwalkers})')
        return SPLIT_HOST, perm, _ptr(perm, _ip)

    def run(self, first_step, nsteps, split='random', store=True):
        mode, keep, pp = self._split(split, nsteps, self.nwalkers)
        _check(self._lib.lcf_sampler_run(self._h, int(first_step), int(nsteps), mode, pp, int(bool(store))))
        self._last = (int(nsteps), bool(store))

    def run_async(self, first_step, nsteps, split='random', store=True):
        """Enqueue the run and return; :meth:`wait` completes it (population mode: many samplers in flight)."""
        mode, keep, pp = self._split(split, nsteps, self.nwalkers)
        _check(self._lib.lcf_sampler_run_async(self._h, int(first_step), int(nsteps), mode, pp, int(bool(store))))
        self._last = (int(nsteps), bool(store))

    def wait(self):
        _check(self._lib.lcf_sampler_wait(self._h))

    def run_sharded(self, comm, first_step, nsteps, split='random', store=True):
        """Collective: the whole run natively over ``comm`` (a :class:`NativeComm`)."""
        mode, keep, pp = self._split(split, nsteps, self.nwalkers)
        _check(self._lib.lcf_sampler_run_sharded(self._h, comm._h, int(first_step), int(nsteps), mode, pp,
                                                 int(bool(store))))
        self._last = (int(nsteps), bool(store))

    def mailbox_export(self):
        """(64-byte IPC handle, local device pointer) of this rank's peer mailbox."""
        h = C.create_string_buffer(64)
        ptr = C.c_void_p()
        _check(self._lib.lcf_sampler_mailbox_export(self._h, h, C.byref(ptr)))
        return h.raw, ptr.value

    def mailbox_connect(self, n_ranks, rank, handles=None, local_ptrs=None):
        """Map every rank's mailbox: ``handles`` = the exported IPC handles of all ranks (other processes), or
        ``local_ptrs`` = their device pointers (ranks emulated inside this process)."""
        hb = C.create_string_buffer(b''.join(handles), 64 * n_ranks) if handles is not None else None
        lp = (C.c_void_p * n_ranks)(*local_ptrs) if local_ptrs is not None else None
        _check(self._lib.lcf_sampler_mailbox_connect(self._h, int(n_ranks), int(rank), hb, lp))

    def board_export(self):
        """(64-byte IPC handle, local device pointer) of this rank's row board (see ``lcf_sampler_run_rows``)."""
        h = C.create_string_buffer(64)
        ptr = C.c_void_p()
        _check(self._lib.lcf_sampler_board_export(self._h, h, C.byref(ptr)))
        return h.raw, ptr.value

    def board_connect(self, n_ranks, rank, handles=None, local_ptrs=None):
        """Map every rank's row board: IPC handles of all ranks, or device pointers of ranks emulated in this process."""
        hb = C.create_string_buffer(b''.join(handles), 64 * n_ranks) if handles is not None else None
        lp = (C.c_void_p * n_ranks)(*local_ptrs) if local_ptrs is not None else None
        _check(self._lib.lcf_sampler_board_connect(self._h, int(n_ranks), int(rank), hb, lp))

    def run_rows(self, first_step, nsteps, split='random', store=True, asynchronous=False):
        """Collective in effect: the sharded run in which nothing is replicated -- every rank moves its share of the
        walkers with the one-workgroup-per-proposal kernel and posts their rows on all ranks' boards (see
        ``lcf_sampler_run_rows``); ``asynchronous``: enqueue only, :meth:`wait` completes it."""
        mode, keep, pp = self._split(split, nsteps, self.nwalkers)
        fn = self._lib.lcf_sampler_run_rows_async if asynchronous else self._lib.lcf_sampler_run_rows
        _check(fn(self._h, int(first_step), int(nsteps), mode, pp, int(bool(store))))
        self._last = (int(nsteps), bool(store))

    def run_peers(self, first_step, nsteps, split='random', store=True, asynchronous=False):
        """Collective in effect: the sharded run over peer mailboxes (see ``lcf_sampler_run_peers``);
        ``asynchronous``: enqueue only, :meth:`wait` completes it."""
        mode, keep, pp = self._split(split, nsteps, self.nwalkers)
        fn = self._lib.lcf_sampler_run_peers_async if asynchronous else self._lib.lcf_sampler_run_peers
        _check(fn(self._h, int(first_step), int(nsteps), mode, pp, int(bool(store))))
        self._last = (int(nsteps), bool(store))

    def begin(self, first_step, nsteps, split='random', store=True):
        mode, keep, pp = self._split(split, nsteps, self.nwalkers)
        _check(self._lib.lcf_sampler_begin(self._h, int(first_step), int(nsteps), mode, pp, int(bool(store))))
        self._last = (int(nsteps), bool(store))

    def propose(self, step, half, stream=0):
        _check(self._lib.lcf_sampler_propose(self._h, int(step), int(half), C.c_void_p(stream)))

    def evaluate(self, lo, hi, stream=0):
        _check(self._lib.lcf_sampler_evaluate(self._h, int(lo), int(hi), C.c_void_p(stream)))

    def accept(self, step, half, stream=0):
        _check(self._lib.lcf_sampler_accept(self._h, int(step), int(half), C.c_void_p(stream)))

    def half_step(self, step, half, lo, hi, stream=0):
        _check(self._lib.lcf_sampler_half_step(self._h, int(step), int(half), int(lo), int(hi), C.c_void_p(stream)))

    def newlp_ptr(self):
        return self._lib.lcf_sampler_newlp_ptr(self._h)

    @property
    def one_launch(self):
        """True if a half-step of this sampler is a single kernel launch (see ``lcf_sampler_one_launch``)."""
        return bool(self._lib.lcf_sampler_one_launch(self._h))

    def last_run_kernel(self):
        """What executed the half-steps of the last run: 'phases' | 'fused' | 'solo' | 'run' (k_solo_run: resident
        workgroups, one launch per block of half-steps) | 'population' (one launch per half-step for all transients of
        a population) | 'population-run' (k_pop_run: resident workgroups for all transients) | 'population-phases'
        (None: no run yet)."""
        return KERNEL_NAMES.get(self._lib.lcf_sampler_last_run_kernel(self._h))

    def last_run_instance(self):
        """``(ND, NP, M, ranks)`` of the template instance the last run's half-step kernel was launched with: the
        compile-time fit dimension (0: generic), parts per workgroup (8: 1024 threads; 0: a population's kernels), the
        model whose own kernel it was (0: none), 1 for a row-board run.  Four times -1 for 'fused' / 'phases' / no run."""
        out = (C.c_int32 * 4)()
        self._lib.lcf_sampler_last_run_instance(self._h, out)
        return tuple(int(v) for v in out)

    def last_run_launches(self):
        """Launches of the half-step kernel in the last single-GPU run (two per step; 'run': one per block of steps)."""
        return int(self._lib.lcf_sampler_last_run_launches(self._h))

    def set_half_step_kernel(self, choice='auto'):
        """Restrict the kernels a single-GPU run uses for a half-step ('auto' | 'solo' | 'fused' | 'phases'; same
        chain bit for bit).  Returns what a run uses now: 'run' (one workgroup per proposal, accept test included,
        resident for a block of half-steps), 'solo' (the same with a launch per half-step), 'fused' (one workgroup per
        proposal and part) or 'phases' (proposal + likelihood launches)."""
        used = C.c_int32()
        _check(self._lib.lcf_sampler_set_half_step_kernel(self._h, {'auto': 0, 'fused': 1, 'phases': 2, 'solo': 3}[choice],
                                                          C.byref(used)))
        return {3: 'run', 2: 'solo', 1: 'fused', 0: 'phases'}[used.value]

    def half_step_rows(self, step, half, lo, hi, stream=0):
        _check(self._lib.lcf_sampler_half_step_rows(self._h, int(step), int(half), int(lo), int(hi),
                                                    C.c_void_p(stream)))

    def rows_ptr(self):
        """(device pointer, doubles per row) of the per-proposal rows of the half-step drawn last."""
        n = C.c_int32()
        return self._lib.lcf_sampler_rows_ptr(self._h, C.byref(n)), int(n.value)

    def check(self):
        _check(self._lib.lcf_sampler_check(self._h))

    def reserve_chain(self, n_steps):
        """Allocate the device memory a stored run of n_steps steps needs now, instead of inside that run."""
        _check(self._lib.lcf_sampler_reserve_chain(self._h, int(n_steps)))

    def get_chain(self):
        nsteps, store = self._last
        chain = np.empty((nsteps, self.nwalkers, self.ndim))
        lp = np.empty((nsteps, self.nwalkers))
        _check(self._lib.lcf_sampler_get_chain(self._h, _ptr(chain), _ptr(lp)))
        return chain, lp

    def snapshot(self):
        """``(coords, log_prob, n_accepted)`` of the sampler's present state in one native call."""
        x = np.empty((self.nwalkers, self.ndim))
        lp = np.empty(self.nwalkers)
        acc = np.empty(self.nwalkers, dtype=np.int64)
        _check(self._lib.lcf_sampler_get_snapshot(self._h, x.ctypes.data, lp.ctypes.data, acc.ctypes.data))
        return x, lp, acc

    def naccepted(self):
        out = np.empty(self.nwalkers, dtype=np.int64)
        _check(self._lib.lcf_sampler_get_naccepted(self._h, _i64p(out)))
        return out

    def last_run_ms(self):
        return float(self._lib.lcf_sampler_last_run_ms(self._h))


class NativeTempered:
    """Thin handle on ``lcf_tempered`` (parallel-tempered ensembles): ``ntemps`` rungs of ``nwalkers`` walkers."""

    STORE = {False: 0, True: 1, 'append': 2}

    def __init__(self, engine, betas, nwalkers, seed=0, a=2.0):
        self._lib = engine._lib
        self.engine = engine
        betas = _f64(betas)
        self.ntemps, self.nwalkers, self.ndim = len(betas), int(nwalkers), engine.ndim
        self._h = C.c_void_p()
        _check(self._lib.lcf_tempered_create(engine.handle, self.ntemps, _ptr(betas), self.nwalkers,
                                             C.c_uint64(int(seed) & (2 ** 64 - 1)), float(a), C.byref(self._h)))

    def close(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self._h = None   # (no module global is touched here: this also runs at interpreter shutdown)
            self._lib.lcf_tempered_destroy(h)

    __del__ = close

    def set_state(self, coords):
        coords = _f64(coords)
        if coords.shape != (self.ntemps, self.nwalkers, self.ndim):
            raise ValueError(f'coords must have shape ({self.ntemps}, {self.nwalkers}, {self.ndim})')
        _check(self._lib.lcf_tempered_set_state(self._h, _ptr(coords)))

    def get_state(self):
        """``(x (K, W, D), lnL (K, W), lnpr (K, W))``"""
        x = np.empty((self.ntemps, self.nwalkers, self.ndim))
        ll, lpr = np.empty(x.shape[:2]), np.empty(x.shape[:2])
        _check(self._lib.lcf_tempered_get_state(self._h, _ptr(x), _ptr(ll), _ptr(lpr)))
        return x, ll, lpr

    def run(self, first_step, nsteps, store=True):
        """``store``: False, True (the run replaces the stored chain) or 'append'."""
        _check(self._lib.lcf_tempered_run(self._h, int(first_step), int(nsteps), self.STORE[store]))

    def get_chain(self, nstored):
        """``(chain (nstored, K, W, D), lnL (nstored, K, W))`` of the ``nstored`` steps the device holds."""
        chain = np.empty((int(nstored), self.ntemps, self.nwalkers, self.ndim))
        ll = np.empty(chain.shape[:3])
        if nstored:
            _check(self._lib.lcf_tempered_get_chain(self._h, _ptr(chain), _ptr(ll)))
        return chain, ll

    def counts(self):
        """``(n_accepted (K, W), swaps_accepted (K-1,), swaps_proposed (K-1,))`` since the last ``set_state``."""
        acc = np.zeros((self.ntemps, self.nwalkers), dtype=np.int64)
        sa, sp = np.zeros(self.ntemps - 1, dtype=np.int64), np.zeros(self.ntemps - 1, dtype=np.int64)
        _check(self._lib.lcf_tempered_get_counts(self._h, _i64p(acc), _i64p(sa), _i64p(sp)))
        return acc, sa, sp

    def mean_loglike(self, discard=0):
        out = np.empty(self.ntemps)
        _check(self._lib.lcf_tempered_mean_loglike(self._h, int(discard), _ptr(out)))
        return out

    def run_adaptive(self, first_step, nsteps, store, lag, time, t0):
        """``run`` with the ladder adapting on the device; ``t0``: the adapting steps made before this run."""
        _check(self._lib.lcf_tempered_run_adaptive(self._h, int(first_step), int(nsteps), self.STORE[store], float(lag),
                                                   float(time), int(t0)))

    def get_betas(self):
        """The ladder now, (K,)."""
        out = np.empty(self.ntemps)
        _check(self._lib.lcf_tempered_get_betas(self._h, _ptr(out)))
        return out

    def get_beta_history(self, nstored):
        """(nstored, K): the ladder every stored step was sampled under."""
        out = np.empty((int(nstored), self.ntemps))
        if nstored:
            _check(self._lib.lcf_tempered_get_beta_history(self._h, _ptr(out)))
        return out

    def stepping_stones(self, discard, batches):
        """``(max, sum, count)``, each (K - 1, batches): the stepping-stone partials of every pair and batch."""
        m, s, n = (np.empty((self.ntemps - 1, int(batches))) for _ in range(3))
        _check(self._lib.lcf_tempered_stepping_stones(self._h, int(discard), int(batches), _ptr(m), _ptr(s), _ptr(n)))
        return m, s, n

    def set_moves(self, kinds, cum_weights, params):
        """The moves of the steps from the next run on: ``kinds`` (n,) of ``MOVE_*``, ``cum_weights`` (n,) ascending to
        exactly 1, ``params`` (n, 2).  ``n = 0`` restores the stretch move alone.  State and counts stay."""
        kinds, cum, params = _i32(kinds).ravel(), _f64(cum_weights).ravel(), _f64(params).reshape(-1, 2)
        if not len(kinds) == len(cum) == len(params):
            raise ValueError('kinds, cum_weights and params must have one length')
        _check(self._lib.lcf_tempered_set_moves(self._h, len(kinds), _ptr(kinds, _ip), _ptr(cum), _ptr(params)))

    def get_move_history(self, nstored):
        """(nstored, K) of ``MOVE_*``: the kind of move every rung made in every stored step."""
        out = np.zeros((int(nstored), self.ntemps), dtype=np.int32)
        if nstored:
            _check(self._lib.lcf_tempered_get_move_history(self._h, _ptr(out, _ip)))
        return out


def population_run(native_samplers, first_step, nsteps, split='random', store=True):
    """One batched native run over several :class:`NativeSampler` objects (population mode).  Returns device ms."""
    lib = load_library()
    n = len(native_samplers)
    arr = _handles(native_samplers)
    mode = {'identity': SPLIT_IDENTITY, 'random': SPLIT_RANDOM}[split]
    ms = C.c_double()
    _check(lib.lcf_population_run(arr, n, int(first_step), int(nsteps), mode, int(bool(store)), C.byref(ms)))
    for s in native_samplers:
        s._last = (int(nsteps), bool(store))
    return ms.value


def rccl_library_path():
    """The librccl.so PyTorch ships (so that one RCCL serves torch.distributed and the native loop), or ''."""
    try:
        import torch
        cand = os.path.join(os.path.dirname(torch.__file__), 'lib', 'librccl.so')
        return cand if os.path.exists(cand) else ''
    except ImportError:
        return ''


class NativeComm:
    """An RCCL communicator owned by the native library, bootstrapped over an initialised torch.distributed group
    (the 128-byte unique id is broadcast from rank 0)."""

    @staticmethod
    def probe():
        """True if RCCL can be bound in this process (local check, no communication)."""
        return load_library().lcf_comm_probe(rccl_library_path().encode()) == 0

    def __init__(self, device, group=None):
        import torch.distributed as dist
        self._lib = load_library()
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        path = rccl_library_path().encode()
        uid = C.create_string_buffer(128)
        if self.rank == 0:
            _check(self._lib.lcf_comm_unique_id(path, uid))
        box = [uid.raw]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        uid = C.create_string_buffer(box[0], 128)
        self._h = C.c_void_p()
        _check(self._lib.lcf_comm_create(path, uid, self.world, self.rank, int(device), C.byref(self._h)))

    def count(self):
        """(number of ranks, this rank) as RCCL's communicator reports them."""
        n, r = C.c_int32(), C.c_int32()
        _check(self._lib.lcf_comm_count(self._h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def time_allgather(self, native_sampler, reps=200):
        """Average ms of one per-half-step all-gather of ``native_sampler``'s rows (collective call)."""
        ms = C.c_double()
        _check(self._lib.lcf_comm_time_allgather(self._h, native_sampler._h, int(reps), C.byref(ms)))
        return ms.value

    def close(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self._h = None   # (no module global is touched here: this also runs at interpreter shutdown)
            self._lib.lcf_comm_destroy(h)

    __del__ = close


class SedEngine:
    """Per-epoch blackbody SED likelihood on the device (``lcf_sed_*``): band tables are fixed at creation,
    observations are set per batch of epochs, candidates are evaluated per call."""

    def __init__(self, tab_off, tab_a, tab_w, device=0, ctab=None, itab=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        off, a, w = _i32(tab_off), _f64(tab_a), _f64(tab_w)
        if ctab is None:
            cargs = (None, None, None, None)
        else:
            cx = [_i32(ctab[0]), _f64(ctab[1]), _f64(ctab[2]), _f64(ctab[3])]
            cargs = (_ptr(cx[0], _ip), _ptr(cx[1]), _ptr(cx[2]), _ptr(cx[3]))
        if itab is None:   # (coef[n_filters, m, 8], tmin[n_filters], u0, h): interpolants of ln S(ln T)
            iargs = (None, None, 0, 0., 0.)
        else:
            ic, it = _f64(itab[0]), _f64(itab[1])
            if ic.ndim != 3 or ic.shape[0] != len(off) - 1 or ic.shape[2] != 8 or it.shape != (len(off) - 1,):
                raise ValueError('inconsistent interpolants')
            iargs = (_ptr(ic), _ptr(it), ic.shape[1], float(itab[2]), float(itab[3]))
        #: whether precision 2 runs through the interpolants.  The library stages them in the fast kernel's LDS
        #: (lcf_sed_create: 80-byte rows, 2 KiB of exponential table, 80 KiB in all -- 13 filters of the per-epoch
        #: engine's 74 intervals); a set that does not fit is not used, and precision 2 then computes what precision 0
        #: does, sample by sample.  (tests/test_gpu_sed_edges.py holds this flag to the library's behaviour.)
        self.has_interpolants = itab is not None and self.interpolants_fit(len(off) - 1, iargs[2])
        _check(self._lib.lcf_sed_create(len(off) - 1, _ptr(off, _ip), _ptr(a), _ptr(w), *cargs, *iargs, int(device),
                                        C.byref(self._h)))
        self.n_epochs = 0
        self.last_kernel_ms = 0.

    @staticmethod
    def interpolants_fit(n_filters, m):
        """lcf_sed_create's rule: ``n_filters`` interpolants of ``m`` intervals fit the fast kernel's LDS."""
        return n_filters * m * 80 + 256 * 8 <= 80 * 1024

    def close(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self._h = None   # (no module global is touched here: this also runs at interpreter shutdown)
            self._lib.lcf_sed_destroy(h)

    __del__ = close

    def set_observations(self, ep_off, filt_idx, y, dy):
        off, f, y, dy = _i32(ep_off), _i32(filt_idx), _f64(y), _f64(dy)
        if not (len(f) == len(y) == len(dy) == off[-1]):
            raise ValueError('filt_idx, y, dy must have ep_off[-1] entries')
        _check(self._lib.lcf_sed_set_observations(self._h, len(off) - 1, _ptr(off, _ip), _ptr(f, _ip), _ptr(y), _ptr(dy)))
        self.n_epochs = len(off) - 1

    def log_likelihood(self, cand, sigma_type=SIGMA_RELATIVE, precision=0, compressed=True):
        """``cand``: (n_epochs, n_cand, 2 or 3) -> (n_epochs, n_cand)."""
        cand = _f64(cand)
        if cand.ndim != 3 or cand.shape[0] != self.n_epochs or cand.shape[2] not in (2, 3):
            raise ValueError(f'candidates must have shape ({self.n_epochs}, n_cand, 2|3), got {cand.shape}')
        out = np.empty(cand.shape[:2])
        ms = C.c_double()
        _check(self._lib.lcf_sed_log_likelihood(self._h, cand.shape[1], cand.shape[2], int(sigma_type), _ptr(cand),
                                                int(precision), int(bool(compressed)), _ptr(out), C.byref(ms)))
        self.last_kernel_ms = ms.value
        return out


def bb_lstsq(ep_off, freq, lum, p0, lo, hi, z=0., cutoff_freq=np.inf, max_iter=500, xtol=1e-12, device=0):
    """``lcf_bb_lstsq``: bounded least-squares blackbody fits of many epochs in one launch.  ``p0``, ``lo``, ``hi``:
    (n_epochs, 2).  Returns ``(out[n_epochs, 8], status[n_epochs])`` (columns: T, R, cost, cov_TT, cov_TR, cov_RR,
    iterations, 0)."""
    lib = load_library()
    off, freq, lum = _i32(ep_off), _f64(freq), _f64(lum)
    n = len(off) - 1
    if n < 0 or off[0] != 0 or not (len(freq) == len(lum) == off[-1]):
        raise ValueError('freq and lum must have ep_off[-1] entries, ep_off[0] == 0')
    p0, lo, hi = (_f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (n, 2))) for a in (p0, lo, hi))
    out = np.empty((n, 8))
    status = np.empty(n, dtype=np.int32)
    _check(lib.lcf_bb_lstsq(int(device), n, _ptr(off, _ip), _ptr(freq), _ptr(lum), _ptr(p0), _ptr(lo), _ptr(hi),
                            float(z), float(cutoff_freq), int(max_iter), float(xtol), _ptr(out), _ptr(status, _ip)))
    return out, status


def bb_luminosity(T, R, z, freq0, n_grid, cutoff_freq=np.inf, device=0):
    """``lcf_bb_luminosity``: (L_pseudo, L_bol) [W] of every (T, R) sample."""
    lib = load_library()
    T, R = _f64(T), _f64(R)
    if T.shape != R.shape:
        raise ValueError('T and R must have the same shape')
    Lp, Lb = np.empty(T.shape), np.empty(T.shape)
    _check(lib.lcf_bb_luminosity(int(device), T.size, _ptr(T), _ptr(R), float(z), float(freq0), int(n_grid),
                                 float(cutoff_freq), _ptr(Lp), _ptr(Lb)))
    return Lp, Lb


def autocorr_time(chain, c=5., device=0):
    """``lcf_autocorr_time``: emcee's integrated autocorrelation time (without the ``tol`` check) of a host chain
    (n_t, n_w, n_d).  Returns ``(tau[n_d], window[n_d])``."""
    lib = load_library()
    x = _f64(chain)
    if x.ndim != 3:
        raise ValueError('chain must have shape (n_t, n_w, n_d)')
    n_t, n_w, n_d = x.shape
    tau, window = np.empty(n_d), np.empty(n_d, dtype=np.int64)
    _check(lib.lcf_autocorr_time(int(device), _ptr(x), n_t, n_w, n_d, float(c), _ptr(tau), _i64p(window)))
    return tau, window


def samplers_autocorr_time(native_samplers, discard=0, thin=1, c=5.):
    """``lcf_samplers_autocorr_time``: the same for the device-resident chains of the last stored run of several
    :class:`NativeSampler` objects (one sequence of launches for all).  Returns a list of ``(tau, window)``."""
    lib = load_library()
    total = sum(s.ndim for s in native_samplers)
    tau, window = np.empty(total), np.empty(total, dtype=np.int64)
    _check(lib.lcf_samplers_autocorr_time(_handles(native_samplers), len(native_samplers), int(discard), int(thin),
                                          float(c), _ptr(tau), _i64p(window)))
    out, k = [], 0
    for s in native_samplers:
        out.append((tau[k:k + s.ndim].copy(), window[k:k + s.ndim].copy()))
        k += s.ndim
    return out


#: ``component`` of the predictive entry points
COMPONENT_MODEL, COMPONENT_SIFTO = 0, 1
#: filters x percentiles one native predictive call takes (include/lcf.h)
PREDICT_MAX_SEARCHES = 512
#: device memory of a predictive call beyond the samples, unless the caller says otherwise
PREDICT_WORKSPACE_BYTES = 1 << 30


def _predict_call(lib, name, grid_engine, samples, discard, thin, tail):
    """``lcf_sampler_<name>`` on the last stored run of a :class:`NativeSampler` (rows ``discard::thin``, read in
    place), else ``lcf_<name>`` on a host array (n, ld); ``tail``: the arguments behind the samples."""
    if isinstance(samples, NativeSampler):
        _check(getattr(lib, 'lcf_sampler_' + name)(grid_engine.handle, samples._h, int(discard), int(thin), *tail))
    else:
        P = _f64(samples)
        if P.ndim != 2:
            raise ValueError('samples must have shape (n, n_columns)')
        _check(getattr(lib, 'lcf_' + name)(grid_engine.handle, _ptr(P), P.shape[0], P.shape[1], *tail))


def predict_quantiles(grid_engine, samples, percentiles, component=COMPONENT_MODEL, workspace_bytes=None, discard=0,
                      thin=1):
    """``lcf_predict_quantiles`` / ``lcf_sampler_predict_quantiles``: percentiles over all samples of the model on
    the points of ``grid_engine`` (an evaluation engine).  ``samples``: a host array (n, ld), or a
    :class:`NativeSampler` whose last stored run is read in place (rows ``discard::thin``).  Returns
    ``(quantiles[n_q, n_points], n_valid[n_points])``."""
    lib = load_library()
    q = _f64(percentiles)
    out = np.empty((len(q), grid_engine.npoints))
    n_valid = np.empty(grid_engine.npoints, dtype=np.int64)
    ws = PREDICT_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    _predict_call(lib, 'predict_quantiles', grid_engine, samples, discard, thin,
                  (int(component), _ptr(q), len(q), ws, _ptr(out), _i64p(n_valid)))
    return out, n_valid


#: the series of a thermal call: T [kK], R_bb [1000 Rsun], L_bol [W]
THERMAL_SERIES = 3


def predict_thermal(grid_engine, samples, percentiles, T_floor=8.12, workspace_bytes=None, discard=0, thin=1):
    """``lcf_predict_thermal`` / ``lcf_sampler_predict_thermal``: percentiles over all samples of T, R_bb and L_bol on
    the times of ``grid_engine`` (an evaluation engine with one point per distinct time), with the validity counters.
    ``samples`` as for :func:`predict_quantiles`; at most ``PREDICT_MAX_SEARCHES // 3`` percentiles.  Returns
    ``(quantiles[3, n_q, n_t], n_valid[3, n_t], n_cold[n_t], n_inside[n_t])``."""
    lib = load_library()
    q = _f64(percentiles)
    n_t = grid_engine.npoints
    out = np.empty((THERMAL_SERIES, len(q), n_t))
    n_valid = np.empty((THERMAL_SERIES, n_t), dtype=np.int64)
    n_cold, n_inside = np.empty(n_t, dtype=np.int64), np.empty(n_t, dtype=np.int64)
    ws = PREDICT_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    _predict_call(lib, 'predict_thermal', grid_engine, samples, discard, thin,
                  (_ptr(q), len(q), float(T_floor), ws, _ptr(out), _i64p(n_valid), _i64p(n_cold), _i64p(n_inside)))
    return out, n_valid, n_cold, n_inside


#: filters of one native colour call (include/lcf.h): 4 KiB of LDS each in a pass workgroup
COLOR_MAX_FILTERS = 16


def _hist_bits(n_series):
    """The largest of 4 ... 11 bits for which ``n_series 2^b`` four-byte counters fit 48 KiB of LDS."""
    b = 4
    while b < 11 and (n_series << (b + 1)) * 4 <= 48 * 1024:
        b += 1
    return b


def color_workspace(n_samples, n_times, n_colors, n_q, tile=1):
    """Device memory [bytes] beyond the samples that :func:`predict_colors` needs to work through ``tile`` times at
    once -- the least ``workspace_bytes`` for that tile ("Colour bands and peaks")::

        fixed    = 64 n_samples + 8 (n_q + 1) n_colors n_times + 4 n_colors n_times + 16 n_colors + 4096
        per time = n_colors n_q (56 + 8 * 2048) + 4 max(n_colors 2^b0, n_colors n_q 2^b1)

    with ``b0`` / ``b1`` the largest of 4 ... 11 for which ``n_colors 2^b0`` / ``n_colors n_q 2^b1`` four-byte counters
    fit 48 KiB of LDS.  Nothing is stored per (sample, time).  The peaks are results per sample and lie OUTSIDE the
    workspace: :func:`color_peak_bytes`."""
    ns = n_colors * n_q
    fixed = 64 * n_samples + 8 * (n_q + 1) * n_colors * n_times + 4 * n_colors * n_times + 16 * n_colors + 4096
    hist = 4 * max(n_colors << _hist_bits(n_colors), ns << _hist_bits(ns))
    return fixed + tile * (ns * (56 + 8 * 2048) + hist)


def color_peak_bytes(n_samples, n_filters):
    """Device memory [bytes] of the peaks of :func:`predict_colors` while the call runs, beyond ``workspace_bytes``: a
    float64 and an int32 per (sample, filter)."""
    return 12 * n_samples * n_filters


def predict_colors(grid_engine, samples, pairs, dzp, percentiles, workspace_bytes=None, peak=True, discard=0, thin=1):
    """``lcf_predict_colors`` / ``lcf_sampler_predict_colors``: percentiles over all samples of the colours ``pairs``
    (n_c, 2) -- indices into the filters of ``grid_engine``, an evaluation engine on the dense grid, filter-major --
    with the zero-point differences ``dzp`` (n_c,), and with ``peak`` every (sample, filter)'s largest value and the
    first time it is attained.  ``samples`` as for :func:`predict_quantiles`; ``n_c * n_q <= PREDICT_MAX_SEARCHES``.
    Returns ``(color[n_q, n_c, n_t], n_valid[n_c, n_t], y_peak[n_f, n] or None, peak_index[n_f, n] or None)``."""
    lib = load_library()
    q = _f64(percentiles)
    pairs, dzp = _i32(pairs), _f64(dzp)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or dzp.shape != (len(pairs),):
        raise ValueError('pairs must have shape (n_c, 2) and dzp shape (n_c,)')
    n_c, n_f = len(pairs), grid_engine.nfilters
    n_t = grid_engine.npoints // max(n_f, 1)
    if not peak:
        n = 0
    elif isinstance(samples, NativeSampler):   # (the peaks are per sample: their number has to be known here)
        n_steps, stored = getattr(samples, '_last', (0, False))
        if not stored or int(discard) < 0 or int(thin) < 1 or int(discard) >= n_steps:
            raise ValueError('the sampler\'s last run stored no chain, or discard / thin leave none of it')
        n = len(range(int(discard), n_steps, int(thin))) * samples.nwalkers
    else:
        n = np.shape(samples)[0]
    out = np.empty((len(q), n_c, n_t))
    n_valid = np.empty((n_c, n_t), dtype=np.int64)
    y_peak = np.empty((n_f, n)) if peak else None
    peak_index = np.empty((n_f, n), dtype=np.int32) if peak else None
    ws = PREDICT_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    _predict_call(lib, 'predict_colors', grid_engine, samples, discard, thin,
                  (n_c, _ptr(pairs, _ip), _ptr(dzp), _ptr(q), len(q), ws, _ptr(out), _i64p(n_valid),
                   _ptr(y_peak) if peak else None, _ptr(peak_index, _ip) if peak else None))
    return out, n_valid, y_peak, peak_index


def luminosity_workspace(n_samples, n_times, n_q, tile=1, peak=True):
    """Device memory [bytes] beyond the samples that :func:`predict_luminosity` needs to work through ``tile`` times at
    once -- the least ``workspace_bytes`` for that tile ("Luminosity bands and peaks")::

        fixed    = (12 if peak else 0) n_samples + 8 (n_q + 1) n_times + 12 n_times + 4096
        per time = 8 n_samples + n_q (56 + 8 * 2048) + 4 max(2048, n_q 2^b)

    with ``b`` the largest of 4 ... 11 for which ``n_q 2^b`` four-byte counters fit 48 KiB of LDS."""
    b = 4
    while b < 11 and (n_q << (b + 1)) * 4 <= 48 * 1024:
        b += 1
    fixed = (12 if peak else 0) * n_samples + 8 * (n_q + 1) * n_times + 12 * n_times + 4096
    return fixed + tile * (8 * n_samples + n_q * (56 + 8 * 2048) + 4 * max(2048, n_q << b))


def predict_luminosity(grid_engine, samples, percentiles, workspace_bytes=None, peak=True):
    """``lcf_predict_luminosity``: percentiles over all samples of ``L(t)`` of a central-engine model on the epochs of
    ``grid_engine`` (an evaluation engine of ``Arnett`` / ``Magnetar``), the valid and dark counts per epoch and, with
    ``peak``, every sample's largest ``L`` and the first epoch it is attained at.  ``samples``: a host array (n, ld);
    at most ``PREDICT_MAX_SEARCHES`` percentiles.  Every value is evaluated once and kept as a key: see
    :func:`luminosity_workspace` for the memory.  Returns ``(quantiles[n_q, n_t], n_valid[n_t], n_dark[n_t], L_peak[n]
    or None, i_peak[n] or None)``."""
    lib = load_library()
    q = _f64(percentiles)
    P = _f64(samples)
    if P.ndim != 2:
        raise ValueError('samples must have shape (n, n_columns)')
    n_t = grid_engine.npoints
    out = np.empty((len(q), n_t))
    n_valid, n_dark = np.empty(n_t, dtype=np.int64), np.empty(n_t, dtype=np.int64)
    L_peak = np.empty(P.shape[0]) if peak else None
    i_peak = np.empty(P.shape[0], dtype=np.int32) if peak else None
    ws = PREDICT_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    _check(lib.lcf_predict_luminosity(grid_engine.handle, _ptr(P), P.shape[0], P.shape[1], _ptr(q), len(q), ws, _ptr(out),
                                      _i64p(n_valid), _i64p(n_dark), _ptr(L_peak) if peak else None,
                                      _ptr(i_peak, _ip) if peak else None))
    return out, n_valid, n_dark, L_peak, i_peak


def custom_workspace(n_samples, n_times, n_filters, n_q, tile=1):
    """Device memory [bytes] beyond the samples that :func:`predict_custom` needs to work through ``tile`` times at
    once -- the least ``workspace_bytes`` for that tile ("Bands of a custom model").  With
    ``S = n_filters + 3`` series per time (the filters, then T, R, L)::

        fixed    = 8 (n_q + 1) S n_times + 20 S n_times + 4096
        per time = S (8 n_samples + n_q (56 + 8 * 2048) + 4 max(2048, n_q 2^b))

    with ``b`` the largest of 4 ... 11 for which ``n_q 2^b`` four-byte counters fit 48 KiB of LDS."""
    b = 4
    while b < 11 and (n_q << (b + 1)) * 4 <= 48 * 1024:
        b += 1
    series = n_filters + THERMAL_SERIES
    fixed = 8 * (n_q + 1) * series * n_times + 20 * series * n_times + 4096
    return fixed + tile * series * (8 * n_samples + n_q * (56 + 8 * 2048) + 4 * max(2048, n_q << b))


def predict_custom(grid_engine, samples, percentiles, T_floor=None, workspace_bytes=None):
    """``lcf_predict_custom``: percentiles over all samples of a custom model's light curves and of the T, R and L
    behind them, on the dense filters x distinct-times grid of ``grid_engine`` (an evaluation engine of a
    ``CustomModel``), with the valid and dark counts and -- with ``T_floor`` -- the samples colder than it per time.
    ``samples``: a host array (n, ld); at most ``PREDICT_MAX_SEARCHES`` percentiles.  The state function runs once per
    (sample, time) and every value is kept as a key: see :func:`custom_workspace` for the memory.  Returns
    ``(quantiles[n_q, n_f + 3, n_t], n_valid[n_f + 3, n_t], n_dark[n_f, n_t], n_cold[n_t] or None)``, filters in the
    engine's order, then T, R, L; times ascending."""
    lib = load_library()
    q = _f64(percentiles)
    P = _f64(samples)
    if P.ndim != 2:
        raise ValueError('samples must have shape (n, n_columns)')
    n_f = grid_engine.nfilters
    n_t = grid_engine.npoints // max(n_f, 1)
    out = np.empty((len(q), n_f + THERMAL_SERIES, n_t))
    n_valid = np.empty((n_f + THERMAL_SERIES, n_t), dtype=np.int64)
    n_dark = np.empty((n_f, n_t), dtype=np.int64)
    n_cold = None if T_floor is None else np.empty(n_t, dtype=np.int64)
    ws = PREDICT_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    _check(lib.lcf_predict_custom(grid_engine.handle, _ptr(P), P.shape[0], P.shape[1], _ptr(q), len(q),
                                  -1. if T_floor is None else float(T_floor), ws, _ptr(out), _i64p(n_valid),
                                  _i64p(n_dark), None if n_cold is None else _i64p(n_cold)))
    return out, n_valid, n_dark, n_cold


#: filters of one native template call (include/lcf.h)
TEMPLATE_MAX_FILTERS = 16
#: per (filter, sample): the values and the indices of :func:`template_features`, in their order
TEMPLATE_FEATURE_VALUES = ('y_peak_base', 'y_peak_template', 'y_dip')
TEMPLATE_FEATURE_INDICES = ('i_peak_base', 'i_peak_template', 'i_cross', 'i_dip')


def template_components(components):
    """``(names in the order the results come out, mask)`` of the ``components`` of :func:`predict_template`: a name or
    a non-empty sequence of distinct names out of ``'total'``, ``'base'``, ``'template'``."""
    if isinstance(components, str):
        components = (components,)
    components = tuple(components)
    bad = [c for c in components if c not in TEMPLATE_MASK]
    if len(components) == 0 or bad or len(set(components)) != len(components):
        raise ValueError("components must be a non-empty selection of distinct names out of 'total', 'base', 'template'"
                         + (f', not {bad[0]!r}' if bad else ''))
    names = tuple(c for c in TEMPLATE_MASK if c in components)
    return names, sum(TEMPLATE_MASK[c] for c in names)


def template_workspace(n_samples, n_times, n_filters, n_components, n_q, tile=1):
    """Device memory [bytes] beyond the samples that :func:`predict_template` needs to work through ``tile`` times at
    once -- the least ``workspace_bytes`` for that tile ("Bands and features of a template fit").  With
    ``S = n_components n_filters`` series per time::

        fixed    = 64 n_samples + 8 (n_q + 1) S n_times + (4 S + 8 n_filters) n_times + 4096
        per time = S n_q (56 + 8 * 2048) + 4 max(S 2^b0, S n_q 2^b1)

    with ``b0`` / ``b1`` the largest of 4 ... 11 for which ``S 2^b0`` / ``S n_q 2^b1`` four-byte counters fit 48 KiB of
    LDS.  Nothing is stored per (sample, time).  The features of :func:`template_features` are a call of their own:
    ``(64 + 40 n_filters) n_samples`` bytes."""
    series = n_components * n_filters
    ns = series * n_q
    fixed = 64 * n_samples + 8 * (n_q + 1) * series * n_times + (4 * series + 8 * n_filters) * n_times + 4096
    hist = 4 * max(series << _hist_bits(series), ns << _hist_bits(ns))
    return fixed + tile * (ns * (56 + 8 * 2048) + hist)


def _template_samples(grid_engine, samples):
    P = _f64(samples)
    if P.ndim != 2:
        raise ValueError('samples must have shape (n, n_columns)')
    n_f = grid_engine.nfilters
    return P, n_f, grid_engine.npoints // max(n_f, 1)


def predict_template(grid_engine, samples, percentiles, components=('total', 'base', 'template'), workspace_bytes=None):
    """``lcf_predict_template``: percentiles over all samples of the sum, the base model's term and the template term of
    an engine with a second component attached, on the dense filters x distinct-times grid of ``grid_engine``
    (filter-major), with the valid counts and the samples whose base term is exactly ``+0.0``.  ``samples``: a host
    array (n, ld); ``n_components * n_filters * n_q <= PREDICT_MAX_SEARCHES``.  Returns ``(quantiles[n_q, n_c, n_f, n_t],
    n_valid[n_c, n_f, n_t], n_dark[n_f, n_t], names)``, the components in the order ``names`` (total, base, template)."""
    lib = load_library()
    q = _f64(percentiles)
    names, mask = template_components(components)
    P, n_f, n_t = _template_samples(grid_engine, samples)
    out = np.empty((len(q), len(names), n_f, n_t))
    n_valid = np.empty((len(names), n_f, n_t), dtype=np.int64)
    n_dark = np.empty((n_f, n_t), dtype=np.int64)
    ws = PREDICT_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    _check(lib.lcf_predict_template(grid_engine.handle, _ptr(P), P.shape[0], P.shape[1], mask, _ptr(q), len(q), ws,
                                    _ptr(out), _i64p(n_valid), _i64p(n_dark)))
    return out, n_valid, n_dark, names


def template_features(grid_engine, samples):
    """``lcf_template_features``: per sample and filter of the same grid, over the times in ascending order, the two
    components' peaks, the first time the template term exceeds the base term and the dip of the sum between the peaks.
    Returns ``(values[3, n_f, n], indices[4, n_f, n])`` in the order of ``TEMPLATE_FEATURE_VALUES`` /
    ``TEMPLATE_FEATURE_INDICES``: a value is NaN where its index is -1."""
    lib = load_library()
    P, n_f, _ = _template_samples(grid_engine, samples)
    values = np.empty((len(TEMPLATE_FEATURE_VALUES), n_f, P.shape[0]))
    indices = np.empty((len(TEMPLATE_FEATURE_INDICES), n_f, P.shape[0]), dtype=np.int32)
    _check(lib.lcf_template_features(grid_engine.handle, _ptr(P), P.shape[0], P.shape[1], _ptr(values),
                                     _ptr(indices, _ip)))
    return values, indices


#: limits of the corner entry points (include/lcf.h)
CORNER_MAX_DIM, CORNER_MAX_BINS = 16, 128


def _native_list(samples):
    """One :class:`NativeSampler` or a non-empty list of them as a list; None for anything else (a host array)."""
    if isinstance(samples, NativeSampler):
        samples = [samples]
    if isinstance(samples, (list, tuple)) and samples and all(isinstance(s, NativeSampler) for s in samples):
        return list(samples)
    return None


def _corner_sources(samples, device):
    """``(native samplers or None, host array or None, column counts)`` of what a corner call reads: one host array
    (n, n_columns), one :class:`NativeSampler` or a list of them."""
    natives = _native_list(samples)
    if natives is not None:
        return natives, None, [s.ndim for s in natives]
    P = _f64(samples)
    if P.ndim != 2:
        raise ValueError('samples must have shape (n, n_columns)')
    return None, P, [P.shape[1]]


def chain_range(samples, discard=0, thin=1, device=0):
    """``lcf_chain_range`` / ``lcf_samplers_chain_range``: per column the minimum and maximum of the non-NaN values
    (NaN, NaN where there is none) and the number of NaNs.  ``samples``: a host array (n, n_columns), or one
    :class:`NativeSampler` or a list of them (one device) whose last stored runs are read in place (rows
    ``discard::thin``).  Returns ``(lo, hi, n_nan)``, or a list of such triples for a list of samplers."""
    lib = load_library()
    natives, P, dims = _corner_sources(samples, device)
    total = sum(dims)
    lo, hi, n_nan = np.empty(total), np.empty(total), np.empty(total, dtype=np.int64)
    if natives is None:
        _check(lib.lcf_chain_range(int(device), _ptr(P), P.shape[0], P.shape[1], P.shape[1], _ptr(lo), _ptr(hi),
                                   _i64p(n_nan)))
        return lo, hi, n_nan
    _check(lib.lcf_samplers_chain_range(_handles(natives), len(natives), int(discard), int(thin), _ptr(lo), _ptr(hi), _i64p(n_nan)))
    at = np.concatenate([[0], np.cumsum(dims)])
    out = [(lo[i:j].copy(), hi[i:j].copy(), n_nan[i:j].copy()) for i, j in zip(at[:-1], at[1:])]
    return out if isinstance(samples, (list, tuple)) else out[0]


def chain_hist(samples, shift, edges, discard=0, thin=1, device=0):
    """``lcf_chain_hist`` / ``lcf_samplers_chain_hist``: the histogram of every column of ``x - shift`` and the joint
    histogram of every pair of columns on the bin ``edges`` (n_columns, bins + 1) -- NumPy's bins for
    ``np.linspace(lo, hi, bins + 1)``.  ``samples`` as for :func:`chain_range`; for a list of samplers ``shift`` and
    ``edges`` are lists with one entry per sampler (the same ``bins`` in all).  Returns ``(hist1d[n_columns, bins],
    hist2d[n_pairs, bins, bins])``, int64, the pair of columns ``b < a`` at index ``a (a - 1) / 2 + b`` with the bins
    of ``b`` on the first axis -- ``np.histogram2d(x[:, b], x[:, a])[0]`` -- or a list of such tuples."""
    lib = load_library()
    natives, P, dims = _corner_sources(samples, device)
    many = isinstance(samples, (list, tuple))
    shifts = [_f64(v).ravel() for v in (shift if many else [shift])]
    tables = [_f64(e) for e in (edges if many else [edges])]
    if len(shifts) != len(dims) or len(tables) != len(dims):
        raise ValueError('shift and edges need one entry per sampler')
    bins = tables[0].shape[-1] - 1 if tables[0].ndim == 2 else -1
    for n_dim, sh, e in zip(dims, shifts, tables):
        if sh.shape != (n_dim,) or e.shape != (n_dim, bins + 1):
            raise ValueError('shift must have shape (n_columns,) and edges (n_columns, bins + 1)')
    pairs = [d * (d - 1) // 2 for d in dims]
    sh, ed = np.concatenate(shifts), np.concatenate([e.ravel() for e in tables])
    h1 = np.zeros(sum(dims) * bins, dtype=np.int64)
    h2 = np.zeros(sum(pairs) * bins * bins, dtype=np.int64)
    h2p = _i64p(h2) if h2.size else None
    if natives is None:
        _check(lib.lcf_chain_hist(int(device), _ptr(P), P.shape[0], P.shape[1], P.shape[1], _ptr(sh), _ptr(ed), bins,
                                  _i64p(h1), h2p))
    else:
        _check(lib.lcf_samplers_chain_hist(_handles(natives), len(natives), int(discard), int(thin), _ptr(sh), _ptr(ed),
                                           bins, _i64p(h1), h2p))
    out, i, j = [], 0, 0
    for d, p in zip(dims, pairs):
        out.append((h1[i:i + d * bins].reshape(d, bins).copy(), h2[j:j + p * bins * bins].reshape(p, bins, bins).copy()))
        i, j = i + d * bins, j + p * bins * bins
    return out if many else out[0]


#: limits of the chain-history entry points (include/lcf.h)
HISTORY_MAX_WALKERS, HISTORY_MAX_PERCENTILES, HISTORY_MAX_VBINS, HISTORY_MAX_TBINS = 16384, 16, 256, 4096


def _history_sources(samples, discard, thin):
    """``(native samplers or None, host chain or None, [(n_keep, n_dim)])`` of what a history call reads: one host
    chain (n_t, n_w, n_dim), one :class:`NativeSampler` or a list of them.  ``n_keep`` is 0 where the native call will
    refuse (no stored run, ``discard`` past it)."""
    def n_keep(n_t):
        return len(range(int(discard), n_t, int(thin))) if thin >= 1 and discard >= 0 else 0
    natives = _native_list(samples)
    if natives is not None:
        steps = [s._last[0] if getattr(s, '_last', (0, False))[1] else 0 for s in natives]
        return natives, None, [(n_keep(n_t), s.ndim) for n_t, s in zip(steps, natives)]
    x = _f64(samples)
    if x.ndim != 3:
        raise ValueError('chain must have shape (n_t, n_w, n_dim)')
    return None, x, [(n_keep(x.shape[0]), x.shape[2])]


def chain_history(samples, percentiles, log_prob=None, discard=0, thin=1, device=0):
    """``lcf_chain_history`` / ``lcf_samplers_chain_history``: for every kept step (stored steps ``discard::thin``) and
    every column -- the log-probability being column ``n_dim`` -- the two order statistics of the walkers' values around
    each percentile (ranks ``lo``, ``hi`` of :func:`~lightcurve_fitting_amd.fitting.quantile_ranks`) and the number of
    non-NaN values, and per kept step the number of walkers whose row differs from the stored step before (-1 for
    stored step 0).  ``samples``: a host chain (n_t, n_w, n_dim) with an optional ``log_prob`` (n_t, n_w), or one
    :class:`NativeSampler` or a list of them (one device) whose last stored runs are read in place.  Returns
    ``(stat_lo[n_q, n_keep, n_dim + 1], stat_hi, n_valid[n_keep, n_dim + 1], n_moved[n_keep])``, or a list of such
    tuples for a list of samplers."""
    lib = load_library()
    natives, x, shapes = _history_sources(samples, discard, thin)
    q = _f64(percentiles).ravel()
    n_q = len(q)
    cells = [n_keep * (n_dim + 1) for n_keep, n_dim in shapes]
    lo, hi = np.empty(max(1, n_q * sum(cells))), np.empty(max(1, n_q * sum(cells)))
    n_valid = np.empty(max(1, sum(cells)), dtype=np.int64)
    n_moved = np.empty(max(1, sum(n_keep for n_keep, _ in shapes)), dtype=np.int64)
    if natives is None:
        lp = None
        if log_prob is not None:
            lp = _f64(log_prob)
            if lp.shape != x.shape[:2]:
                raise ValueError(f'log_prob must have shape {x.shape[:2]}, got {lp.shape}')
        _check(lib.lcf_chain_history(int(device), _ptr(x), None if lp is None else _ptr(lp), x.shape[0], x.shape[1],
                                     x.shape[2], int(discard), int(thin), _ptr(q), n_q, _ptr(lo), _ptr(hi),
                                     _i64p(n_valid), _i64p(n_moved)))
    else:
        if log_prob is not None:
            raise ValueError('log_prob goes with a host chain; a sampler brings its own')
        _check(lib.lcf_samplers_chain_history(_handles(natives), len(natives), int(discard), int(thin), _ptr(q), n_q,
                                              _ptr(lo), _ptr(hi), _i64p(n_valid), _i64p(n_moved)))
    out, c, k = [], 0, 0
    for (n_keep, n_dim), n_cell in zip(shapes, cells):
        shape = (n_q, n_keep, n_dim + 1)
        out.append((lo[n_q * c:n_q * (c + n_cell)].reshape(shape).copy(),
                    hi[n_q * c:n_q * (c + n_cell)].reshape(shape).copy(),
                    n_valid[c:c + n_cell].reshape(n_keep, n_dim + 1).copy(), n_moved[k:k + n_keep].copy()))
        c, k = c + n_cell, k + n_keep
    return out if isinstance(samples, (list, tuple)) else out[0]


def chain_raster(samples, t_bins, edges, discard=0, thin=1, device=0):
    """``lcf_chain_raster`` / ``lcf_samplers_chain_raster``: ``counts[n_dim, t_bins, v_bins]``, int64 -- the (kept step,
    walker) pairs with step bin ``(k * t_bins) // n_keep`` and the column's value in the bin of ``edges`` (n_dim,
    v_bins + 1) that :func:`chain_hist` would count it in.  ``samples`` as for :func:`chain_history`; for a list of
    samplers ``edges`` is a list with one table per sampler (the same ``v_bins`` in all) and a list is returned."""
    lib = load_library()
    natives, x, shapes = _history_sources(samples, discard, thin)
    many = isinstance(samples, (list, tuple))
    tables = [_f64(e) for e in (edges if many else [edges])]
    if len(tables) != len(shapes):
        raise ValueError('edges needs one entry per sampler')
    v_bins = tables[0].shape[-1] - 1 if tables[0].ndim == 2 else -1
    for (_, n_dim), e in zip(shapes, tables):
        if e.shape != (n_dim, v_bins + 1):
            raise ValueError('edges must have shape (n_columns, v_bins + 1)')
    t_bins = int(t_bins)
    ed = np.concatenate([e.ravel() for e in tables])
    sizes = [n_dim * max(t_bins, 0) * max(v_bins, 0) for _, n_dim in shapes]
    counts = np.zeros(max(1, sum(sizes)), dtype=np.int64)
    if natives is None:
        _check(lib.lcf_chain_raster(int(device), _ptr(x), x.shape[0], x.shape[1], x.shape[2], int(discard), int(thin),
                                    t_bins, _ptr(ed), v_bins, _i64p(counts)))
    else:
        _check(lib.lcf_samplers_chain_raster(_handles(natives), len(natives), int(discard), int(thin), t_bins, _ptr(ed),
                                             v_bins, _i64p(counts)))
    out, i = [], 0
    for (_, n_dim), size in zip(shapes, sizes):
        out.append(counts[i:i + size].reshape(n_dim, t_bins, v_bins).copy())
        i += size
    return out if many else out[0]
