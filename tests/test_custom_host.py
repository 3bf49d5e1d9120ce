"""Custom models (``CustomModel``, ``lcf_custom_*``) where there is no device: the run-time compile for a named
architecture, its cache, what a broken source reports, the model's metadata, and engine calls failing with a status."""
import numpy as np
import pytest

from lightcurve_fitting_amd import engine as E, models as M

ARCH = 'gfx950'

# ShockCooling2 (models.py:403-406) as a user writes it; consts = A, a, alpha, epsilon_1, epsilon_2
SC2_SOURCE = r'''
__device__ void lcf_user_state(double t_in, const double* p, const double* consts, double z,
                               double& T_kK, double& R_1000Rsun) {
    const double t = t_in - p[3];
    T_kK = p[0] * lcf::pw(t, 2. * consts[3] - 0.5);
    const double L = p[1] * exp(-lcf::pw(consts[1] * t / p[2], consts[2])) * lcf::pw(t, -2. * consts[4]) * 1e42;
    R_1000Rsun = lcf::kC3 * sqrt(L) * lcf::pw(T_kK, -2.);
}
'''
SC2_NAMES = ['T_1', 'L_1', 't_\\mathrm{tr}', 't_0']
SC2_UNITS = ['kK', '10^42 erg/s', 'd', 'd']
SC2_CONSTS = (0.94, 1.67, 0.8, 0.027, 0.086)


def test_a_valid_source_compiles_to_a_code_object_and_is_cached():
    prog = E.CustomProgram(SC2_SOURCE, ARCH)
    code = prog.code
    assert len(code) > 1000 and (code[:4] == b'\x7fELF' or code.startswith(b'__CLANG_OFFLOAD_BUNDLE__'))
    assert b'lcf_custom_points' in code                          # the kernel the engine asks the module for
    assert 'error' not in prog.log
    again = E.CustomProgram(SC2_SOURCE, ARCH)
    assert again.handle.value == prog.handle.value and again.code == code      # the cached program
    other = E.CustomProgram(SC2_SOURCE + '\n// another text\n', ARCH)
    assert other.handle.value != prog.handle.value
    m = M.CustomModel(SC2_SOURCE, SC2_NAMES, SC2_UNITS, consts=SC2_CONSTS)
    assert m.compile(ARCH).handle.value == prog.handle.value and m.compile(ARCH) is m.compile(ARCH)


def test_an_error_is_reported_at_the_users_own_line():
    lines = SC2_SOURCE.strip('\n').split('\n')
    lines[2] = '    const double t = t_in - q[3];'                # line 3 of the source: q is not declared
    with pytest.raises(E.LcfError) as exc:
        E.CustomProgram('\n'.join(lines), ARCH)
    text = str(exc.value)
    assert exc.value.status == 1 and 'user_model:3' in text and "'q'" in text
    first = next(line for line in text.split('\n') if 'error' in line)
    assert first.startswith('user_model:3:'), first               # the first offending line is the user's


def test_a_source_without_the_state_function_names_it():
    with pytest.raises(E.LcfError) as exc:
        E.CustomProgram('__device__ double twice(double x) { return 2. * x; }\n', ARCH)
    assert exc.value.status == 1 and 'does not define lcf_user_state' in str(exc.value)
    with pytest.raises(E.LcfError, match='lcf_user_state'):       # defined, with other parameters: the compiler names it
        E.CustomProgram('__device__ void lcf_user_state(double t, double& T, double& R) { T = R = t; }\n', ARCH)


def test_model_metadata():
    m = M.CustomModel(SC2_SOURCE, SC2_NAMES, SC2_UNITS, consts=SC2_CONSTS, redshift=0.01)
    assert m.nparams == 4 and m.n_model_params == 4 and m.z == 0.01 and m.output_quantity == 'lum'
    assert m.model_id == E.MODEL_CUSTOM == 9 and m._consts() == list(SC2_CONSTS)
    assert m.axis_labels == ['$T_1$ (kK)', '$L_1$ (10^42 erg/s)', '$t_\\mathrm{tr}$ (d)', '$t_0$ (d)']
    m.input_names.append('\\sigma')                               # what lightcurve_mcmc(use_sigma=True) does
    m.units.append('')
    assert m.nparams == 5 and m.n_model_params == 4 and m.axis_labels[-1] == '$\\sigma$'
    bare = M.CustomModel(SC2_SOURCE, ['a', 'b'])
    assert bare.axis_labels == ['$a$', '$b$'] and bare.z == 0.
    with pytest.raises(ValueError, match='units'):
        M.CustomModel(SC2_SOURCE, ['a', 'b'], ['kK'])
    with pytest.raises(ValueError, match='consts'):
        M.CustomModel(SC2_SOURCE, ['a'], consts=range(13))
    with pytest.raises(ValueError, match='parameters'):
        M.CustomModel(SC2_SOURCE, ['p%d' % k for k in range(16)])


def test_engine_calls_without_a_device_fail_with_a_status():
    lib = E.load_library()
    if lib.lcf_device_count() > 0:
        pytest.skip('a GPU is visible')
    m = M.CustomModel(SC2_SOURCE, SC2_NAMES, SC2_UNITS, consts=SC2_CONSTS)
    lc = {'MJD': [1., 2.], 'filter': ['g', 'r'], 'lum': [1e20, 1e20], 'dlum': [1e18, 1e18]}
    for call in (lambda: m.log_likelihood(lc, np.array([10., 1., 10., 0.])),
                 lambda: m(np.array([1., 2.]), ['g', 'r'], 10., 1., 10., 0.),
                 lambda: m.temperature_radius(np.array([1., 2.]), 10., 1., 10., 0.),
                 lambda: m.compile()):                            # (no architecture named: the device's is asked for)
        with pytest.raises(E.LcfError, match='LCF_ERR_NO_DEVICE'):
            call()
    assert lib.lcf_engine_set_custom(None, None) == 1 and lib.lcf_engine_set_custom_redshift(None, 0.) == 1
    assert lib.lcf_custom_log(None) == b'' and lib.lcf_custom_code(None, None) is None
