"""The plumbing the models share: the device-path
protocol (`NoDevicePath`, `device_call`), the one fit loop and the base class
of the Gaussian process models -- with stand-in kernels, no GPU needed."""
import json
import os
import re
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_golden_model_base as recorded      # noqa: E402


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'fit_loops.json')) as f:
        return json.load(f)


# -- the protocol ---------------------------------------------------------------
def test_no_device_path_is_a_type_error():
    from graphdot_amd.kernel import NoDevicePath
    from graphdot_amd.kernel._device_path import NoDevicePath as same
    assert NoDevicePath is same and issubclass(NoDevicePath, TypeError)


def test_device_call_returns_none_without_a_device_path():
    from graphdot_amd.kernel import NoDevicePath
    from graphdot_amd.model._device_kernel import device_call

    class Plain:
        pass

    class Refuses:
        def device_gram(self, X, eval_gradient=False):
            raise NoDevicePath('device_gram needs the HIP backend')

    class Offers:
        def device_gram(self, X, eval_gradient=False):
            return ('K', X, eval_gradient)

    assert device_call(Plain(), 'device_gram', [1]) is None
    assert device_call(Refuses(), 'device_gram', [1]) is None
    assert device_call(Offers(), 'device_gram', [1], eval_gradient=True) \
        == ('K', [1], True)


def test_device_call_propagates_a_plain_type_error():
    """The class of bug behind the swallowed `local_gradient=` keyword: a
    TypeError that is not the kernel's "no device path" is an error."""
    from graphdot_amd.model._device_kernel import device_call

    class NoSuchKeyword:
        def device_gram(self, X, eval_gradient=False):
            return 'K'

    class BadOperand:
        def device_gram(self, X, eval_gradient=False):
            return None + 1

    with pytest.raises(TypeError, match='local_gradient'):
        device_call(NoSuchKeyword(), 'device_gram', [1],
                    local_gradient='overlapped')
    with pytest.raises(TypeError, match='unsupported operand'):
        device_call(BadOperand(), 'device_gram', [1])


def test_regressor_does_not_swallow_a_type_error_of_the_kernel():
    """... and through a model: with the algebra on a (pretended) GPU, a
    kernel whose `device_gram` does not take the regressor's keyword raises
    instead of sending the evaluation through host arrays."""
    import types
    from graphdot_amd.model.gaussian_process import GaussianProcessRegressor
    from graphdot_amd.kernel import NoDevicePath

    class Kernel(recorded.RBF):
        def device_gram(self, X, eval_gradient=False):
            raise AssertionError('not reached')

    class Refuses(recorded.RBF):
        def device_gram(self, X, eval_gradient=False, local_gradient=False):
            raise NoDevicePath('no HIP backend')

    la = types.SimpleNamespace(device=types.SimpleNamespace(type='cuda'))
    X, _, _ = recorded.data()
    gpr = GaussianProcessRegressor(Kernel(), device='cpu')
    with pytest.raises(TypeError, match='local_gradient'):
        gpr._device_gramian(la, gpr.kernel, X, True, local_gradient=True)
    assert gpr._device_gramian(la, Refuses(), X, True,
                               local_gradient=True) is None
    # kernel options, or the algebra on the CPU: the kernel is not asked
    assert gpr._device_gramian(gpr._dense(), gpr.kernel, X, True) is None
    opts = GaussianProcessRegressor(Kernel(), kernel_options={'nodal': False},
                                    device='cpu')
    assert opts._device_gramian(la, opts.kernel, X, True) is None


def test_active_planes():
    from graphdot_amd.model._device_kernel import active_planes

    class K:
        active_theta_mask = np.array([True, False, True, True])

    assert active_planes(K, 4).tolist() == [0, 2, 3]     # all columns handed
    assert active_planes(K, 3).tolist() == [0, 1, 2]     # the active ones only
    assert active_planes(object(), 2).tolist() == [0, 1]


# -- the conventions, at source level ---------------------------------------------
def _sources(*parts):
    top = os.path.join(ROOT, 'graphdot_amd', *parts)
    if os.path.isfile(top):
        yield top
        return
    for d, _, files in os.walk(top):
        for f in files:
            if f.endswith('.py'):
                yield os.path.join(d, f)


def _count(pattern, paths):
    hits = {}
    for p in paths:
        with open(p) as f:
            n = len(re.findall(pattern, f.read()))
        if n:
            hits[os.path.relpath(p, ROOT)] = n
    return hits


def test_conventions_live_in_one_place():
    model = list(_sources('model'))
    assert _count(r'except\s+\(?[^:\n]*TypeError', model
                  + list(_sources('kernel', 'fix.py'))) == {}
    assert _count(r'except\s+NoDevicePath', list(_sources())) == {
        os.path.join('graphdot_amd', 'model', '_device_kernel.py'): 1}
    assert _count(r'\bminimize\(', model) == {
        os.path.join('graphdot_amd', 'model', '_fit.py'): 1}
    potrf = os.path.join('graphdot_amd', 'model', 'gaussian_process',
                         '_potrf.py')
    assert list(_count(r'gave up waiting', list(_sources()))) == [potrf]
    assert list(_count(r'16 \+ 2 \* nb', list(_sources()))) == [potrf]
    assert _count(r'=\s*GaussianProcessRegressor\.\w', model) == {}


def test_models_share_the_base_class():
    from graphdot_amd.model.gaussian_process import (
        GaussianProcessRegressor, LowRankApproximateGPR, GPROutlierDetector)
    from graphdot_amd.model.gaussian_process._base import (
        GaussianProcessRegressorBase as Base)
    from graphdot_amd.model.gaussian_process.gpr import _Dense, _torch  # noqa
    for cls in (GaussianProcessRegressor, LowRankApproximateGPR,
                GPROutlierDetector):
        assert issubclass(cls, Base)
        for name in ('X', 'y', 'mask', '_regularize', '_gramian', '_dense',
                     'save', 'load', '_prologue', '_optimize'):
            assert name not in vars(cls), (cls, name)


# -- the fit loop -----------------------------------------------------------------
def test_multistart_is_lazy_and_keeps_the_best_successful_result():
    from graphdot_amd.model._fit import multistart
    log = []

    def starts():
        for x in ([3.0], [0.5], [-2.0]):
            log.append(('start', x[0]))
            yield np.array(x)

    def fun(x):
        log.append(('fun', None))
        return float(((x * x - 1)**2 + 0.3 * x).sum()), \
            4 * x * (x * x - 1) + 0.3

    best = multistart(fun, starts(), 'L-BFGS-B', [(-4, 4)], 1e-8)
    assert best.success and best.x[0] == pytest.approx(-1.0354, abs=1e-3)
    # every start is drawn after the run before it has ended
    kinds = [k for k, _ in log]
    first = [i for i, k in enumerate(kinds) if k == 'start']
    assert len(first) == 3 and all(
        kinds[i + 1] == 'fun' for i in first) and first[1] > 2

    class Failing:
        success, fun = False, 0.0

    import graphdot_amd.model._fit as fit
    results = iter([Failing(), Failing()])
    keep, fit.minimize = fit.minimize, lambda **kw: next(results)
    try:
        # the first result stands even if it failed and no later one succeeds
        assert multistart(fun, [[0.0], [1.0]], 'L-BFGS-B', None, 1e-8) \
            .success is False
    finally:
        fit.minimize = keep


@pytest.mark.parametrize('name', ['gpr', 'nystrom', 'outlier', 'gfr'])
def test_fit_loops_reproduce_the_recorded_runs(golden, name):
    """The starts each model draws from `np.random`, in the order it draws
    them, and the result its loop keeps: equal to what the four separate
    loops gave (tests/golden/make_golden_model_base.py, recorded before
    they became one)."""
    got, want = recorded.FITS[name](), golden['fits'][name]
    assert got['calls'] == want['calls']
    if name == 'gfr':
        np.testing.assert_allclose(got['theta'], want['theta'], rtol=1e-12)
        return
    assert got['nfev'] == want['nfev']
    np.testing.assert_allclose(got['x'], want['x'], rtol=1e-12)
    assert got['fun'] == pytest.approx(want['fun'], rel=1e-12)


# -- persistence --------------------------------------------------------------------
def test_models_saved_before_the_base_class_load_and_predict(golden):
    golden_dir = os.path.join(HERE, 'golden')
    _, _, Z = recorded.data()
    for name, _, fresh in recorded.saved_models():
        want = golden['saved'][name]
        fresh.load(golden_dir, name)
        np.testing.assert_array_equal(fresh.kernel.theta, want['theta'])
        mean, std = fresh.predict(Z, return_std=True)
        np.testing.assert_allclose(mean, want['mean'], rtol=1e-10)
        np.testing.assert_allclose(std, want['std'], rtol=1e-8, atol=1e-12)


def test_save_stores_the_same_attributes(tmp_path):
    """... and what `save` writes today has the keys of those files."""
    import pickle
    for name, model, _ in recorded.saved_models():
        model.save(str(tmp_path), name)
        with open(os.path.join(HERE, 'golden', name), 'rb') as f:
            old = pickle.load(f)
        with open(tmp_path / name, 'rb') as f:
            new = pickle.load(f)
        assert set(new) == set(old)
        assert 'kernel' not in new and '_la' not in new
