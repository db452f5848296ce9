"""KernelOverMetric on the CPU: parity with values recorded from the
reference (tests/golden/make_golden_kernel_over_metric.py), the reference's
own tests restated, the clone fix, the generated device source (theta-free,
compiles for gfx950, TypeError for what the printer cannot express) and the
package's exports."""
import json
import os
import shutil
import subprocess
import sys
import numpy as np
import pytest

from graphdot_amd.kernel import KernelOverMetric

HERE = os.path.dirname(os.path.abspath(__file__))


class PairwiseDistance:
    """The reference test's distance |x - y| * scale, one theta."""

    def __init__(self, scale):
        self.scale = scale

    def __call__(self, X, Y=None, eval_gradient=False):
        distance = np.abs(np.subtract.outer(X, Y if Y is not None else X))
        if eval_gradient is True:
            return self.scale * distance, distance.reshape(*distance.shape, 1)
        else:
            return self.scale * distance

    @property
    def hyperparameters(self):
        return (self.scale,)

    @property
    def theta(self):
        return np.log([self.scale])

    @theta.setter
    def theta(self, value):
        self.scale = np.exp(value)[0]

    @property
    def bounds(self):
        return np.log([[1e-4, 1e4]])

    def clone_with_theta(self, theta=None):
        if theta is None:
            theta = self.theta
        clone = type(self)(scale=self.scale)
        clone.theta = theta
        return clone


class ReplayDistance:
    """Fixed float32 matrices over a pool of samples: X, Y are index arrays,
    the distance is D[X][:, Y] and its gradient dD[X][:, Y] (n_theta
    columns); theta only travels along."""

    def __init__(self, D, dD, theta):
        self.D = np.asarray(D, dtype=np.float32)
        self.dD = np.asarray(dD, dtype=np.float32).reshape(
            *self.D.shape, len(theta))
        self._theta = np.array(theta, dtype=float)

    def __call__(self, X, Y=None, eval_gradient=False):
        Y = X if Y is None else Y
        D = self.D[np.ix_(X, Y)]
        if eval_gradient is True:
            return D, self.dD[np.ix_(X, Y)]
        return D

    @property
    def hyperparameters(self):
        return tuple(np.exp(self._theta))

    @property
    def theta(self):
        return self._theta.copy()

    @theta.setter
    def theta(self, value):
        self._theta = np.array(value, dtype=float)

    @property
    def bounds(self):
        return np.log(np.tile([[1e-3, 1e3]], (len(self._theta), 1)))

    def clone_with_theta(self, theta=None):
        if theta is None:
            theta = self.theta
        return type(self)(self.D, self.dD, theta)


def _golden():
    with open(os.path.join(HERE, 'golden', 'kernel_over_metric.json')) as f:
        return json.load(f)


GOLDEN = _golden()
FORMULAS = {f['name']: f for f in GOLDEN['formulas']}


def _distance(spec):
    if spec['kind'] == 'pairwise':
        return PairwiseDistance(spec['scale'])
    return ReplayDistance(spec['D'], spec['dD'], spec['theta'])


def _kernel(case):
    f = FORMULAS[case['formula']]
    spec = GOLDEN['distances'][case['distance']]['spec']
    return KernelOverMetric(_distance(spec), f['expr'], 'd', **f['hypers'])


def _inputs(case):
    d = GOLDEN['distances'][case['distance']]
    cast = (lambda a: np.array(a, dtype=np.int64)) \
        if d['spec']['kind'] == 'replay' else np.array
    return cast(d['X']), cast(d['Y'])


def _close(a, b):
    """Equal to float64 round-off (the reference's compiled ufunc and
    numpy's libm may differ in the last bits)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.allclose(a, b, rtol=1e-12, atol=1e-14), \
        np.max(np.abs(a - b))


CASE_IDS = [f"{c['formula']}-{c['distance']}" for c in GOLDEN['cases']]


@pytest.mark.parametrize('case', GOLDEN['cases'], ids=CASE_IDS)
def test_golden_parity(case):
    k = _kernel(case)
    X, Y = _inputs(case)
    K, G = k(X, eval_gradient=True)
    assert K.dtype.str == case['K_X_dtype'] and G.dtype.str == \
        case['G_X_dtype']
    _close(K, case['K_X'])
    _close(G, np.array(case['G_X']).reshape(G.shape))
    assert G.flags.f_contiguous
    Kv = k(X)
    assert Kv.dtype.str == case['K_X_dtype']
    _close(Kv, case['K_X_nograd'])
    K, G = k(X, Y, eval_gradient=True)
    assert K.dtype.str == case['K_XY_dtype'] and G.dtype.str == \
        case['G_XY_dtype']
    _close(K, case['K_XY'])
    _close(G, np.array(case['G_XY']).reshape(G.shape))
    d = k.diag(X)
    assert d.dtype.str == case['diag_dtype']
    _close(d, case['diag'])
    _close(k.theta, case['theta'])
    assert np.array_equal(k.bounds, np.array(case['bounds']))
    hp = k.hyperparameters
    assert type(hp).__name__ == case['hyperparameters']['typename']
    assert list(hp._fields) == case['hyperparameters']['fields']
    for a, b in zip(hp, case['hyperparameters']['values']):
        _close(np.ravel(a), np.ravel(b))
    c = k.clone_with_theta(np.array(case['clone_theta_in']))
    assert isinstance(c, KernelOverMetric)
    _close(c.theta, case['clone_theta'])
    _close(c(X), case['clone_K_X'])
    _close(k.theta, case['original_theta_after_clone'])
    assert len(k.active_theta_mask) == len(k.theta)
    assert np.all(k.active_theta_mask)


def test_distance_array_left_intact():
    """The reference writes K into the distance's array; the port does
    not."""
    D = np.array([[0.0, 0.5], [0.5, 0.0]], dtype=np.float32)

    class Fixed(PairwiseDistance):
        def __call__(self, X, Y=None, eval_gradient=False):
            return D
    k = KernelOverMetric(Fixed(1.0), 'exp(-d)', 'd')
    K = k([0, 1])
    assert K.dtype == np.float32
    assert np.array_equal(D, [[0.0, 0.5], [0.5, 0.0]])
    assert np.allclose(K, np.exp(-D))


def test_hyperparameter_forms():
    k = KernelOverMetric(PairwiseDistance(1.0), 'a * b * c * d * exp(-x)',
                         'x', a=2.0, b=(3.0,), c=(0.5, (0.1, 1.0)),
                         d=(4.0, 1.0, 8.0))
    assert np.allclose(np.exp(k.theta), [2.0, 3.0, 0.5, 4.0, 1.0])
    b = np.exp(k.bounds)
    assert np.allclose(b[:2], [[0, np.inf], [0, np.inf]])
    assert np.allclose(b[2:], [[0.1, 1.0], [1.0, 8.0], [1e-4, 1e4]])
    assert list(k.get_params()) == ['a', 'b', 'c', 'd']
    k.theta = np.log([1.0, 2.0, 0.3, 5.0, 2.0])
    assert k.get_params()['d'] == pytest.approx(5.0)
    assert k.distance.scale == pytest.approx(2.0)


# -- the reference's own tests (test/kernel/test_kernel_over_metric.py) -------------
def test_gauss():
    kernel = KernelOverMetric(
        distance=PairwiseDistance(1.0),
        expr='v * exp(-d^2 / ell^2)',
        x='d',
        v=(1.0, (1e-2, 1e2)),
        ell=(1.0, (1e-2, 1e2))
    )
    X = np.arange(3)
    Y = np.arange(4)
    assert kernel(X).shape == (len(X), len(X))
    assert kernel(Y).shape == (len(Y), len(Y))
    assert kernel(X, X).shape == (len(X), len(X))
    assert kernel(Y, Y).shape == (len(Y), len(Y))
    assert kernel(X, Y).shape == (len(X), len(Y))
    assert kernel(X).diagonal() == pytest.approx(kernel.diag(X))
    assert kernel(Y).diagonal() == pytest.approx(kernel.diag(Y))
    assert len(kernel.theta) == len(kernel.distance.theta) + 2
    assert kernel.bounds.shape == (len(kernel.theta), 2)
    assert len(kernel.hyperparameters) == 3
    kclone = kernel.clone_with_theta()
    assert isinstance(kclone, KernelOverMetric)


@pytest.mark.parametrize('X', [
    np.linspace(-1, 1, 4),
    np.linspace(-1, 1, 40),
    np.linspace(-10, 10, 40),
    np.random.default_rng(0).normal(size=10) * 3.0,
    np.random.default_rng(1).uniform(size=10) * 3.0,
])
@pytest.mark.parametrize('make', [
    lambda: KernelOverMetric(
        distance=PairwiseDistance(1.0), expr='v * exp(-d^2 / ell^2)',
        x='d', v=(1.0, (1e-2, 1e2)), ell=(1.0, (1e-2, 1e2))),
    lambda: KernelOverMetric(
        distance=PairwiseDistance(1.0), expr='v * exp(-d^2 / ell^2)',
        x='d', v=(1.0, (1e-2, 1e2)), ell=(2.0, (1e-2, 1e2))),
    lambda: KernelOverMetric(
        distance=PairwiseDistance(1.5),
        expr='v * (1 + d**2 / (2 * a * ell**2)) ** -a', x='d',
        v=(1.2, (1e-5, 1e5)), a=(0.9, (1e-5, 1e5)), ell=(1.1, (1e-2, 1e2))),
])
def test_gradient(X, make):
    kernel = make()
    _, grad = kernel(X, eval_gradient=True)
    assert grad.shape == (len(X), len(X), len(kernel.theta))
    delta = 1e-2
    for i, _ in enumerate(kernel.theta):
        h_pos, h_neg = np.exp(kernel.theta), np.exp(kernel.theta)
        h_pos[i] += delta
        h_neg[i] -= delta
        pos = kernel.clone_with_theta(np.log(h_pos))
        neg = kernel.clone_with_theta(np.log(h_neg))
        diff = (pos(X) - neg(X)) / (2 * delta)
        assert np.allclose(grad[:, :, i], diff, rtol=1e-3, atol=1e-3)


# -- clone_with_theta on a distance whose clone needs theta ---------------------------
class StrictDistance(PairwiseDistance):
    """clone_with_theta(theta) with a required argument, as MaxiMin's
    (MarginalizedGraphKernel.clone_with_theta)."""

    def clone_with_theta(self, theta):
        clone = type(self)(scale=self.scale)
        clone.theta = theta
        return clone


def test_clone_with_strict_distance():
    k = KernelOverMetric(StrictDistance(1.5), 'v * exp(-d / ell)', 'd',
                         v=2.0, ell=0.5)
    c = k.clone_with_theta()
    assert np.array_equal(c.theta, k.theta)
    assert c.distance is not k.distance
    t = np.log([1.0, 2.0, 3.0])
    c = k.clone_with_theta(t)
    assert np.allclose(c.theta, t)
    assert np.allclose(k.theta, np.log([2.0, 0.5, 1.5]))


def test_clone_with_maximin():
    """A MaxiMin distance (host backend not needed: no evaluation)."""
    from graphdot_amd.metric.maximin import MaxiMin
    import cases
    knode, kedge, q = cases.config3_kernels()
    mm = MaxiMin(knode, kedge, q=q, backend='hip')
    k = KernelOverMetric(mm, 'v * exp(-d^2 / ell^2)', 'd', v=1.0, ell=0.5)
    t = k.theta + 0.1
    c = k.clone_with_theta(t)
    assert np.allclose(c.theta, t)
    assert c.distance is not mm
    assert len(k.active_theta_mask) == len(k.theta) == 2 + len(mm.theta)


# -- the generated device source --------------------------------------------------
def test_source_is_theta_free():
    from graphdot_amd.kernel._kom_map import DeviceMap
    a = KernelOverMetric(PairwiseDistance(1.0), 'v * exp(-d^2 / ell^2)',
                         'd', v=1.0, ell=0.5)
    b = a.clone_with_theta(a.theta + 0.7)
    assert not np.allclose(a.theta, b.theta)
    ma, mb = a._map(), b._map()
    assert ma.source == mb.source and ma.key == mb.key
    c = DeviceMap('v * exp(-d^2 / ell^2)', 'd', ('v', 'ell'))
    assert c.source == ma.source
    for v in ('1.0', '0.5'):
        assert f'= {v}' not in ma.source
    other = DeviceMap('v * exp(-d / ell)', 'd', ('v', 'ell'))
    assert other.key != ma.key


@pytest.mark.skipif(shutil.which('hipcc') is None
                    and not os.path.exists('/opt/rocm/bin/hipcc'),
                    reason='hipcc not installed')
@pytest.mark.parametrize('name', sorted(FORMULAS))
def test_source_compiles(name, tmp_path):
    """hipcc --offload-arch=gfx950 (no device needed) builds the map of
    every golden formula, with all entry points."""
    from graphdot_amd.kernel._kom_map import DeviceMap
    from graphdot_amd.hip import jit
    f = FORMULAS[name]
    m = DeviceMap(f['expr'], 'd', tuple(f['hypers']))
    src = tmp_path / 'kom.hip'
    src.write_text(m.source)
    out = tmp_path / 'kom.hsaco'
    r = subprocess.run([jit.HIPCC, *jit.BASE_FLAGS, '-fno-fast-math',
                        f'-I{jit.DEVICE_INCLUDE}', str(src), '-o', str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    image = out.read_bytes()
    for mode in ('value', 'dense', 'lazy'):
        for a in ('f32', 'f64'):
            for b in ('f32', 'f64'):
                assert f'kom_{mode}_{a}_{b}'.encode() in image


def test_unsupported_function():
    """besselk has no device spelling: the device methods raise TypeError
    (the consumers' cue for the host path), the host path still works."""
    class DeviceStub(PairwiseDistance):
        def device_distance(self, X, Y=None, eval_gradient=False):
            raise AssertionError('the distance must not be evaluated')
    k = KernelOverMetric(DeviceStub(1.0), 'v * besselk(1, d + 1)', 'd',
                         v=2.0)
    for call in (lambda: k.device_gram([0.0, 1.0]),
                 lambda: k.device_gram([0.0, 1.0], eval_gradient=True),
                 lambda: k.device_cross_gram([0.0], [1.0])):
        with pytest.raises(TypeError):
            call()
    X = np.array([0.0, 0.5, 2.0])
    import scipy.special
    K, G = k(X, eval_gradient=True)
    D = np.abs(np.subtract.outer(X, X))
    assert np.allclose(K, 2.0 * scipy.special.kv(1, D + 1), rtol=1e-12)
    assert np.allclose(G[:, :, 0], scipy.special.kv(1, D + 1), rtol=1e-12)


def test_no_device_distance():
    k = KernelOverMetric(PairwiseDistance(1.0), 'exp(-d)', 'd')
    for call in (lambda: k.device_gram([0.0, 1.0]),
                 lambda: k.device_cross_gram([0.0], [1.0]),
                 lambda: k.device_diag([0.0])):
        with pytest.raises(TypeError):
            call()


def test_exports_without_gpu():
    """The package exports the reference's three kernels; importing it
    loads neither torch nor the HIP runtime."""
    code = ('import sys\n'
            'from graphdot_amd.kernel import (KernelOverMetric, '
            'MarginalizedGraphKernel, Tang2019MolecularKernel)\n'
            'import graphdot_amd.kernel as k\n'
            'from graphdot_amd.hip import runtime\n'
            'assert set(k.__all__) == {"KernelOverMetric", '
            '"MarginalizedGraphKernel", "Tang2019MolecularKernel"}\n'
            'assert "torch" not in sys.modules\n'
            'assert runtime._lib is None\n')
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, '-c', code], cwd=root,
                       capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=root))
    assert r.returncode == 0, r.stderr
