"""A kernel made from a distance and a formula: ``k(x, y) = f(d(x, y))``.

Behaviour of the reference's ``graphdot.kernel.KernelOverMetric``
(kernel/_kernel_over_metric.py): the same constructor, hyperparameter forms,
``theta`` / ``bounds`` layout, ``hyperparameters`` tuple and output dtypes
(K in the distance's dtype, the gradient in float64), evaluated on the host
with ``sympy.lambdify`` instead of a compiled ``ufuncify`` (no C toolchain at
run time).  The reference writes K into the distance's array; here K is a new
array.  ``clone_with_theta`` passes the distance its own theta (the
reference calls ``distance.clone_with_theta()`` without one, which
`MaxiMin` does not accept).

With a distance that offers ``device_distance`` (`MaxiMin` on the HIP
backend), ``device_gram``, ``device_cross_gram`` and ``device_diag`` keep
the distance and the kernel on the GPU: kernel_over_metric.hip maps D (and
its gradient planes) to K and the gradient in one pass (_kom_map.py;
DESIGN.md section 21).
"""
from collections import OrderedDict
import functools
import numpy as np
import sympy
from ..util.pretty_tuple import pretty_tuple
from ._device_path import NoDevicePath, active_planes

#: what the host evaluation of a formula may call (scipy: special functions
#: such as besselk, which have no device spelling)
_MODULES = ('scipy', 'numpy')


@functools.lru_cache(maxsize=64)
def _host_functions(expr, x, names):
    """f, [df/dh for h in names] and df/dx as numpy functions of (x,
    *names); shared by every kernel (and clone: a regressor clones the
    kernel at every evaluation) with the same formula."""
    xs = sympy.symbols(x)
    hs = [sympy.symbols(h) for h in names]
    args = (xs, *hs)
    return (sympy.lambdify(args, expr, _MODULES),
            [sympy.lambdify(args, sympy.diff(expr, t), _MODULES) for t in hs],
            sympy.lambdify(args, sympy.diff(expr, xs), _MODULES))


class KernelOverMetric:
    """Kernel ``expr(x; hyperparameters)`` over the values ``x`` of
    `distance`.

    Parameters
    ----------
    distance: a metric with ``__call__(X, Y=None, eval_gradient=False)``,
        ``theta``, ``bounds``, ``hyperparameters`` and ``clone_with_theta``.
    expr: str or sympy expression of the distance symbol and the
        hyperparameters.
    x: str
        The name of the distance in `expr`.
    hyperparameters:
        ``name=value``, ``name=(value,)`` (bounds (0, inf)),
        ``name=(value, (lo, hi))`` or ``name=(value, lo, hi)``.
    """

    def __init__(self, distance, expr, x, **hyperparameters):
        self._init_args = (expr, x)
        self._init_kwargs = hyperparameters
        self.distance = distance
        self.expr = sympy.sympify(expr)
        self._hyperparams = OrderedDict()
        self._hyperbounds = OrderedDict()
        for key, val in hyperparameters.items():
            if not hasattr(val, '__iter__'):
                self._hyperparams[key] = val
                self._hyperbounds[key] = (0, np.inf)
            elif len(val) == 1:
                self._hyperparams[key] = val[0]
                self._hyperbounds[key] = (0, np.inf)
            elif len(val) == 2:
                self._hyperparams[key] = val[0]
                self._hyperbounds[key] = val[1]
            elif len(val) == 3:
                self._hyperparams[key] = val[0]
                self._hyperbounds[key] = (val[1], val[2])
        self.x = x
        self._fun, self._grad, self._grad_m = _host_functions(
            self.expr, x, tuple(self._hyperparams))
        self._device_map = None

    # -- host path -----------------------------------------------------------------
    def _eval(self, fn, d):
        """float64 values of `fn` at the float64 array `d` (a formula that
        does not depend on d still gives an array of d's shape)."""
        d = np.asarray(d, dtype=np.float64)
        return np.broadcast_to(
            np.asarray(fn(d, *self._hyperparams.values()), dtype=np.float64),
            d.shape)

    def __call__(self, X, Y=None, eval_gradient=False):
        if eval_gradient is False:
            return self._gramian(self.distance(X, Y))
        M, dM = self.distance(X, Y, eval_gradient=True)
        nh = len(self._grad)
        grad = np.empty((*M.shape, len(self.theta)), order='F')
        for i, g in enumerate(self._grad):
            grad[:, :, i] = self._eval(g, M)
        if len(self.distance.theta) > 0:
            grad[:, :, nh:] = self._eval(self._grad_m, M)[:, :, None]
            np.multiply(grad[:, :, nh:], dM, out=grad[:, :, nh:])
        return self._gramian(M), grad

    def _gramian(self, d):
        """f(d), in d's dtype (the reference's ufunc writes into d)."""
        d = np.asarray(d)
        dtype = d.dtype if np.issubdtype(d.dtype, np.floating) else np.float64
        return self._eval(self._fun, d).astype(dtype)

    def diag(self, X):
        return np.array(self._eval(self._fun, np.zeros(len(X))))

    def get_params(self):
        return self._hyperparams

    @property
    def theta(self):
        return np.concatenate((
            np.log(list(self._hyperparams.values())),
            self.distance.theta
        ))

    @theta.setter
    def theta(self, args):
        for k, v in zip(self._hyperparams, np.exp(args)):
            self._hyperparams[k] = v
        self.distance.theta = args[len(self._hyperparams):]

    @property
    def bounds(self):
        with np.errstate(divide='ignore'):           # log(0) = -inf
            own = np.log(np.vstack(list(self._hyperbounds.values()))
                         if self._hyperbounds else np.zeros((0, 2)))
        return np.vstack((own, self.distance.bounds))

    @property
    def hyperparameters(self):
        return pretty_tuple(
            'RBFKernel',
            list(self._hyperparams.keys()) + ['distance']
        )(
            *self._hyperparams.values(),
            self.distance.hyperparameters
        )

    @property
    def active_theta_mask(self):
        """Every entry of `theta` is free (the distance's own `theta` holds
        its free hyperparameters only)."""
        return np.ones(len(self.theta), dtype=bool)

    def clone_with_theta(self, theta=None):
        if theta is None:
            theta = self.theta
        # (the reference passes no theta here; MaxiMin requires one)
        k = type(self)(self.distance.clone_with_theta(self.distance.theta),
                       *self._init_args, **self._init_kwargs)
        k.theta = theta
        return k

    # -- device path ---------------------------------------------------------------
    def _map(self):
        """The compiled element-wise map; NoDevicePath if the formula or one of
        its derivatives has no device spelling."""
        if self._device_map is None:
            from ._kom_map import device_map
            self._device_map = device_map(str(self.expr), self.x,
                                          tuple(self._hyperparams))
        return self._device_map

    def _device_inputs(self, X, Y, eval_gradient):
        """(map, D, dD planes, active plane indices) on the GPU from the
        distance's ``device_distance``; NoDevicePath where there is none."""
        fn = getattr(self.distance, 'device_distance', None)
        if fn is None:
            raise NoDevicePath('the distance has no device_distance')
        dmap = self._map()
        import torch
        torch.cuda.is_available()    # (torch's HIP runtime before libgdhip's)
        out = fn(X, Y, eval_gradient=eval_gradient)
        D, dD = out if eval_gradient else (out, None)
        D = torch.as_tensor(D, device='cuda')
        planes = np.zeros(0, dtype=np.int64)
        if dD is not None:
            dD = torch.as_tensor(dD, device='cuda')
            planes = active_planes(self.distance, dD.shape[2])
            if len(planes) != len(self.distance.theta):
                raise NoDevicePath('the distance gradient has '
                                   f'{len(planes)} active columns, its theta '
                                   f'{len(self.distance.theta)}')
        return dmap, D, dD, planes

    def _h(self):
        return np.array(list(self._hyperparams.values()), dtype=np.float64)

    def device_gram(self, X, eval_gradient=False, local_gradient=False):
        """`__call__(X)` on the GPU: K as a float64 torch tensor and, with
        `eval_gradient`, the dense float64 (n, n, len(theta)) gradient,
        column-major.  (`local_gradient` is accepted for the regressor's call
        and not forwarded, as in kernel/fix.py.)  NoDevicePath if the distance
        or the formula has no device path."""
        dmap, D, dD, planes = self._device_inputs(X, None, eval_gradient)
        if not eval_gradient:
            return dmap(D, self._h())
        return dmap(D, self._h(), dD, planes, form='dense')

    def device_cross_gram(self, X, Y, eval_gradient=False):
        """`__call__(X, Y)` on the GPU: a float64 torch tensor and, with
        `eval_gradient`, a `LazyGradient` -- the df/dh columns in front, then
        the distance's active planes as stored, scaled element-wise by
        df/dx."""
        import torch
        from .fix import LazyGradient
        dmap, D, dD, planes = self._device_inputs(X, Y, eval_gradient)
        if not eval_gradient:
            return dmap(D, self._h())
        K, G, S = dmap(D, self._h(), form='lazy')
        if len(planes) == 0:
            return K, LazyGradient(G)
        P = dD if len(planes) == dD.shape[2] else dD.index_select(
            2, torch.as_tensor(planes, device=dD.device))
        return K, LazyGradient(P, scale=S,
                               lead=G if G.shape[2] else None)

    def device_diag(self, X, eval_gradient=False):
        """`diag(X)` as float64 torch tensors: f(0) and, with
        `eval_gradient`, df/dh at 0 followed by zeros for the distance's
        columns (a distance vanishes on the diagonal)."""
        if getattr(self.distance, 'device_distance', None) is None:
            raise NoDevicePath('the distance has no device_distance')
        import torch
        n = len(X)
        z = np.zeros(1)
        k = torch.full((n,), float(self._eval(self._fun, z)[0]),
                       dtype=torch.float64, device='cuda')
        if not eval_gradient:
            return k
        g = np.zeros(len(self.theta))
        for i, fn in enumerate(self._grad):
            g[i] = self._eval(fn, z)[0]
        dk = torch.as_tensor(g, device='cuda').expand(n, len(g)).clone()
        return k, dk
