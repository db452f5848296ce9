"""Kernel transformers on top of the kernel protocol: cosine normalisation
and exponentiation (behaviour of the reference's ``graphdot/kernel/fix.py:
7-215``).  They only post-process ``kernel(X, Y, eval_gradient)`` and
``kernel.diag(X)`` with numpy, so they work with any kernel that follows the
protocol, the HIP marginalized graph kernel included.

A shared base forwards the hyperparameter interface; a transformer implements
`_apply` (values) and `_apply_jac` (values + gradient) on the raw matrix and
the two diagonals.
"""
import copy
import numpy as np
from ..util.pretty_tuple import pretty_tuple
from ._device_path import NoDevicePath


class _Transformed:
    """kernel -> kernel, same protocol."""

    def __init__(self, kernel):
        self.kernel = kernel

    # -- hyperparameter interface: the wrapped kernel's by default -----------
    @property
    def hyperparameters(self):
        return self.kernel.hyperparameters

    @property
    def theta(self):
        return self.kernel.theta

    @theta.setter
    def theta(self, value):
        self.kernel.theta = value

    @property
    def hyperparameter_bounds(self):
        return self.kernel.hyperparameter_bounds

    @property
    def bounds(self):
        return self.kernel.bounds

    def clone_with_theta(self, theta):
        clone = copy.deepcopy(self)
        clone.theta = theta
        return clone

    # -- optional device path (see MarginalizedGraphKernel.device_gram) --------
    @property
    def active_theta_mask(self):
        return self.kernel.active_theta_mask

    def _inner_device_gram(self, X, eval_gradient):
        """float64 torch tensors (K, dK over all hyperparameter columns) of
        the wrapped kernel on the GPU; NoDevicePath if it has none."""
        inner = getattr(self.kernel, 'device_gram', None)
        if inner is None:
            raise NoDevicePath('the wrapped kernel has no device_gram')
        import torch
        out = inner(X, eval_gradient=eval_gradient)
        R, dR = out if eval_gradient else (out, None)
        R = torch.as_tensor(R, device='cuda').to(torch.float64)
        if dR is not None:
            dR = torch.as_tensor(dR, device='cuda').to(torch.float64)
        return R, dR

    def _inner_cross(self, X, Y, eval_gradient):
        """float64 torch tensor of the wrapped kernel's ``(X, Y)`` matrix
        and its gradient as a `LazyGradient`, from the kernel's device
        methods; NoDevicePath if it has none."""
        inner = getattr(self.kernel, 'device_cross_gram', None)
        if inner is None:
            raise NoDevicePath('the wrapped kernel has no device_cross_gram')
        import torch
        out = inner(X, Y, eval_gradient=eval_gradient)
        R, dR = out if eval_gradient else (out, None)
        R = torch.as_tensor(R, device='cuda').to(torch.float64)
        if dR is not None and not isinstance(dR, LazyGradient):
            dR = LazyGradient(torch.as_tensor(dR, device='cuda'))
        return R, dR

    def _inner_diag(self, X, eval_gradient):
        """float64 torch tensors of the wrapped kernel's `device_diag`."""
        inner = getattr(self.kernel, 'device_diag', None)
        if inner is None:
            raise NoDevicePath('the wrapped kernel has no device_diag')
        import torch
        out = inner(X, eval_gradient=eval_gradient)
        d, dd = out if eval_gradient else (out, None)
        d = torch.as_tensor(d, device='cuda').to(torch.float64)
        if dd is not None:
            dd = torch.as_tensor(dd, device='cuda').to(torch.float64)
        return d, dd


class LazyGradient:
    r"""The gradient ``dK[i, c, k]`` of an N x M kernel matrix, kept in
    factors on the device instead of as an N x M x n float64 tensor:

    .. math::
        dK_{ick} = \mathrm{lead}_{ick}                       \quad k < n_l

        dK_{ick} = a_i b_c S_{ic} P_{ic(k - n_l)}               \quad k \ge n_l

    plus, over every column, the terms
    :math:`\sum_t L^t_{ic} (u^t_{ik} + v^t_{ck})`.  `P` are the graph
    kernel's raw planes in the type it stored them in (column-major, as
    `device_cross_gram` hands them over); `a`, `b` per-row and per-column
    factors, `S` an element-wise factor (None: ones); `lead` a few float64
    columns put in front (`Exponentiation`'s exponent).  `contract(W)` costs
    one pass over `P` (lowrank.hip on the GPU) and O(N M) per other term;
    `dense()` materialises the float64 tensor (tests, host paths)."""

    def __init__(self, planes, row=None, col=None, scale=None, lead=None,
                 terms=()):
        self.planes = planes
        self.row, self.col, self.scale = row, col, scale
        self.lead = lead
        self.terms = list(terms)

    @property
    def shape(self):
        N, M, n = self.planes.shape
        return (N, M, n + (self.lead.shape[2] if self.lead is not None
                           else 0))

    def _factor(self):
        """a b^T * S as one float64 (N, M) tensor, or None for ones."""
        import torch
        f = self.scale
        if self.row is not None:
            rc = self.row[:, None] * self.col[None, :]
            f = rc if f is None else f * rc
        if f is not None:
            f = f.to(torch.float64)
        return f

    def scaled(self, row=None, col=None, scale=None):
        """The gradient with every column multiplied element-wise by
        ``row[i] col[c] scale[i, c]`` (any of them None: ones)."""
        def mul(a, b):
            return b if a is None else (a if b is None else a * b)
        rc = None
        if row is not None:
            rc = row[:, None] * col[None, :]
        full = mul(rc, scale)
        return LazyGradient(
            self.planes,
            mul(self.row, row), mul(self.col, col), mul(self.scale, scale),
            self.lead if self.lead is None or full is None
            else self.lead * full[:, :, None],
            [(L if full is None else L * full, u, v)
             for L, u, v in self.terms])

    def with_term(self, L, u, v):
        """Plus ``L[i, c] (u[i, k] + v[c, k])`` over every column."""
        return LazyGradient(self.planes, self.row, self.col, self.scale,
                            self.lead, self.terms + [(L, u, v)])

    def with_lead(self, column):
        """With the float64 (N, M) `column` put in front of the others."""
        import torch
        lead = column[:, :, None] if self.lead is None else torch.cat(
            (column[:, :, None], self.lead), dim=2)
        zero = [(L, torch.cat((torch.zeros_like(u[:, :1]), u), dim=1),
                 torch.cat((torch.zeros_like(v[:, :1]), v), dim=1))
                for L, u, v in self.terms]
        return LazyGradient(self.planes, self.row, self.col, self.scale,
                            lead, zero)

    def contract(self, W, rows=None):
        """``out[k] = sum_{r, c} W[r, c] dK[rows[r], c, k]``: W a float64
        (Nr, M) tensor on the gradient's device, `rows` None (all N rows) or
        the Nr row indices (a host array) W stands for.  Returns the float64
        sums (a tensor of `shape[2]`), enqueued in stream order."""
        import torch
        from ..model.gaussian_process import _lowrank
        idx = None
        if rows is not None:
            idx = torch.as_tensor(np.asarray(rows, dtype=np.int64),
                                  device=W.device)

        def pick(a):
            return a if idx is None else a.index_select(0, idx)
        f = self._factor()
        Wp = W if f is None else W * pick(f)
        if self.planes.is_cuda:
            out = _lowrank.contract(self.planes, Wp, rows)
        else:
            out = _lowrank.contract_torch(self.planes, Wp, rows)
        if self.lead is not None:
            out = torch.cat((torch.einsum('ic,ick->k', W, pick(self.lead)),
                             out))
        for L, u, v in self.terms:
            A = W * pick(L)
            out = out + pick(u).T @ A.sum(1) + v.T @ A.sum(0)
        return out

    def dense(self):
        """The float64 (N, M, n) tensor."""
        import torch
        g = self.planes.to(torch.float64)
        f = self._factor()
        if f is not None:
            g = g * f[:, :, None]
        if self.lead is not None:
            g = torch.cat((self.lead, g), dim=2)
        for L, u, v in self.terms:
            g = g + L[:, :, None] * (u[:, None, :] + v[None, :, :])
        return g


class Normalization(_Transformed):
    r""":math:`k_n(x, y) = k(x, y) / \sqrt{k(x, x)\,k(y, y)}`."""

    def __call__(self, X, Y=None, eval_gradient=False, **options):
        k = self.kernel
        if eval_gradient is True:
            R, dR = k(X, Y, eval_gradient=True, **options)
            if Y is None:
                dl, ddl = R.diagonal(), np.einsum('iik->ik', dR)
                dr, ddr = dl, ddl
            else:
                dl, ddl = k.diag(X, True, **options)
                dr, ddr = k.diag(Y, True, **options)
        else:
            R = k(X, Y, **options)
            if Y is None:
                dl = dr = R.diagonal()
            else:
                dl, dr = k.diag(X, **options), k.diag(Y, **options)
        sl, sr = dl**-0.5, dr**-0.5
        K = sl[:, None] * R * sr[None, :]
        if eval_gradient is not True:
            return K
        # d(R / sqrt(a b)) = dR / sqrt(a b) - K (da / a + db / b) / 2
        dK = (sl[:, None, None] * dR * sr[None, :, None]
              - 0.5 * K[:, :, None] * ((ddl / dl[:, None])[:, None, :]
                                       + (ddr / dr[:, None])[None, :, :]))
        return K, np.asfortranarray(dK)

    def device_gram(self, X, eval_gradient=False, local_gradient=False):
        """`__call__(X)` computed on the GPU from the wrapped kernel's device
        buffers; returns torch tensors.  (`local_gradient`: accepted for the
        regressor's call and not forwarded -- the transformation needs the
        whole gradient planes, not one rank's pairs.)"""
        R, dR = self._inner_device_gram(X, eval_gradient)
        d = R.diagonal()
        s = d.rsqrt()
        K = s[:, None] * R * s[None, :]
        if not eval_gradient:
            return K
        rel = dR.diagonal(dim1=0, dim2=1).T / d[:, None]      # d log k(x, x)
        dK = (s[:, None, None] * dR * s[None, :, None]
              - 0.5 * K[:, :, None] * (rel[:, None, :] + rel[None, :, :]))
        return K, dK

    def device_cross_gram(self, X, Y, eval_gradient=False):
        """`__call__(X, Y)` on the GPU from the wrapped kernel's device
        methods: a float64 torch tensor and, with `eval_gradient`, a
        `LazyGradient` over all of the wrapped kernel's columns,
        ``s_i t_c dR - K (rel_x[i] + rel_c[c]) / 2`` with ``s, t`` the
        inverse square roots of the two diagonals and ``rel`` their
        logarithmic derivatives."""
        R, dR = self._inner_cross(X, Y, eval_gradient)
        dx, ddx = self._inner_diag(X, eval_gradient)
        dy, ddy = self._inner_diag(Y, eval_gradient)
        s, t = dx.rsqrt(), dy.rsqrt()
        K = s[:, None] * R * t[None, :]
        if not eval_gradient:
            return K
        dK = dR.scaled(row=s, col=t).with_term(
            K, -0.5 * ddx / dx[:, None], -0.5 * ddy / dy[:, None])
        return K, dK

    def device_diag(self, X, eval_gradient=False):
        """`diag(X)` as float64 torch tensors: ones, and, like `diag`, ones
        for the gradient (over all of the wrapped kernel's columns)."""
        import torch
        one = torch.ones(len(X), dtype=torch.float64, device='cuda')
        if not eval_gradient:
            return one
        n = len(np.asarray(self.kernel.active_theta_mask))
        return one, torch.ones((len(X), n), dtype=torch.float64,
                               device='cuda')

    def diag(self, X, eval_gradient=False, **options):
        """Ones (and, like the reference, ones for the 'gradient')."""
        one = np.ones(len(X))
        if eval_gradient is True:
            return one, np.ones((len(X), len(self.kernel.theta)))
        return one


class Exponentiation(_Transformed):
    r""":math:`k_\xi(x, y) = k(x, y)^\xi`; the exponent is the first
    hyperparameter (`xi_bounds`: its search range)."""

    def __init__(self, kernel, xi=1.0, xi_bounds=(0.1, 20.0)):
        super().__init__(kernel)
        self.xi = xi
        self.xi_bounds = xi_bounds

    def __call__(self, X, Y=None, eval_gradient=False, **options):
        if eval_gradient is not True:
            return self.kernel(X, Y, **options)**self.xi
        R, dR = self.kernel(X, Y, eval_gradient=True, **options)
        K = R**self.xi
        # columns: d/d xi = K log R, then xi R^(xi - 1) dR/d theta
        dK = np.concatenate(((K * np.log(R))[:, :, None],
                             (self.xi * R**(self.xi - 1))[:, :, None] * dR),
                            axis=2)
        return K, dK

    def device_gram(self, X, eval_gradient=False, local_gradient=False):
        """(`local_gradient` is accepted and not forwarded: see
        `Normalization.device_gram`.)"""
        import torch
        R, dR = self._inner_device_gram(X, eval_gradient)
        K = R**self.xi
        if not eval_gradient:
            return K
        return K, torch.cat(((K * R.log())[:, :, None],
                             (self.xi * R**(self.xi - 1))[:, :, None] * dR),
                            dim=2)

    def device_cross_gram(self, X, Y, eval_gradient=False):
        """`__call__(X, Y)` on the GPU: a float64 torch tensor and a
        `LazyGradient` whose first column is ``K log R`` and whose others
        are the wrapped kernel's, times ``xi R^(xi - 1)``."""
        R, dR = self._inner_cross(X, Y, eval_gradient)
        K = R**self.xi
        if not eval_gradient:
            return K
        return K, dR.scaled(scale=self.xi * R**(self.xi - 1)).with_lead(
            K * R.log())

    def device_diag(self, X, eval_gradient=False):
        """`diag(X)` on the GPU, as float64 torch tensors."""
        import torch
        d, dd = self._inner_diag(X, eval_gradient)
        k = d**self.xi
        if not eval_gradient:
            return k
        return k, torch.cat(((k * d.log())[:, None],
                             (self.xi * d**(self.xi - 1))[:, None] * dd),
                            dim=1)

    @property
    def active_theta_mask(self):
        return np.concatenate(([True], self.kernel.active_theta_mask))

    def diag(self, X, eval_gradient=False, **options):
        """``kernel.diag(X) ** xi`` (with the gradient, which the reference's
        class does not offer, so that Normalization can wrap this one for
        X-versus-Y evaluations too)."""
        if eval_gradient is not True:
            return self.kernel.diag(X, **options)**self.xi
        d, dd = self.kernel.diag(X, True, **options)
        k = d**self.xi
        return k, np.concatenate(((k * np.log(d))[:, None],
                                  (self.xi * d**(self.xi - 1))[:, None] * dd),
                                 axis=1)

    @property
    def hyperparameters(self):
        return pretty_tuple('Exponentiation', ['xi', 'kernel'])(
            self.xi, self.kernel.hyperparameters)

    @property
    def theta(self):
        return np.concatenate((np.log([self.xi]), self.kernel.theta))

    @theta.setter
    def theta(self, value):
        self.xi = float(np.exp(value[0]))
        self.kernel.theta = value[1:]

    @property
    def hyperparameter_bounds(self):
        return pretty_tuple('Exponentiation', ['xi', 'kernel'])(
            self.xi_bounds, self.kernel.hyperparameter_bounds)

    @property
    def bounds(self):
        return np.vstack((np.log([self.xi_bounds]), self.kernel.bounds))
