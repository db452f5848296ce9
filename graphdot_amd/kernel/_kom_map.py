"""Host side of kernel_over_metric.hip, the element-wise map of
`KernelOverMetric` on the GPU: fills the template with the formula and its
derivatives (the sympy printer of graphdot_amd.codegen, float64 spelling),
compiles it once per formula (JIT cache of graphdot_amd.hip.jit, IEEE
arithmetic: no fast-math) and runs it on torch's *current* stream of the
distance's device, in stream order with the torch operations around it.  One
launch per call and no host synchronisation.

The hyperparameter values are a kernel argument: the generated source, and
so the cache key, depends only on the expression, the distance symbol and the
hyperparameter names, and an optimiser's steps never compile again."""
import functools
import os
import numpy as np
import sympy
from ..hip.source_module import SourceModule, current_stream, suffix
from ._device_path import NoDevicePath

_TEMPLATE = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         'kernel_over_metric.hip')
_BLOCK = 256


def _print(expr, symbols):
    """Device C++ (float64) for `expr`; NoDevicePath if the printer cannot
    express it."""
    from ..codegen.sympy_printer import hipcxxcode, to_real_expr
    try:
        text = hipcxxcode(expr, symbols)
    except Exception as e:   # (PrintMethodNotImplementedError and kin)
        raise NoDevicePath(f'no device spelling for {expr}: {e}') from None
    if 'Not supported' in text or 'not supported' in text:
        raise NoDevicePath(f'no device spelling for {expr}')
    return to_real_expr(text, 'float64')


def generate(expr, x, names):
    """The HIP source of the map for ``f = expr(x; names)``: f, df/dx and
    df/dh for every name in order.  NoDevicePath where the printer cannot
    express one of them."""
    from ..codegen import Template
    expr = sympy.sympify(expr)
    xs = sympy.Symbol(x)
    hs = [sympy.Symbol(h) for h in names]
    symbols = {x: 'd'}
    symbols.update({h: f'H.h[{k}]' for k, h in enumerate(names)})
    for s in expr.free_symbols:
        if str(s) not in symbols:
            raise NoDevicePath(f'free symbol {s} is neither the distance '
                               f'{x!r} nor a hyperparameter')
    fun = _print(expr, symbols)
    dfdx = _print(sympy.diff(expr, xs), symbols)
    own = [f'    G[e + N * {k}] = {_print(sympy.diff(expr, h), symbols)};'
           for k, h in enumerate(hs)]
    with open(_TEMPLATE) as f:
        template = Template(f.read())
    return template.render(n_hyper=len(names), fun=fun, dfdx=dfdx,
                           own='\n'.join(own) if own else '    (void)d;')


@functools.lru_cache(maxsize=64)
def device_map(expr, x, names):
    """The `DeviceMap` of a formula, shared by every kernel (and clone)
    that uses it."""
    return DeviceMap(expr, x, names)


class DeviceMap(SourceModule):
    """The compiled map of one formula."""

    def __init__(self, expr, x, names):
        super().__init__(source=generate(expr, x, names))
        self.n_hyper = len(names)

    def __call__(self, D, h, P=None, planes=(), form='value'):
        """Map the distance matrix D (an (nr, nc) float32 / float64 CUDA
        tensor, any strides) at the hyperparameter values `h`.  `form`:
        'value' -> K; 'dense' -> (K, G) with G the (nr, nc, n_h + len(planes))
        gradient, the planes `planes` of P (nr, nc, n_planes; any strides)
        times df/dx; 'lazy' -> (K, G_own, S) with G_own the n_h planes df/dh
        and S = df/dx.  Every output float64, column-major, enqueued on
        torch's current stream."""
        import torch
        if D.dim() != 2 or not D.is_cuda:
            raise TypeError('D: a 2-D CUDA tensor expected')
        h = np.asarray(h, dtype=np.float64).ravel()
        if len(h) != self.n_hyper:
            raise ValueError(f'{self.n_hyper} hyperparameter values '
                             f'expected, got {len(h)}')
        planes = np.asarray(planes, dtype=np.int64).ravel()
        if form != 'dense':
            planes = planes[:0]
        np_ = len(planes)
        nr, nc = D.shape
        dev = D.device
        if np_:
            if P is None or P.dim() != 3 or tuple(P.shape[:2]) != (nr, nc):
                raise ValueError(f'P: shape ({nr}, {nc}, n_planes) expected')
            if P.device != dev:
                raise ValueError('P and D on different devices')
            if planes.min() < 0 or planes.max() >= P.shape[2]:
                raise IndexError('plane index out of range')
        with torch.cuda.device(dev):
            def fortran(*shape):
                return torch.empty(shape[::-1], dtype=torch.float64,
                                   device=dev).permute(
                                       *range(len(shape) - 1, -1, -1))
            K = fortran(nr, nc)
            G = S = None
            if form == 'dense':
                G = fortran(nr, nc, self.n_hyper + np_)
            elif form == 'lazy':
                G = fortran(nr, nc, self.n_hyper)
                S = fortran(nr, nc)
            elif form != 'value':
                raise ValueError(f'unknown form {form!r}')
            if nr and nc:
                name = (f'kom_{form}_{suffix(D.dtype)}_'
                        f'{suffix(P.dtype if np_ else D.dtype)}')
                pk = torch.from_numpy(planes).to(dev) if np_ else None
                gx = -(-nr // _BLOCK)
                if gx * nc >= 2**31:
                    raise ValueError(f'{nr} x {nc}: too many workgroups')
                self.launch(
                    name, gx * nc, _BLOCK,
                    'Qqqqqq' + 'Qqqq' + 'Qq' + 'QQQ'
                    + f'{max(self.n_hyper, 1)}d',
                    D.data_ptr(), D.stride(0), D.stride(1), nr, nc, gx,
                    P.data_ptr() if np_ else 0,
                    *(P.stride()[:3] if np_ else (0, 0, 0)),
                    pk.data_ptr() if np_ else 0, np_,
                    K.data_ptr(), G.data_ptr() if G is not None else 0,
                    S.data_ptr() if S is not None else 0,
                    *(h if self.n_hyper else [0.0]),
                    stream=current_stream(dev))
        if form == 'value':
            return K
        if form == 'dense':
            return K, G
        return K, G, S
