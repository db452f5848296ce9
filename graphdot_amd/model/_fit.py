"""The multi-start hyperparameter search every model's `fit` runs."""
from scipy.optimize import minimize


def multistart(fun, starts, method, bounds, tol):
    """``scipy.optimize.minimize`` of `fun` (value and gradient) from every
    start in turn; keeps the first result, then any successful one with a
    smaller value.  `starts` is consumed lazily: a generator that draws its
    random numbers between the runs keeps its order of draws."""
    best = None
    for x0 in starts:
        res = minimize(fun=fun, method=method, x0=x0, bounds=bounds, jac=True,
                       tol=tol)
        if best is None or (res.success and res.fun < best.fun):
            best = res
    return best
