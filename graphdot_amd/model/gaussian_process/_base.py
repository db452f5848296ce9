"""What the Gaussian process models share (the responsibilities of the
reference's model/gaussian_process/base.py): the training data and the
masking of unusable targets, the regularised kernel matrices, the dense
algebra's device, the prologue of every objective, the multi-start
hyperparameter search and persistence."""
import os
import pickle
import numpy as np
from .._fit import multistart


class GaussianProcessRegressorBase:

    def __init__(self, kernel, beta, optimizer, normalize_y, regularization,
                 kernel_options, device):
        self.kernel = kernel
        self.beta = beta
        self.optimizer = 'L-BFGS-B' if optimizer is True else optimizer
        self.normalize_y = normalize_y
        self.regularization = regularization
        self.kernel_options = dict(kernel_options)
        self.device = device

    # -- data ---------------------------------------------------------------
    @property
    def X(self):
        try:
            return self._X
        except AttributeError:
            raise AttributeError(
                'Training data does not exist. Please provide using fit().')

    @X.setter
    def X(self, X):
        self._X = np.asarray(X)

    @property
    def y(self):
        try:
            return self._y * self._ystd + self._ymean
        except AttributeError:
            raise AttributeError(
                'Training data does not exist. Please provide using fit().')

    @staticmethod
    def mask(iterable):
        """(mask of usable targets, the usable targets as float64)."""
        values = list(iterable)
        mask = np.array([v is not None and bool(np.isfinite(v))
                         for v in values], dtype=bool)
        masked = np.array([float(v) for v, m in zip(values, mask) if m],
                          dtype=np.float64)
        return mask, masked

    @y.setter
    def y(self, y):
        self._y_mask, y_masked = self.mask(y)
        if self.normalize_y is True:
            self._ymean, self._ystd = y_masked.mean(), y_masked.std()
            self._y = (y_masked - self._ymean) / self._ystd
        else:
            self._ymean, self._ystd = 0, 1
            self._y = y_masked

    # -- kernel matrices --------------------------------------------------------
    def _regularize(self, K, alpha):
        if self.regularization in ('+', 'additive'):
            return K + alpha
        if self.regularization in ('*', 'multiplicative'):
            return K * (1 + alpha)
        raise RuntimeError(
            f'Unknown regularization method {self.regularization}.')

    def _gramian(self, alpha, X, Y=None, kernel=None, jac=False, diag=False):
        kernel = kernel or self.kernel
        opts = self.kernel_options
        if Y is not None:
            if diag is True:
                raise ValueError(
                    'Diagonal Gramian does not exist between two sets.')
            return kernel(X, Y, eval_gradient=True, **opts) if jac \
                else kernel(X, Y, **opts)
        if diag is True:
            return self._regularize(kernel.diag(X, **opts), alpha)
        if jac is True:
            K, J = kernel(X, eval_gradient=True, **opts)
        else:
            K, J = kernel(X, **opts), None
        K = np.array(K, dtype=np.float64)
        step = len(K) + 1
        K.flat[::step] = self._regularize(K.flat[::step], alpha)
        return (K, J) if jac is True else K

    def _dense(self):
        from .gpr import _Dense
        if not isinstance(getattr(self, '_la', None), _Dense) \
                or self._la_device != self.device:
            self._la, self._la_device = _Dense(self.device), self.device
        return self._la

    # -- objectives ---------------------------------------------------------------
    def _targets(self, X, y):
        """(X, usable targets, their mask) of explicit arguments or of the
        training set."""
        X = X if X is not None else self._X
        if y is not None:
            y_mask, y = self.mask(y)
        else:
            y, y_mask = self._y, self._y_mask
        return X, y, y_mask

    def _kernel_at(self, theta, clone_kernel):
        """The kernel at `theta`: a clone, or the model's own kernel moved
        there."""
        if clone_kernel is True:
            return self.kernel.clone_with_theta(theta)
        self.kernel.theta = theta
        return self.kernel

    def _prologue(self, theta, X, y, clone_kernel):
        """(theta, X, y, y_mask, kernel) every objective starts from."""
        theta = np.array(theta if theta is not None else self.kernel.theta,
                         dtype=float)
        X, y, y_mask = self._targets(X, y)
        return theta, X, y, y_mask, self._kernel_at(theta, clone_kernel)

    # -- fitting ------------------------------------------------------------------
    def _optimize(self, objective, loss, tol, repeat, theta_jitter, verbose):
        """Move the kernel to the best of `repeat` minimisations of
        `objective`: from its theta, then from theta plus normal noise of
        scale `theta_jitter` (all drawn before the first run)."""
        x0 = np.array(self.kernel.theta, dtype=float)
        starts = [x0] + [x0 + theta_jitter * np.random.randn(len(x0))
                         for _ in range(repeat - 1)]
        best = multistart(
            lambda t: objective(t, eval_gradient=True, clone_kernel=False,
                                verbose=verbose),
            starts, self.optimizer, self.kernel.bounds, tol)
        if verbose:
            print(f'Optimization result:\n{best}')
        if not best.success:
            raise RuntimeError(
                f'Training using the {loss} loss did not converge, got:\n'
                f'{best}')
        self.kernel.theta = best.x
        #: the optimiser's report (scipy OptimizeResult: nit, nfev, fun)
        self.optimization_result = best

    # -- persistence ---------------------------------------------------------------
    def save(self, path, filename='model.pkl', overwrite=False):
        """Pickle the trained state (without the kernel object; its
        hyperparameters are stored as `theta`)."""
        f_model = os.path.join(path, filename)
        if os.path.isfile(f_model) and not overwrite:
            raise RuntimeError(
                f'Path {f_model} already exists. To overwrite, set '
                '`overwrite=True`.')
        store = {k: v for k, v in self.__dict__.items()
                 if k not in ('kernel', '_la')}
        store['theta'] = np.array(self.kernel.theta)
        with open(f_model, 'wb') as f:
            pickle.dump(store, f, protocol=4)

    def load(self, path, filename='model.pkl'):
        with open(os.path.join(path, filename), 'rb') as f:
            store = pickle.load(f)
        theta = store.pop('theta')
        self.__dict__.update(**store)
        self.kernel.theta = theta
