"""The device-path protocol of the kernels.

A kernel (or distance) that can leave its result in GPU memory implements
``device_gram`` / ``device_cross_gram`` / ``device_diag``
(``device_distance``) and ``active_theta_mask``.  Where such a method cannot
run on the device -- no HIP backend, pairs sharded over ranks, a wrapped
kernel without the method, a formula without a device spelling -- it raises
`NoDevicePath`, and the caller takes the host path.  Any other exception,
a plain `TypeError` included, is an error and propagates."""
import numpy as np


class NoDevicePath(TypeError):
    """This kernel (in this configuration, on these inputs) has no device
    path.  A `TypeError` for callers that caught that before."""


def active_planes(kernel, n_columns):
    """Indices of the gradient columns that belong to the active
    hyperparameters, out of the `n_columns` a device method handed over: a
    graph kernel hands over all its columns (then `active_theta_mask` picks),
    transformers and formulas only the active ones (then all of them)."""
    mask = np.asarray(getattr(kernel, 'active_theta_mask',
                              np.ones(n_columns, dtype=bool)))
    if len(mask) == n_columns:
        return np.flatnonzero(mask)
    return np.arange(n_columns)
