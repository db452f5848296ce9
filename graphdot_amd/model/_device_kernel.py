"""How the models ask a kernel for its device path:
the one place that catches `NoDevicePath`, the preconditions the models
share, and the adoption of the kernel's device views."""
from ..kernel._device_path import NoDevicePath, active_planes  # noqa: F401


def device_call(kernel, method, *args, **kwargs):
    """``kernel.method(*args, **kwargs)``, or None if the kernel has no such
    method or the method raised `NoDevicePath`.  Every other exception --
    a `TypeError` for a wrong keyword or graphs of mixed attribute types
    included -- propagates."""
    fn = getattr(kernel, method, None)
    if fn is None:
        return None
    try:
        return fn(*args, **kwargs)
    except NoDevicePath:
        return None


def on_device(la, kernel_options):
    """May a model with the dense algebra `la` ask for the device path at
    all?  The algebra runs on a GPU and no kernel options are in the way
    (the device methods do not take them)."""
    return la.device.type == 'cuda' and not kernel_options


def as_float64(view, device):
    """The kernel's device view (or tensor) as a float64 tensor on
    `device`."""
    import torch
    return torch.as_tensor(view, device=device).to(torch.float64)
