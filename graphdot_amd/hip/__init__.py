"""HIP runtime plumbing for the MI355X backend: ctypes binding of
``libgdhip.so`` (C ABI in ``include/gdhip.h``) and the hipcc JIT driver.
Takes the role of the reference's ``graphdot/cuda`` package (PyCUDA)."""

__all__ = ['lib', 'HIPError', 'DeviceBuffer', 'device_props', 'ensure_device']


def __getattr__(name):
    # the binding comes in with its first use: the host-side modules (hostlib,
    # the solver menu of kernel/marginalized/_menu.py) import this package
    # without it
    if name in __all__:
        from . import runtime
        return getattr(runtime, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
