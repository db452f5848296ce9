"""Same import path as the reference's ``graphdot.experimental.metric``."""
from .m3 import M3

__all__ = ['M3']
