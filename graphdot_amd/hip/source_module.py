"""Host side shared by the fused dense kernels (the ``.hip`` files next to the
models that use them): `SourceModule` compiles one HIP source into the JIT
cache of `jit` and loads it once per process; `STATIC` lists the sources that
are files of the package, each with its flags, for their host modules and for
``__graft_entry__.build()``, `TEXT_UNITS` those that are a device header of
csrc/device and a few lines of text, and `FILE_UNITS` and `MODEL_UNITS` those
that are the text of a header next to its model.  Below them, the few lines every
torch-facing launch repeats.  Nothing here imports torch (or a package that
does) at module level: `build()` compiles through this module before
``libgdhip.so`` is used.
"""
import os
import struct
import threading

from . import jit, runtime

_PACKAGE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: IEEE arithmetic: none of jit.BASE_FLAGS' fast-math for these kernels
DENSE_FLAGS = ('-fno-fast-math',)
_lock = threading.Lock()
_loaded = {}        # jit cache key -> runtime.Module (one per code object)


class SourceModule:
    """One HIP translation unit, given as the path of a file or as text."""

    def __init__(self, path=None, source=None, flags=DENSE_FLAGS):
        assert (path is None) != (source is None)
        self.path = path
        self._source = source
        self.flags = tuple(flags)
        self._key = None

    @property
    def source(self):
        if self._source is None:
            with open(self.path) as f:
                self._source = f.read()
        return self._source

    @property
    def key(self):
        if self._key is None:
            self._key = jit.cache_key(self.source, self.flags)
        return self._key

    def precompile(self):
        """Compile into the JIT cache (hipcc, no device needed); the path of
        the code object."""
        return jit.compile_source(self.source, self.flags)

    @property
    def module(self):
        """The loaded `runtime.Module`: one per process and code object,
        whichever `SourceModule` of that source asks first.  (Kept in this
        module, not in the object: a kernel that holds its map can still be
        copied or pickled.)"""
        mod = _loaded.get(self.key)
        if mod is None:
            with _lock:
                mod = _loaded.get(self.key)
                if mod is None:
                    mod = _loaded[self.key] = runtime.Module(
                        jit.load_image(self.precompile()))
        return mod

    def function(self, name):
        """Kernel `name` (looked up on first use; HIPError if the code object
        has none of that name)."""
        return self.module.function(name)

    def launch(self, name, grid, block, fmt, *args, stream=None):
        """Launch kernel `name` with the arguments `args` packed as the
        struct format `fmt` (native alignment, as the kernel's parameters)."""
        runtime.launch(self.function(name), grid, block,
                       struct.pack('@' + fmt, *args), stream=stream)


#: the sources that are files of the package, relative to it
STATIC_SOURCES = (
    'model/gaussian_process/potrf.hip',
    'model/active_learning/select.hip',
    'model/gaussian_process/lowrank.hip',
    'model/gaussian_field/field.hip',
    'model/gaussian_process/outlier.hip',
    'model/gaussian_process/posterior.hip',
    'model/gaussian_process/laplace.hip',
    'model/decomposition/subspace.hip',
    'model/clustering/lloyd.hip',
    'model/svm/smo.hip',
    'model/svm/svr.hip',
    'model/alignment/alignment.hip',
    'model/two_sample/mmd.hip',
)
#: file name -> SourceModule
STATIC = {os.path.basename(p): SourceModule(os.path.join(_PACKAGE, p))
          for p in STATIC_SOURCES}


def _wrappers(*kernels):
    """The ``extern "C"`` wrappers of a text unit: (name, device function,
    parameters as 'type name, ...') each."""
    out = []
    for name, stage, params in kernels:
        names = ', '.join(p.split()[-1].lstrip('*') for p in params.split(','))
        out.append(f'extern "C" __global__ __launch_bounds__(BLOCK) void\n'
                   f'{name}({params})\n{{\n    {stage}({names});\n}}\n')
    return '\n'.join(out)


_KNN_TOPK = ('int64_t b, int64_t n, int64_t s_row, int64_t s_col, '
             'const double *dq, const double *dt, int k, int exclude_self, '
             'int64_t parts, double *out_d2, int64_t *out_idx, int *flag')
#: name -> SourceModule of the translation units that are text: a device
#: header of csrc/device and the wrappers that name its kernels
TEXT_UNITS = {'knn': SourceModule(source='#include "knn.h"\n\n' + _wrappers(
    ('knn_topk_f32', 'knn::topk_stage<float>', 'const float *K, ' + _KNN_TOPK),
    ('knn_topk_f64', 'knn::topk_stage<double>',
     'const double *K, ' + _KNN_TOPK),
    ('knn_merge', 'knn::merge_stage',
     'const double *ws_d2, const int64_t *ws_idx, int64_t b, int64_t parts, '
     'int k, double *out_d2, int64_t *out_idx'),
    ('knn_average', 'knn::average_stage',
     'const double *d2, const int64_t *idx, int64_t b, int k, '
     'const double *T, int64_t n, int64_t m, int mode, double *out'),
    ('knn_lrd', 'knn::lrd_stage',
     'const double *d2, const int64_t *idx, int64_t b, int k, '
     'const double *kdist, int64_t n, double *lrd'),
    ('knn_ratio', 'knn::ratio_stage',
     'const int64_t *idx, int64_t b, int k, const double *lrd_train, '
     'int64_t n, const double *lrd, double *lof'),
))}


def _text(relative):
    with open(os.path.join(_PACKAGE, relative)) as f:
        return f.read()


#: the translation units that are the text of one file of the package which
#: is no ``.hip`` file, relative to the package
FILE_UNIT_SOURCES = {'tsne': 'model/manifold/tsne.h'}
#: name -> SourceModule of that text: an edit of the file changes the key of
#: its own unit and of no other
FILE_UNITS = {name: SourceModule(source=_text(p))
              for name, p in FILE_UNIT_SOURCES.items()}

#: the same for the models that came after those lists were closed: a new
#: unit joins this one
MODEL_UNIT_SOURCES = {'geodesic': 'model/manifold/geodesic.h',
                      'mst': 'model/clustering/mst.h'}
MODEL_UNITS = {name: SourceModule(source=_text(p))
               for name, p in MODEL_UNIT_SOURCES.items()}

#: planes / candidates per register chunk (the template parameter KC of the
#: kernels that keep a chunk of accumulators in registers)
CHUNKS = (1, 2, 4, 8, 16)


def chunk(n):
    """The chunk size for `n` planes: the smallest of CHUNKS that holds them,
    the largest when none does."""
    return next(k for k in CHUNKS if k >= min(max(n, 1), CHUNKS[-1]))


def suffix(dtype):
    """'f32' / 'f64', as the kernels' names spell a torch dtype."""
    import torch
    if dtype == torch.float32:
        return 'f32'
    if dtype == torch.float64:
        return 'f64'
    raise TypeError(f'float32 or float64 expected, got {dtype}')


def current_stream(device):
    """Raw handle of torch's current stream on `device` (None: the null
    stream).  Launches go there to be ordered against the torch operations
    around them -- and torch's caching allocator then hands a workspace freed
    after a launch out again only behind that launch."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream or None
