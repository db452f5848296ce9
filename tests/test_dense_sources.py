"""The fused dense kernels' loader (graphdot_amd.hip.source_module) without a
GPU: every source of its list compiles for gfx950 with every kernel it
defines, no .hip file of the package is missing from the list, and the shared
chunk size is what each host module used to spell out for itself."""
import glob
import os

import pytest

from graphdot_amd.hip import jit
from graphdot_amd.hip.source_module import (
    CHUNKS, STATIC, STATIC_SOURCES, chunk)

PACKAGE = os.path.dirname(os.path.dirname(os.path.abspath(jit.__file__)))
#: templates: compiled per kernel / per formula, not as they lie
TEMPLATES = {'kernel/marginalized/template.hip',
             'kernel/kernel_over_metric.hip'}


@pytest.mark.parametrize('name', list(STATIC))
def test_static_source_compiles_for_gfx950(name):
    module = STATIC[name]
    path = module.precompile()
    assert os.path.getsize(path) > 0
    names = jit.entry_points(module.source)
    assert names, f'{name}: no kernel found in the source'
    image = jit.load_image(path)
    for kernel in names:
        assert kernel.encode() in image, f'{name}: {kernel} not in code object'


def test_every_hip_file_is_listed():
    found = {os.path.relpath(p, PACKAGE).replace(os.sep, '/')
             for p in glob.glob(os.path.join(PACKAGE, '**', '*.hip'),
                                recursive=True)
             if not os.path.relpath(p, PACKAGE).startswith('_jit_cache')}
    assert found - TEMPLATES == set(STATIC_SOURCES)
    assert len(STATIC) == len(STATIC_SOURCES)        # (distinct file names)
    for rel in STATIC_SOURCES:
        assert STATIC[os.path.basename(rel)].path == os.path.join(
            PACKAGE, *rel.split('/'))


def test_chunk_size_agrees_with_the_former_spellings():
    assert CHUNKS == (1, 2, 4, 8, 16)
    for n in range(41):
        # _lowrank.grid; then _outlier.grid, _posterior.grid, _field.grid
        assert chunk(n) == next(k for k in CHUNKS if k >= min(n, CHUNKS[-1]))
        assert chunk(n) == next(k for k in CHUNKS
                                if k >= min(max(n, 1), CHUNKS[-1]))
        assert chunk(n) >= min(n, 16) and (chunk(n) < 2 * n or n == 0)

