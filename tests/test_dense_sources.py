"""The fused dense kernels' loader (graphdot_amd.hip.source_module) without a
GPU: every source of its list compiles for gfx950 with every kernel it
defines, no .hip file of the package is missing from the list, and the shared
chunk size is what each host module used to spell out for itself."""
import glob
import json
import os
import re

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


def test_recorded_instruction_streams_equal_the_parents():
    """profiles/dense_isa.json (this tree) and profiles/dense_isa_parent.json
    (the tree before the host and device helpers moved; DESIGN.md section
    34), both written by scripts/isa_fingerprint.py --dense: the same kernels
    with the same hashes and resource figures, of every listed file.  Nothing
    is compiled here."""
    root = os.path.dirname(PACKAGE)
    with open(os.path.join(root, 'profiles', 'dense_isa.json')) as f:
        now = json.load(f)
    with open(os.path.join(root, 'profiles', 'dense_isa_parent.json')) as f:
        parent = json.load(f)
    assert len(now) == 190 and sorted(now) == sorted(parent)
    for symbol, figures in now.items():
        assert figures == parent[symbol], symbol
        assert re.fullmatch(r'[0-9a-f]{16} \d+ lines( \w+=\d+){4}', figures), \
            (symbol, figures)
    files = {symbol.split(':')[0] for symbol in now}
    assert {os.path.basename(rel) for rel in STATIC_SOURCES} <= files
    assert len(STATIC_SOURCES) == 13


def _count(pattern, suffixes):
    hits = {}
    for d, _, names in os.walk(PACKAGE):
        if '_jit_cache' in d:
            continue
        for name in names:
            if name.endswith(suffixes):
                with open(os.path.join(d, name)) as f:
                    n = len(re.findall(pattern, f.read()))
                if n:
                    hits[os.path.relpath(os.path.join(d, name), PACKAGE)] = n
    return hits


def test_shared_device_helpers_are_there_once():
    header = os.path.join('csrc', 'device', 'dense_reduce.h')
    for pattern in (r'bool is_finite\(', r'void load_k\(',
                    r'#define SMO_PAIR_UPDATE\('):
        assert _count(pattern, ('.hip', '.h', '.py')) == {header: 1}, pattern


def test_no_host_module_reaches_into_another_model_package():
    """A host module of a model package imports private names from
    model/_*.py, hip/ and kernel/ alone."""
    model = os.path.join(PACKAGE, 'model')
    packages = {d for d in os.listdir(model)
                if os.path.isdir(os.path.join(model, d))}
    assert {'svm', 'clustering', 'decomposition', 'alignment', 'two_sample',
            'gaussian_process'} <= packages
    found = []
    for package in sorted(packages):
        for d, _, names in os.walk(os.path.join(model, package)):
            for name in names:
                if not name.endswith('.py'):
                    continue
                with open(os.path.join(d, name)) as f:
                    text = f.read()
                # from ..other._module import x; from ..other.module import _x;
                # from ..other import _module
                for other, module, what in re.findall(
                        r'from \.\.(\w+)(?:\.(\w+))? import (\([^)]*\)|[^\n]+)',
                        text):
                    names_ = [w.strip(' ()\n') for w in what.split(',')]
                    if other in packages and other != package and (
                            module.startswith('_')
                            or any(w.startswith('_') for w in names_)):
                        found.append((package, name, other, module, what))
    assert found == []
    for name in ('_check_K', '_f64', 'matrix_strides', 'plane_strides',
                 'triangle_grid', '_contract_planes'):
        assert _count(rf'(?m)^def {name}\(', ('.py',)) == {
            os.path.join('model', '_dense_host.py'): 1}, name


def test_chunk_size_agrees_with_the_former_spellings():
    assert CHUNKS == (1, 2, 4, 8, 16)
    for n in range(41):
        # _lowrank.grid; then _outlier.grid, _posterior.grid, _field.grid
        assert chunk(n) == next(k for k in CHUNKS if k >= min(n, CHUNKS[-1]))
        assert chunk(n) == next(k for k in CHUNKS
                                if k >= min(max(n, 1), CHUNKS[-1]))
        assert chunk(n) >= min(n, 16) and (chunk(n) < 2 * n or n == 0)

