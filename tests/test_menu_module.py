"""The solver menu as a module of its own, `kernel/marginalized/_menu.py`, and
each LDS layout stated once, without a device: the
figures of tests/golden/lds_bytes.json -- recorded by
tests/golden/make_golden_lds_bytes.py at the commit before the move -- number
for number, the two layout functions against them, a `SolverMenu` built with
no backend against the backend, and what the module imports."""
import ast
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from graphdot_amd.kernel.marginalized import _backend_hip, _menu
from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
from graphdot_amd.kernel.marginalized._menu import (OCVariant, SolverMenu,
                                                    Variant)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
MARGINALIZED = os.path.join(ROOT, 'graphdot_amd', 'kernel', 'marginalized')

#: what the issue moved, by name: records, constants, sentinels
MOVED_NAMES = (
    'Variant', 'OCVariant', 'OCStatic', 'VARIANTS', 'OC_QUOTIENT_LAYOUTS',
    'OC_STATIC_VARIANTS', 'OC_FLY_VARIANTS', 'OC_VARIANTS', 'FLY_MIN_DEGREE',
    'GENERAL', 'TABLES', 'MFMA', 'STREAM', '_LARGE_PAIR_SOLVERS',
    'GENERAL_THREADS', 'STREAM_THREADS', 'MFMA_MAX_NODES', 'STREAM_ROWS',
    'STREAM_CAP', 'STREAM_MAX_PARTS', 'STREAM_LDS_BUDGET', 'LDS_LIMIT',
    'TABLE_LDS_LIMIT', 'GLOBAL_TABLE_LIMIT', 'STREAM_PART_EFFICIENCY',
    'stream_parts', 'ClassPairs', 'Partition', 'CallShape',
    'NotOwnerComputes')
#: ... and the methods `HIPBackend` now inherits
MOVED_METHODS = (
    'waves_per_eu', '_oc_waves', '_waves_without_lds_diagonals',
    '_static_enabled', 'grid_of', 'swaps_roles', '_grid_takes',
    '_dense_bytes', 'stream_virtual_rows', 'stream_lds_bytes',
    'lds_slot_bytes', 'diagonals_in_lds', 'lds_bytes', 'slots_needed',
    'oc_trips', 'oc_slots_needed', 'classify', '_classify_classes',
    'TRIP_BATCHES', '_degree_hists', '_trip_table', '_classify_pairs',
    '_partition', '_launch_lds', '_fit_launches_into_lds', '_WAVES_F32_VALUE',
    '_WAVES_F32_GRADIENT', '_WAVES_F64_VALUE', '_WAVES_F64_GRADIENT',
    '_WAVES_F32_VALUE_W4', '_WAVES_F64_VALUE_W4', '_OC_WAVES', '_STATIC_OFF',
    '_FLY_WAVES')


@pytest.fixture(scope='module')
def script():
    spec = importlib.util.spec_from_file_location(
        'make_golden_lds_bytes',
        os.path.join(GOLDEN, 'make_golden_lds_bytes.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope='module')
def record():
    with open(os.path.join(GOLDEN, 'lds_bytes.json')) as f:
        return json.load(f)


def _variant(fields):
    if len(fields) == 3:
        return Variant(*fields)
    return OCVariant(*fields[:4], None if fields[4] is None
                     else tuple(fields[4]))


def test_lds_bytes_equals_the_record(script, record):
    """Every recorded figure, one call per number and one call per grid."""
    assert [tuple(p) for p in record['points']] == list(script.POINTS)
    assert {a for a, _ in script.POINTS} == set(script.VECTORS)
    assert {b for _, b in script.POINTS} == set(script.IMAGES)
    nt, gb = map(np.array, zip(*script.POINTS))
    seen = set()
    for real in script.REALS:
        menu = SolverMenu(real=real)
        for key, v, C, nodal, tab in script.grid_cases(menu):
            want = record['grids'][record['lds_bytes'][key]]
            got = [int(menu.lds_bytes(v, C, a, b, tab, nodal))
                   for a, b in script.POINTS]
            assert got == want, key
            assert menu.lds_bytes(v, C, nt, gb, tab, nodal).tolist() == want
            seen.add(key)
    assert seen == set(record['lds_bytes'])
    # both families, both arithmetics, the tables
    assert len(seen) == 2 * 4 * (len(_menu.OC_VARIANTS)
                                 + 2 * len(_menu.VARIANTS))


def test_lds_bytes_is_static_plus_dynamic_of_the_layout(script, record):
    nt, gb = map(np.array, zip(*script.POINTS))
    for real in script.REALS:
        menu = SolverMenu(real=real)
        for key, v, C, nodal, tab in script.grid_cases(menu):
            if isinstance(v, OCVariant):
                static, dynamic = menu._oc_lds(v, C, nodal, menu._pcap(nt), gb)
            else:
                static, dynamic = menu._two_stage_lds(v, C, menu._ucap(nt),
                                                      gb, tab)
            assert np.ndim(static) == 0 and static > 0
            assert (static + dynamic).tolist() == \
                record['grids'][record['lds_bytes'][key]], key
    # the caps, at the multiples they round to
    assert SolverMenu._pcap(np.array([0, 2, 3, 4, 6, 7])).tolist() == \
        [4, 4, 4, 8, 8, 8]
    assert SolverMenu._ucap(np.array([0, 1, 64, 65])).tolist() == \
        [64, 128, 128, 192]


def test_dynamic_lds_of_the_recorded_launches(script, record):
    """`_partition` gives the recorded launches, and the dynamic LDS of every
    slot and two-stage launch is the layout's `dynamic` at the launch's own
    caps (the image cap rounded to 16 bytes)."""
    seen = set()
    for key, real, options, graphs, kernels, kw in script.small_calls():
        want = record['launches'][key]
        b = HIPBackend(real=real, **options)
        _, plan = script.host_plan_of(b, graphs, kernels, kw)
        s = plan.shape
        assert dict(C=s.C, nodal=bool(s.nodal), tab_bytes=int(s.tab_bytes),
                    launches=[script.launch_record(L)
                              for L in plan.part[3]]) == want, key
        for L in want['launches']:
            v = _variant(L['variant'])
            assert L['gcap'] % 16 == 0
            if v.W <= 0 or (isinstance(v, OCVariant) and v.S == 0):
                continue       # sentinels; the dense arrays' own addition
            if isinstance(v, OCVariant):
                dyn = b._oc_lds(v, want['C'], want['nodal'], L['ucap'],
                                L['gcap'])[1]
            else:
                dyn = b._two_stage_lds(v, want['C'], L['ucap'], L['gcap'],
                                       want['tab_bytes'])[1]
            assert int(dyn) == L['dynamic_lds'], (key, v)
            seen.add((isinstance(v, OCVariant), bool(v[4:] and v.L)))
        assert all(type(L['dynamic_lds']) is int for L in plan.part[3])
    assert sorted(record['launches']) == sorted(
        c[0] for c in script.small_calls())
    # two-stage, dynamic and static owner-computes launches were all met
    assert seen == {(False, False), (True, False), (True, True)}


def test_a_menu_without_a_backend_partitions_like_the_backend(script, record):
    made = 0
    for key, real, options, graphs, kernels, kw in script.small_calls():
        b = HIPBackend(real=real, native=False, **options)
        jobs, plan = script.host_plan_of(b, graphs, kernels, kw)
        menu = SolverMenu(real, native=False, min_launch=b.min_launch,
                          **options)
        assert not isinstance(menu, HIPBackend)
        got = menu._partition(plan.dgraphs, jobs, plan.shape)
        want = plan.part
        assert np.array_equal(got[0], want[0]), key
        assert got[1] == want[1], key
        assert got[2].dtype == want[2].dtype
        assert np.array_equal(got[2], want[2]), key
        assert got[3] == want[3], key
        assert got.merge_map == want.merge_map, key
        assert got.jobs_sorted is None and want.jobs_sorted is None
        made += len(got[3])
    assert made == sum(len(c['launches'])
                       for c in record['launches'].values())


def test_the_menu_imports_no_device_and_no_code_generator():
    heavy = ['torch', 'graphdot_amd.hip.runtime', 'graphdot_amd.hip.jit']
    out = subprocess.run(
        [sys.executable, '-c',
         'import sys\n'
         'import graphdot_amd.kernel.marginalized._menu as m\n'
         'import numpy\n'
         'm.SolverMenu(real=numpy.float64, native=False)\n'
         f'print([k for k in {heavy!r} if k in sys.modules])'],
        cwd=ROOT, capture_output=True, text=True,
        env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == '[]'
    # module level: numpy and ._devicegraph (and the standard library)
    with open(os.path.join(MARGINALIZED, '_menu.py')) as f:
        tree = ast.parse(f.read())
    modules = set()
    for node in tree.body:
        if isinstance(node, ast.Import):
            modules |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            modules.add('.' * node.level + (node.module or ''))
    assert modules == {'collections', 'typing', 'numpy', '._devicegraph'}


def test_the_moved_names_are_the_same_objects():
    for name in MOVED_NAMES:
        assert getattr(_backend_hip, name) is getattr(_menu, name), name
    assert HIPBackend.__mro__[1] is SolverMenu
    # inherited, not forwarded
    for name in MOVED_METHODS:
        assert name in vars(SolverMenu), name
        assert name not in vars(HIPBackend), name
    for real in (np.float32, np.float64):
        b = HIPBackend(real=real)
        assert b.f64 == (real is np.float64)
        assert b.rsize == np.dtype(real).itemsize
        assert not {'f64', 'rsize'} & set(vars(b))      # computed, not cached
        assert b.variants == SolverMenu(real=real).variants
    with pytest.raises(TypeError, match='unknown HIPBackend options'):
        HIPBackend(no_such_option=1)


def test_each_rule_is_spelled_once():
    """The counts of DESIGN.md section 37 that source text can show."""
    text = ''
    for name in ('_menu.py', '_backend_hip.py'):
        with open(os.path.join(MARGINALIZED, name)) as f:
            text += f.read()

    def count(pattern):
        return len(re.findall(pattern, text))
    # region sums of the owner-computes and of the two-stage layout
    assert count(r'\* C \* \w+ \+ 4 \* NR \+ 2 \*') == 1
    assert count(r'ucap \* C \* \w+ \+ 2 \*') == 1
    assert count(r'NR_y = 0 if') == 1                       # the [Y] rule
    assert count(r'// 4\) \* 4') == 1                       # pcap
    assert count(r'// 64\) \* 64 \+ 64') == 1               # ucap
    assert count(r'np\.dtype\(self\.real\) [!=]= np\.float(32|64)') <= 1
    assert count(r'np\.dtype\(self\.real\)\.itemsize') <= 1
    assert count(r"'n_orig', None\) is not None") == 0      # quotient_images
