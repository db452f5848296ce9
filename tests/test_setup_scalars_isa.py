"""Pair-independent work is out of the set-up of the one-wave quotient value
kernels (mgk_oc.h QSET / EVSC / LANE_TABS, DESIGN.md section 4a "set-up
scalars"): in the instruction streams of the (12,3) and the (16,3,1) kernel,
double, tables on,

  * no double reciprocal in front of the `stage` mark (1 / (1 - q)^2 and
    q^2 / q0^2 come from behind the tables),
  * at most 12 `v_writelane_b32` in the whole kernel (the parent moved the 40
    integers of the rectangle tables into their lanes one by one),
  * no `global_load_dword` in the epilogue beyond those the parent has outside
    its reads of `starts` and `order` (which are scalar loads next to the
    headers now),
  * and the vector instructions of prologue + stage + rectangles + rowmap
    together at least 60 below the parent's.

The parent's figures are constants below, taken with scripts/isa_phases.py at
commit dc85a95.  (The scheduler moves instructions across the marks: the
parent's four phases read 32 / 75 / 4 / 52 and 34 / 75 / 4 / 85 by this counter,
the sums 163 and 198; only the sums are compared.)

At the commit that adds this file the sums are 103 and 138, 60 below the
parent's in both kernels: 17 / 15 / 19 / 52 and 19 / 15 / 19 / 85.  The bound of
60 follows from the static counts of what the change removes (the two
divisions 21, the lane writes and their moves about 35, the staging guards
about 20), not from a timing.

Host only: compiles two kernels to assembly, about half a minute."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', 'scripts'))
import isa_phases                                              # noqa: E402

SETUP = ('prologue', 'stage', 'rectangles', 'rowmap')
#: the parent's static counts (scripts/isa_phases.py, commit dc85a95)
PARENT = {
    (12, 3): {'setup_valu': 32 + 75 + 4 + 52, 'writelane': 40,
              'epilogue_load_dword': 4, 'epilogue_starts_order_reads': 4},
    (16, 3, 1): {'setup_valu': 34 + 75 + 4 + 85, 'writelane': 40,
                 'epilogue_load_dword': 4, 'epilogue_starts_order_reads': 4},
}


@pytest.fixture(scope='module', params=[(12, 3), (16, 3, 1)],
                ids=lambda L: 'x'.join(map(str, L)))
def kernel(request):
    L = request.param
    isa = isa_phases.marked_isa(['1', '1', '1', '--f64', '--oc=4', '--tab',
                                 '--quot', '--layout=' + 'x'.join(map(str, L))])
    return L, isa


def _ops(isa, first=None, last=None):
    """Mnemonics between the marks `first` and `last` (None: the ends)."""
    on, out = first is None, []
    for line in isa.split('\n'):
        m = re.search(r'GDMARK (\w+)', line)
        if m:
            if m.group(1) == first:
                on = True
            elif m.group(1) == last:
                break
            continue
        m = re.match(r'\s+([a-z_0-9]+)\s', line)
        if on and m and not line.lstrip().startswith(('.', ';')):
            out.append(m.group(1))
    return out


def test_no_division_in_front_of_the_staging(kernel):
    L, isa = kernel
    assert 'v_rcp_f64_e32' not in _ops(isa, None, 'stage')
    assert not [op for op in _ops(isa, None, 'stage') if op.startswith('v_rcp_f64')]


def test_rectangle_tables_without_lane_writes(kernel):
    L, isa = kernel
    n = sum(op.startswith('v_writelane_b32') for op in _ops(isa))
    print(L, 'v_writelane_b32', n, 'parent', PARENT[L]['writelane'])
    assert n <= 12


def test_epilogue_loads_no_output_address(kernel):
    L, isa = kernel
    n = sum(op == 'global_load_dword' for op in _ops(isa, 'epilogue'))
    p = PARENT[L]
    print(L, 'global_load_dword in epilogue', n, 'parent',
          p['epilogue_load_dword'])
    assert n <= p['epilogue_load_dword'] - p['epilogue_starts_order_reads']


def test_setup_vector_instructions(kernel):
    L, isa = kernel
    counts = isa_phases.phase_counts(isa)
    assert list(counts)[:4] == list(SETUP)
    now = sum(counts[ph]['valu'] for ph in SETUP)
    print(L, {ph: counts[ph]['valu'] for ph in SETUP}, 'sum', now, 'parent',
          PARENT[L]['setup_valu'])
    assert now <= PARENT[L]['setup_valu'] - 60
