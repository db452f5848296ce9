"""The slot set-up of the quotient value kernels keeps its table loads in
flight (mgk_oc.h GPRE): in the instruction stream of the
(12,3) and the (16,3,1) kernel, double, tables on, the `slots` phase has at most
R + 1 exposed loads by the counter of scripts/isa_phases.py -- loads whose next
`s_waitcnt vmcnt` is a full wait with no other load issued in between -- and
the kernel needs no scratch at its occupancy target.

By this counter the `slots` phase had 12 and 16 exposed loads before the grid's
table values were loaded ahead of the slot loop (one per cell of the grid; 14
and 19 `global_load_dwordx2` of the whole kernel stood within three lines of a
`vmcnt(0)`); it has 0 and 0 now, at 120 and 154 registers.

Host only: compiles two kernels to assembly, about half a minute.  Looks at
the order of loads and waits and at the compiler's resource report, nothing
else in the assembly."""
import os
import sys

import numpy as np
import pytest

from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend, OCStatic

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', 'scripts'))
import isa_phases                                              # noqa: E402


@pytest.fixture(scope='module', params=[(12, 3), (16, 3, 1)],
                ids=lambda L: 'x'.join(map(str, L)))
def kernel(request):
    L = request.param
    isa = isa_phases.marked_isa(['1', '1', '1', '--f64', '--oc=4', '--tab',
                                 '--quot', '--layout=' + 'x'.join(map(str, L))])
    return L, isa


def test_slot_setup_has_its_table_loads_in_flight(kernel):
    L, isa = kernel
    counts = isa_phases.phase_counts(isa)
    assert list(counts)[:2] == ['prologue', 'stage'] and 'slots' in counts
    slots = counts['slots']
    print(L, dict(slots))
    # (the grid's cells and the running-walk slots all read the table)
    assert slots['vmem'] >= sum(L)
    assert slots['exposed'] <= len(L) + 1, dict(slots)


def test_no_scratch_at_the_occupancy_target(kernel):
    L, isa = kernel
    r = isa_phases.resources(isa)
    target = HIPBackend(real=np.float64)._oc_waves(OCStatic(*L), 1)
    print(L, r, 'target', target)
    assert r['scratch'] == 0
    assert r['occupancy'] >= target
