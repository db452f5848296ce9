"""The slot set-up of the double quotient kernels reads one 16-byte record per
half-term (mgk_oc.h RECS) where it read the nonzero, its
edge class and two scales: in the instruction stream of the (12,3) and the
(16,3,1) kernel, double, tables on, every half-term of a lane -- 7 of the
4 x 3 grid plus two per slot of the running walk -- costs the `slots` phase at
least one LDS instruction less than the 69 and 87 it had before, without
scratch and inside the register allocation of the occupancy target.

The bounds follow from that count, not from a measurement.  Host only:
compiles two kernels to assembly."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', 'scripts'))
import isa_phases                                              # noqa: E402

#: layout -> (LDS instructions of `slots` before, half-terms per lane,
#: registers of the occupancy target: 512 / 4 waves, 512 / 3 waves)
CASES = {(12, 3): (69, 7 + 2 * 3, 128), (16, 3, 1): (87, 7 + 2 * 4, 168)}


@pytest.fixture(scope='module', params=list(CASES),
                ids=lambda L: 'x'.join(map(str, L)))
def kernel(request):
    L = request.param
    isa = isa_phases.marked_isa(['1', '1', '1', '--f64', '--oc=4', '--tab',
                                 '--quot', '--layout=' + 'x'.join(map(str, L))])
    return L, isa


def test_every_half_term_saves_an_lds_read(kernel):
    L, isa = kernel
    before, half_terms, _ = CASES[L]
    slots = isa_phases.phase_counts(isa)['slots']
    print(L, dict(slots))
    assert slots['lds'] <= before - half_terms, dict(slots)
    # the records come as whole 16-byte reads
    body = isa.split('GDMARK slots')[1].split('GDMARK rows')[0]
    assert body.count('ds_read_b128') >= half_terms


def test_no_scratch_and_registers_of_the_occupancy_target(kernel):
    L, isa = kernel
    r = isa_phases.resources(isa)
    print(L, r)
    assert r['scratch'] == 0
    assert r['vgpr'] <= CASES[L][2]
