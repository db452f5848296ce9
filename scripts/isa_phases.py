#!/usr/bin/env python3
"""Instruction counts per phase of one owner-computes solver: compiles the
variant with -DGD_MARKS (mgk_oc.h GD_MARK) through scripts/dump_isa.py and
counts VALU / SALU / LDS / VMEM instructions between the marks, in program
order of the ISA.

    python scripts/isa_phases.py W S R [C] [--f64] [--layout=16x4x4x1] [--tab=2] [--quot]

The last column, "exposed", counts the VMEM loads of a phase that wait alone:
the next `s_waitcnt vmcnt` after the load is a full wait, vmcnt(0), and no
other VMEM load is issued between the two -- the wave then sits out one whole
round trip to memory for that load.  A group of loads issued back to back and
drained by one vmcnt(0) counts once (its last load); a group waited for with
falling counts, vmcnt(3) (2) (1) (0), counts nothing.

`phase_counts(isa)` and `resources(isa)` serve tests/test_quotient_setup_isa.py.
"""
import collections
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ('valu', 'salu', 'lds', 'vmem', 'exposed')


def marked_isa(args):
    """ISA text of the variant `args` (dump_isa.py's) built with -DGD_MARKS."""
    env = dict(os.environ)
    env['GD_HIPCC_EXTRA'] = (env.get('GD_HIPCC_EXTRA', '') + ' -DGD_MARKS').strip()
    return subprocess.run([sys.executable, os.path.join(HERE, 'dump_isa.py')]
                          + list(args), env=env, capture_output=True, text=True,
                          check=True).stdout


def phase_counts(isa):
    """{phase: Counter of KINDS} in program order of the ISA text."""
    phase = 'prologue'
    counts = collections.OrderedDict()
    pending = None      # phase of the last VMEM load that no wait has followed
    for line in isa.split('\n'):
        m = re.search(r'GDMARK (\w+)', line)
        if m:
            phase = m.group(1)
            continue
        m = re.match(r'\s+([a-z_0-9]+)\s', line)
        if not m or line.lstrip().startswith(('.', ';')):
            continue
        op = m.group(1)
        vmem = op.startswith(('global_', 'buffer_', 'scratch_', 'flat_'))
        kind = ('valu' if op.startswith('v_') else
                'salu' if op.startswith('s_') else
                'lds' if op.startswith('ds_') else
                'vmem' if vmem else None)
        if kind is None:
            continue
        c = counts.setdefault(phase, collections.Counter())
        c[kind] += 1
        if vmem and '_load' in op:
            pending = phase
        elif op == 's_waitcnt':
            m = re.search(r'vmcnt\((\d+)\)', line)
            if m:
                if int(m.group(1)) == 0 and pending is not None:
                    counts[pending]['exposed'] += 1
                pending = None
    return counts


def resources(isa):
    """{'vgpr', 'scratch', 'occupancy'} of the compiler's resource report."""
    def field(name):
        return int(re.search(r';\s*%s:\s*(\d+)' % name, isa).group(1))
    return {'vgpr': field('NumVgprs'), 'scratch': field('ScratchSize'),
            'occupancy': field('Occupancy')}


def main():
    isa = marked_isa(sys.argv[1:])
    print(f'{"phase":12s} ' + ' '.join(f'{k:>7s}' for k in KINDS))
    for ph, c in phase_counts(isa).items():
        print(f'{ph:12s} ' + ' '.join(f'{c[k]:7d}' for k in KINDS))
    r = resources(isa)
    print(f'vgpr {r["vgpr"]}  scratch {r["scratch"]} bytes  '
          f'occupancy {r["occupancy"]} waves')


if __name__ == '__main__':
    main()
