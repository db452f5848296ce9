#!/usr/bin/env python
"""Record the drop-in seam: what the REFERENCE's MarginalizedGraphKernel hands
its backend (writes dropin_seam.json in this directory).

Runs only where the reference checkout is (make_golden.REF); the test-suite
only reads the JSON (`tests/test_host_model.py::
test_reference_kernel_object_drives_the_hip_backend`).

A HIPBackend instance is handed to the *reference's* MarginalizedGraphKernel
(`graphdot/kernel/marginalized/_kernel.py:60-73`, `_backend_factory.py:7-9`)
together with the reference's own Graph / microkernel objects (the four case
families of its test oracle, the same graphs as mlgk_cases.json).  Its
`__call__` (`_kernel.py:114-264`, backend call `:224-242`) and `diag`
(`:266-408`, backend call `:363-381`) construct the arguments -- allocators
`backend.array / zeros / empty`, job list, `starts`, output buffers, traits --
for value, value + gradient, nodal, nodal + gradient, an X x Y block, lmin and
the three `diag` modes.  `HIPBackend.__call__` is intercepted: the arguments
are recorded together with the kernel-argument values packed from the
reference's hyperparameter objects; no launch."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402
from make_golden import REF, install_shims, jsonable, load_test_oracle  # noqa: E402,E501

# the calls of a case, in order (the labels of dropin_seam.json)
CALLS = ('K', 'K,dK', 'nodal', 'nodal,dK', 'XxY', 'lmin=1', 'diag',
         'diag,dK', 'diag nodal', 'diag block')


def struct_values(buf):
    """The numbers of a (nested) structured scalar, in field order."""
    if buf is None:
        return []
    if buf.dtype.names is None:
        return [float(v) for v in np.ravel(buf)]
    return [v for name in buf.dtype.names for v in struct_values(buf[name])]


def packed_theta(backend, graphs, node_kernel, edge_kernel, p, traits):
    """Kernel-argument values of a call, as `HIPBackend.prepare` packs them
    (the edge kernel after the weighted wrapper)."""
    from graphdot_amd.kernel.marginalized._backend_hip import pack_theta
    ngrad = traits.eval_gradient is True and traits.nodal is True
    if traits.eval_gradient is True and traits.nodal == 'block':
        traits = traits._replace(eval_gradient=False)
    _, ek, _, _ = backend._graphs_and_kernels(graphs, node_kernel,
                                              edge_kernel, traits, None, ngrad)
    return {field: struct_values(pack_theta(obj, backend.real)[1])
            for field, obj in (('node_kernel', node_kernel),
                               ('edge_kernel', ek), ('p_start', p))}


def main():
    install_shims()
    sys.path.insert(0, REF)
    from graphdot.kernel.marginalized import MarginalizedGraphKernel
    from graphdot.kernel.marginalized._backend import Backend as RefBackend
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend

    seen = []

    # the reference's factory accepts instances of ITS Backend ABC
    class DropIn(HIPBackend, RefBackend):
        def __call__(self, graphs, node_kernel, edge_kernel, p, q, eps, ftol,
                     gtol, jobs, starts, gramian, gradient, nX, nY, nJ,
                     traits, timer):
            seen.append({
                'n_graphs': len(graphs), 'q': q, 'eps': eps, 'ftol': ftol,
                'gtol': gtol, 'jobs_i': jobs['i'], 'jobs_j': jobs['j'],
                'jobs_dtype': jobs.dtype.descr, 'starts': starts,
                'starts_dtype': starts.dtype.str,
                'gramian': [gramian.dtype.str, gramian.ndim, gramian.size],
                'gradient': None if gradient is None else
                [gradient.dtype.str, gradient.ndim, gradient.size],
                'nX': nX, 'nY': nY, 'nJ': nJ, 'traits': traits._asdict(),
                'theta': packed_theta(self, graphs, node_kernel, edge_kernel,
                                      p, traits)})
            gramian[:] = 1.0                     # (no launch: placeholders)
            if gradient is not None:
                gradient[:] = 0.0

    ns = load_test_oracle()
    backend = DropIn()
    out = {}
    for name, case in ns['case_dict'].items():
        k = MarginalizedGraphKernel(case['knode'], case['kedge'], q=0.05,
                                    backend=backend)
        assert k.backend is backend
        G = case['graphs']
        before = len(seen)
        k(G)
        k(G, eval_gradient=True)
        k(G, nodal=True)
        k(G, nodal=True, eval_gradient=True)
        k(G[:1], G[1:])
        k(G, lmin=1)
        k.diag(G)
        k.diag(G, eval_gradient=True)
        k.diag(G, nodal=True)
        k.diag(G, nodal='block')
        calls = seen[before:]
        assert len(calls) == len(CALLS)
        out[name] = {'q': 0.05, 'calls': [dict(c, call=label)
                                          for label, c in zip(CALLS, calls)]}
        print(name, '->', len(calls), 'backend calls')
    with open(os.path.join(HERE, 'dropin_seam.json'), 'w') as f:
        json.dump(jsonable(out), f)


if __name__ == '__main__':
    main()
