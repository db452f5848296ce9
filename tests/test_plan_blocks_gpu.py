"""What `HIPBackend.prepare` hands to the launches -- kernel names, launch
geometry and the argument blocks, byte by byte -- against
tests/golden/plan_blocks.json, which `python tests/test_plan_blocks_gpu.py
OUT.json` recorded before the host plan of a call became one record
("The host plan of a call").  Only `prepare`,
`maximin_distance`, `m3_distance` and `last_plan` are used.

Device addresses differ from run to run: every pointer field of an argument
block is recorded as (buffer it points into, offset), 0 stays 0.  The grid,
the parts and the argument block of the launches whose geometry depends on
the chip (STREAM, GENERAL) are compared only on a device with the
`compute_units` of the golden."""
import json
import os
import sys
import zlib

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'plan_blocks.json')


def _buffers(backend, plan):
    """(name, DeviceBuffer) of everything an argument block may point into."""
    out = [('arena', plan.layout.arena_buf)]
    out += [(k, b) for k, b in sorted(plan.buffers.items()) if b is not None]
    if getattr(plan, 'sync', None) is not None:
        out.append(('sync', plan.sync[0]))
    out += [('pool:' + k, b) for k, b in sorted(backend._pool.items())]
    return out


def _member_bytes(dtype):
    """Which bytes of a record belong to a member (the others are padding,
    which numpy leaves as it finds it when it copies a record)."""
    mask = np.zeros(dtype.itemsize, dtype=bool)
    if dtype.subdtype is not None:
        item = dtype.subdtype[0]
        mask[:] = np.tile(_member_bytes(item), dtype.itemsize // item.itemsize)
    elif dtype.names is None:
        mask[:] = True
    else:
        for name in dtype.names:
            member, offset = dtype.fields[name][:2]
            mask[offset:offset + member.itemsize] = _member_bytes(member)
    return mask


def _block(backend, plan, args, kernels):
    """Argument bytes with the padding and the pointer fields zeroed (hex),
    and where every pointer went.  `kernels`: (node kernel, edge kernel, p)
    as `prepare` got them."""
    pd = plan.params_dtype
    whole = pd
    if len(args) != pd.itemsize:       # the finite-difference block around it
        from graphdot_amd.microkernel import TensorProduct, Product
        kn, ke, p = kernels            # (weighted graphs: `prepare` wraps ke)
        whole = [dt for dt in (
            backend._params_fd_dtype(kn, ek, p)
            for ek in (ke, TensorProduct(weight=Product(), label=ke)))
            if dt.itemsize == len(args) and dt['base'] == pd][0]
    raw = np.frombuffer(bytearray(args), dtype=np.uint8)
    raw[~_member_bytes(whole)] = 0
    a = raw[:pd.itemsize].view(pd)                # (writes through to raw)
    bufs = _buffers(backend, plan)
    pointers = {}
    for name in pd.names:
        if pd[name] != np.dtype(np.uintp):
            continue
        p = int(a[name][0])
        if p:
            for bname, b in bufs:
                if b.ptr <= p < b.ptr + max(b.nbytes, 1):
                    pointers[name] = [bname, p - b.ptr]
                    break
            else:
                pointers[name] = ['?', 0]
        a[name] = 0
    return dict(pointers=pointers, flags=int(a['flags'][0]),
                n_bytes=len(raw), crc=zlib.crc32(raw.tobytes()),
                bytes=raw.tobytes().hex())


def _record(backend, plan, kernels):
    from graphdot_amd.kernel.marginalized._backend_hip import F_DENSE
    launches = []
    for L in plan.pre_launches + plan.launches:
        names = [n for n, h in L['module']._functions.items()
                 if h == L['fn']]
        rec = dict(kernel=names[0], variant=str(L['variant']),
                   grid=int(L['grid']), threads=int(L['threads']),
                   dynamic_lds=int(L['dynamic_lds']),
                   cooperative=bool(L.get('cooperative', False)),
                   parts=int(L.get('parts', 1)))
        rec.update(_block(backend, plan, L['args'], kernels))
        launches.append(rec)
    return dict(stream_hint=plan.stream_hint, n_out=int(plan.n_out),
                n_grad=int(plan.n_grad), quotient=bool(plan.quotient),
                flags=launches[-1]['flags'] & ~F_DENSE,
                n_pre=len(plan.pre_launches), launches=launches)


class _Spy:
    """Records every plan `backend.prepare` returns (and the arguments of
    the call)."""

    def __init__(self, backend):
        self.backend, self.plans, self.calls = backend, [], []
        inner = backend.prepare

        def prepare(*args, **kwargs):
            plan = inner(*args, **kwargs)
            self.calls.append((args, kwargs))
            self.plans.append(_record(backend, plan, args[1:4]))
            return plan
        backend.prepare = prepare

    def done(self):
        """Take the recorder off the backend again (the default backend of a
        model is shared); returns the recorded plans."""
        del self.backend.prepare
        return self.plans


def _mgk_case(graphs, kernels, real, packed=False, backend_args=(), **call):
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    kn, ke, q = kernels
    be = HIPBackend(real=real, **dict(backend_args))
    spy = _Spy(be)
    MarginalizedGraphKernel(kn, ke, q=q, backend=be)(graphs, **call)
    if packed:
        args, kwargs = spy.calls[-1]
        del spy.plans[:]
        be.prepare(*args, **dict(kwargs, packed=True))
    return spy.done()


def _maximin_case():
    from _fixtures import load, graphs_from, kernel_from_repr
    from graphdot_amd.metric.maximin import MaxiMin
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    fx = load('maximin.json')
    be = HIPBackend(real=np.float64)
    spy = _Spy(be)
    mm = MaxiMin(kernel_from_repr(fx['knode']), kernel_from_repr(fx['kedge']),
                 q=fx['q'], eps=fx['eps'], backend=be, reference_compat=True)
    mm(graphs_from(fx['graphs']), eval_gradient=True)
    assert be.last_plan.maximin and be.last_plan.ngrad
    return spy.done()


def _m3_case():
    from test_m3 import atoms
    from graphdot_amd.experimental.metric import M3
    m = M3()
    spy = _Spy(m.kernel.backend)
    m.pairwise([atoms(n) for n in ('CH4', 'H2O', 'CH5NOS', 'C2H6O')])
    assert m.kernel.backend.last_plan.maximin
    return spy.done()


def record():
    import cases
    c3 = cases.config3_kernels()
    g8, g24 = cases.config3_graphs(8), cases.config3_graphs(24)
    tang = cases.tang2019_kernels()
    f32, f64 = np.float32, np.float64
    out = {}
    out['config3_8/f64/value'] = _mgk_case(g8, c3, f64)
    out['config3_8/f32/nodal'] = _mgk_case(g8, c3, f32, nodal=True)
    out['config3_8/f64/gradient'] = _mgk_case(g8, c3, f64, eval_gradient=True)
    out['config3_8/f64/packed'] = _mgk_case(g8, c3, f64, packed=True)
    no_merge = (('min_launch', 0),)
    out['config3_24/f64/lmin1'] = _mgk_case(g24, c3, f64, lmin=1,
                                             backend_args=no_merge)
    out['config3_24/f64/value'] = _mgk_case(g24, c3, f64,
                                             backend_args=no_merge)
    out['tang2019_6/f32/value'] = _mgk_case(cases.tang2019_graphs(6), tang,
                                            f32)
    out['large_2/f64/value'] = _mgk_case(
        cases.protein_like_graphs(2, nmin=150, nmax=420, seed=41), tang, f64)
    out['maximin/f64/gradient_refcompat'] = _maximin_case()
    out['m3/f64'] = _m3_case()
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    return dict(compute_units=int(HIPBackend().props.compute_units),
                cases=out)


def _comparable(doc, same_chip):
    """The part of a recording that holds on every device: the geometry of
    STREAM and GENERAL launches follows the number of compute units."""
    doc = json.loads(json.dumps(doc))
    if same_chip:
        return doc['cases']
    for plans in doc['cases'].values():
        for plan in plans:
            for L in plan['launches']:
                if 'stream' in L['kernel'] or 'general' in L['kernel']:
                    for key in ('grid', 'parts', 'cooperative', 'pointers',
                                'crc', 'bytes'):
                        del L[key]
    return doc['cases']


@pytest.mark.gpu
def test_prepare_hands_the_launches_what_it_did():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = record()
    # the arms the cases are there for (decided when the golden was made)
    cases_ = want['cases']
    assert cases_['config3_8/f64/value'][0]['quotient']
    assert cases_['config3_8/f64/value'][0]['n_pre'] == 1
    for key in ('config3_24/f64/lmin1', 'config3_24/f64/value'):
        assert len(cases_[key][0]['launches']) - cases_[key][0]['n_pre'] > 2
        assert cases_[key][0]['stream_hint'] == 2
    assert not cases_['config3_24/f64/lmin1'][0]['quotient']
    assert any(L['cooperative']
               for L in cases_['large_2/f64/value'][0]['launches'])
    assert len(cases_['maximin/f64/gradient_refcompat']) == 2
    same_chip = got['compute_units'] == want['compute_units']
    got, want = _comparable(got, same_chip), _comparable(want, same_chip)
    assert sorted(got) == sorted(want)
    for key in want:
        assert len(got[key]) == len(want[key]), key
        for a, b in zip(got[key], want[key]):
            la, lb = a.pop('launches'), b.pop('launches')
            assert a == b, key
            assert len(la) == len(lb), key
            for x, y in zip(la, lb):
                assert x == y, (key, y['kernel'])


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    with open(sys.argv[1], 'w') as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write('\n')
