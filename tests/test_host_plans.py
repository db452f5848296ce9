"""The host plan of a call ("The host plan of a call"), without a
device: the plans of a fixed list of small calls against
tests/golden/host_plans.json -- recorded by ``scripts/host_plan_digest.py
--small`` before `precompile`, `prepare` and the shard planner shared one
function -- and that the three do reach the same plan."""
import importlib.util
import json
import os

import numpy as np
import pytest

import cases
from graphdot_amd.hip import jit, runtime
from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
from graphdot_amd.kernel.marginalized._backend_hip import (
    HIPBackend, VARIANTS, _ids)
from graphdot_amd.kernel.marginalized._sharded import measured_shard_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
job_t = np.dtype([('i', np.uint32), ('j', np.uint32)])


def test_small_calls_plan_as_recorded():
    spec = importlib.util.spec_from_file_location(
        'host_plan_digest', os.path.join(ROOT, 'scripts',
                                         'host_plan_digest.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    got = json.loads(json.dumps(module.digest(small=True)))
    with open(os.path.join(ROOT, 'tests', 'golden', 'host_plans.json')) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    assert any(c['quotient'] for c in want.values())
    assert not all(c['quotient'] for c in want.values())


class _Done(Exception):
    pass


class HostOnly(HIPBackend):
    """`prepare` as far as its host plan, without a device: the arena is not
    uploaded, the layout is neither cached nor uploaded, and the call ends
    where the modules would be loaded.  Counts the partitions made."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.partitioned, self.host = [], None

    def _partition(self, dgraphs, jobs, shape, merge_map=None):
        self.partitioned.append(shape.quot)
        return super()._partition(dgraphs, jobs, shape, merge_map)

    def _arena(self, dgraphs, fields=(None, None)):
        return self._host_arena(dgraphs, fields), None, list(dgraphs)

    def _layout(self, jobs, starts, timer, dgraphs, fields, shape, merge_map,
                make):
        return make()

    def _modules_of(self, host, node_kernel, p, timer=None):
        self.host = host
        raise _Done

    def host_half_of_prepare(self, k, graphs, jobs, traits, **kwargs):
        del self.partitioned[:]
        n = len(graphs)
        with pytest.raises(_Done):
            self.prepare(graphs, k.node_kernel, k.edge_kernel, k.p, k.q,
                         k.eps, k.ftol, k.gtol, jobs,
                         np.arange(n + 1, dtype=np.uint32), n, n, 0, traits,
                         **kwargs)
        return self.host, list(self.partitioned)


def _keys(b, sources):
    return sorted(jit.cache_key(s, b.hipcc_extra) for s in sources)


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('case', ['quotient', 'full', 'refused'])
def test_the_three_consumers_reach_one_plan(case, real, monkeypatch):
    """`precompile`, the host half of `prepare` and `measured_shard_plan`:
    the same images, the same launch merging, the same sources -- and
    `prepare` makes no plan it does not take."""
    monkeypatch.setattr(runtime, 'ensure_device', lambda *a: None)
    compiled = []
    monkeypatch.setattr(jit, 'compile_many',
                        lambda sources, extra: compiled.append(list(sources))
                        or [])
    G = cases.config3_graphs(24)
    kn, ke, q = cases.config3_kernels()
    b = HostOnly(real=real, **(dict(variants=list(VARIANTS))
                               if case == 'refused' else {}))
    k = MarginalizedGraphKernel(kn, ke, q=q, backend=b)
    i, j = np.triu_indices(len(G))
    jobs = np.column_stack((i, j)).astype(np.uint32).ravel().view(job_t)
    traits = k.traits(symmetric=True, lmin=1 if case == 'full' else 0)
    quot = case == 'quotient'

    host, made = b.host_half_of_prepare(k, G, jobs, traits)
    assert host.shape.quot is quot
    assert (getattr(host.dgraphs[0], 'n_orig', None) is not None) is quot
    # the full images are not partitioned when the quotient is taken; they
    # are after the quotient's layout was refused, and lmin = 1 offers none
    assert made == {'quotient': [True], 'full': [False],
                    'refused': [True, False]}[case]
    sources = b._sources(host.part[1], kn, host.edge_kernel, k.p,
                         host.dgraphs, host.shape)

    b.precompile(G, kn, ke, k.p, jobs, traits)
    assert _keys(b, compiled[-1]) == _keys(b, sources.values())

    del b.partitioned[:]
    plans = list(b._host_plans(G, kn, ke, jobs, traits))
    assert b.partitioned == made + [False] * quot
    assert _ids(plans[0].dgraphs) == _ids(host.dgraphs)
    assert plans[0].shape == host.shape
    assert plans[0].part.merge_map == host.part.merge_map
    assert plans[0].part[1] == host.part[1]
    assert np.array_equal(plans[0].part[2], host.part[2])
    assert plans[0].part[3] == host.part[3]

    sp = measured_shard_plan(b, G, kn, ke, jobs, len(G), len(G), traits, 0, 2)
    assert sp.merge_map == plans[-1].part.merge_map
    assert sp.quotient == (host.part.merge_map if quot else None)
    assert np.array_equal(sp._model['launch_order'], plans[-1].part[2])
    # a shard runs on the images, and with the merging, of its whole list
    for shard in sp.shards:
        mine = np.ascontiguousarray(jobs[shard])
        shost, smade = b.host_half_of_prepare(
            k, G, mine, traits, packed=True, merge_map=sp.merge_map,
            quotient=sp.quotient)
        assert shost.shape == host.shape and smade == [quot]
        assert _ids(shost.dgraphs) == _ids(host.dgraphs)
        assert shost.part.merge_map == host.part.merge_map
        assert set(shost.part[1]) <= set(host.part[1])
