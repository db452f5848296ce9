"""The loops of graphdot_amd/model/svm/_smo.py, each of which is there once
(DESIGN.md section 34): the torch loop behind `smo_torch`, `smo_torch_from`
and `smo2_torch` bit for bit against what the separate loops gave
(tests/golden/make_golden_smo_loops.py, recorded before they became one), the
counts at source level, and on an MI355X the relaunch loop behind `smo`,
`smo_from` and `smo2` one step per launch against one long slice."""
import json
import os
import re
import sys
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_golden_smo_loops as recorded      # noqa: E402


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'smo_loops.json')) as f:
        return json.load(f)


def _same_bits(got, want):
    """Equal values where neither is a NaN, NaNs in the same places."""
    import torch
    nan = torch.isnan(want)
    return got.dtype == want.dtype and got.shape == want.shape \
        and torch.equal(torch.isnan(got), nan) \
        and torch.equal(got[~nan], want[~nan])


@pytest.mark.parametrize('name', list(recorded.CASES))
def test_torch_loops_reproduce_the_recorded_runs(golden, name):
    import torch
    assert set(golden) == set(recorded.CASES)
    runs = recorded.run(name)
    assert set(runs) == set(golden[name]) == set(recorded.LOOPS)
    for loop, r in runs.items():
        want = golden[name][loop]
        for field in ('alpha', 'G', 'info'):
            assert _same_bits(
                getattr(r, field),
                torch.tensor(want[field], dtype=torch.float64)), (loop, field)
        assert r.slices == want['slices'], loop


@pytest.mark.parametrize('name', list(recorded.CASES))
def test_smo_torch_is_the_loop_from_the_plain_start(golden, name):
    """`smo_torch_from` handed `start` gives what `smo_torch` was recorded
    to give."""
    import torch
    from graphdot_amd.model.svm import _smo
    (K, y, U, *_), max_iter = recorded.problem(name)
    r = _smo.smo_torch_from(K, y, U, *_smo.start(len(y), len(K), K.device),
                            recorded.TOL, max_iter)
    want = golden[name]['smo_torch']
    for field in ('alpha', 'G', 'info'):
        assert _same_bits(getattr(r, field), torch.tensor(
            want[field], dtype=torch.float64)), field
    assert r.slices == want['slices']


def test_the_recorded_cases_are_what_they_are_there_for(golden):
    for loop in recorded.LOOPS:
        assert 1.0 in [row[3] for row in golden['n7_p3_nan'][loop]['info']]
        steps = [row[0] for row in golden['n65_p4_max_iter_3'][loop]['info']]
        assert max(steps) == 3.0
        assert golden['n65_p4_max_iter_3'][loop]['slices'] == 4
    for name in recorded.CASES:
        (K, y, U, *_), _ = recorded.problem(name)
        assert bool((U == 0).any(1).all())
        assert len(K) == 1 or bool(((y > 0).any(1) & (y < 0).any(1)).all())


def test_each_loop_is_there_once():
    with open(os.path.join(ROOT, 'graphdot_amd', 'model', 'svm',
                           '_smo.py')) as f:
        text = f.read()
    assert len(re.findall(r'\.max\(1\)', text)) == 1    # working-set selection
    assert len(re.findall(r'info\.cpu\(\)', text)) == 1     # the host's look
    assert len(re.findall(r'^\s*while True:', text, re.M)) == 2
    assert len(re.findall(r'K\.data_ptr\(\) % 16', text)) == 1


# -- on the device: the relaunch loop ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_one_step_per_launch_against_one_slice(dtype):
    """n = 65 (past a wave), P = 2: `smo`, `smo_from` (from `one_class_start`)
    and `smo2` with ``steps=1`` give the bits of ``steps=SLICE``.  A launch of
    one step writes m and M as they are after that step, so a problem that
    stops after s steps by the tolerance is seen stopped by the look after
    launch max(s, 1): `slices` is the largest of these."""
    import torch
    import graphdot_amd.model.svm  # noqa: F401 (torch first)
    from graphdot_amd.model.svm import _smo
    K, y, U, nu, z, eps = (t.cuda() for t in recorded.batch(65, 2))
    K = K.to(getattr(torch, dtype))
    tol = recorded.TOL

    def runs(steps):
        return {
            'smo': _smo.smo(K, y, U, tol, steps=steps),
            'smo_from': _smo.smo_from(
                K, torch.ones_like(y), U, *_smo.one_class_start(K, nu, U),
                tol, steps=steps),
            'smo2': _smo.smo2(K, U, z, eps, tol, steps=steps)}

    whole, single = runs(_smo.SLICE), runs(1)
    torch.cuda.synchronize()
    for name, w in whole.items():
        s = single[name]
        steps = w.info[:, 0].cpu()
        print(f'{name} {dtype}: steps {steps.tolist()}, slices {w.slices} '
              f'and {s.slices}')
        assert bool((w.info[:, 3] == 0).all()) and int(steps.max()) < _smo.SLICE
        assert w.slices == 1, name
        for field in ('alpha', 'G', 'info'):
            assert torch.equal(getattr(w, field), getattr(s, field)), \
                (name, field)
        assert s.slices == max(1, int(steps.max())), name
