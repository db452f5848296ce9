"""select.hip on an MI355X, state by state: what every kernel of the two
greedy loops wrote (`_select.select(..., state={})`) against the definition of
that state in numpy float64 (test_active_learning.py: its matrices, its two
references and its bounds), on the stored matrix widened to double and along
the device's own picks.

The tolerance of every compared quantity is 8 x max(E_host, 4 eps) x scale:
E_host is the error of the host loops' recurrence against the definition on
the same matrix and picks, computed in the same test.  Every product and sum
of the kernels is double, so float and double storage get the same bounds.

The edges of the launch shapes: the 64 rows of an `al_colreduce_*` pass and
the block of 256 on both sides, n == N, three blocks, and more picks than one
pass of the coefficient staging holds (CHUNK).  Then what the argmax does
where the index alone decides, what a NaN criterion does, the layouts
`column_major` accepts, and the status words through `_greedy.run`."""
import re

import numpy as np
import pytest

import test_active_learning as cpu

pytestmark = pytest.mark.gpu

METHODS = ['determinant', 'variance']
DTYPES = ['float64', 'float32']


def _torch():
    import torch
    import graphdot_amd.model.active_learning  # noqa: F401
    return torch


def _upload(K):
    return _torch().from_numpy(np.array(K)).cuda()     # (a writable copy)


def _select(K, n, method, alpha=0.0, state=None):
    """`_select.select` with the tolerances of `_greedy.run`; `K`: numpy
    (uploaded as it is stored) or a device tensor."""
    from graphdot_amd.model.active_learning import _greedy
    from graphdot_amd.model.active_learning._select import select
    if isinstance(K, np.ndarray):
        K = _upload(K)
    tol = _greedy.DM_TOL if method == 'determinant' else _greedy.VM_TOL
    return select(K, n, method, alpha=alpha, tol=tol, state=state)


def _device_state(K, n, method, alpha):
    """(picks, status, the state as numpy arrays named like the
    references', chosen)."""
    N = len(K)
    st = {}
    picks, status = _select(K, n, method, alpha, state=st)
    assert set(st) == {'crit', 'V', 'W', 'chosen', 'scal', 'partials'}
    st = {k: v.cpu().numpy() for k, v in st.items()}
    V = st['V'].reshape(n, N).T
    if method == 'determinant':
        got = dict(crit=st['crit'], Q=V[:, :n - 1], w=V[:, n - 1],
                   C=st['W'].reshape(n, N)[:n - 1], scal=st['scal'])
    else:
        got = dict(crit=st['crit'], L=V, p=st['W'])
    return picks, status, got, st['chosen']


def check_state(matrix, n, method):
    """Case (a) / (b) on one stored matrix: the state against the definition,
    the picks against the definition's criteria and the host loop."""
    K = cpu.stored(matrix)
    alpha = cpu.alpha_of(matrix, method)
    picks, status, got, chosen = _device_state(K, n, method, alpha)
    assert status == 0
    assert len(picks) == n and len(set(picks.tolist())) == n
    assert np.flatnonzero(chosen).tolist() == sorted(picks.tolist())
    K64 = K.astype(np.float64)
    want, hist, scale, e_host = cpu.host_error(K64, picks, method, alpha)
    bound = cpu.bounds(scale, e_host)
    share = {k: np.abs(got[k] - want[k]).max() / bound[k] for k in bound}
    margin, gap = cpu.history_margins(hist, picks)
    print(f'{cpu.matrix_id((matrix, n))} {method}: E_host ' +
          ' '.join(f'{k} {v:.1e}' for k, v in e_host.items()) +
          '; share of the bound ' +
          ' '.join(f'{k} {v:.2f}' for k, v in share.items()) +
          f'; margin {margin / bound["crit"]:.1e} '
          f'gap {gap / bound["crit"]:.1e} of the bound')
    assert set(share) == {k for k, v in want.items() if v.size}
    assert max(share.values()) <= 1.0, share
    assert margin <= 2 * bound['crit']
    # (test_active_learning.py asserts the same of the host's picks: no
    # rounding within the bound can change a pick of these matrices)
    assert gap > 1000 * bound['crit']
    assert picks.tolist() == list(cpu.host_picks(matrix, method, n, alpha))
    return share


# ------------------------------------------ (a) the state, at the launch edges
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,n', cpu.SHAPES)
def test_state_equals_its_definition(N, n, dtype, method):
    check_state(('spd', N, 10 + N, dtype), n, method)


# ------------------------------------- (b) beyond one chunk of coefficients
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_state_beyond_one_chunk_of_coefficients(dtype, method):
    N, n = cpu.BEYOND_ONE_CHUNK
    # the second pass of the staging loops needs more than CHUNK earlier
    # steps: the last two steps here have a second chunk of 1 and of 3
    assert n > cpu.chunk_of_select_hip() + 1
    check_state(('spd', N, 10 + N, dtype), n, method)


# ------------------------------------------------------------------ (c) ties
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['pairs', 'identity'])
def test_equal_criteria_go_to_the_smallest_index(name, dtype, method):
    """Every pick is decided by the index alone: among the lanes of a wave,
    the waves of a block and the three blocks."""
    n = 300
    picks, status = _select(cpu.tie_matrix(name, dtype), n, method)
    want = list(range(0, 520, 2)) + list(range(1, 80, 2)) \
        if name == 'pairs' else list(range(n))
    assert status == 0
    assert picks.tolist() == want
    assert want == list(cpu.host_picks((name, dtype), method, n))


# --------------------------------------------------------- (d) NaN criteria
def _with_nan_pair(N, i, j, dtype):
    K = cpu.spd(N, 1, dtype).copy()
    K[i, j] = K[j, i] = np.nan
    return K


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,i,j', [
    (N, i, 7) for N in (300, 200) for i in (0, 5, 64, 255, 256) if i < N])
def test_nan_criteria_are_passed_over(N, i, j, dtype, method):
    """One NaN pair makes the criteria of i and j NaN and nothing else: the
    device selects among the others as the host does, whichever lane, wave
    or block holds the NaN.  (A lane of the butterfly that kept its own NaN
    hid every candidate it was to hand on: 24 of these 32 cases picked
    another sample or found no candidate before `better` ranked a NaN
    incumbent below every number.)"""
    from graphdot_amd.model.active_learning import _greedy
    n = 20
    K = _with_nan_pair(N, i, j, dtype)
    alpha = cpu.ALPHA if method == 'variance' else 0.0
    host = _greedy.run(K.astype(np.float64), n, method, alpha=alpha)
    assert len(set(host)) == n and not {i, j} & set(host)
    picks, status = _select(K, n, method, alpha)
    assert status == 0
    assert picks.tolist() == host


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N', [200, 300])
def test_all_nan_matrix_has_no_candidate(N, dtype, method):
    from graphdot_amd.model.active_learning import _greedy, SelectionError
    K = np.full((N, N), np.nan, dtype=dtype)
    for path in (K.astype(np.float64), _upload(K)):
        with pytest.raises(SelectionError, match='no candidate'):
            _greedy.run(path, 5, method)


# -------------------------------------------------------------- (e) layouts
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_layouts_and_repeats_give_the_same_bits(dtype, method):
    torch = _torch()
    N, n = 257, 33
    matrix = ('spd', N, 10 + N, dtype)
    alpha = cpu.alpha_of(matrix, method)
    Kd = _upload(cpu.stored(matrix))
    big = torch.zeros(N + 30, N + 61, dtype=Kd.dtype, device='cuda')
    big[:N, :N] = Kd
    layouts = [Kd, Kd.T, Kd.T.contiguous(), big[:N, :N], Kd]
    assert layouts[1].stride() == (1, N) and layouts[3].stride()[0] > N
    seen = []
    for A in layouts:
        st = {}
        picks, status = _select(A, n, method, alpha, state=st)
        assert status == 0
        seen.append((picks.tolist(), st['crit'].cpu().numpy().tobytes()))
    assert seen[0][0] == list(cpu.host_picks(matrix, method, n, alpha))
    assert all(s == seen[0] for s in seen[1:])


# -------------------------------------------- (f) the status words, by run()
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_duplicated_samples_end_with_the_hosts_error(dtype, method):
    """Every sample twice: 40 picks, then no residual -- the same error with
    the same picks and the same pick number on both paths."""
    from graphdot_amd.model.active_learning import _greedy, SelectionError
    K = np.repeat(np.repeat(cpu.spd(40, 50, dtype), 2, axis=0), 2, axis=1)
    errors = []
    for path in (K.astype(np.float64), _upload(K)):
        with pytest.raises(SelectionError) as e:
            _greedy.run(path, 41, method, alpha=0.0)
        errors.append(e.value)
    host, dev = errors
    assert len(host.picks) == 40 and len({i // 2 for i in host.picks}) == 40
    assert [int(i) for i in dev.picks] == host.picks
    number = [int(re.search(r'pick (\d+)', str(e)).group(1)) for e in errors]
    assert number == [40, 40]
