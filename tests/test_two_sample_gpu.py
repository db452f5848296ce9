"""The device path of KernelTwoSampleTest on an MI355X: the launches of
mmd.hip on exact integer data bit for bit against numpy; against the definition
of the sums on index sets in numpy double (test_two_sample.py: its data, its
definition and its rounding bounds) on the stored matrix widened to double, for
float and double storage and both layouts, repeats bit for bit; against
`forms_torch` on the same device tensors; the independence of a split's sums
of its row and of the number of rows; the arguments; and the model on the HIP
backend against the definition on the very matrix it worked on -- no host
kernel evaluation.

The edges of the launch shapes.  N: one tile (2, 3, 63, 64), the tile edge on
both sides (63, 64, 65), a diagonal plus off-diagonal tiles (65, 129, 257; at
257 a strip with a full and a one-row tile to its right).  Rows of Z: one and
two splits, one wave's sixteen and one more (16, 17), one chunk of 64 and one
more (64, 65), three chunks in a group of four (130), and 257 = 64 * 4 + 1:
a full group of the largest KC and a second group, at N = 65 only.  The
launch takes the chunk size KC that holds the chunks, 4 at the most; the tests
also hand it the smallest and the largest (`_chunk_sizes`) and ask for the
same bits.  First-sample sizes 1, N / 2 and
N - 1."""
import numpy as np
import pytest

import test_two_sample as cpu

pytestmark = pytest.mark.gpu

EPS = cpu.EPS
SIZES = [2, 3, 63, 64, 65, 129, 257]
ROWS = [1, 2, 16, 17, 64, 65, 130]
#: one split past a full group of the largest chunk size
PAST_A_GROUP = 64 * 4 + 1


def _torch():
    import torch
    import graphdot_amd.model.two_sample  # noqa: F401 (torch first)
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a))


def _matrix(K, dtype, layout):
    """K stored as `dtype` on the device, contiguous along the index `layout`
    names."""
    A = _t(K.astype(dtype)).cuda()
    return A.t().contiguous().t() if layout == 'column-major' else A


def _rows_of(n):
    return ROWS + ([PAST_A_GROUP] if n == 65 else [])


def _cases(n):
    """(first-sample size, rows, Z, s) for every size of the first sample and
    every number of rows."""
    from graphdot_amd.model.two_sample import _mmd
    for n1 in cpu.first_sizes(n):
        z0 = np.arange(n) < n1
        for rows in _rows_of(n):
            yield n1, rows, _mmd.splits(z0, rows - 1, seed=rows + n1), \
                cpu.weights(z0)


def test_the_chunk_sizes():
    from graphdot_amd.model.two_sample import _mmd
    assert _mmd.KCS == (1, 2, 4) and PAST_A_GROUP == 64 * _mmd.KCS[-1] + 1
    assert _mmd.grid(65, PAST_A_GROUP) == (4, 2, 2)
    assert _mmd.grid(65, PAST_A_GROUP - 1) == (4, 2, 1)
    assert _mmd.grid(257, 130) == (4, 5, 1)
    assert _mmd.grid(64, 65) == (2, 1, 1)
    assert _mmd.grid(64, 1) == (1, 1, 1)
    assert _mmd.grid(4000, 10000) == (4, 63, 40)
    assert _mmd.grid(65, 130, 1) == (1, 2, 3)
    with pytest.raises(ValueError, match='kc'):
        _mmd.grid(65, 130, 8)


def _chunk_sizes(rows):
    """The chunk sizes a number of rows is run with: the launch's own choice,
    the smallest and the largest."""
    from graphdot_amd.model.two_sample import _mmd
    return sorted({1, _mmd.grid(64, rows)[0], _mmd.KCS[-1]})


# -- 1. exact data ---------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_exact_data_bit_for_bit(n):
    """Symmetric integer matrices with entries in [-8, 8]: every product and
    every partial sum is an integer far below 2^53, so that any order gives
    the same double, and numpy's is the exact one.  A wrong lane map of the
    matrix instruction shows here."""
    from graphdot_amd.model.two_sample import _mmd
    rng = np.random.default_rng(n)
    K = rng.integers(-8, 9, size=(n, n)).astype(np.float64)
    K = np.triu(K) + np.triu(K, 1).T
    assert np.array_equal(K, K.T)
    for n1, rows, Z, s in _cases(n):
        Zd = Z.astype(np.float64)
        want = np.stack((((Zd @ K) * Zd).sum(1), Zd @ K.sum(1),
                         Zd @ np.diag(K)), axis=1)
        assert np.array_equal(want, np.round(want))
        for dtype in (np.float32, np.float64):
            for layout in ('row-major', 'column-major'):
                for kc in _chunk_sizes(rows):
                    sums, r, d, w = _mmd.forms(_matrix(K, dtype, layout),
                                               _t(Z).cuda(), _t(s), kc)
                    assert np.array_equal(sums.cpu().numpy(), want), \
                        (n1, rows, dtype, layout, kc)
                    assert np.array_equal(r.cpu().numpy(), K.sum(1))
                    assert np.array_equal(d.cpu().numpy(), np.diag(K))


# -- 2. against the definition ---------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', SIZES)
def test_fused_against_the_definition(n, dtype):
    from graphdot_amd.model.two_sample import _mmd
    torch = _torch()
    K, _ = cpu.stored(n, dtype)
    share = 0.0
    for n1, rows, Z, s in _cases(n):
        for layout in ('row-major', 'column-major'):
            Kd = _matrix(K, dtype, layout)
            assert Kd.stride() == ((n, 1) if layout == 'row-major'
                                   else (1, n))
            a = _mmd.forms(Kd, _t(Z).cuda(), _t(s).cuda())
            for kc in [None] + _chunk_sizes(rows):
                b = _mmd.forms(Kd, _t(Z).cuda(), _t(s).cuda(), kc)
                for x, y in zip(a, b):
                    assert x.is_cuda and x.dtype == torch.float64
                    assert torch.equal(x, y), (n1, rows, layout, kc)
            share = max(share, cpu.check_sums(a, K, Z, s))
    print(f'n {n} {np.dtype(dtype).name}: the sums are off by at most '
          f'{share:.3g} of their bounds')


# -- 3. against the restatement --------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [3, 65, 257])
def test_fused_against_the_restatement(n, dtype):
    """Both chains on the same device tensors: each within the bound of the
    definition, so within twice the bound of each other."""
    from graphdot_amd.model.two_sample import _mmd
    K, _ = cpu.stored(n, dtype)
    share = 0.0
    for n1, rows, Z, s in _cases(n):
        if rows not in (1, 65, 130, PAST_A_GROUP):
            continue
        want, bound, _, _, _ = cpu.define_sums(K, Z)
        Kd, Zd, sd = _matrix(K, dtype, 'column-major'), _t(Z).cuda(), \
            _t(s).cuda()
        fused, said = _mmd.solve(Kd, Zd, sd)
        assert said is True
        restated = _mmd.forms_torch(Kd, Zd, sd)
        assert all(x.is_cuda for x in restated)
        share = max(share, cpu.check_sums(restated, K, Z, s))
        assert np.all(np.abs(fused[0].cpu().numpy()
                             - restated[0].cpu().numpy()) <= 2 * bound)
        A = np.abs(K)
        assert np.all(np.abs((fused[1] - restated[1]).cpu().numpy())
                      <= 2 * n * EPS * A.sum(1))
        assert np.all(np.abs((fused[3] - restated[3]).cpu().numpy())
                      <= 4 * n * EPS * (A @ np.abs(s)))
    print(f'n {n} {np.dtype(dtype).name}: the restatement on the device is '
          f'off by at most {share:.3g} of the bounds')


# -- 4. position independence ----------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [3, 65, 257])
def test_sums_do_not_depend_on_the_row(n, dtype):
    from graphdot_amd.model.two_sample import _mmd
    torch = _torch()
    K, _ = cpu.stored(n, dtype)
    Kd = _matrix(K, dtype, 'row-major')
    z0 = np.arange(n) < max(1, n // 2)
    s = _t(cpu.weights(z0))
    for rows in (130,) + ((PAST_A_GROUP,) if n == 65 else ()):
        Z = _mmd.splits(z0, rows - 1, seed=n)
        one = Z[7 % rows].copy()
        where = [0, 5, 16, 63, 64, rows - 1]
        Z[where] = one
        for kc in (None, 1):
            full = _mmd.forms(Kd, _t(Z).cuda(), s, kc)[0]
            for b in where[1:]:
                assert torch.equal(full[b], full[0]), (rows, b, kc)
            for k in (1, 17, 65):
                part = _mmd.forms(Kd, _t(Z[:k]).cuda(), s)[0]
                assert torch.equal(part, full[:k]), (rows, k, kc)


# -- 5. arguments ------------------------------------------------------------------------
def test_launches_check_their_arguments():
    from graphdot_amd.model.two_sample import _mmd
    torch = _torch()
    n = 8
    K = torch.eye(n, dtype=torch.float64, device='cuda')
    z0 = np.arange(n) < 3
    Z, s = _t(_mmd.splits(z0, 4, seed=0)).cuda(), _t(cpu.weights(z0)).cuda()
    with pytest.raises(TypeError, match='CUDA'):
        _mmd.forms(K.cpu(), Z, s)
    with pytest.raises(TypeError, match='K'):
        _mmd.forms(K[:, :4], Z, s)
    with pytest.raises(TypeError, match='K'):
        _mmd.forms(K.to(torch.float16), Z, s)
    with pytest.raises(TypeError, match='Z'):
        _mmd.forms(K, Z.to(torch.float64), s)
    with pytest.raises(TypeError, match='Z'):
        _mmd.forms(K, Z[:, :4], s)
    with pytest.raises(TypeError, match='Z'):
        _mmd.forms(K, Z[:0], s)
    with pytest.raises(TypeError, match='s'):
        _mmd.forms(K, Z, s[:4])
    with pytest.raises(ValueError, match='negative strides'):
        _mmd.forms(K.as_subclass(cpu.negative_strides()), Z, s)
    out, fused = _mmd.solve(K.cpu(), Z, s)
    assert fused is False and not out[0].is_cuda
    # K = I: q = u = dz = the size of the first sample, r = d = 1, w = s
    sums, r, d, w = _mmd.forms(K, Z.cpu(), s.cpu())
    assert sums.cpu().numpy().tolist() == [[3.0, 3.0, 3.0]] * 5
    assert r.cpu().numpy().tolist() == d.cpu().numpy().tolist() == [1.0] * n
    assert torch.equal(w, s)
    # a strided matrix is read as it is
    M, _ = cpu.stored(65)
    Md = _t(M).cuda()
    big = torch.zeros((130, 130), dtype=torch.float64, device='cuda')
    big[::2, ::2] = Md
    z0 = np.arange(65) < 30
    Z, s = _t(_mmd.splits(z0, 20, seed=1)), _t(cpu.weights(z0))
    for x, y in zip(_mmd.forms(big[::2, ::2], Z, s), _mmd.forms(Md, Z, s)):
        assert torch.equal(x, y)


# -- 6. the model on QM7-like graphs ---------------------------------------------------
N_GRAPHS = 12
N_PERMUTATIONS = 99


def _kernel(real, transform):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    knode, kedge, q = cases.config3_fit_kernels()
    k = MarginalizedGraphKernel(
        knode, kedge, q=q, q_bounds=(1e-3, 0.5),
        backend=HIPBackend(real=real),
        ftol=1e-13 if real is np.float64 else 1e-8)
    return Normalization(k) if transform == 'normalized' else k


@pytest.mark.parametrize('real', [np.float32, np.float64])
@pytest.mark.parametrize('transform', ['plain', 'normalized'])
def test_model_on_the_device_path(real, transform, monkeypatch):
    """The model's statistic and null against the definition on the very
    matrix it handed to the launches (downloaded here, for the test), within
    the propagated bound of test_two_sample.py."""
    import cases
    from graphdot_amd.model.two_sample import KernelTwoSampleTest, _mmd
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    torch = _torch()
    G = np.asarray(list(cases.config3_graphs(N_GRAPHS, seed=23)),
                   dtype=object)
    kernel = _kernel(real, transform)
    theta0 = np.array(kernel.theta)
    seen, calls = [], []
    solve = _mmd.solve

    def recording(K, Z, s):
        out, fused = solve(K, Z, s)
        seen.append((K.to(torch.float64).cpu().numpy(), K.dtype,
                     Z.cpu().numpy(), out[0].cpu().numpy()))
        return out, fused

    def counting(self, *args, **kwargs):
        calls.append(type(self).__name__)
        raise AssertionError('host kernel evaluation on the device path')
    monkeypatch.setattr(_mmd, 'solve', recording)
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', counting)
        monkeypatch.setattr(cls, 'diag', counting)
    for n1 in (6, 2):
        for estimator in cpu.ESTIMATORS:
            m = KernelTwoSampleTest(kernel, n_permutations=N_PERMUTATIONS,
                                    estimator=estimator, random_state=11,
                                    device='cuda').fit(G[:n1], G[n1:])
            assert m.last_timing['adopted'] is True
            assert m.last_timing['fused'] is True
            assert (m.n_, m.m_, m.seed_) == (n1, N_GRAPHS - n1, 11)
            K, stored_as, Z, sums = seen[-1]
            assert K.shape == (N_GRAPHS, N_GRAPHS)
            assert stored_as == (torch.float64 if transform == 'normalized'
                                 or real is np.float64 else torch.float32)
            z0 = np.arange(N_GRAPHS) < n1
            assert np.array_equal(
                Z, cpu.restated_splits(z0, N_PERMUTATIONS, 11))
            want, bound, _, _, tb = cpu.define_sums(K, Z)
            assert np.all(np.abs(sums - want) <= bound)
            stat = np.array([cpu.define_mmd(K, z, estimator) for z in Z])
            sb = cpu.statistic_bound(bound, tb, n1, N_GRAPHS - n1, estimator)
            got = np.concatenate(([m.statistic_], m.null_))
            print(f'{real.__name__} {transform} {n1} {estimator}: statistic '
                  f'{m.statistic_:.6g}, p {m.pvalue_:.3g}, off by at most '
                  f'{cpu.worst(got, stat, sb):.3g} of the bounds')
            assert np.all(np.abs(got - stat) <= sb)
            assert m.pvalue_ == (1 + np.sum(m.null_ >= m.statistic_)) \
                / (1 + N_PERMUTATIONS)
            s = cpu.weights(z0)
            assert np.all(np.abs(m.witness_ - K @ s) <= 2 * N_GRAPHS * EPS
                          * (np.abs(K) @ np.abs(s)))
    assert np.array_equal(kernel.theta, theta0)
    assert calls == []


# -- 7. not finite -----------------------------------------------------------------------
@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_entries_that_are_not_finite(bad):
    from graphdot_amd.model.two_sample import KernelTwoSampleTest
    n = 65
    K, lab = cpu.stored(n)
    good = KernelTwoSampleTest('precomputed', n_permutations=19,
                               random_state=0, device='cuda')
    good.fit(_t(K).cuda(), lab == 0)
    assert good.last_timing['fused'] is True
    assert good.statistic_ == pytest.approx(
        cpu.define_mmd(K, lab == 0, 'unbiased'), rel=1e-10)
    Kb = K.copy()
    Kb[40, 3] = Kb[3, 40] = bad
    with pytest.raises(ValueError, match='not finite'):
        KernelTwoSampleTest('precomputed', n_permutations=19, random_state=0,
                            device='cuda').fit(_t(Kb).cuda(), lab == 0)
