"""The device path of KernelTSNE on an MI355X: every kernel of
model/manifold/tsne.h alone against the definition of exact t-SNE in numpy
(test_tsne.py: its definition, its data and its rounding bounds) on the stored
matrix widened to double, for float and double storage, both layouts and
several splits of the columns; then the model on a CUDA matrix and on a graph
kernel of the HIP backend.

`forces`, `objective` and `step` are fed the tables the definition calibrated,
so that each kernel is tested alone.  The shapes are those of test_tsne.py
(below a wave, a strip plus one, a tile plus one, two tiles plus two, 257) --
from 65 samples on the columns are split by `parts_for` itself, and every
shape runs with the split given by hand as well (3 parts: with n <= 128 some
are empty) -- and 2049 for the calibration, the first size whose rows are not
staged in LDS.  The data have duplicated samples (d2 == 0 off the diagonal),
the embeddings two equal points (w == 1)."""
import numpy as np
import pytest

import test_tsne as cpu

pytestmark = pytest.mark.gpu

SHAPES = cpu.SHAPES
DTYPES = [np.float32, np.float64]
LAYOUTS = ['row-major', 'column-major']
PARTS = [None, 1, 3]


def _torch():
    import torch
    import graphdot_amd.model.manifold  # noqa: F401 (torch first)
    return torch


def _t(a):
    return cpu._t(a)


def _matrix(K, layout):
    """K on the device, contiguous along the index `layout` names."""
    A = _t(K).cuda()
    return A.t().contiguous().t() if layout == 'column-major' else A


def _bits(*tensors):
    torch = _torch()
    return [t.clone().view(torch.int64 if t.dtype == torch.float64
                           else torch.int32).cpu() for t in tensors]


def _same(a, b):
    torch = _torch()
    return all(torch.equal(x, y) for x, y in zip(a, b))


# -- 1. the calibration ----------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, perplexity', SHAPES)
def test_calibration_against_the_definition(n, perplexity, dtype):
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    K, d2, cal, P = cpu.case(n, perplexity, dtype)
    first = None
    for layout in LAYOUTS:
        Kd = _matrix(K, layout)
        diag = Kd.diagonal().to(torch.float64).contiguous()
        got = _tsne.calibrate(Kd, diag, perplexity)
        again = _tsne.calibrate(Kd, diag, perplexity)
        assert _same(_bits(*got), _bits(*again))
        # (the matrix is symmetric: either layout holds the same numbers at
        # the same places of a row)
        first = first or _bits(*got)
        assert _same(_bits(*got), first)
        beta, m, rZ, steps, flag = (g.cpu().numpy() for g in got)
        assert int(flag[0]) == 0 and steps.dtype == np.int32
        worst = cpu.check_calibration((beta, m, rZ, steps), d2, perplexity)
        assert (steps < 100).all()
        assert np.allclose(beta, cal[0], rtol=1e-4, atol=0)
    print(f'n = {n}: entropy within {worst:.2e} of log(perplexity)')


def test_calibration_of_rows_beyond_lds():
    """2049 columns: the rows are read from the matrix in every pass."""
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    n, perplexity = 2049, 30.0
    K = cpu.kernel_matrix(cpu.points(n, 1))
    d2 = cpu.define_d2(K)
    Kd = _t(K).cuda()
    diag = Kd.diagonal().to(torch.float64).contiguous()
    got = _tsne.calibrate(Kd, diag, perplexity)
    assert _same(_bits(*got), _bits(*_tsne.calibrate(Kd, diag, perplexity)))
    beta, m, rZ, steps, flag = (g.cpu().numpy() for g in got)
    assert int(flag[0]) == 0
    cpu.check_calibration((beta, m, rZ, steps), d2, perplexity)
    # the staged rows of the first 2048 samples alone hold other numbers; the
    # same code must agree with the definition there as well
    sub = _tsne.calibrate(Kd[:2048, :2048].contiguous(), diag[:2048].contiguous(),
                          perplexity)
    cpu.check_calibration([g.cpu().numpy() for g in sub[:4]],
                          d2[:2048, :2048], perplexity)


def test_equal_entries_cannot_be_calibrated():
    torch = _torch()
    from graphdot_amd.model.manifold import KernelTSNE, _tsne
    n = 33
    K = np.full((n, n), 0.3) + 0.7 * np.eye(n)
    Kd = _t(K).cuda()
    beta, m, rZ, steps, flag = _tsne.calibrate(
        Kd, Kd.diagonal().to(torch.float64).contiguous(), 5.0)
    assert int(flag) == 0
    assert bool((steps == 100).all()) and bool(torch.isfinite(beta).all())
    P = cpu.define_P(cpu.define_d2(K), beta.cpu().numpy(), m.cpu().numpy(),
                     rZ.cpu().numpy())
    off = ~np.eye(n, dtype=bool)
    assert np.abs(P[off] * (n * (n - 1)) - 1.0).max() <= cpu.bound(n)
    model = KernelTSNE('precomputed', perplexity=5.0, init='random',
                       max_iter=50)
    with pytest.warns(UserWarning, match='bisection of 33 of 33 rows'):
        model.fit(Kd)
    assert model.n_uncalibrated_ == n and model.last_timing['fused'] is True


# -- 2. the pass over the pairs --------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, perplexity', SHAPES)
def test_objective_against_the_definition(n, perplexity, dtype):
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    K, d2, cal, P = cpu.case(n, perplexity, dtype)
    tab = cpu.tables(cal, 'cuda')
    worst = 0.0
    for layout in LAYOUTS:
        Kd = _matrix(K, layout)
        diag = Kd.diagonal().to(torch.float64).contiguous()
        for a in (1.0, 12.0):
            for d in (2, 3):
                for scale in (1e-4, 10.0):
                    Y = cpu.embedding(n, d, scale)
                    Yd = _t(Y).cuda()
                    for parts in PARTS:
                        kl, grad = _tsne.objective(Kd, diag, *tab, Yd, a,
                                                   parts)
                        worst = max(worst, cpu.check_objective(
                            kl.cpu(), grad.cpu(), P, Y, a))
                    again = _tsne.objective(Kd, diag, *tab, Yd, a, parts)
                    assert _same(_bits(kl, grad), _bits(*again))
    assert _tsne.parts_for(n) == (1 if n <= 64 else -(-n // 64))
    print(f'n = {n}: at most {worst:.3f} of the bound')


@pytest.mark.parametrize('d', [2, 3])
@pytest.mark.parametrize('n, perplexity', [(33, 5.0), (130, 10.0)])
def test_the_clamp_of_q(n, perplexity, d):
    """One far outlier, whose pairs have w / Zq < eps: only there does the
    clamp of q change the gradient, and `forces` leaves those pairs to the
    walk of `tsne_update_*`."""
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    K, d2, cal, P = cpu.case(n, perplexity)
    tab = cpu.tables(cal, 'cuda')
    Kd = _t(K).cuda()
    diag = Kd.diagonal().to(torch.float64).contiguous()
    Y = cpu.outlier_embedding(n, d)
    Yd = _t(Y).cuda()
    if d == 2:
        assert cpu.clamp_matters(P, Y)
    for parts in PARTS:
        F = _tsne.forces(Kd, diag, *tab, Yd, parts).sum(0).cpu().numpy()
        tail = F[:, 2 * d + 1]
        assert tail[3] == n - 1 and (np.delete(tail, 3) == 1).all()
        kl, grad = _tsne.objective(Kd, diag, *tab, Yd, 1.0, parts)
        cpu.check_objective(kl.cpu(), grad.cpu(), P, Y, 1.0)
    # no pair is below tau in an embedding of ordinary size
    F = _tsne.forces(Kd, diag, *tab, _t(cpu.embedding(n, d, 10.0)).cuda())
    assert not F[:, :, 2 * d + 1].any()


# -- 3. the step -----------------------------------------------------------------------
def _step(Kd, diag, tab, P, Y, update, gains, a, mom, lr, parts=None):
    """One `step` on the device from the given state, checked against the
    numpy step; the bits of what it left."""
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    state = _tsne.State(_t(Y).cuda())
    state.update, state.gains = _t(update).cuda(), _t(gains).cuda()
    F = _tsne.forces(Kd, diag, *tab, state.Y, parts)
    g2 = torch.empty(len(Y), dtype=torch.float64, device='cuda')
    before = state.Y
    _tsne.step(state, F, a, mom, lr, g2)
    assert torch.equal(before.cpu(), _t(Y))      # (the old Y is whole)
    got = (state.Y.cpu(), state.update.cpu(), state.gains.cpu())
    sure, same = cpu.check_step(got, P, Y, update, gains, a, mom, lr)
    cpu.check_norms(g2.cpu(), got[2], P, Y, a)
    return _bits(*got, g2), sure, same


def test_step_from_the_states_of_a_run():
    torch = _torch()
    n, perplexity = 33, 5.0
    K, d2, cal, P = cpu.case(n, perplexity)
    tab = cpu.tables(cal, 'cuda')
    Kd = _t(K).cuda()
    diag = Kd.diagonal().to(torch.float64).contiguous()
    for Y, update, gains, a, mom, lr in cpu.states(n, perplexity):
        bits, sure, same = _step(Kd, diag, tab, P, Y, update, gains, a, mom,
                                 lr)
        assert same >= 2 * n - 2 and (sure >= 2 * n - 2 or not update.any())
        again = _step(Kd, diag, tab, P, Y, update, gains, a, mom, lr)[0]
        assert _same(bits, again)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n, perplexity', SHAPES)
def test_step_against_the_definition(n, perplexity, dtype):
    """A state with updates of either sign and gains of several sizes, some
    at the floor."""
    torch = _torch()
    K, d2, cal, P = cpu.case(n, perplexity, dtype)
    tab = cpu.tables(cal, 'cuda')
    rng = np.random.RandomState(n)
    for layout in LAYOUTS:
        Kd = _matrix(K, layout)
        diag = Kd.diagonal().to(torch.float64).contiguous()
        for d in (2, 3):
            Y = cpu.embedding(n, d, 3.0)
            update = 0.1 * rng.standard_normal((n, d))
            gains = rng.choice([0.01, 0.0125, 0.8, 1.0, 2.2], size=(n, d))
            for parts in PARTS:
                for a, mom in ((12.0, 0.5), (1.0, 0.8)):
                    bits, sure, same = _step(Kd, diag, tab, P, Y, update,
                                             gains, a, mom, 50.0, parts)
                    assert same >= n * d - 2 and sure >= n * d - 2 * d - 2


# -- 4. flags and arguments ------------------------------------------------------------
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_entries_that_are_not_finite(bad):
    """The flag word of the calibration, and the model's ValueError: a flag
    in memory, read with the first look."""
    torch = _torch()
    from graphdot_amd.model.manifold import KernelTSNE, _tsne
    K = cpu.kernel_matrix(cpu.points(65, 65)).copy()
    K[64, 3] = K[3, 64] = bad
    Kd = _t(K).cuda()
    diag = Kd.diagonal().to(torch.float64).contiguous()
    assert int(_tsne.calibrate(Kd, diag, 5.0)[4]) == 1
    for init in ('random', 'kpca'):
        with pytest.raises(ValueError, match='not finite'):
            KernelTSNE('precomputed', perplexity=5.0, init=init).fit(Kd)
    K[64, 3] = K[3, 64] = 0.5
    assert int(_tsne.calibrate(_t(K).cuda(), diag, 5.0)[4]) == 0


def test_launches_check_their_arguments():
    torch = _torch()
    from graphdot_amd.model.manifold import _tsne
    n = 33
    K, d2, cal, P = cpu.case(n, 5.0)
    tab = cpu.tables(cal, 'cuda')
    Kd = _t(K).cuda()
    diag = Kd.diagonal().to(torch.float64).contiguous()
    Y = _t(cpu.embedding(n, 2, 1.0)).cuda()
    with pytest.raises(TypeError, match='CUDA'):
        _tsne.calibrate(Kd.cpu(), diag.cpu(), 5.0)
    with pytest.raises(TypeError, match='contiguous'):
        _tsne.calibrate(_t(np.zeros((n, 2 * n))).cuda()[:, ::2], diag, 5.0)
    with pytest.raises(TypeError, match='diag'):
        _tsne.calibrate(Kd, diag[:-1], 5.0)
    with pytest.raises(TypeError, match='float32 or float64'):
        _tsne.calibrate(Kd.half(), diag, 5.0)
    with pytest.raises(TypeError, match='n_components'):
        _tsne.forces(Kd, diag, *tab, _t(cpu.embedding(n, 4, 1.0)).cuda())
    with pytest.raises(TypeError, match='Y'):
        _tsne.forces(Kd, diag, *tab, Y[:-1])
    with pytest.raises(TypeError, match='beta'):
        _tsne.forces(Kd, diag, tab[0].float(), tab[1], tab[2], Y)
    with pytest.raises(ValueError, match='parts'):
        _tsne.forces(Kd, diag, *tab, Y, parts=0)
    state = _tsne.State(Y)
    with pytest.raises(TypeError, match='F'):
        _tsne.step(state, _tsne.forces(Kd, diag, *tab, Y)[:, :-1], 1.0, 0.5,
                   50.0)
    assert _tsne._declines(Kd) is None and _tsne._declines(Kd, 3) is None
    assert _tsne._declines(Kd, 4) and _tsne._declines(Kd.cpu())


# -- 5. the model ----------------------------------------------------------------------
def test_model_on_a_device_matrix():
    torch = _torch()
    from graphdot_amd.model.manifold import KernelTSNE
    K = cpu.model_kernel()
    kw = dict(perplexity=cpu.PERPLEXITY_MODEL)
    for dtype in DTYPES:
        Kd = _t(K.astype(dtype)).cuda()
        stored = Kd.clone()
        model = KernelTSNE('precomputed', **kw).fit(Kd)
        assert model.last_timing['fused'] is True
        assert model.last_timing['looks'] == 21
        cpu.check_model(model, K.astype(dtype), 1000)
        again = KernelTSNE('precomputed', **kw).fit(Kd)
        assert np.array_equal(again.embedding_, model.embedding_)
        assert again.kl_divergence_ == model.kl_divergence_
        assert torch.equal(Kd, stored)
    Kd = _t(K).cuda()
    three = KernelTSNE('precomputed', n_components=3, max_iter=300,
                       **kw).fit(Kd)
    assert three.last_timing['fused'] is True
    cpu.check_model(three, K, 300)
    four = KernelTSNE('precomputed', n_components=4, max_iter=300,
                      **kw).fit(Kd)
    assert four.last_timing['fused'] is False
    cpu.check_model(four, K, 300)
    stop = KernelTSNE('precomputed', min_grad_norm=np.inf, init='random',
                      **kw).fit(Kd)
    assert stop.n_iter_ == 50 and stop.last_timing['looks'] == 2
    assert stop.last_timing['stopped'] == 'gradient norm'


def test_quality_band_of_scikit_learn():
    from graphdot_amd.model.manifold import KernelTSNE

    def fit(K, init):
        model = KernelTSNE('precomputed', perplexity=cpu.PERPLEXITY_MODEL,
                           init=init).fit(_t(K).cuda())
        assert model.last_timing['fused'] is True
        return model
    cpu.check_bands(fit)


def test_nothing_of_the_size_of_the_matrix_is_allocated():
    """`fit` on a float (1000, 1000) CUDA matrix, 4 MB: above it, one set of
    partial sums (16 parts, 768 KB), the KL terms of a look (16 parts, 128 KB)
    and (n, 64) doubles for the state, the tables and KernelPCA's blocks --
    less than half of the matrix."""
    torch = _torch()
    from graphdot_amd.model.manifold import KernelTSNE, _tsne
    n = 1000
    Kd = _t(cpu.kernel_matrix(cpu.points(n, 2), np.float32)).cuda()
    model = KernelTSNE('precomputed', max_iter=100)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    model.fit(Kd)
    peak = torch.cuda.max_memory_allocated() - base
    print(f'{peak} bytes above the matrix of {Kd.numel() * 4}')
    assert model.last_timing['fused'] is True and model.n_iter_ == 100
    parts = _tsne.parts_for(n)
    assert parts == 16
    most = 8 * (parts * n * 6 + parts * n + 64 * n)
    assert peak <= most < Kd.numel() * 4 // 2


N_GRAPHS = 40


def _kernel(real):
    import cases
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.marginalized._backend_hip import HIPBackend
    from graphdot_amd.kernel.fix import Normalization
    knode, kedge, q = cases.config3_fit_kernels()
    return Normalization(MarginalizedGraphKernel(
        knode, kedge, q=q, q_bounds=(1e-3, 0.5),
        backend=HIPBackend(real=real),
        ftol=1e-13 if real is np.float64 else 1e-8))


@pytest.mark.parametrize('real', [np.float32, np.float64])
def test_model_on_the_device_path(real, monkeypatch):
    """A graph kernel on the HIP backend: the matrix is adopted where the
    solver wrote it, no host kernel evaluation, and the map is that of the
    restatement on the CPU on the very matrix the device path worked on."""
    import cases
    from graphdot_amd.model.manifold import KernelTSNE
    from graphdot_amd.kernel.marginalized import MarginalizedGraphKernel
    from graphdot_amd.kernel.fix import Normalization
    torch = _torch()
    G = np.asarray(list(cases.config3_graphs(N_GRAPHS, seed=29)),
                   dtype=object)
    kernel = _kernel(real)
    theta0 = np.array(kernel.theta)
    K = torch.as_tensor(kernel.device_gram(G), device='cuda').cpu().numpy()
    calls = []

    def counting(self, *args, **kwargs):
        calls.append(type(self).__name__)
        raise AssertionError('host kernel evaluation on the device path')
    for cls in (MarginalizedGraphKernel, Normalization):
        monkeypatch.setattr(cls, '__call__', counting)
    kw = dict(perplexity=8.0, max_iter=300)
    model = KernelTSNE(kernel, device='cuda', **kw)
    Y = model.fit_transform(G)
    assert model.last_timing['adopted'] is True
    assert model.last_timing['fused'] is True
    assert np.array_equal(kernel.theta, theta0) and calls == []
    cpu.check_model(model, K, 300)
    again = KernelTSNE(kernel, device='cuda', **kw).fit_transform(G)
    assert np.array_equal(again, Y)
    # the start alone: KernelPCA's coordinates on the adopted matrix
    start = KernelTSNE(kernel, device='cuda', max_iter=0,
                       perplexity=8.0).fit(G)
    assert start.n_iter_ == 0 and start.last_timing['looks'] == 1
    assert start.embedding_[:, 0].std() == pytest.approx(1e-4, rel=1e-12)
    assert np.array_equal(kernel.theta, theta0) and calls == []
