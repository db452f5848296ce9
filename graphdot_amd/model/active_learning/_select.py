"""Host side of select.hip: compiles the selection kernels once (JIT cache of
graphdot_amd.hip.jit, IEEE arithmetic: no fast-math) and drives the greedy
loops on a kernel matrix that stays in device memory.  Every launch goes to
torch's *current* stream of the matrix's device, in stream order, two or
three per pick; the pivot index never leaves the device, and the only host
synchronisation is the one download at the end (the picks and the status
word)."""
from ...hip.source_module import STATIC, current_stream, suffix

_module = STATIC['select.hip']
_BLOCK = 256
_WAVES = _BLOCK // 64

#: status words of select.hip
ST_OK, ST_DM_RESIDUAL, ST_VM_RESIDUAL, ST_NO_CANDIDATE = 0, 1, 2, 3


def column_major(K):
    """`K` (a square float32 / float64 CUDA tensor, assumed symmetric) as a
    tensor whose memory is the column-major matrix: a row-major symmetric
    matrix is its own column-major image; anything else is copied."""
    import torch
    assert K.is_cuda and K.dim() == 2 and K.shape[0] == K.shape[1]
    if K.dtype not in (torch.float32, torch.float64):
        K = K.to(torch.float64)
    n = K.shape[0]
    if n <= 1 or K.stride() in ((1, n), (n, 1)):
        return K
    return K.contiguous()


def select(K, n, method, alpha=0.0, tol=0.0, state=None):
    """Greedy selection of `n` indices on the device.  `K`: square float32 or
    float64 CUDA tensor, symmetric (read as column-major; see
    `column_major`).  `method`: 'determinant' or 'variance' (`alpha` is then
    added to the diagonal as it is read).  Returns (picks as a numpy int64
    array, status word).

    `state`: a dict that receives the device tensors the loop worked on, as
    the last launch left them, under the names `crit`, `V`, `W`, `chosen`,
    `scal` and `partials` (for the tests; the models pass none, and nothing
    is launched or waited for on its account).  Column s of `V` (Q or L) is
    at s N; 'determinant' keeps row s of `W` (C) at s N, 'variance' one
    column (p) in `W`.  The last pick gets no `al_update_argmax`: `crit` is
    the criterion after n - 1 updates, column n - 1 of `V` the direction w
    before its scaling (determinant; `scal[0]` = 1 / |w|, and row n - 1 of
    `W` is not written) or the column l (variance; `W` is then the posterior
    column p of the last pick)."""
    import numpy as np
    import torch
    K = column_major(K)
    N = K.shape[0]
    assert 1 <= n <= N
    sfx = suffix(K.dtype)
    G = -(-N // _BLOCK)
    dev = K.device
    f64 = dict(dtype=torch.float64, device=dev)
    stream = current_stream(dev)
    with torch.cuda.device(dev):
        # [status, direction counter, update counter, pad, picks[n]]
        # (picks not reached stay -1: the caller counts the valid ones)
        iw = torch.full((4 + n,), -1, dtype=torch.int32, device=dev)
        iw[:4] = 0
        chosen = torch.zeros(N, dtype=torch.uint8, device=dev)
        bidx = torch.empty(G, dtype=torch.int32, device=dev)
        crit = torch.empty(N, **f64)
        V = torch.empty(n * N, **f64)         # Q or L, column s at s N
        W = torch.empty(n * N if method == 'determinant' else N, **f64)
        partials = torch.empty(2 * G, **f64)
        bval = torch.empty(G, **f64)
        scal = torch.empty(1, **f64)
    p_k, p_iw = K.data_ptr(), iw.data_ptr()
    p_status, p_dcnt, p_ucnt, p_picks = p_iw, p_iw + 4, p_iw + 8, p_iw + 16
    p_V, p_W = V.data_ptr(), W.data_ptr()

    def launch(name, grid, fmt, *args):
        _module.launch(name, grid, _BLOCK, fmt, *args, stream=stream)

    def update(s, op, nxt):
        launch('al_update_argmax', G, 'iiiiQQQQQiQQQQQQ', N, s, op, nxt,
               crit.data_ptr(), p_V, p_W, scal.data_ptr(), partials.data_ptr(),
               G, chosen.data_ptr(), p_picks, p_status, bval.data_ptr(),
               bidx.data_ptr(), p_ucnt)

    cgrid = -(-N // _WAVES)
    if method == 'determinant':
        launch('al_colreduce_' + sfx, cgrid, 'QiidQQQQ', p_k, N, 1, 0.0, 0, 0,
               p_status, crit.data_ptr())
        update(0, 0, 0)
        for s in range(n):
            launch('al_dm_direction_' + sfx, G, 'QiidQQQQQQQ', p_k, N, s, tol,
                   p_V, p_W, p_picks, p_status, partials.data_ptr(), p_dcnt,
                   scal.data_ptr())
            if s + 1 == n:
                break           # (the last pick: only its residual is checked)
            launch('al_colreduce_' + sfx, cgrid, 'QiidQQQQ', p_k, N, 0, 0.0,
                   p_V + 8 * s * N, scal.data_ptr(), p_status,
                   p_W + 8 * s * N)
            update(s, 1, s + 1)
    elif method == 'variance':
        launch('al_colreduce_' + sfx, cgrid, 'QiidQQQQ', p_k, N, 2,
               float(alpha), 0, 0, p_status, crit.data_ptr())
        update(0, 0, 0)
        for s in range(n):
            launch('al_vm_column_' + sfx, G, 'QiiddQQQQQQ', p_k, N, s,
                   float(alpha), tol, p_V, p_W, p_picks, chosen.data_ptr(),
                   p_status, partials.data_ptr())
            if s + 1 == n:
                break
            update(s, 2, s + 1)
    else:
        raise ValueError(f'unknown selection method {method!r}')
    # the one download (it waits for the stream); the workspaces stay alive
    # until here, behind every launch that uses them
    out = iw.cpu().numpy()
    if state is not None:
        state.update(crit=crit, V=V, W=W, chosen=chosen, scal=scal,
                     partials=partials)
    return out[4:].astype(np.int64), int(out[0])
