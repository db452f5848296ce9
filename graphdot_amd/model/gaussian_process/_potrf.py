"""Host side of potrf.hip, the one-launch Cholesky factorisation and inverse:
compiles the kernel once (JIT cache of graphdot_amd.hip.jit, IEEE arithmetic:
no fast-math) and runs it on float64 torch tensors.  The launch goes to
torch's *current* stream of the tensor's device, so that it is ordered
against the torch operations around it (the clone before, whatever reads the
inverse after) whatever stream the caller works on."""
from ...hip.source_module import STATIC, current_stream

_module = STATIC['potrf.hip']
_B = 64


class FactorisationError(RuntimeError):
    """The data-flow launch gave up on a wait (its status word is set)."""


def _dataflow(A, invert, stamps=None):
    """One launch of `spd_factor_invert_f64` on the row-contiguous float64
    CUDA tensor `A` (overwritten: L in its lower tiles).  Returns (Kinv or
    None, head): `head` is the int32 tensor whose first 16 + 2 nb words are
    [next role, status, pad][nb doubles: log-determinant shares of the
    diagonal blocks] -- one small download tells the caller whether the
    launch completed and what log|L| is."""
    import torch
    n = A.shape[0]
    nb = -(-n // _B)
    ld = A.stride(0) if n > 1 else 1
    with torch.cuda.device(A.device):
        head = torch.zeros(16 + 2 * nb + 2 * nb * nb, dtype=torch.int32,
                           device=A.device)
        linv = torch.empty(nb * _B * _B, dtype=torch.float64, device=A.device)
        if invert:
            Kinv = torch.empty((n, n), dtype=torch.float64, device=A.device)
            Z = torch.empty(nb * nb * _B * _B, dtype=torch.float64,
                            device=A.device)
        else:
            Kinv = Z = None
    roles = nb * nb + (nb * (nb + 1) // 2 if invert else 0)
    # (roles are handed out by an atomic counter in dependency order: any
    # grid size is deadlock-free; 512 = two workgroups per compute unit)
    _module.launch('spd_factor_invert_f64', min(roles, 512), 256,
                   'QQQQQiiiiQ', A.data_ptr(),
                   Kinv.data_ptr() if invert else 0,
                   Z.data_ptr() if invert else 0, linv.data_ptr(),
                   head.data_ptr(), ld, n, n, 1 if invert else 0,
                   stamps.data_ptr() if stamps is not None else 0,
                   stream=current_stream(A.device))
    return Kinv, head


def parse_head(words, nb):
    """(completed, log|L|) from the first 16 + 2 nb int32 words of the
    launch's sync buffer, given as 8 + nb float64 (how the regressor packs
    them into its one download) or as the int32 words themselves."""
    import numpy as np
    words = np.ascontiguousarray(words)
    status = int(words.view(np.int32)[1])
    shares = words.view(np.float64)[8:8 + nb]
    return status == 0, float(shares.sum())


def read_head(head, nb):
    """(completed, log|L|) from the first words of the launch's sync buffer:
    ONE device-to-host copy (it synchronises with the launch)."""
    return parse_head(head[:16 + 2 * nb].cpu().numpy(), nb)


def packed_head(head, nb):
    """The head of `factor_inverse` as a float64 tensor, for the caller to
    concatenate with its own float64 results into ONE download."""
    import torch
    return head[:16 + 2 * nb].view(torch.float64)


def logdet(packed, nb):
    """(``log|K|``, the caller's own numbers) from a download that starts
    with `packed_head`.  NaN when `K` is not positive definite;
    `FactorisationError` when the launch did not complete."""
    completed, logdet_l = parse_head(packed[:8 + nb], nb)
    if not completed:
        raise FactorisationError(
            'spd_factor_invert_f64 gave up waiting for a tile')
    return 2.0 * logdet_l, packed[8 + nb:]


def factor_inverse(K):
    """``K^-1`` and ``log|K|`` of the symmetric positive definite float64
    CUDA tensor `K` in ONE launch (potrf.hip, `spd_factor_invert_f64`):
    returns (Kinv, head, nb); `read_head(head, nb)` gives (completed,
    log|L|) -- ``log|K| = 2 log|L|``, NaN when `K` is not positive definite.
    `K` is left untouched (the factor is computed in a copy)."""
    import torch
    assert K.is_cuda and K.dtype == torch.float64 and K.dim() == 2
    n = K.shape[0]
    assert K.shape[1] == n and n >= 1
    return factor_inverse_(K.clone(memory_format=torch.contiguous_format))


def factor_inverse_(A):
    """`factor_inverse` of a matrix the caller has no further use for: the
    factor is computed in the memory of the row-major contiguous `A` (L in
    its lower tiles afterwards) instead of in a copy."""
    import torch
    assert A.is_cuda and A.dtype == torch.float64 and A.dim() == 2
    n = A.shape[0]
    assert A.shape[1] == n and n >= 1
    assert n == 1 or A.stride() == (n, 1)
    Kinv, head = _dataflow(A, True)
    return Kinv, head, -(-n // _B)


def cholesky_(A):
    """Lower Cholesky factor of the symmetric positive definite float64 CUDA
    tensor `A` (n x n), computed in the memory of `A` (the same launch without
    the roles of the inverse).  Returns a tensor (a view of `A`) with L in its
    lower triangle *of every diagonal block and below*; tiles above the
    diagonal keep the input -- take ``torch.tril`` of what is returned.  Rows
    or columns must be contiguous (a column-major matrix is its own
    transpose's row-major image: symmetric, so the view ``A.T`` is factored).
    Not positive definite: NaN on the diagonal."""
    import torch
    assert A.is_cuda and A.dtype == torch.float64 and A.dim() == 2
    n = A.shape[0]
    assert A.shape[1] == n
    if n > 1 and A.stride(1) != 1:
        assert A.stride(0) == 1, 'rows or columns must be contiguous'
        A = A.T
    _, head = _dataflow(A, False)
    A._gd_head = head          # (the launch's status word, for the tests)
    return A
