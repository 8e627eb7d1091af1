"""One bf16-operand kernel per direction: the fp32-tensor bf16-operand entry points (U3D_BF16_OPERANDS of u3d_linear_act /
u3d_linear_dact / u3d_gemm_nt_add, and u3d_gemm_tn_bf16) must give the bits of u3d_gemm_nt_b16 / u3d_gemm_tn_b16 at flags 0 -- the
same RNE-rounded operands in the same LDS layout, the same MFMAs in the same order, the same epilogue.  The two NT routes pick their
tiles differently (cost model against "largest tile that fills the CUs"), so the NT cases also pin that the tile changes no bit.
Shapes: one K-step and one row | two steps, ragged second row tile | three steps (the un-peeled loop body runs once), N no multiple of
128 | four steps, columns past N dropped by the descriptor.  TN: M <= 64 gives one row split under both plans; one and two trips, a
ragged last trip, with and without the column sums."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16_OPERANDS = 16                      # include/u3d.h U3D_BF16_OPERANDS
NT_SHAPES = [(1, 64, 32), (129, 64, 64), (130, 192, 96), (257, 20, 128)]


def _nt_inputs(M, N, K):
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.1).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    aux = torch.randn(M, N, generator=g).to(DEV)
    return x, w, b, aux


def _b16(x, w, bias, epi, aux):
    from unidet3d_amd import _lib as L
    M, K = x.shape
    N = w.shape[0]
    c = torch.full((M, N), float('nan'), device=DEV)
    L.call('u3d_gemm_nt_b16', L.ptr(x), L.ptr(w), L.ptr(bias), epi, L.ptr(aux), L.ptr(c), 0, M, N, K, 0.0, L.stream())
    return c


@pytest.mark.parametrize('M,N,K', NT_SHAPES)
def test_nt_fp32_tensor_route_gives_the_bits_of_the_b16_kernel(M, N, K):
    from unidet3d_amd import _lib as L
    x, w, b, aux = _nt_inputs(M, N, K)
    y = torch.full((M, N), float('nan'), device=DEV)
    for act in (0, 1):                                                           # bias | bias + ReLU
        L.call('u3d_linear_act', L.ptr(x), L.ptr(w), L.ptr(b), act | BF16_OPERANDS, None, L.ptr(y), M, N, K, None, 0.0, L.stream())
        assert torch.equal(y, _b16(x, w, b, act, None)), f'act {act}'
    mask = torch.relu(aux)                                                       # the ReLU output the mask is read from
    L.call('u3d_linear_dact', L.ptr(x), L.ptr(w), L.ptr(mask), 1 | BF16_OPERANDS, L.ptr(y), M, N, K, None, 0.0, L.stream())
    assert torch.equal(y, _b16(x, w, None, 3, mask)), 'ReLU mask'
    L.call('u3d_gemm_nt_add', L.ptr(x), L.ptr(w), L.ptr(aux), BF16_OPERANDS, L.ptr(y), M, N, K, None, 0.0, L.stream())
    assert torch.equal(y, _b16(x, w, None, 5, aux)), 'addend'
    assert not torch.isnan(y).any()


@pytest.mark.parametrize('colsum', [False, True])
@pytest.mark.parametrize('M,N,K', [(33, 64, 64), (64, 20, 32)])
def test_tn_fp32_tensor_route_gives_the_bits_of_the_b16_kernel(M, N, K, colsum):
    from unidet3d_amd import _lib as L
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    dy = torch.randn(M, N, generator=g).to(DEV)
    x = torch.randn(M, K, generator=g).to(DEV)
    lib = L.lib()
    out = []
    for name, flags, ws_bytes in (('u3d_gemm_tn_bf16', (), lib.u3d_gemm_tn_ws_bytes(M, N, K)),
                                  ('u3d_gemm_tn_b16', (0,), lib.u3d_gemm_tn_b16_ws_bytes(M, N, K))):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        dw = torch.full((N, K), float('nan'), device=DEV)
        db = torch.full((N,), float('nan'), device=DEV) if colsum else None
        L.call(name, L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(db), *flags, M, N, K, L.ptr(ws), 0.0, L.stream())
        out.append((dw, db))
    assert torch.equal(out[0][0], out[1][0]) and not torch.isnan(out[0][0]).any()
    if colsum:
        assert torch.equal(out[0][1], out[1][1]) and not torch.isnan(out[0][1]).any()
