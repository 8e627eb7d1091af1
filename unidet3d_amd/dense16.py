"""The decoder's Linear / MLP / LayerNorm ops with bf16 ACTIVATIONS in HBM (include/u3d.h K14b, csrc/gemm_b16.hip).

BASELINE configs[2] is the reference's ``--amp`` run (tools/train.py:86-99): autocast hands every ``nn.Linear`` /
``nn.MultiheadAttention`` of unidet3d/encoder.py:19-21,55-61,138-163 a 16-bit input and gets a 16-bit output back, while LayerNorm
results and the residual stream stay fp32.  ``precision.bf16_act()`` turns the same data flow on here (it implies bf16 MFMA
operands, ``precision.bf16()``):

* a LayerNorm writes its fp32 result AND a bf16 copy of it (``attach_b16`` -- an attribute of the fp32 tensor, like the batch-norm
  shadows of sparse.py); the Linear that follows streams the copy.  The LayerNorm backward does the same for the gradient it hands
  to the layer in front of it;
* the hidden tensors of an MLP (FFN pre-activation / activation, 1024 wide; ReLU hidden of ``input_proj`` / ``outs_cls``) and their
  gradients exist ONLY in bf16: written by a GEMM epilogue, read by the GELU pass and by the next GEMM;
* the packed q / k / v projection, the attention output and their gradients are bf16 tensors as well (the attention kernels read and
  write them as they are: include/u3d.h u3d_attn_varlen_*_b16);
* results that feed a LayerNorm, the residual stream or the criterion stay fp32.

Products are the ones ``dense.py`` forms under ``precision.bf16()`` (bf16 operands rounded to nearest even, fp32 accumulation): a
bf16 copy holds exactly the rounding the fp32-tensor kernels apply in flight.  What differs is where a value is rounded ONCE MORE: the
GELU and its derivative see the rounded pre-activation, and the hidden gradient is rounded before the derivative multiplies it.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import dense as D
from . import wgrad_stream as WS      # noqa: F401  (the one mode binding; the side-stream protocol itself is dense._weight_grad_overlapped)
from .dense import EPI_BIAS, EPI_RELU, EPI_RELU_MASK, EPI_ADD      # noqa: F401  (the epi codes of u3d_gemm_nt_b16)

A16, B16, C16 = 1, 2, 4          # include/u3d.h U3D_A_BF16 / U3D_B_BF16 / U3D_C_BF16

STATS = {'hit': 0, 'miss': 0}


def attach_b16(t: torch.Tensor, copy: torch.Tensor):
    """``copy`` = ``t`` rounded to bf16 (same shape): remembered on the tensor object, valid while ``t`` is not modified in place."""
    t._u3d_b16 = (copy, t._version)


def b16_of(t: torch.Tensor):
    e = getattr(t, '_u3d_b16', None)
    if e is not None and e[1] == t._version and e[0].shape == t.shape and e[0].device == t.device:
        STATS['hit'] += 1
        return e[0]
    STATS['miss'] += 1
    return None


def _operand(t: torch.Tensor):
    """the tensor to stream for ``t``: a bf16 tensor itself, the bf16 copy of an fp32 tensor when it has one, else the fp32 tensor"""
    if t.dtype == torch.bfloat16:
        return t
    c = b16_of(t)
    return c if c is not None else t


def gemm_nt(a, w, bias=None, epi=EPI_BIAS, aux=None, out_bf16=False, planes=None):
    """epi(a [M,K] . w [N,K]^T): ``a`` fp32 or bf16, ``w`` / ``bias`` fp32; result bf16 when ``out_bf16`` else fp32.  (``planes`` is
    the other flow's: these kernels split nothing.)"""
    M, K = a.shape
    N = w.shape[0]
    c = torch.empty(M, N, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=a.device)
    if M:
        flags = (A16 if a.dtype == torch.bfloat16 else 0) | (C16 if out_bf16 else 0)
        fl = D._book(M, N, K, M * K * a.element_size() + N * K * 4 + M * N * c.element_size() * (2 if aux is not None else 1))
        L.call('u3d_gemm_nt_b16', L.ptr(a), L.ptr(w), L.ptr(bias), epi, L.ptr(aux), L.ptr(c), flags, M, N, K, fl, L.stream())
    return c


def _tn_q(t):
    """column granule of a TN operand: 8 for a bf16 tensor, 4 for an fp32 one"""
    return 8 if t.dtype == torch.bfloat16 else 4


def _tn(dy, x, want_bias):
    """``gemm_tn`` for a dy whose column count is a multiple of its granule"""
    M, N = dy.shape
    K = x.shape[1]
    dev = dy.device
    if K % _tn_q(x):
        raise L.U3DError(f'gemm_tn_b16: K={K} must be a multiple of {_tn_q(x)}')
    dw = torch.empty(N, K, dtype=torch.float32, device=dev)
    db = torch.empty(N, dtype=torch.float32, device=dev) if want_bias else None
    if M:
        ws = L.scratch(L.lib().u3d_gemm_tn_b16_ws_bytes(M, N, K), dev)
        flags = (A16 if dy.dtype == torch.bfloat16 else 0) | (B16 if x.dtype == torch.bfloat16 else 0)
        fl = D._book(M, N, K, M * N * dy.element_size() + M * K * x.element_size() + N * K * 4)
        L.call('u3d_gemm_tn_b16', L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(db), flags, M, N, K, L.ptr(ws), fl, L.stream())
    else:
        dw.zero_()
        if db is not None:
            db.zero_()
    return dw, db


def _ffn(x, w1, b1, w2, b2, act, p1, p2):
    """(None, a, z) of z = relu(x W1^T + b1) W2^T + b2 with the hidden tensor in bf16 only (GELU runs as a pass of its own)"""
    a = gemm_nt(x, w1, b1, EPI_RELU, out_bf16=True)
    return None, a, gemm_nt(a, w2, b2)


def _relu_nt(x, w, bias, planes=None):
    """relu(x W^T + b) in bf16: the first half of ``_ffn``"""
    return gemm_nt(x, w, bias, EPI_RELU, out_bf16=True)


def _ln_linear(x, gamma, beta, eps, w, bias):
    """(nq, nq16, stats, y) = (LayerNorm(x), its bf16 copy, row statistics, nq W^T + b) with the Linear streaming nq16"""
    nq, nq16, stats = D._layer_norm_fwd(FLOW, x, None, gamma, beta, eps, None)
    return nq, nq16, stats, gemm_nt(nq16, w, bias)


class FLOW:
    """The bf16-activation data flow as dense.py's ops see it (the counterpart of dense._Flow32; a namespace, never instantiated)."""
    act16 = True
    q = 32                                              # reduction-depth granule of u3d_gemm_nt_b16
    gelu = ('u3d_gelu_fwd_b16', 'u3d_gelu_bwd_b16')
    operand = staticmethod(_operand)
    nt = staticmethod(gemm_nt)
    tn = staticmethod(_tn)
    tn_q = staticmethod(_tn_q)
    ffn = staticmethod(_ffn)
    relu_nt = staticmethod(_relu_nt)
    ln_linear = staticmethod(_ln_linear)
    attach = staticmethod(attach_b16)

    @staticmethod
    def b16_like(t):
        return torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)


def gemm_tn(dy, x, want_bias):
    """(dy^T x [N,K] fp32, column sums of dy [N] or None); either operand fp32 or bf16; the columns of dy are zero-padded to its
    granule when needed (tiny heads: N = 19)"""
    return D._weight_grad(FLOW, dy, x, want_bias)
