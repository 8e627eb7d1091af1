"""nn.Linear through the gfx950 fp32 MFMA GEMM kernels (include/u3d.h K14): forward, input gradient and
weight gradient of the decoder's Linear layers (unidet3d/encoder.py:19-21,55-61,138-140,153-155,163)."""
from __future__ import annotations

import os

import torch

from . import _lib as L
from . import precision as P
from . import account
from . import wgrad_stream as WS

_PROFILE_FLOPS = False


def set_profile_flops(on: bool):
    global _PROFILE_FLOPS
    _PROFILE_FLOPS = bool(on)


ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
# Epilogue of a data flow's NT product (``nt`` of the flow objects below; the values are the epi codes of u3d_gemm_nt_b16):
# + bias | relu(+ bias) | times relu'(aux), aux = the ReLU output | + aux.  EPI_GELU_MASK: times gelu'(aux), aux = the GELU
# pre-activation -- the fp32-tensor flow under FUSE_GELU only.
EPI_BIAS, EPI_RELU, EPI_RELU_MASK, EPI_ADD = 0, 1, 3, 5
EPI_GELU_MASK = 4


def _book(M, N, K, nbytes=None, extra_mn=0):
    """algorithmic flops of an [M,K] x [K,N] product, booked with its bytes (``nbytes``; default: fp32 operands + result (+ extra
    [M,N] streams))"""
    if not _PROFILE_FLOPS:
        return 0.0
    if nbytes is None:
        nbytes = 4.0 * (M * K + N * K + M * N * (1 + extra_mn))
    account.add('gemm', 2.0 * M * N * K, float(nbytes))
    return 2.0 * M * N * K


def _pad_cols(t, q):
    """the last dim of a 2-D tensor zero-padded to a multiple of ``q`` (``t`` itself when it is one): the reduction depth of an NT
    product, or the columns of dy in front of a TN product (tiny heads: N = 19, 8)"""
    n = t.shape[1]
    return t if n % q == 0 else torch.nn.functional.pad(t, (0, q - n % q))


# ---- transposed weight copies of a whole forward pass in one launch ----------------------------------------------------------------
# dX = dY . W runs as an NT product over W^T, so every Linear's backward needs a [K, N] copy of its [N, K] weight: ~31 transpose
# launches of ~4 us per training step.  ``transposed_weights(module)`` makes them all with ONE u3d_transpose_batch launch when the
# forward pass starts; the Linear / MLP functions pick their copy up in FORWARD (while the context is active) and keep it for their
# backward, so a copy can never outlive the weights it was made from (weights are not modified between a forward and its backward).
# Outside the context every op falls back to its own u3d_transpose launch.
_WT_ACTIVE = None          # data_ptr of a weight -> its [K, N] copy, while a transposed_weights() context is open


class transposed_weights:
    def __init__(self, module: torch.nn.Module):
        self.module = module

    def __enter__(self):
        global _WT_ACTIVE
        self.prev = _WT_ACTIVE
        ws = []
        if torch.is_grad_enabled():
            seen = set()
            for w in self.module.parameters():          # every [N, K] matrix: nn.Linear weights, in_proj_weight, 1x1x1 convolutions
                if not (w.dim() == 2 or (w.dim() == 5 and tuple(w.shape[1:4]) == (1, 1, 1))):
                    continue
                if not w.is_cuda or not w.requires_grad or w.data_ptr() in seen or not w.is_contiguous():
                    continue
                N, K = w.shape[0], w.numel() // w.shape[0]
                if N % 16 == 0 and K % 4 == 0:
                    seen.add(w.data_ptr())
                    ws.append((w, N, K))
        if ws:
            dev = ws[0][0].device
            flat = torch.empty(sum(N * K for _, N, K in ws), dtype=torch.float32, device=dev)
            rows, blocks, off, table, vers = [], 0, 0, {}, {}
            for w, N, K in ws:
                wt = flat[off:off + N * K].view(K, N)
                off += N * K
                rows.append([w.data_ptr(), wt.data_ptr(), N, K, blocks])
                blocks += ((N + 31) // 32) * ((K + 31) // 32)
                table[w.data_ptr()] = wt
                vers[w.data_ptr()] = w._version
            desc = L.h2d(rows, torch.int64, dev)
            L.call('u3d_transpose_batch', L.ptr(desc), len(rows), blocks, L.stream())
            table['_keep'] = (flat, desc)
            table['_versions'] = vers
            if _W_PLANES and not P.bf16() and P.get_fp32_math() == 'bf16x3':
                # three-plane products: the planes of every weight AND of its transposed copy, one launch (u3d_weight_planes_batch);
                # planes[(data_ptr of the fp32 matrix)] -> bf16 [3, rows, cols]
                mats = [(w, N * K) for w, N, K in ws] + [(table[w.data_ptr()], N * K) for w, N, K in ws]
                pflat = torch.empty(3 * sum(n for _, n in mats), dtype=torch.bfloat16, device=dev)
                prow, pblocks, poff, planes = [], 0, 0, {}
                for m, n in mats:
                    pl = pflat[poff:poff + 3 * n]
                    poff += 3 * n
                    prow.append([m.data_ptr(), pl.data_ptr(), n // 8, pblocks])
                    pblocks += (n // 8 + 255) // 256
                    planes[m.data_ptr()] = pl
                pdesc = L.h2d(prow, torch.int64, dev)
                L.call('u3d_weight_planes_batch', L.ptr(pdesc), len(prow), pblocks, L.stream())
                table['_planes'] = planes
                table['_keep'] += (pflat, pdesc)
            _WT_ACTIVE = table
        else:
            _WT_ACTIVE = None
        return self

    def __exit__(self, *exc):
        global _WT_ACTIVE
        _WT_ACTIVE = self.prev
        return False


# Pre-split W operands of the three-plane NT products (u3d_weight_planes_batch, `w_planes` of the NT calls): built, bit-identical, and OFF by
# default -- measured on MI355X (round 5, same box, two runs each): all GEMMs 5.40 / 5.34 ms with the planes, 5.41 / 5.41 without, step
# 293.5 / 292.5 vs 294.8 / 295.7 scenes/s.  The W split is a third of the NT kernel's split arithmetic (loop VALU 156 -> 110
# instructions, tools/isa_mix.py) and removing it buys nothing: the kernel is not bound by its VALU issue.  U3D_W_PLANES=1 turns it on.
_W_PLANES = os.environ.get('U3D_W_PLANES', '0') == '1'


def _planes_of(mat):
    """bf16 [3 * N * K] planes of an fp32 matrix (a weight or its transposed copy) made by the enclosing transposed_weights()
    context; None outside one.  Callers keep the tensor (ctx) for as long as a launch may read it."""
    if _WT_ACTIVE is None or mat is None or '_planes' not in _WT_ACTIVE:
        return None
    # a weight modified in place since the context was entered: its planes are stale, like its transposed copy (``_wt_of``) -> None,
    # and the kernel splits the operand itself.  (A transposed copy has no entry in ``_versions``: ``_wt_of`` has vouched for it.)
    if _WT_ACTIVE.get('_versions', {}).get(mat.data_ptr(), mat._version) != mat._version:
        return None
    return _WT_ACTIVE.get('_planes', {}).get(mat.data_ptr())


def _wt_of(weight):
    """the [K, N] copy of ``weight`` made by the enclosing transposed_weights() context (None outside one / for other tensors)"""
    if _WT_ACTIVE is None:
        return None
    wt = _WT_ACTIVE.get(weight.data_ptr())
    if wt is None or wt.shape != (weight.numel() // weight.shape[0], weight.shape[0]):
        return None
    # a parameter modified in place since the context was entered (EMA update, in-forward optimizer step): its copy is
    # stale -> None, and the op transposes for itself
    return wt if _WT_ACTIVE.get('_versions', {}).get(weight.data_ptr()) == weight._version else None


def _transposed(weight, q, wt=None, planes=None):
    """([K, Np] copy of ``weight`` [N, K] with the reduction dim N zero-padded to a multiple of ``q``, its pre-split planes or None).
    ``wt`` / ``planes``: the copy transposed_weights() made for this forward pass and its planes; they serve when no padding is needed."""
    N, K = weight.shape
    if N % q == 0:
        if wt is not None:
            return wt, planes
        wt = torch.empty(K, N, dtype=torch.float32, device=weight.device)
        L.call('u3d_transpose', L.ptr(weight.contiguous()), L.ptr(wt), N, K, L.stream())
        return wt, None
    wt = torch.zeros(K, (N + q - 1) // q * q, dtype=torch.float32, device=weight.device)       # tiny heads (N = 19, 8)
    wt[:, :N] = weight.t()
    return wt, None


# ---- the two data flows ------------------------------------------------------------------------------------------------------------
# Every op below exists once; what differs between fp32 tensors in HBM and the bf16 activations of precision.bf16_act() is behind a
# flow object: ``operand(t)`` (the tensor a GEMM streams for t), ``nt`` / ``tn`` (the products), ``ffn`` / ``ln_linear`` (the forward
# entry points that fuse two steps), ``gelu`` (the names of the stand-alone GELU passes), ``q`` / ``tn_q(dy)`` (padding granules of
# the NT reduction depth / of dy's columns in a TN product), ``b16_like(t)`` (the bf16 copy a LayerNorm writes next to t, or None).
# The fp32-tensor flow is here (FP32, and BF16 with bf16 MFMA operands); the bf16-activation flow is dense16.FLOW.
class _Flow32:
    """every activation and gradient is an fp32 tensor; ``bf``: the MFMA operands are rounded to bf16 in flight (precision.bf16())"""
    act16 = False
    gelu = ('u3d_gelu_fwd', 'u3d_gelu_bwd')

    def __init__(self, bf):
        self.bf = bf
        self.flag = P.BF16_FLAG if bf else 0
        self.q = 32 if bf else 16                       # reduction-depth granule of the NT kernels

    @staticmethod
    def operand(t):
        return t

    @staticmethod
    def tn_q(dy):
        return 4

    @staticmethod
    def b16_like(t):
        return None

    def nt(self, a, w, bias=None, epi=EPI_BIAS, aux=None, out_bf16=False, planes=None):
        """epi(a [M,K] . w [N,K]^T), fp32 (``out_bf16`` is for the other flow); ``planes``: the pre-split planes of ``w`` (three-plane
        products only).  Under bf16 operands K of the plain product is zero-padded to a multiple of 32 when needed."""
        M, K = a.shape
        N = w.shape[0]
        c = torch.empty(M, N, dtype=torch.float32, device=a.device)
        if not M:
            return c
        if epi == EPI_BIAS:
            if self.bf:
                a, w = _pad_cols(a, 32), _pad_cols(w, 32)
                L.call('u3d_linear_act', L.ptr(a), L.ptr(w), L.ptr(bias), P.BF16_FLAG, None, L.ptr(c), M, N, a.shape[1], None,
                       _book(M, N, a.shape[1]), L.stream())
            else:
                L.call('u3d_gemm_nt', L.ptr(a), L.ptr(w), L.ptr(bias), L.ptr(c), M, N, K, L.ptr(planes), _book(M, N, K), L.stream())
        elif epi == EPI_ADD:
            L.call('u3d_gemm_nt_add', L.ptr(a), L.ptr(w), L.ptr(aux), self.flag, L.ptr(c), M, N, K, None, _book(M, N, K, extra_mn=1),
                   L.stream())
        else:                                            # the input gradient THROUGH the activation (u3d_linear_dact)
            act = {EPI_RELU_MASK: ACT_RELU, EPI_GELU_MASK: ACT_GELU}[epi]
            L.call('u3d_linear_dact', L.ptr(a), L.ptr(w), L.ptr(aux), act | self.flag, L.ptr(c), M, N, K, L.ptr(planes),
                   _book(M, N, K, extra_mn=1), L.stream())
        return c

    def tn(self, dy, x, want_bias):
        """(dy^T x [N,K], column sums of dy [N] or None): one pass of u3d_gemm_tn (+ fixed-order reduce); N % 4 == 0"""
        M, N = dy.shape
        K = x.shape[1]
        dw = torch.empty(N, K, dtype=torch.float32, device=dy.device)
        db = torch.empty(N, dtype=torch.float32, device=dy.device) if want_bias else None       # rides along
        if M:
            ws = L.scratch(L.lib().u3d_gemm_tn_ws_bytes(M, N, K), dy.device)
            L.call('u3d_gemm_tn_bf16' if self.bf else 'u3d_gemm_tn', L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(db), M, N, K, L.ptr(ws),
                   _book(M, N, K), L.stream())
        else:
            dw.zero_()
            if db is not None:
                db.zero_()
        return dw, db

    def ffn(self, x, w1, b1, w2, b2, act, p1, p2):
        """(h, a, z) of z = act(x W1^T + b1) W2^T + b2 (include/u3d.h u3d_ffn_fwd): bias and activation live in the first GEMM's
        epilogue; a = the activation, h = the GELU pre-activation (None for ReLU)"""
        M, d_in = x.shape
        hid, d_out = w1.shape[0], w2.shape[0]
        a = torch.empty(M, hid, dtype=torch.float32, device=x.device)
        h = torch.empty(M, hid, dtype=torch.float32, device=x.device) if act == ACT_GELU else None
        z = torch.empty(M, d_out, dtype=torch.float32, device=x.device)
        if M:
            _book(M, hid, d_in, extra_mn=1 if act == ACT_GELU else 0)
            _book(M, d_out, hid)
            L.call('u3d_ffn_fwd', L.ptr(x), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), act | self.flag, L.ptr(h), L.ptr(a), L.ptr(z),
                   M, d_in, hid, d_out, L.ptr(p1), L.ptr(p2), 1.0 if _PROFILE_FLOPS else 0.0, L.stream())
        return h, a, z

    def relu_nt(self, x, w, bias, planes=None):
        """relu(x W^T + b) as one call (u3d_linear_act): the first half of ``ffn`` when something runs between the two GEMMs"""
        M, K = x.shape
        N = w.shape[0]
        a = torch.empty(M, N, dtype=torch.float32, device=x.device)
        if M:
            L.call('u3d_linear_act', L.ptr(x), L.ptr(w), L.ptr(bias), ACT_RELU | self.flag, None, L.ptr(a), M, N, K, L.ptr(planes),
                   _book(M, N, K), L.stream())
        return a

    def ln_linear(self, x, gamma, beta, eps, w, bias):
        """(nq, None, stats, y) = (LayerNorm(x), no bf16 copy, row statistics, nq W^T + b): include/u3d.h u3d_ln_linear"""
        M, C = x.shape
        N = w.shape[0]
        nq = torch.empty_like(x)
        stats = torch.empty(M, 2, dtype=torch.float32, device=x.device)
        y = torch.empty(M, N, dtype=torch.float32, device=x.device)
        if M:
            L.call('u3d_ln_linear', L.ptr(x), None, L.ptr(gamma), L.ptr(beta), float(eps), None, L.ptr(nq), L.ptr(stats), L.ptr(w),
                   L.ptr(bias), self.flag, None, L.ptr(y), M, C, N, None, _book(M, N, C), L.stream())
        return nq, None, stats, y


FP32, BF16 = _Flow32(False), _Flow32(True)


def _act16(x, *reduction_dims):
    """the bf16-activation data flow of dense16.py applies: precision.bf16_act(), a device tensor, every reduction depth % 32 == 0"""
    return P.bf16_act() and x.is_cuda and all(d % 32 == 0 for d in reduction_dims)


def _flow(x, *reduction_dims):
    """The data flow of one op: chosen ONCE, by its public wrapper, and kept on ctx -- backward runs the flow its forward ran, whatever
    the precision settings are by then."""
    if _act16(x, *reduction_dims):
        from . import dense16                           # (imports this module)
        return dense16.FLOW
    return BF16 if P.bf16() else FP32


def _layer_norm_fwd(flow, x, res, gamma, beta, eps, s):
    """(y, y16, stats) = (LayerNorm(x + res), its bf16 copy where the flow keeps one, row statistics); ``s`` receives x + res"""
    M, C = x.shape
    y = torch.empty_like(x)
    y16 = flow.b16_like(x)
    stats = torch.empty(M, 2, dtype=torch.float32, device=x.device)
    if M and y16 is None:
        L.call('u3d_layer_norm_fwd', L.ptr(x), L.ptr(res), L.ptr(gamma), L.ptr(beta), M, C, float(eps), L.ptr(s), L.ptr(y),
               L.ptr(stats), L.stream())
    elif M:
        L.call('u3d_layer_norm_fwd_b16', L.ptr(x), L.ptr(res), L.ptr(gamma), L.ptr(beta), M, C, float(eps), L.ptr(s), L.ptr(y),
               L.ptr(y16), L.ptr(stats), L.stream())
    return y, y16, stats


def _layer_norm_bwd(x, dy, gamma, stats):
    """(dx, dgamma, dbeta) of y = LayerNorm(x) for ONE incoming gradient (the tail of ``_LNLinearFn.backward``)"""
    M, C = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    if M:
        ws = L.scratch(L.lib().u3d_layer_norm_ws_bytes(M, C), x.device)
        L.call('u3d_layer_norm_bwd', L.ptr(x), L.ptr(dy), L.ptr(gamma), L.ptr(stats), M, C, L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(ws),
               L.stream())
    else:
        dg.zero_(); db.zero_()
    return dx, dg, db


def _gelu_pass(name, *ts):
    """a stand-alone GELU pass over whole tensors: a = gelu(h) for (h,), dh = da * gelu'(h) for (da, h)"""
    out = torch.empty_like(ts[0])
    if out.numel():
        L.call(name, *[L.ptr(t) for t in ts], L.ptr(out), out.numel(), L.stream())
    return out


def _input_grad(flow, dy, weight, wt=None, wt_planes=None, epi=EPI_BIAS, aux=None, out_bf16=False):
    """dX[M,K] = epi(dY[M,N] . W[N,K]): an NT product over the transposed (and, for the tiny heads, zero-padded) weight.  EPI_*_MASK:
    the input gradient THROUGH the activation that produced this layer's input (aux = its ReLU output / GELU pre-activation)."""
    wt, wt_planes = _transposed(weight, flow.q, wt, wt_planes)
    return flow.nt(_pad_cols(dy, flow.q), wt, None, epi, aux, out_bf16, wt_planes)


def _weight_grad(flow, dy, x, want_bias):
    """(dW[N,K] = dY^T X, db[N] = column sums of dY or None); the columns of dY zero-padded to the TN kernel's granule (N = 19)"""
    N = dy.shape[1]
    dyp = _pad_cols(dy, flow.tn_q(dy))
    dw, db = flow.tn(dyp, x, want_bias)
    if dyp is not dy:
        dw, db = dw[:N].contiguous(), (db[:N].contiguous() if db is not None else None)
    return dw, db


def _weight_grad_overlapped(flow, dy, x, want_bias, weight, bias):
    """``_weight_grad`` on the weight-gradient side stream when set_wgrad_overlap(2) is on (wgrad_stream.py; nothing downstream of a
    Linear needs its dW: the GEMM joins the sparse convolutions' weight-gradient chain and the dX chain goes on without it).  Only for
    leaf parameters without an existing .grad -- autograd then just stores the tensor; anything else is computed in line."""
    if not (WS.mode() == 2 and _OVERLAP_TN and dy.is_cuda and WS.async_dw_ok(weight, bias)):
        return _weight_grad(flow, dy, x, want_bias)
    _, grads = WS.run_on_side_stream(dy.device, lambda: _weight_grad(flow, dy, x, want_bias), reads=(dy, x))
    WS.queue_join(dy.device)
    return grads


_OVERLAP_TN = os.environ.get('U3D_OVERLAP_TN', '1') != '0'


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b.  x and (in backward) dy are streamed as ``flow.operand`` gives them.  Under dense16.FLOW the result is fp32, or
    -- ``out_bf16``: the packed q / k / v projection, whose only consumer is the attention kernel -- a bf16 tensor (its gradient then
    arrives as one); a bf16 INPUT (the attention output in front of ``out_proj``) gets a bf16 gradient back."""

    @staticmethod
    def forward(ctx, flow, x, weight, bias, out_bf16):
        x = x.contiguous()
        xa = flow.operand(x)
        w = weight.contiguous()
        ctx.save_for_backward(xa, w)
        ctx.flow = flow
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        ctx.wt = _wt_of(weight)
        ctx.wt_planes = _planes_of(ctx.wt)
        ctx.dx_bf16 = x.dtype == torch.bfloat16
        return flow.nt(xa, w, bias, out_bf16=bool(out_bf16) and w.shape[0] % 2 == 0, planes=_planes_of(weight))

    @staticmethod
    def backward(ctx, dy):
        xa, weight = ctx.saved_tensors
        flow = ctx.flow
        dy = dy.contiguous()
        da = flow.operand(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[2]:           # first: on the side stream it then waits for dy only, not for the dX product below
            dw, db = _weight_grad_overlapped(flow, da, xa, ctx.has_bias and ctx.needs_input_grad[3], weight, ctx.bias_ref)
        if ctx.needs_input_grad[1]:
            dx = _input_grad(flow, da, weight, ctx.wt, ctx.wt_planes, out_bf16=ctx.dx_bf16)
        if db is None and ctx.has_bias and ctx.needs_input_grad[3]:
            db = dy.float().sum(0)
        return None, dx, dw, db, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias=None, out_bf16: bool = False) -> torch.Tensor:
    """y = x W^T + b for 2-D x [M, K] (K % 16 == 0).  ``out_bf16``: under precision.bf16_act() the result is a bf16 tensor (for a
    consumer that reads one: the attention kernels); ignored otherwise."""
    if not x.shape[0] and getattr(x, '_u3d_rows_only', None) is not None:      # sparse.rows_only: a zero-row placeholder, not a matrix to multiply
        raise L.U3DError('linear: this tensor exists as bf16 rows only (fused inference wrote it for a sparse convolution): no fp32 values to read')
    return _LinearFn.apply(_flow(x, x.shape[1]), x, weight, bias, out_bf16)


# GELU in the GEMM epilogues (True) or as stand-alone passes u3d_gelu_fwd / u3d_gelu_bwd between plain GEMMs (False).  ReLU is
# always fused (one v_max / one compare per element).  Measured on MI355X (tools/prof_mlp.py, FFN 256 -> 1024 -> 256 over 16.8 k
# rows, forward + backward): fused 0.761 ms, stand-alone passes 0.682 ms (bf16 operands: 0.487 / 0.438) -- the ~15 VALU
# instructions per element of the erf GELU are not hidden in a GEMM epilogue (one wave per SIMD), while the stand-alone pass
# runs at HBM speed; so the default is the stand-alone pass.  (The bf16-activation flow has the stand-alone pass only.)
FUSE_GELU = os.environ.get('U3D_FUSE_GELU', '0') == '1'


def _dropout_pass(name, t, p, key):
    """one launch of the elementwise dropout kernel over a 2-D tensor (fp32, or bf16 for the ``_b16`` names): t . M / (1 - p)"""
    out = torch.empty_like(t)
    if t.numel():
        L.call(name, L.ptr(t), L.ptr(out), t.shape[0], t.shape[1], float(p), int(key[0]), int(key[1]), L.stream())
    return out


def _dropout_name(t, direction):
    return f'u3d_dropout_{direction}' + ('_b16' if t.dtype == torch.bfloat16 else '')


class _DropoutFn(torch.autograd.Function):
    """y = x . M / (1 - p) with M = the mask of ``key`` over (row, column) (csrc/dropout.h); nothing is saved but the key -- backward
    regenerates the mask.  The tensor keeps its type: fp32, or bf16 under dense16.FLOW (the attention output)."""

    @staticmethod
    def forward(ctx, x, p, key):
        x = x.contiguous()
        ctx.p, ctx.key = p, key
        return _dropout_pass(_dropout_name(x, 'fwd'), x, p, key)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        return _dropout_pass(_dropout_name(dy, 'bwd'), dy, ctx.p, ctx.key), None, None


def dropout(x: torch.Tensor, p: float, key) -> torch.Tensor:
    """Dropout of a 2-D tensor [n, C] (fp32: C % 4 == 0; bf16: C % 8 == 0) with probability ``p`` and the mask of ``key = (seed,
    offset)``: the same key gives the same mask (``ops.dropout_mask_rows`` dumps it).  One launch each way."""
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.bfloat16):
        raise L.U3DError('dropout: a 2-D fp32 or bf16 tensor is expected')
    return _DropoutFn.apply(x, float(p), (int(key[0]), int(key[1])))


class _MLPFn(torch.autograd.Function):
    """z = act(x W1^T + b1) W2^T + b2.  Fused (ReLU always, GELU under FUSE_GELU): bias and activation live in the first GEMM's
    epilogue (``flow.ffn``), the activation's derivative in the epilogue of the GEMM that produces the hidden gradient -- no
    elementwise kernels.  Under dense16.FLOW the hidden tensors (and their gradients) exist in bf16 only; z is fp32.
    ``drop = (p, key)``: dropout on the hidden activation (the reference's FFN, unidet3d/encoder.py:55-61).  The dropped tensor is what
    the second Linear reads and what is saved for its weight gradient; the hidden gradient is masked and scaled before the activation's
    derivative, which reads the saved activation ``a`` (ReLU: the undropped one -- a dropped element's gradient is already zero -- so
    the fused epilogue still applies) or pre-activation ``h`` (GELU).  The two GEMMs then run as calls of their own with the dropout
    pass between them."""

    @staticmethod
    def forward(ctx, flow, x, w1, b1, w2, b2, act, drop=None):
        x = x.contiguous()
        xa = flow.operand(x)
        w1c, w2c = w1.contiguous(), w2.contiguous()
        ctx.flow = flow
        ctx.wt1, ctx.wt2 = _wt_of(w1c), _wt_of(w2c)
        ctx.wtp1, ctx.wtp2 = _planes_of(ctx.wt1), _planes_of(ctx.wt2)
        p1, p2 = _planes_of(w1c), _planes_of(w2c)
        ctx.fused = act != ACT_GELU or (FUSE_GELU and not flow.act16)
        ctx.drop = drop
        if drop is not None:                            # GEMM (+bias, activation) -> dropout pass -> plain GEMM
            if act == ACT_GELU:
                ctx.fused = False
                h = flow.nt(xa, w1c, b1, out_bf16=True, planes=p1)
                a = _gelu_pass(flow.gelu[0], h)
                a = _dropout_pass(_dropout_name(a, 'fwd'), a, *drop)          # the undropped activation is not needed again
            else:
                h = None
                a = flow.relu_nt(xa, w1c, b1, p1)
                a = _dropout_pass(_dropout_name(a, 'fwd'), a, *drop)
            z = flow.nt(a, w2c, b2, planes=p2)
        elif ctx.fused:
            h, a, z = flow.ffn(xa, w1c, b1, w2c, b2, act, p1, p2)
        else:                                           # plain GEMM (+bias) -> GELU pass -> plain GEMM
            h = flow.nt(xa, w1c, b1, out_bf16=True, planes=p1)
            a = _gelu_pass(flow.gelu[0], h)
            z = flow.nt(a, w2c, b2, planes=p2)
        ctx.save_for_backward(xa, w1c, w2c, a, h)
        ctx.act, ctx.bias = act, (b1 is not None, b2 is not None)
        ctx.bias_refs = (b1, b2)
        return z

    @staticmethod
    def backward(ctx, dz):
        xa, w1, w2, a, h = ctx.saved_tensors
        flow = ctx.flow
        dz = dz.contiguous()
        dza = flow.operand(dz)
        need = ctx.needs_input_grad[1:]
        dw2, db2 = _weight_grad_overlapped(flow, dza, a, ctx.bias[1] and need[4], w2, ctx.bias_refs[1]) if need[3] else (None, None)
        if ctx.drop is not None:
            # da = dz W2, masked and scaled, then the activation's derivative.  ReLU's derivative is a 0 / 1 factor that commutes with
            # the mask exactly, and [a_dropped > 0] equals relu'(pre) wherever the mask keeps the element: the fused epilogue on the
            # saved (dropped) activation, then the mask.
            if ctx.act == ACT_GELU:
                da = _input_grad(flow, dza, w2, ctx.wt2, ctx.wtp2, out_bf16=True)
                dh = _gelu_pass(flow.gelu[1], _dropout_pass(_dropout_name(da, 'bwd'), da, *ctx.drop), h)
            else:
                da = _input_grad(flow, dza, w2, ctx.wt2, ctx.wtp2, EPI_RELU_MASK, a, out_bf16=True)
                dh = _dropout_pass(_dropout_name(da, 'bwd'), da, *ctx.drop)
        elif ctx.fused:
            epi, aux = (EPI_GELU_MASK, h) if ctx.act == ACT_GELU else (EPI_RELU_MASK, a)
            dh = _input_grad(flow, dza, w2, ctx.wt2, ctx.wtp2, epi, aux, out_bf16=True)
        else:
            dh = _gelu_pass(flow.gelu[1], _input_grad(flow, dza, w2, ctx.wt2, ctx.wtp2, out_bf16=True), h)
        dw1, db1 = _weight_grad_overlapped(flow, dh, xa, ctx.bias[0] and need[2], w1, ctx.bias_refs[0]) if need[1] else (None, None)
        dx = _input_grad(flow, dh, w1, ctx.wt1, ctx.wtp1) if need[0] else None
        if db2 is None and ctx.bias[1] and need[4]:          # a trainable bias on a frozen weight: no TN product to ride along with
            db2 = dz.float().sum(0)
        if db1 is None and ctx.bias[0] and need[2]:
            db1 = dh.float().sum(0)
        return None, dx, dw1, db1, dw2, db2, None, None


def mlp(x, w1, b1, w2, b2, act: str, drop=None) -> torch.Tensor:
    """Linear -> ReLU / GELU -> Linear on 2-D x (d_in, hidden % 16 == 0).  ``drop = (p, (seed, offset))``: dropout on the hidden
    activation, between the activation and the second Linear."""
    if drop is not None:
        drop = (float(drop[0]), (int(drop[1][0]), int(drop[1][1])))
    return _MLPFn.apply(_flow(x, x.shape[1], w1.shape[0]), x, w1, b1, w2, b2, {'relu': ACT_RELU, 'gelu': ACT_GELU}[act], drop)


def _aliases(y, n_out):
    """``y`` as ``n_out`` autograd outputs that share its storage: one per consumer, so that their gradients arrive separately at the
    producing Function's backward -- which sums them while it reads them -- instead of being added by autograd's elementwise kernels"""
    return y if n_out == 1 else (y,) + tuple(y.view_as(y) for _ in range(n_out - 1))


def _grads_in(dys):
    """the incoming gradients of ``_aliases`` outputs: (first, second or None, third or None) of those that arrived"""
    g = [d.contiguous() for d in dys if d is not None]
    if len(g) > 3:
        raise L.U3DError('layer_norm: at most three consumers of the result are summed in the backward kernel')
    return g + [None] * (3 - len(g))


class _LayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x + res) over the last dimension (include/u3d.h K15); the gradient of x and res is the same tensor.  ``n_out`` > 1:
    the result is returned that many times (one output per consumer) and the backward kernel sums their gradients (u3d_layer_norm_bwd_sum).
    Under dense16.FLOW the outputs are (y, ..., y16) -- the bf16 copy, not differentiable, which ``layer_norm`` attaches to every y --
    and backward attaches the copy of dx it writes."""

    @staticmethod
    def forward(ctx, flow, x, res, weight, bias, eps, n_out=1):
        x = x.contiguous()
        s = x
        if res is not None:
            res = res.contiguous()
            s = torch.empty_like(x)
        y, y16, stats = _layer_norm_fwd(flow, x, res, weight, bias, eps, s if res is not None else None)
        ctx.save_for_backward(s, weight, stats)
        ctx.flow = flow
        ctx.has_res = res is not None
        ctx.set_materialize_grads(False)
        ys = _aliases(y, n_out)
        if y16 is None:
            return ys
        ctx.mark_non_differentiable(y16)
        return (ys if n_out > 1 else (ys,)) + (y16,)

    @staticmethod
    def backward(ctx, *dys):
        s, weight, stats = ctx.saved_tensors
        dy, dy2, dy3 = _grads_in(dys[:-1] if ctx.flow.act16 else dys)
        if dy is None:
            return (None,) * 7
        M, C = s.shape
        dx = torch.empty_like(s)
        dx16 = ctx.flow.b16_like(s)
        dg = torch.empty(C, dtype=torch.float32, device=s.device)
        db = torch.empty(C, dtype=torch.float32, device=s.device)
        if M:
            ws = L.scratch(L.lib().u3d_layer_norm_ws_bytes(M, C), s.device)
            L.call('u3d_layer_norm_bwd_sum', L.ptr(s), L.ptr(dy), L.ptr(dy2), L.ptr(dy3), L.ptr(weight), L.ptr(stats), M, C, L.ptr(dx),
                   L.ptr(dx16), L.ptr(dg), L.ptr(db), L.ptr(ws), L.stream())
        else:
            dg.zero_(); db.zero_()
        if dx16 is not None:
            ctx.flow.attach(dx, dx16)
        return None, dx, (dx if ctx.has_res else None), dg, db, None, None


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5, res: torch.Tensor = None, n_out: int = 1):
    """LayerNorm(x + res) for 2-D x [M, C] (C % 4 == 0, C <= 1024).  ``n_out`` in (2, 3): a tuple of that many tensors, all THE result
    (shared storage) -- hand each consumer its own and the backward kernel sums their gradients (no elementwise add passes)."""
    flow = _flow(x, x.shape[1])
    out = _LayerNormFn.apply(flow, x, res, weight, bias, eps, n_out)
    if not flow.act16:
        return out
    *ys, y16 = out
    for y in ys:
        flow.attach(y, y16)
    return ys[0] if n_out == 1 else tuple(ys)


class _LNLinearFn(torch.autograd.Function):
    """(nq, nq16, y) = (LayerNorm(x), its bf16 copy or None, nq W^T + b): the head (out_norm -> out_bboxes.linear,
    unidet3d/encoder.py:187-196).  The Linear and its weight gradient stream nq16 where there is one.  Backward folds the two
    gradient contributions of ``nq`` (its own consumers + this Linear) into the GEMM that produces the second (EPI_ADD), then runs
    the LayerNorm backward once."""

    @staticmethod
    def forward(ctx, flow, x, gamma, beta, eps, weight, bias):
        x = x.contiguous()
        w = weight.contiguous()
        nq, nq16, stats, y = flow.ln_linear(x, gamma, beta, eps, w, bias)
        ctx.save_for_backward(x, gamma, stats, nq if nq16 is None else nq16, w)
        ctx.flow = flow
        ctx.has_bias = bias is not None
        if nq16 is not None:
            ctx.mark_non_differentiable(nq16)
        return nq, nq16, y

    @staticmethod
    def backward(ctx, dnq, _unused, dy):
        x, gamma, stats, nqa, w = ctx.saved_tensors
        dw = db = None
        if dy is not None:
            dy = dy.contiguous()
            dw, db = _weight_grad(ctx.flow, dy, nqa, ctx.has_bias)
            if dnq is None:
                dtot = _input_grad(ctx.flow, dy, w)
            else:                                        # dtot = dy W + dnq in one GEMM
                dtot = _input_grad(ctx.flow, dy, w, epi=EPI_ADD, aux=dnq.contiguous())
        else:
            dtot = dnq.contiguous()
        dx, dg, dbeta = _layer_norm_bwd(x, dtot, gamma, stats)
        return None, dx, dg, dbeta, None, dw, db


def ln_linear(x, gamma, beta, eps, weight, bias):
    """-> (LayerNorm(x), LayerNorm(x) W^T + b) for 2-D x [M, C]."""
    flow = _flow(x, x.shape[1])
    if flow is BF16 and x.shape[1] % 32:                # the fused entry point pads no reduction depth
        flow = FP32
    nq, nq16, y = _LNLinearFn.apply(flow, x, gamma, beta, eps, weight, bias)
    if nq16 is not None:
        flow.attach(nq, nq16)
    return nq, y


class LayerNorm(torch.nn.LayerNorm):
    """``nn.LayerNorm(d_model)`` of the reference (same parameters / state_dict keys) on the HIP kernels, optionally fused with the
    residual add in front of it."""

    def forward(self, x, res=None, n_out=1):
        return layer_norm(x, self.weight, self.bias, self.eps, res, n_out)
