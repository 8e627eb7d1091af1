"""Sparse-voxel tensor + layers over the gfx950 kernels (host side of the boundary).

Mirrors the subset of ``spconv.pytorch`` the reference uses
(unidet3d/spconv_unet.py:5-7,34-72,146-192; unidet3d/unidet3d.py:96-111,353-354):
``SparseConvTensor`` (features / indices / spatial_shape / batch_size /
replace_feature / per-forward ``indice_dict`` rulebook cache keyed by
``indice_key``), ``SparseSequential``, ``SubMConv3d``, ``SparseConv3d``,
``SparseInverseConv3d``; plus the BatchNorm the reference takes from torch
(``nn.SyncBatchNorm`` / ``nn.BatchNorm1d``), spconv's ``SparseMaxPool3d`` /
``SparseAvgPool3d`` on the strided convolution's geometry, ``SparseConvTranspose3d``
(with ``output_padding``), and the two operations a generative decoder puts behind it: ``sparse_add`` (spconv's
``functional.sparse_add``: operands on different voxel sets, result on their union) and ``prune`` / ``SparsePrune``
(MinkowskiEngine's ``MinkowskiPruning``: drop voxels by a mask), and the dense interchange almost every spconv network ends with:
``SparseConvTensor.dense`` / ``SparseConvTensor.from_dense`` / ``ToDense``, and the per-scene operations: ``topk_mask`` / ``prune_topk`` /
``SparseTopKPrune`` (the k best-scored voxels of every scene) and ``global_pool`` / ``SparseGlobalMaxPool`` / ``SparseGlobalAvgPool``.  Same constructor arguments, same parameter names (``weight``,
``bias`` with ``bias=True``) and weight layout ``[C_out, k, k, k, C_in]``.

Every compute step is a call through the C ABI (include/u3d.h); there is no
PyTorch fallback.  Rows must be in canonical order (ascending
((b*X+x)*Y+y)*Z+z) -- which is what ``ops.voxelize`` / ``UniDet3D.collate``
produce.

What a layer leaves for the next one rides on the feature TENSOR (bf16 shadow, ``_u3d_from_conv``, the batch-norm statistics of a
convolution's epilogue, in inference the norm's whole result: ``shadow_of`` / ``stats_of`` / ``activated_of``); ``SparseConvTensor``
carries geometry only (and, in its ``indice_dict``, the ``FusionRun`` of a forward on the fused inference path).  A norm on a sparse tensor is one
call, ``SparseBatchNorm.on``; a convolution layer is: find the geometry, ``_ConvBase._conv``, build the output tensor.

The geometry itself (``OccupancyIndex``, ``Rulebook``, the four rulebook builders, the layer-geometry helpers, the ``indice_dict`` level
cache ``cached_level`` / ``strided_geometry``) moved to ``unidet3d_amd.geometry``; its public names are re-exported here.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from types import SimpleNamespace
from typing import Dict, Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from . import dense
from . import precision as P
from . import account
from . import wgrad_stream as WS
from .geometry import (OccupancyIndex, Rulebook, UpLevel, build_subm_rulebook, build_conv_rulebook, build_convt_rulebook, conv_geometry,
                       output_padding_of, strided_geometry, cached_level, layer_geometry, saved_under, tensor_index, _DOWN_K2S2,
                       UnionLevel, build_union_level, compact_mask, dense_cells, active_cells, cells_coords, scene_offsets,
                       check_scene_order, mark_canonical, is_canonical)
from .geometry import build_down_rulebook, conv_out_shape, convt_out_shape, _geom_array, _TILE_HISTORY      # noqa: F401  (re-exported)
from .wgrad_stream import set_wgrad_overlap, async_dw_ok, join_wgrad_stream, end_of_backward, _ASYNC_DW_SEEN      # noqa: F401  (re-exported)


# ----------------------------------------------------------------------------------------
# convolution (forward / dgrad / wgrad through the C ABI)
# ----------------------------------------------------------------------------------------
def _plan(Cs, Cd, K, n_dst, rows_kernel=False):
    """(rows per wave-tile, offset groups) the kernel wants for this shape (``rows_kernel``: u3d_spconv_gmm_bf16a's own plan)."""
    R, G = ctypes.c_int(0), ctypes.c_int(0)
    fn = L.lib().u3d_spconv_plan_bf16a if rows_kernel else L.lib().u3d_spconv_plan
    if n_dst <= 0 or fn(Cs, Cd, K, n_dst, ctypes.byref(R), ctypes.byref(G)) != 0:
        raise L.U3DError(f'sparse conv: channel combination {Cs}->{Cd} unsupported by the gfx950 kernels')
    return R.value, G.value


# ---- bf16 shadows of the rows the sparse convolutions gather (precision.bf16_rows) ------------------------------------------
# A shadow is an attribute of the fp32 tensor it was rounded from: it travels with that tensor object through autograd (torch keeps
# a tensor's Python object, attributes included, alive as long as the tensor itself) and dies with it; a tensor autograd built by
# ADDING two gradients is a new object without one, and its consumer then gathers the fp32 rows -- same values, same results.
SHADOW_STATS = {'hit': 0, 'miss': 0}


def to_shadow(t: torch.Tensor) -> torch.Tensor:
    """The bf16 shadow of an fp32 [n, C] tensor (C % 32 == 0) as the batch-norm kernels write it: rounded to nearest even, each
    32-channel group in MFMA fragment order -- 8-byte pieces (quad q, half h) at position 2q + h, i.e. the 16 bytes at byte 16 q hold
    channels 4q..4q+3 and 16+4q..16+4q+3 (csrc/bn.hip store_shadow).  Torch ops, for tests and tools."""
    n, C = t.shape
    return t.detach().reshape(n, C // 32, 2, 4, 4).permute(0, 1, 3, 2, 4).to(torch.bfloat16).reshape(n, C).contiguous()


def attach_shadow(t: torch.Tensor, shadow: torch.Tensor):
    t._u3d_shadow = (shadow, t._version)


def rows_only(shadow: torch.Tensor) -> torch.Tensor:
    """A tensor that exists as bf16 rows ONLY (fused inference under ``precision.bf16_rows``: the convolution epilogue wrote a norm's result
    in the one form its reader gathers): a zero-row fp32 placeholder of the same width that carries the rows as its shadow.  It has no
    values to read by accident; ``shadow_of`` hands the rows to a pair-list convolution, every other reader refuses it (``refuse_rows_only``)."""
    t = torch.empty(0, shadow.shape[1], dtype=torch.float32, device=shadow.device)
    t._u3d_rows_only = shadow
    return t


def rows_only_of(t):
    return getattr(t, '_u3d_rows_only', None)


def refuse_rows_only(t, reader: str):
    if not t.shape[0] and getattr(t, '_u3d_rows_only', None) is not None:      # (the placeholder has no rows: everything else leaves at the first test)
        raise L.U3DError(f'{reader}: this tensor exists as bf16 rows only (fused inference wrote it for a sparse convolution that gathers '
                         f'bf16 rows): it has no fp32 values to read')


def shadow_of(t: torch.Tensor):
    e = getattr(t, '_u3d_rows_only', None)
    if e is not None:
        SHADOW_STATS['hit'] += 1
        return e
    e = getattr(t, '_u3d_shadow', None)
    if e is not None and e[1] == t._version and e[0].shape == t.shape and e[0].device == t.device:
        SHADOW_STATS['hit'] += 1
        return e[0]
    SHADOW_STATS['miss'] += 1
    return None


# ---- batch-norm statistics from the convolution epilogue (_EPILOGUE_STATS) ---------------------------------------------------
# The per-tile column sums a convolution launch wrote travel to the norm behind it the way a shadow does: on the output tensor, valid
# for the same object at the same ``_version`` on the same device.  Any other tensor has none, and the norm makes its own pass.
def attach_stats(t: torch.Tensor, partial: torch.Tensor, n_tiles: int):
    t._u3d_stats = (partial, int(n_tiles), t._version)


def stats_of(t: torch.Tensor):
    """(partial float [n_tiles, 2, C], n_tiles) as the producing convolution attached them, or None"""
    e = getattr(t, '_u3d_stats', None)
    if e is not None and e[2] == t._version and e[0].device == t.device:
        return e[:2]
    return None


# ---- batch norm + ReLU from the convolution epilogue (fused inference) ---------------------------------------------------------
# The activated tensor(s) a convolution launch wrote for the norm(s) behind it travel the same way, keyed by the norm module: a norm in
# inference finds its own entry on exactly the tensor it is called on and returns it without a launch.
def attach_activated(t: torch.Tensor, norm, y: torch.Tensor, relu: bool):
    e = getattr(t, '_u3d_act', None)
    if e is None or e[0] != t._version:
        e = t._u3d_act = (t._version, {})
    e[1][norm] = (y, bool(relu))


def activated_of(t: torch.Tensor, norm, relu: bool):
    """``norm``(t) (+ ReLU as ``relu`` says) as the producing convolution(s) wrote it, or None"""
    e = getattr(t, '_u3d_act', None)
    if e is not None and e[0] == t._version:
        hit = e[1].get(norm)
        if hit is not None and hit[1] == bool(relu) and hit[0].device == t.device:
            return hit[0]
    return None


# ---- all weight packs of a model in one launch ------------------------------------------------------------------------------
_PACKED: Dict = {}          # (weight data_ptr, transposed, bf16) -> (buffer, weight tensor, version at pack time)


class WeightPacks:
    """MFMA-fragment-order copies (u3d_weight_pack[_bf16]) of every convolution weight of a module tree, both orientations,
    refreshed by ONE launch (u3d_weight_pack_batch) instead of one pack launch in front of each of the ~90 convolution launches
    of a step.

    Validity contract: in TRAINING mode -- and in eval mode whenever autograd is enabled and a convolution weight requires a gradient
    (fine-tuning with frozen batch norm) -- every ``refresh()`` repacks (one launch per step -- what a changed weight costs anyway),
    and the first eval-mode ``refresh()`` after a training-mode one repacks too, so no optimizer can leave a stale pack behind.
    Otherwise (eval mode) a pack is reused while ``(data_ptr, Tensor._version)`` of every weight is unchanged.  ``_version`` is
    bumped by torch's for-loop / foreach optimizers, ``load_state_dict`` and in-place ops on the parameter, but NOT by
    ``torch.optim.AdamW(fused=True)`` (``_fused_adamw_`` leaves it alone -- round 2's version-keyed cache therefore ran the
    backbone of every bench step after the first on the step-0 weights) and NOT by writes through ``.data``
    (``p.data.copy_()``, mmengine's EMAHook parameter swap): a writer of that kind in eval mode must call ``invalidate()``
    (``UniDet3D.invalidate_weight_packs()``) afterwards."""

    def __init__(self, root: nn.Module):
        self.root = root
        self.convs = [m for m in root.modules() if isinstance(m, _ConvBase) and m.in_channels % 16 == 0 and m.kernel_size != 1]
        self.state = None
        self.bufs: Dict = {}
        self.desc = None
        self.blocks = 0
        self.dirty = False          # a training-mode refresh happened: an optimizer may have stepped since

    def __del__(self):
        for key in list(getattr(self, 'bufs', {})):
            _PACKED.pop(key, None)

    def invalidate(self):
        """Forget the packs (for writers that bypass ``Tensor._version``, see the class docstring)."""
        self.dirty = True
        if self.state is not None:
            self.state = self.state[:2] + (tuple((a, -1) for a, _ in self.state[2]),)
        for key, (buf, w) in self.bufs.items():
            _PACKED[key] = (buf, w, -1)

    def refresh(self):
        if not self.convs:
            return
        bf = P.conv_format()           # 0 fp32 fragments, 1 bf16, 2 three bf16 planes (precision.conv_format)
        dev = self.convs[0].weight.device
        state = (bf, str(dev), tuple((m.weight.data_ptr(), m.weight._version) for m in self.convs))
        # a root kept in eval() (frozen batch norm) while an optimizer steps it: a trainable weight can change behind _version's back
        # (fused AdamW), so every GRAD-ENABLED forward over trainable convolution weights repacks, exactly like training mode.  The
        # test is on requires_grad, not on .grad: zero_grad(set_to_none=True) -- torch's default, and mmengine's order step ->
        # zero_grad -- leaves every .grad None at the time the next forward runs.  Inference (torch.no_grad() /
        # inference_mode, or frozen weights) keeps the version-keyed reuse.
        tuned = torch.is_grad_enabled() and any(m.weight.requires_grad for m in self.convs)
        if state == self.state and not self.root.training and not self.dirty and not tuned:
            return
        self.dirty = bool(self.root.training or tuned)
        rebuild = self.state is None or self.state[0] != bf or self.state[1] != str(dev) or \
            [a for a, _ in self.state[2]] != [a for a, _ in state[2]]
        if rebuild:
            rows, blocks = [], 0
            for key in [k for k in _PACKED if k in self.bufs]:
                _PACKED.pop(key, None)
            self.bufs = {}
            for m in self.convs:
                w = m.weight
                K = m.K
                for transposed, (Cd, Cs) in ((0, (m.out_channels, m.in_channels)), (1, (m.in_channels, m.out_channels))):
                    if Cd % 32 or Cs % 16:
                        continue
                    use_bf = bf if Cs % 32 == 0 else 0
                    buf = torch.empty(_pack_floats(w.numel(), use_bf), dtype=torch.float32, device=dev)
                    nvec = w.numel() // (8 if use_bf else 4)          # threads of the pack kernel (x3: three vectors per thread)
                    rows.append([w.data_ptr(), buf.data_ptr(), Cd, K, Cs, transposed, int(use_bf), blocks])
                    blocks += (nvec + 255) // 256
                    self.bufs[(w.data_ptr(), transposed, use_bf)] = (buf, w)
            self.desc = L.h2d(rows, torch.int64, dev)
            self.blocks = blocks
        L.call('u3d_weight_pack_batch', L.ptr(self.desc), self.desc.shape[0], self.blocks, L.stream())
        for key, (buf, w) in self.bufs.items():
            _PACKED[key] = (buf, w, w._version)
        self.state = state


_GMM_ENTRY = {0: ('u3d_weight_pack', 'u3d_spconv_gmm'), 1: ('u3d_weight_pack_bf16', 'u3d_spconv_gmm_bf16'), 2: ('u3d_weight_pack_x3', 'u3d_spconv_gmm_x3')}


def _pack_floats(numel: int, fmt: int) -> int:
    """size of a packed weight buffer in floats: fp32 fragments, bf16 (half), three bf16 planes (one and a half)"""
    return {0: numel, 1: numel // 2, 2: numel * 3 // 2}[fmt]


# Tile-stationary SubM kernel (csrc/spconv_ts.hip; round 6) for the three-plane fp32 path wherever
# u3d_spconv_ts_plan has a shape for it.  OFF by default: correct (tables bit-exact, fp32-level errors, tests/test_gpu_kernels.py) but
# measured BEHIND the pair-list kernels at every real layer shape of cfg2 (level 1, 32 -> 32: 148 us against 128; level 2, 64 -> 64:
# 165 against 112; DESIGN.md 4.15 has the ablations and the cycle trace that say why).  U3D_CONV_TS=1 / set_conv_ts(True) turns it on.
_CONV_TS = os.environ.get('U3D_CONV_TS', '0') == '1'
# Register-stationary form (spconv_rs_k: weights of a 32 x 32 block in registers, persistent workgroups): U3D_CONV_RS=1 / set_conv_rs
_CONV_RS = os.environ.get('U3D_CONV_RS', '0') == '1'
_RS_MIN_ROWS = int(os.environ.get('U3D_CONV_RS_MIN_ROWS', '40000'))      # below that a level cannot feed one workgroup per CU
_RS_MAX_BLOCKS = int(os.environ.get('U3D_CONV_RS_MAX_BLOCKS', '8'))      # Cs/32 x Cd/32 block launches per convolution at most
# bf16 operands from bf16 rows (BASELINE configs[2]): the one-plane form spconv_rsb_k; U3D_CONV_RS_BF16=1 / set_conv_rs_bf16
_CONV_RS_BF16 = os.environ.get('U3D_CONV_RS_BF16', '0') == '1'


def _flag_toggle(name: str):
    """(setter returning the previous value, context manager) of the boolean module flag ``name``.  The value stays in this module's
    globals, where ``_conv_route`` reads it at call time and tests / tools patch it."""
    def set_flag(on: bool) -> bool:
        prev, globals()[name] = globals()[name], bool(on)
        return prev

    @contextlib.contextmanager
    def flag(on: bool):
        prev = set_flag(on)
        try:
            yield
        finally:
            set_flag(prev)
    return set_flag, flag


set_conv_ts, conv_ts = _flag_toggle('_CONV_TS')
set_conv_rs, conv_rs = _flag_toggle('_CONV_RS')
set_conv_rs_bf16, conv_rs_bf16 = _flag_toggle('_CONV_RS_BF16')
# Fused inference: in eval mode under torch.no_grad() the pair-list convolutions write the batch norm + ReLU of the
# norm(s) that read their result on the way out of the LDS tile (u3d_spconv_gmm_ep), and the U-Net's concat buffer directly.  Same bits
# as the unfused path.  Under ``precision.bf16_rows`` the epilogue writes every norm result whose only reader is a planned convolution as
# bf16 rows, the shadow u3d_bn_apply writes, and nothing else (``rows_only``): the reader gathers them with the bf16-row kernel, as on the
# unfused path.  Three states: None (the default) = on, except under ``precision.bf16_rows`` -- there the default stays
# the unfused sequence (tests/test_fused_inference_cpu.py pins it; the measurements are in DESIGN.md 4.28); True = on everywhere; False = off.
# U3D_FUSED_INFERENCE=1 / 0, set_fused_inference(True / False / None).
_FUSED_INFERENCE = {'1': True, '0': False}.get(os.environ.get('U3D_FUSED_INFERENCE', ''))


def set_fused_inference(on):
    """True / False / None (module comment above); returns the previous state"""
    global _FUSED_INFERENCE
    prev, _FUSED_INFERENCE = _FUSED_INFERENCE, None if on is None else bool(on)
    return prev


@contextlib.contextmanager
def fused_inference(on):
    prev = set_fused_inference(on)
    try:
        yield
    finally:
        set_fused_inference(prev)


def fused_inference_on() -> bool:
    return (not P.bf16_rows()) if _FUSED_INFERENCE is None else _FUSED_INFERENCE


def fusion_active(*modules) -> bool:
    """The one condition of the fused inference path: toggle on, no autograd, none of ``modules`` in training mode, and none of the
    experimental kernels ('rs' / 'ts' / 'rsb') selected -- ``_conv_route`` then sends every convolution to the pair-list kernels."""
    return (fused_inference_on() and not torch.is_grad_enabled() and not (_CONV_TS or _CONV_RS or _CONV_RS_BF16)
            and not any(m.training for m in modules))


def _ts_plan(Cs, Cd, n):
    T, H = ctypes.c_int(0), ctypes.c_int(0)
    if L.lib().u3d_spconv_ts_plan(Cs, Cd, n, ctypes.byref(T), ctypes.byref(H)) != 0:
        return None
    return T.value, H.value


def _conv_route(Cs, Cd, n_dst, rb, bf, has_rows, want_stats):
    """Which kernel runs a convolution of ``n_dst`` > 0 dst rows, decided here and nowhere else: (route, operand format, plan).
      'rsb'    register-stationary, bf16 rows (u3d_spconv_rs_bf16a); plan = H, halo rows per pass.  Writes no statistics, asked or not;
      'rs'     register-stationary, three planes (u3d_spconv_rs_x3); plan = H;
      'ts'     tile-stationary, three planes (u3d_spconv_ts_x3) where u3d_spconv_ts_plan has a shape; plan = (T, H);
      'pairs'  the pair-list kernels (_GMM_ENTRY, or u3d_spconv_gmm_bf16a on bf16 rows); plan = (R, G, gathers bf16 rows).  Source
               channel counts that are not a multiple of 32 (the 6 -> 32 input convolution, padded to 16) stay on the fp32 kernel.
    The first three are SubM-only experiments behind their toggles, tried in that order; only the pair kernels' epilogue can write the
    batch-norm statistics, so 'rs' / 'ts' step aside when those are wanted (``want_stats`` under _EPILOGUE_STATS).
    They read ``rb.coords`` / ``rb.index`` as "the 27 neighbours of SubM k=3, dilation 1" (u3d_subm_halo): a general or dilated rulebook
    (``build_conv_rulebook``) must never set them -- it would get that layer's neighbours, not its own -- and so always lands on 'pairs'."""
    bf = int(bf)
    subm32 = rb.coords is not None and Cs % 32 == 0
    rs_shape = subm32 and Cd % 32 == 0 and n_dst >= _RS_MIN_ROWS and (Cs // 32) * (Cd // 32) <= _RS_MAX_BLOCKS
    if _CONV_RS_BF16 and has_rows and bf == P.FMT_BF16 and rs_shape:
        return 'rsb', bf, int(os.environ.get('U3D_RSB_H', '448'))
    if bf == P.FMT_X3 and not (want_stats and _EPILOGUE_STATS):
        if _CONV_RS and rs_shape:
            return 'rs', bf, int(os.environ.get('U3D_RS_H', '320'))
        ts = _ts_plan(Cs, Cd, n_dst) if _CONV_TS and subm32 else None
        if ts is not None:
            return 'ts', bf, ts
    if Cs % 32:
        bf = P.FMT_FP32
    # gather the bf16 shadow: same packed weights, u3d_spconv_gmm_bf16a and its own plan -- where that kernel has the width; elsewhere the
    # fp32 rows are gathered and rounded as the operands are formed (same values, same results)
    rows = has_rows and bf == P.FMT_BF16 and bool(L.lib().u3d_spconv_gmm_bf16a_supported(Cs, Cd))
    return 'pairs', bf, _plan(Cs, Cd, rb.K, n_dst, rows) + (rows,)


def _packed_weight(weight, transposed, fmt, Cd, K, Cs, device):
    """``weight`` in MFMA-fragment order for format ``fmt``: the copy WeightPacks.refresh() packed with all the model's weights while
    it is current, else packed here by a launch of its own."""
    hit = _PACKED.get((weight.data_ptr(), int(transposed), fmt))
    if hit is not None and hit[2] == weight._version and hit[1].device == device:
        return hit[0]
    wp = torch.empty(_pack_floats(weight.numel(), fmt), dtype=torch.float32, device=device)
    L.call(_GMM_ENTRY[fmt][0], L.ptr(weight), L.ptr(wp), Cd, K, Cs, int(transposed), L.stream())
    return wp


def _gmm(src, weight, transposed, rb, gather, scatter, role, n_dst, addend, flops, bf=0, stats=None, src_rows_bf16=None):
    """weight: the layer's [C_out, K, C_in] tensor; transposed=True runs the input-gradient (dst channels = C_in).
    ``stats`` (an empty dict of ``sparse_conv``'s, or None): asks the kernel's epilogue for the per-tile column sums of dst that the
    batch norm behind this convolution needs (``partial`` float [n_tiles, 2, Cd], ``n_tiles``).  ONE rule: it is filled only by a
    pair-list launch that gathers fp32 rows, under _EPILOGUE_STATS, with a single offset group; every other launch leaves it EMPTY and
    the norm makes its own pass (offsets split over groups: deep levels of a few thousand rows; bf16 rows; the 'rsb' / 'rs' / 'ts' kernels).
    ``bf``: operand format (precision.conv_format: 0 fp32 MFMAs, 1 bf16 operands, 2 fp32 products from three bf16 planes).
    ``src_rows_bf16``: the bf16 shadow of ``src`` (``shadow_of``) -- the launch then gathers those rows.
    Which kernel runs: ``_conv_route``; its packed weight: ``_packed_weight``."""
    Cs, Cd = src.shape[1], (weight.shape[2] if transposed else weight.shape[0])
    dst = torch.empty(n_dst, Cd, dtype=torch.float32, device=src.device)
    if not n_dst:
        return dst
    if not src.shape[0]:        # an empty source level (a strided convolution without output rows, read back by its inverse / input gradient): no pairs
        return dst.zero_() if addend is None else dst.copy_(addend)
    route, fmt, plan = _conv_route(Cs, Cd, n_dst, rb, bf, src_rows_bf16 is not None, stats is not None)
    if _PROFILE_FLOPS:      # N(Cs+Cd)s + 2P*idx + K*Cs*Cd*s  (s = 4 B, idx = 4 B)
        account.add('conv_gmm', flops, 4.0 * (src.shape[0] * Cs + n_dst * Cd) + 8.0 * rb.total_pairs + 4.0 * rb.K * Cs * Cd)
    wp = _packed_weight(weight, transposed, fmt, Cd, rb.K, Cs, src.device)      # (the tensor, held until the launch below is queued)
    if route == 'pairs':
        R, G, rows = plan
        ws = torch.empty(G * n_dst * Cd, dtype=torch.float32, device=src.device) if G > 1 else None
        tiles = rb.tile_starts(role, R)
        if rows:
            L.call('u3d_spconv_gmm_bf16a', L.ptr(src_rows_bf16), src.shape[0], L.ptr(wp), L.ptr(gather), L.ptr(scatter), L.ptr(tiles),
                   rb.K, rb.cap, Cs, Cd, n_dst, R, G, L.ptr(addend), L.ptr(dst), L.ptr(ws), float(flops), L.stream())
        else:
            partial = None
            if stats is not None and G == 1 and _EPILOGUE_STATS:
                n_tiles = (n_dst + R - 1) // R
                partial = torch.empty(n_tiles, 2, Cd, dtype=torch.float32, device=src.device)
                stats.update(partial=partial, n_tiles=n_tiles)
            L.call(_GMM_ENTRY[fmt][1], L.ptr(src), src.shape[0], L.ptr(wp), L.ptr(gather), L.ptr(scatter), L.ptr(tiles),
                   rb.K, rb.cap, Cs, Cd, n_dst, R, G, L.ptr(addend), L.ptr(dst), L.ptr(ws), L.ptr(partial), float(flops), L.stream())
    elif route == 'ts':
        T, H = plan
        nhalo, halo, loc, pmask = rb.halo(T, H)
        L.call('u3d_spconv_ts_x3', L.ptr(src), n_dst, L.ptr(wp), L.ptr(nhalo), L.ptr(halo), L.ptr(loc), L.ptr(pmask), T, H, int(transposed),
               Cs, Cd, L.ptr(addend), L.ptr(dst), float(flops), L.stream())
    else:
        nhalo, halo, loc, _pm = rb.halo(64, plan)
        fn, rows = ('u3d_spconv_rs_bf16a', src_rows_bf16) if route == 'rsb' else ('u3d_spconv_rs_x3', src)
        L.call(fn, L.ptr(rows), n_dst, L.ptr(wp), L.ptr(nhalo), L.ptr(halo), L.ptr(loc), plan, int(transposed),
               Cs, Cd, L.ptr(addend), L.ptr(dst), int(os.environ.get('U3D_RS_WGS', '0')), float(flops), L.stream())
    return dst


_PROFILE_FLOPS = False      # bench.py turns this on so that launches carry exact algorithmic flops
# Batch-norm statistics from the convolution epilogue (per-tile column sums, no pass over the conv output): built and tested
# (tests/test_gpu_kernels.py), but OFF by default -- measured on MI355X at cfg2 (round 3, visit C): no time gained (32.60 vs 32.62
# ms/step: 21 statistics passes of ~5 us saved, paid for in the convolution epilogues), 0.9 GB/step less HBM traffic, and the
# fp32 per-tile sums of x^2 make the backbone gradients 35x less accurate (L2 error vs the fp64 oracle on the same activation
# pattern 6.2e-4 instead of 1.8e-5: var = E[x^2] - mean^2 is taken through ~90 ill-conditioned batch-norm backwards).  The norm's
# own pass accumulates in fp64.  U3D_EPILOGUE_STATS=1 turns it on.
_EPILOGUE_STATS = os.environ.get('U3D_EPILOGUE_STATS', '0') == '1'


def set_profile_flops(on: bool):
    """Launches carry their algorithmic flops to the C side (HIP-event timing per kernel family) and are booked in
    ``account`` (sparse conv here, dense GEMMs and attention in dense.py / encoder.py)."""
    global _PROFILE_FLOPS
    _PROFILE_FLOPS = bool(on)
    dense.set_profile_flops(on)
    account.enable(on)


def _roles(rb: Rulebook, mode: str, transposed: bool = False):
    """(gather rows, scatter rows, role of the scattered side, its row count) of a launch over ``rb``.  mode 'fwd' reads pair_in rows
    and writes pair_out rows (SubM and strided conv), 'inv' the other way round (SparseInverseConv3d); the input gradient
    (``transposed``) swaps them once more.  The weight gradient walks the forward's roles."""
    if (mode == 'fwd') != transposed:
        return rb.pair_in, rb.pair_out, 'out', rb.n_out
    return rb.pair_out, rb.pair_in, 'in', rb.n_in


class _SparseConvFn(torch.autograd.Function):
    """mode: 'fwd' or 'inv' (``_roles``).  ``stats``: ``_gmm``'s, a dict that ``sparse_conv`` owns."""

    @staticmethod
    def forward(ctx, src, weight, rb: Rulebook, mode: str, addend, stats=None):
        cout, cin = weight.shape[0], weight.shape[-1]
        w = weight.reshape(cout, rb.K, cin)
        src = src.contiguous()
        g, s, role, n_dst = _roles(rb, mode)
        flops = 2.0 * rb.total_pairs * cin * cout if _PROFILE_FLOPS else 0.0
        ctx.bf = P.conv_format()
        ctx.rows = ctx.bf == P.FMT_BF16 and P.bf16_rows() and cin % 32 == 0
        ctx.src_shadow = shadow_of(src) if ctx.rows else None          # bf16 rows of src: gathered here and by the weight gradient
        dst = _gmm(src, w.contiguous(), False, rb, g, s, role, n_dst, None if addend is None else addend.contiguous(), flops, ctx.bf,
                   stats, ctx.src_shadow)
        ctx.save_for_backward(src, weight)
        ctx.rb, ctx.mode, ctx.has_addend = rb, mode, addend is not None
        return dst

    @staticmethod
    def backward(ctx, dout):
        src, weight = ctx.saved_tensors
        rb, mode = ctx.rb, ctx.mode
        cout, cin = weight.shape[0], weight.shape[-1]
        dout = dout.contiguous()
        dsrc = dw = None
        flops = 2.0 * rb.total_pairs * cin * cout if _PROFILE_FLOPS else 0.0
        side = None
        dout_shadow = shadow_of(dout) if ctx.bf == P.FMT_BF16 and P.bf16_rows() and cout % 32 == 0 else None
        if ctx.needs_input_grad[1] and not (dout.shape[0] and src.shape[0]):
            dw = torch.zeros_like(weight)        # an empty level on either side: no pairs, no launch
        elif ctx.needs_input_grad[1]:
            dw = torch.empty_like(weight)
            rx, rg, role, n_dy = _roles(rb, mode)
            if _PROFILE_FLOPS:
                account.add('conv_wgrad', flops, 4.0 * (src.shape[0] * cin + n_dy * cout) + 8.0 * rb.total_pairs + 4.0 * rb.K * cin * cout)
            Tw = L.lib().u3d_spconv_wgrad_tile_rows(rb.K, n_dy, cin, cout)
            ws_bytes = L.lib().u3d_spconv_wgrad_ws_bytes(rb.K, n_dy, cin, cout)
            ts = rb.tile_starts(role, Tw, wgrad=(cin, cout))
            # the weight-gradient walk is bound by its row gathers: bf16 operands pay off only where the matrix
            # work is a visible share -- measured (tools/prof_wgrad.py): 32x32 channels 179 us fp32 vs 221 us bf16, 64x64 150 vs 104
            wg = 'u3d_spconv_wgrad_bf16' if ctx.bf == P.FMT_BF16 and cin * cout >= 64 * 64 else 'u3d_spconv_wgrad'
            xw, gw = src, dout
            if ctx.src_shadow is not None and dout_shadow is not None and L.lib().u3d_spconv_wgrad_rows_supported(cin, cout):
                # both operands exist as bf16 rows: whole-row gathers, LDS transpose reads, bf16 MFMAs over 32 pairs (spconv_wgrad_rows.hip)
                wg, xw, gw = 'u3d_spconv_wgrad_rows', ctx.src_shadow, dout_shadow

            def launch():
                ws = L.scratch(ws_bytes, weight.device)       # keyed by stream: on the side stream, that stream's own workspace
                L.call(wg, L.ptr(xw), xw.shape[0], L.ptr(gw), L.ptr(rx), L.ptr(rg), L.ptr(ts),
                       rb.K, rb.cap, n_dy, Tw, cin, cout, L.ptr(dw), L.ptr(ws), float(flops), L.stream())

            overlap = WS.mode() if ctx.needs_input_grad[0] else 0       # (the first convolution has no input gradient to run next to)
            if overlap == 2 and not async_dw_ok(weight):
                overlap = 1      # autograd will ADD dw to an existing .grad (or feed it to another node / a hook) on this stream right away: join first
            if overlap:
                side, _ = WS.run_on_side_stream(weight.device, launch, reads=(xw, gw, dw, ts, rx, rg))
                if overlap == 2:
                    WS.queue_join(weight.device)
                    side = None
            else:
                launch()
        if ctx.needs_input_grad[0]:
            g, s, role, n_dst = _roles(rb, mode, transposed=True)
            dsrc = _gmm(dout, weight.reshape(cout, rb.K, cin).contiguous(), True, rb, g, s, role, n_dst, None, flops, ctx.bf,
                        None, dout_shadow)
        if side is not None:          # mode 1: joined only now, after the input gradient was queued next to it
            torch.cuda.current_stream().wait_stream(side)
        return dsrc, dw, None, None, (dout if ctx.has_addend else None), None


def _conv_check(src, weight, rb: Rulebook, mode: str, addend):
    """What must agree before a convolution over ``rb`` is launched: the feature rows with the rulebook's source level for ``mode``, their
    width with the weight's C_in, an addend with the result.  The kernels read through bounded buffers, so a rulebook of another level
    (a SubM ``indice_key`` met again on other rows, an inverse layer fed from the wrong level) would not fault: rows past the tensor
    would come back as zeros and the result would be silently wrong."""
    if mode not in ('fwd', 'inv'):
        raise L.U3DError(f"sparse_conv: mode must be 'fwd' or 'inv', got {mode!r}")
    where = '' if rb.tag is None else f' (rulebook {rb.tag!r})'
    n_src, n_dst = (rb.n_in, rb.n_out) if mode == 'fwd' else (rb.n_out, rb.n_in)
    if src.dim() != 2 or src.shape[0] != n_src:
        raise L.U3DError(f"sparse_conv: {tuple(src.shape)} features, the rulebook has {n_src} source rows in mode '{mode}'{where}: it was "
                         f'built for another level')
    if src.shape[1] != weight.shape[-1]:
        raise L.U3DError(f'sparse_conv: the features have {src.shape[1]} channels, the weight takes {weight.shape[-1]}{where}')
    if addend is not None and tuple(addend.shape) != (n_dst, weight.shape[0]):
        raise L.U3DError(f'sparse_conv: the addend is {tuple(addend.shape)}, the result [{n_dst}, {weight.shape[0]}]{where}')


def sparse_conv(src, weight, rb, mode='fwd', addend=None, want_stats=False):
    """``want_stats``: a batch norm in training mode reads the result: what the launch wrote for it (``_gmm``) rides on the returned
    tensor (``stats_of``)."""
    st = {} if want_stats else None
    refuse_rows_only(src, 'sparse_conv')
    _conv_check(src, weight, rb, mode, addend)
    dst = _SparseConvFn.apply(src, weight, rb, mode, addend, st)
    if st:
        attach_stats(dst, st['partial'], st['n_tiles'])
    if P.bf16_rows():
        dst._u3d_from_conv = True      # the batch norm behind this output hands its gradient back with a bf16 shadow (bf16_rows)
    return dst


# ---- bias of a convolution layer (csrc/sparse_bias.hip) --------------------------------------------------------------------------
def _bias_check(t: torch.Tensor, what: str, bias=None):
    refuse_rows_only(t, what)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise L.U3DError(f'{what}: rows must be fp32 [n, C], got {t.dtype} {tuple(t.shape)}')
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (t.shape[1],) or bias.device != t.device):
        raise L.U3DError(f'{what}: the bias must be fp32 [{t.shape[1]}] on {t.device}, got {bias.dtype} {tuple(bias.shape)} on {bias.device} '
                         f'(the bias add stays fp32 under every operand format)')


def bias_add_(y: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """y += bias over every row, in place (u3d_bias_add: the bits of the fp32 y + b); no rows, no launch"""
    _bias_check(y, 'bias_add', bias)
    if y.shape[0]:
        L.call('u3d_bias_add', L.ptr(y), L.ptr(bias), y.shape[0], y.shape[1], L.stream())
    return y


def bias_grad(dy: torch.Tensor) -> torch.Tensor:
    """column sums of dy [n, C] (u3d_bias_grad: fp64 partials in a fixed order, one rounding); no rows, no launch and zeros"""
    _bias_check(dy, 'bias_grad')
    dy = dy.contiguous()
    n, C = dy.shape
    if not n:
        return torch.zeros(C, dtype=torch.float32, device=dy.device)
    db = torch.empty(C, dtype=torch.float32, device=dy.device)
    w = L.ws(L.lib().u3d_bias_grad_ws_bytes(n, C), dy.device)
    L.call('u3d_bias_grad', L.ptr(dy), n, C, L.ptr(db), L.ptr(w), L.stream())
    return db


class _BiasFn(torch.autograd.Function):
    """y + bias in place on a convolution's fresh result (nothing in ``_SparseConvFn`` saves its output).  The backward hands dy on
    untouched and sums it only when the bias asks for a gradient -- then always, whatever the weight does."""

    @staticmethod
    def forward(ctx, y, bias):
        ctx.mark_dirty(y)
        return bias_add_(y, bias)

    @staticmethod
    def backward(ctx, dy):
        return dy, (bias_grad(dy) if ctx.needs_input_grad[1] else None)


def sparse_bias(y: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """(conv [+ addend]) + bias, fp32 under every operand format.  The result carries nothing for the layer behind it: no epilogue
    statistics (they would be those of the value before the bias; the layer asks for none), no bf16 shadow and no ``_u3d_from_conv``
    mark -- its reader takes the path of any tensor without one."""
    if not y.is_contiguous():
        raise L.U3DError('sparse_bias: non-contiguous convolution result')
    out = _BiasFn.apply(y, bias)
    for attr in ('_u3d_from_conv', '_u3d_stats', '_u3d_shadow'):
        if hasattr(out, attr):
            delattr(out, attr)
    return out


_EP_FORMATS = None


def _ep_writes_rows() -> bool:
    """u3d_spconv_gmm_ep_formats() bit 1, asked once: only a library that reports it is handed U3D_EP_BF16_ROWS (one from before the flag
    would read it as "ReLU" and write fp32 into the bf16 buffer)"""
    global _EP_FORMATS
    if _EP_FORMATS is None:
        _EP_FORMATS = int(L.lib().u3d_spconv_gmm_ep_formats())
    return bool(_EP_FORMATS & 2)


def sparse_conv_fused(src, weight, rb, mode, addend, raw, acts):
    """Forward convolution of the fused inference path (no autograd): u3d_spconv_gmm_ep.
    ``raw``: (fp32 buffer [n_dst, ld], first column) that receives dst, or None for no raw output; ``acts``: up to two
    (buffer [n_dst, ld], first column, scale, shift, relu) that receive relu(dst * scale + shift) -- scale / shift indexed by the buffer's
    own columns; a bfloat16 buffer receives bf16 rows (``to_shadow``'s layout, U3D_EP_BF16_ROWS), an fp32 one the values.  Same kernel,
    operand format and offset groups as ``_gmm`` takes for this shape, so dst has the bits ``sparse_conv`` returns.  A ``rows_only`` source
    is gathered as bf16 rows (fmt 3) under the bf16-row kernel's own plan, or refused where the launch would gather anything else."""
    cout, cin = weight.shape[0], weight.shape[-1]
    w = weight.reshape(cout, rb.K, cin).contiguous()
    only = rows_only_of(src)
    src = src.contiguous()
    g, s, role, n_dst = _roles(rb, mode)
    if not n_dst:
        return
    flops = 2.0 * rb.total_pairs * cin * cout if _PROFILE_FLOPS else 0.0
    bf = P.conv_format()
    shadow = shadow_of(src) if (bf == P.FMT_BF16 and P.bf16_rows() and cin % 32 == 0) or only is not None else None
    n_src = src.shape[0] if only is None else only.shape[0]
    route, fmt, plan = _conv_route(cin, cout, n_dst, rb, bf, shadow is not None, False)
    if route != 'pairs':
        raise L.U3DError(f'fused inference: the {route!r} kernel has no output epilogue')
    R, G, rows = plan
    if not rows:
        refuse_rows_only(src, f'sparse_conv_fused ({cin} -> {cout} channels, operand format {fmt})')
    if _PROFILE_FLOPS:
        account.add('conv_gmm', flops, 4.0 * (n_src * cin + n_dst * cout) + 8.0 * rb.total_pairs + 4.0 * rb.K * cin * cout)
    wp = _packed_weight(w, False, fmt, cout, rb.K, cin, src.device)
    ep = L.ConvEpilogue()
    if raw is not None:
        ep.raw, ep.raw_ld, ep.raw_col = raw[0].data_ptr(), raw[0].shape[1], raw[1]
    ep.n_act = len(acts)
    for j, (buf, col, scale, shift, relu) in enumerate(acts):
        flags = L.EP_RELU if relu else 0
        if buf.dtype == torch.bfloat16:
            if not _ep_writes_rows():
                raise L.U3DError('fused inference: this kernel library writes no bf16-row activated outputs: rebuild it')
            flags |= L.EP_BF16_ROWS
        ep.act[j], ep.act_ld[j], ep.act_col[j] = buf.data_ptr(), buf.shape[1], col
        ep.scale[j], ep.shift[j], ep.relu[j] = L.ptr(scale), L.ptr(shift), flags
    ws = torch.empty(G * n_dst * cout, dtype=torch.float32, device=src.device) if G > 1 else None
    tiles = rb.tile_starts(role, R)
    L.call('u3d_spconv_gmm_ep', 3 if rows else fmt, L.ptr(shadow if rows else src), n_src, L.ptr(wp), L.ptr(g), L.ptr(s), L.ptr(tiles),
           rb.K, rb.cap, cin, cout, n_dst, R, G, L.ptr(None if addend is None else addend.contiguous()), L.ptr(ws), None, ctypes.byref(ep),
           float(flops), L.stream())


FUSE_KEY = '__fused_inference__'       # indice_dict entry of a forward on the fused inference path: its FusionRun


class FusionRun:
    """One forward pass on the fused inference path: the plan (``spconv_unet.fusion_plan``: which norm(s) read each convolution's
    result, which column block of a U-Net concat buffer it writes) and the buffers of this pass.  It rides in the ``indice_dict`` all
    sparse tensors of a forward share; ``_ConvBase._conv`` looks its layer up there."""

    def __init__(self, plan):
        self.plan = plan
        self.cats: Dict = {}
        self.used = False                  # set when the planned U-Net starts its forward: a pass's buffers are never handed out twice
        self._rows: Dict = {}

    def rows(self, norm) -> bool:
        """``norm``'s result is written as bf16 rows and as nothing else: bf16 operands with ``precision.bf16_rows``, the only reader a
        planned convolution (``FusionPlan.rows_capable``) of a shape the bf16-row kernel has -- that launch then gathers fmt 3 under
        the bf16-row plan, exactly what the unfused path runs on the shadow u3d_bn_apply wrote.  In every other mode: never."""
        hit = self._rows.get(norm)
        if hit is None:
            hit = self._rows[norm] = bool(
                P.conv_format() == P.FMT_BF16 and P.bf16_rows() and self.plan.rows_capable(norm)
                and L.lib().u3d_spconv_gmm_bf16a_supported(norm.num_features, self.plan.norms[norm].reader.out_channels))
        return hit

    def cat(self, owner, n: int, device):
        """(raw, activated) [n, 2c] buffers of U-Net level ``owner``: the concatenation its tail blocks read, and the first tail norm of it
        (bf16 rows where ``rows`` says so)"""
        if owner not in self.cats:
            c = self.plan.cats[owner]
            self.cats[owner] = (torch.empty(n, c.width, dtype=torch.float32, device=device),
                                torch.empty(n, c.width, dtype=torch.bfloat16 if self.rows(c.norm) else torch.float32, device=device))
        return self.cats[owner]

    def conv(self, layer, cp, x: 'SparseConvTensor', rb: Rulebook, mode: str, addend=None) -> torch.Tensor:
        src, weight = _pad16(x.features), layer._w16()
        n_dst, Cd, dev = _roles(rb, mode)[3], layer.out_channels, src.device
        if cp.raw is None:                 # only the norm behind this layer reads the result
            raw, dst = None, torch.empty(0, Cd, dtype=torch.float32, device=dev)
            dst._u3d_no_raw = True
        elif cp.raw == 'own':
            dst = torch.empty(n_dst, Cd, dtype=torch.float32, device=dev)
            raw = (dst, 0)
        else:
            buf = self.cat(cp.raw[0], n_dst, dev)[0]
            raw, dst = (buf, cp.raw[1]), buf[:, cp.raw[1]:cp.raw[1] + Cd]
        acts, own = [], []
        for norm, relu, where in cp.acts:
            scale, shift = norm.eval_affine()
            if where is None:
                rows = self.rows(norm)
                y = torch.empty(n_dst, Cd, dtype=torch.bfloat16 if rows else torch.float32, device=dev)
                acts.append((y, 0, scale, shift, relu))
                own.append((norm, rows_only(y) if rows else y, relu))
            else:
                acts.append((self.cat(where[0], n_dst, dev)[1], where[1], scale, shift, relu))
        sparse_conv_fused(src, weight, rb, mode, addend, raw, acts)
        for norm, y, relu in own:
            attach_activated(dst, norm, y, relu)
        return dst

    def concat(self, owner, n: int, device) -> torch.Tensor:
        """The concatenation of level ``owner`` after both producers ran, with its first tail norm's result attached"""
        buf, act = self.cat(owner, n, device)
        c = self.plan.cats[owner]
        attach_activated(buf, c.norm, rows_only(act) if act.dtype == torch.bfloat16 else act, c.relu)
        return buf


# ----------------------------------------------------------------------------------------
# pooling over a rulebook (csrc/sparse_pool.hip, include/u3d.h section P1)
# ----------------------------------------------------------------------------------------
_POOL_MODES = {'max': L.POOL_MAX, 'avg': L.POOL_AVG}


def _pool_check(x: torch.Tensor, mode: str):
    if mode not in _POOL_MODES:
        raise L.U3DError(f"sparse_pool: mode must be 'max' or 'avg', got {mode!r}")
    if not x.is_cuda:
        raise L.U3DError('sparse_pool: u3d kernels need CUDA (HIP) tensors: the product path has no CPU fallback')
    if x.dim() != 2 or x.dtype != torch.float32:
        raise L.U3DError(f'sparse_pool: features must be fp32 [n, C], got {x.dtype} {tuple(x.shape)}')
    _pool_width(x.shape[1])


def _pool_width(C: int):
    if C % 4 or not 4 <= C <= 512:
        raise L.U3DError(f'sparse_pool: {C} channels: the gfx950 kernels take a multiple of 4 in 4..512')


def sparse_pool_forward(x: torch.Tensor, rb: Rulebook, mode: str):
    """(y [n_out, C], aux) without autograd: aux is ``arg`` (uint8 [n_out, C], the selected offset of every element) for 'max' and
    ``count`` (int32 [n_out], the pairs of every row) for 'avg' -- what the backward reads instead of x and y."""
    _pool_check(x, mode)
    x = x.contiguous()
    if x.shape[0] != rb.n_in:
        raise L.U3DError(f'sparse_pool: {x.shape[0]} feature rows, the rulebook has {rb.n_in} input rows')
    C, dev = x.shape[1], x.device
    y = torch.empty(rb.n_out, C, dtype=torch.float32, device=dev)
    arg = torch.empty(rb.n_out, C, dtype=torch.uint8, device=dev) if mode == 'max' else None
    count = torch.empty(rb.n_out, dtype=torch.int32, device=dev) if mode == 'avg' else None
    if rb.n_out:           # (an output row has at least one pair: n_in > 0 as well)
        L.call('u3d_sparse_pool_fwd', L.ptr(x), L.ptr(rb.neighbours('out')), rb.n_out, rb.K, C, _POOL_MODES[mode], L.ptr(y), L.ptr(arg),
               L.ptr(count), L.stream())
    return y, (arg if mode == 'max' else count)


def sparse_pool_backward(dy: torch.Tensor, rb: Rulebook, mode: str, aux: torch.Tensor) -> torch.Tensor:
    """dx [n_in, C] from dy [n_out, C] and the forward's ``aux``; every element is written by the kernel, an empty level launches nothing"""
    _pool_check(dy, mode)
    dy = dy.contiguous()
    C, dev = dy.shape[1], dy.device
    if not (rb.n_in and rb.n_out):
        return torch.zeros(rb.n_in, C, dtype=torch.float32, device=dev)
    dx = torch.empty(rb.n_in, C, dtype=torch.float32, device=dev)
    arg, count = (aux, None) if mode == 'max' else (None, aux)
    L.call('u3d_sparse_pool_bwd', L.ptr(dy), L.ptr(rb.neighbours('in')), rb.n_in, rb.K, C, _POOL_MODES[mode], L.ptr(arg), L.ptr(count),
           L.ptr(dx), L.stream())
    return dx


class _SparsePoolFn(torch.autograd.Function):
    """Saves the selected offsets (max) or the pair counts (avg), and neither x nor y."""

    @staticmethod
    def forward(ctx, x, rb: Rulebook, mode: str):
        y, aux = sparse_pool_forward(x, rb, mode)
        ctx.save_for_backward(aux)
        ctx.rb, ctx.mode = rb, mode
        return y

    @staticmethod
    def backward(ctx, dy):
        (aux,) = ctx.saved_tensors
        return sparse_pool_backward(dy, ctx.rb, ctx.mode, aux), None, None


def sparse_pool(x: torch.Tensor, rb: Rulebook, mode: str) -> torch.Tensor:
    """Max / average pooling of the rows x [n_in, C] over the windows of ``rb`` (a strided convolution's rulebook) -> [n_out, C].
    'max': over the inputs present in a window, first maximal element on a tie, NaN if the window holds one; the gradient goes to the
    selected element alone.  'avg': sum / number of present inputs.  Fixed summation order, no atomics: bit-reproducible."""
    _pool_check(x, mode)
    refuse_rows_only(x, 'sparse_pool')
    return _SparsePoolFn.apply(x, rb, mode)


# ----------------------------------------------------------------------------------------
# batch norm (+ReLU)
# ----------------------------------------------------------------------------------------
def _dist_on():
    from .dist import collectives_on          # > 1 rank, or any initialised group under dist.force_collectives()
    return collectives_on()


def allreduce_bn_sums(sums: torch.Tensor, group=None):
    """SyncBatchNorm exchange: one all-reduce of the fp64 [.., count] vector (RCCL over xGMI
    on the GPU box, gloo in the CPU tests)."""
    dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
    return sums


class _BNReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, x, gamma, beta, running_mean, running_var):
        """``cfg``: everything that is not a tensor autograd tracks, as one object that stays on ctx (built by ``SparseBatchNorm.forward``):
        eps, momentum, relu, training, sync, want_skip, and
        ``nbt``: num_batches_tracked where the statistics kernel is to increment it, else None;
        ``stats``: (partial, n_tiles) from the epilogue of the convolution that produced x (``stats_of``), or None;
        ``affine``: the [4, C] rows mean | invstd | scale | shift of the running statistics (eval mode: computed once per parameter
        version, ``SparseBatchNorm.eval_affine``), or None;
        ``yb`` (bf16 [n, C] or None): receives y rounded to bf16 in the same pass (precision.bf16_rows); ``dx_shadow``: the backward
        writes such a copy of dx too and attaches it to the gradient it returns (x came out of a sparse convolution)."""
        x = x.contiguous()
        n, C = x.shape
        dev = x.device
        relu, yb, nbt = int(cfg.relu), cfg.yb, cfg.nbt
        # mean, invstd, scale, shift: in inference the module's cached rows (``SparseBatchNorm.eval_affine``), never written here
        cached = cfg.affine is not None and not cfg.training and cfg.affine.device == dev
        st = cfg.affine if cached else torch.empty(4, C, dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        ws = L.scratch(L.lib().u3d_bn_ws_bytes(C), dev)
        part, n_tiles = cfg.stats or (None, 0)
        sync_on = cfg.sync and _dist_on()
        batch = cfg.training and (n or sync_on)   # a rank without rows still joins the exchange (zero sums, zero count), like nn.SyncBatchNorm
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev) if batch else None      # [sum x, sum x^2, rows]
        if batch and not sync_on:                 # one call: stats -> finalize -> apply
            L.call('u3d_bn_forward', L.ptr(x), n, C, L.ptr(part), n_tiles, L.ptr(gamma), L.ptr(beta), cfg.eps, cfg.momentum,
                   L.ptr(running_mean), L.ptr(running_var), L.ptr(nbt), relu, L.ptr(y), L.ptr(yb), L.ptr(st), L.ptr(sums), L.ptr(ws), L.stream())
        else:
            if batch:
                if n:
                    L.call('u3d_bn_stats', L.ptr(x), n, C, L.ptr(part), n_tiles, L.ptr(sums), L.ptr(ws), L.stream())
                else:
                    sums.zero_()
                allreduce_bn_sums(sums)           # rows ride along: no host read-back on the critical path
                L.call('u3d_bn_finalize', L.ptr(sums), -1.0, L.ptr(gamma), L.ptr(beta), cfg.eps, cfg.momentum, L.ptr(running_mean),
                       L.ptr(running_var), C, L.ptr(st[0]), L.ptr(st[1]), L.ptr(st[2]), L.ptr(st[3]), L.ptr(nbt), L.stream())
            elif not cached:                      # the running statistics
                st[0] = running_mean
                st[1] = torch.rsqrt(running_var + cfg.eps)
                st[2] = gamma * st[1]
                st[3] = beta - running_mean * st[2]
            if n:
                L.call('u3d_bn_apply', L.ptr(x), L.ptr(st[2]), L.ptr(st[3]), relu, n, C, L.ptr(y), L.ptr(yb), L.stream())
        ctx.save_for_backward(x, st, sums)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)          # an unused skip output sends None, not a zero tensor
        if cfg.want_skip:
            # second output = x itself, for the identity branch that leaves the block input next to this norm (residual skip,
            # U-Net concat): its gradient then arrives HERE, together with dy, and is added inside the backward kernel
            # instead of by autograd's accumulation kernel
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        cfg = ctx.cfg
        x, st, fsums = ctx.saved_tensors
        dx, dgb = dskip, [None, None]                  # as they stay when only the identity branch carried a gradient
        if dy is not None:
            dy = dy.contiguous()
            dskip = None if dskip is None else dskip.contiguous()
            n, C = x.shape
            dev = x.device
            dx = torch.empty_like(x)
            dxb = torch.empty(n, C, dtype=torch.bfloat16, device=dev) if cfg.dx_shadow and n else None
            # dgamma, dbeta (local sums: DDP averages later); separate tensors so that autograd can adopt them as .grad without a copy
            dgb = [torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)]
            batch = cfg.training and fsums is not None          # the forward normalised with batch statistics
            sync_on = batch and cfg.sync and _dist_on()
            if not n:
                if sync_on:                              # keep the collective sequence of the other ranks
                    dist.all_reduce(torch.zeros(2 * C, dtype=torch.float64, device=dev), op=dist.ReduceOp.SUM)
                dgb[0].zero_()
                dgb[1].zero_()
            else:
                ws = L.scratch(L.lib().u3d_bn_ws_bytes(C), dev)
                sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
                xdy = (L.ptr(x), L.ptr(dy), L.ptr(st[0]), L.ptr(st[1]), L.ptr(st[2]), L.ptr(st[3]), int(cfg.relu))
                if batch and not sync_on:                # one call: bwd_stats -> bwd_apply (+ dgamma / dbeta)
                    L.call('u3d_bn_backward', L.ptr(x), L.ptr(dy), L.ptr(st), int(cfg.relu), L.ptr(fsums), L.ptr(sums), n, C, L.ptr(dx), L.ptr(dxb),
                           L.ptr(dgb[0]), L.ptr(dgb[1]), L.ptr(dskip), L.ptr(ws), L.stream())
                else:
                    if sync_on:
                        sums[2 * C:] = fsums[2 * C:]     # global row count of the forward pass
                    L.call('u3d_bn_bwd_stats', *xdy, n, C, L.ptr(sums), L.ptr(ws), L.stream())
                    dgb[1] = sums[:C].to(torch.float32)
                    dgb[0] = sums[C:2 * C].to(torch.float32)
                    if sync_on:
                        dist.all_reduce(sums[:2 * C], op=dist.ReduceOp.SUM)
                    else:                                # eval: statistics are constants -> dx = scale * dy'
                        sums.zero_()
                        sums[2 * C] = 1.0
                    L.call('u3d_bn_bwd_apply', *xdy, L.ptr(sums), -1.0, n, C, L.ptr(dx), L.ptr(dxb), None, None, L.ptr(dskip), L.stream())
                if dxb is not None:
                    attach_shadow(dx, dxb)
        return None, dx, dgb[0], dgb[1], None, None


class SparseBatchNorm(nn.Module):
    """BatchNorm over voxel rows with the parameter/buffer names of nn.BatchNorm1d /
    nn.SyncBatchNorm (weight, bias, running_mean, running_var, num_batches_tracked).
    ``sync=True`` all-reduces the statistics across ranks when a process group exists
    (nn.SyncBatchNorm degenerates to plain batch norm without one -- SURVEY.md 2.3)."""

    _affine_cache = None        # eval-mode (scale, shift) rows, ``_eval_rows``

    def __init__(self, num_features, eps=1e-4, momentum=0.1, sync=True):
        super().__init__()
        self.num_features, self.eps, self.momentum, self.sync = num_features, eps, momentum, sync
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer('running_mean', torch.zeros(num_features))
        self.register_buffer('running_var', torch.ones(num_features))
        self.register_buffer('num_batches_tracked', torch.tensor(0, dtype=torch.long))
        self._affine_cache = None

    def _eval_rows(self):
        """(key, st [4, C] = mean | invstd | scale | shift, (scale, shift)) of the running statistics, by exactly the torch expressions
        the eval arm of ``_BNReLUFn.forward`` evaluates; recomputed when ``_version`` (or the storage) of weight, bias, running_mean or
        running_var changed.  What changes them behind ``_version``'s back is covered the way ``WeightPacks`` covers it: a training-mode
        forward (the statistics kernels update the running buffers in place) drops the rows, and rows computed while an optimizer may be
        stepping weight / bias (autograd enabled, either requires a gradient: fused AdamW leaves ``_version`` alone) are used once and
        recomputed by the next call.  Other writers that bypass ``_version`` (``.data``): ``invalidate_affine`` /
        ``UniDet3D.invalidate_weight_packs``."""
        src = (self.weight, self.bias, self.running_mean, self.running_var)
        # (rows made under torch.inference_mode() cannot be saved for a later backward pass: they are not shared across that boundary)
        key = tuple((t._version, t.data_ptr()) for t in src) + (float(self.eps), str(self.running_var.device), torch.is_inference_mode_enabled())
        c = getattr(self, '_affine_cache', None)
        tuned = torch.is_grad_enabled() and (self.weight.requires_grad or self.bias.requires_grad)
        if c is None or c[0] != key or c[3] or tuned:
            with torch.no_grad():
                st = torch.empty(4, self.running_var.shape[0], dtype=torch.float32, device=self.running_var.device)
                st[0] = self.running_mean
                st[1] = torch.rsqrt(self.running_var + self.eps)
                st[2] = self.weight * st[1]
                st[3] = self.bias - self.running_mean * st[2]
            c = self._affine_cache = (key, st, (st[2], st[3]), tuned)
        return c

    def eval_affine(self):
        """The cached (scale, shift) of inference: y = x * scale + shift.  The same two tensors until a parameter or buffer changes."""
        return self._eval_rows()[2]

    def invalidate_affine(self):
        self._affine_cache = None

    def forward(self, x: torch.Tensor, relu: bool = False, skip: bool = False, shadow: bool = True):
        """``skip=True`` -> (y, x_id): ``x_id`` is x for a second consumer (the identity branch next to this norm); the gradient that
        consumer sends back is added to dx inside this layer's backward kernel.
        In inference (eval mode under ``torch.no_grad()``) the result the producing convolution's epilogue attached for this norm to
        exactly this ``x`` (``activated_of``) is returned where there is one: no launch.
        In training mode the per-tile column sums the producing convolution's epilogue attached to exactly this ``x`` (``stats_of``)
        are used where there are any: the statistics then cost no pass over x."""
        # bf16 operands with bf16 rows in HBM (precision.bf16_rows): y (when a ReLU follows -- the input of a sparse convolution -- and
        # the channel count suits the bf16 kernels) and the gradient handed back to a producing convolution get a bf16 shadow
        refuse_rows_only(x, 'SparseBatchNorm')
        if self.training and self._affine_cache is not None:
            self._affine_cache = None       # the running statistics (and, by the optimizer, weight and bias) move without a ``_version`` bump
        if not self.training and not torch.is_grad_enabled():
            # fused inference: the convolution(s) that produced x wrote this norm's result already (``attach_activated``)
            y = activated_of(x, self, relu)
            if y is not None:
                return (y, x) if skip else y
            if getattr(x, '_u3d_no_raw', False):
                raise L.U3DError('SparseBatchNorm: the producing convolution wrote no raw output and nothing for this norm')
        rows = P.bf16_rows() and x.is_cuda and x.shape[0] > 0 and x.shape[1] % 32 == 0
        yb = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if rows and relu and shadow else None
        # num_batches_tracked is incremented by the statistics kernel (one launch less per layer)
        cfg = SimpleNamespace(eps=self.eps, momentum=self.momentum, relu=relu, training=self.training, sync=self.sync, want_skip=skip,
                              nbt=self.num_batches_tracked if self.training and (x.shape[0] or (self.sync and _dist_on())) else None,
                              stats=stats_of(x) if self.training else None, affine=None if self.training else self._eval_rows()[1], yb=yb, dx_shadow=bool(rows and getattr(x, '_u3d_from_conv', False)))
        out = _BNReLUFn.apply(cfg, x, self.weight, self.bias, self.running_mean, self.running_var)
        if yb is not None:
            attach_shadow(out[0] if skip else out, yb)
        return out

    def on(self, x: 'SparseConvTensor', relu: bool = False, skip: bool = False, *, feeds_conv: bool):
        """This norm on a sparse tensor: the new tensor, and with ``skip`` the identity tensor (``forward``'s x_id) as well.
        ``feeds_conv``: a sparse convolution reads the result (with ``relu``, the only reader a bf16 shadow of y is of use to)."""
        out = self(x.features, relu=relu, skip=skip, shadow=feeds_conv)
        if skip:
            return x.replace_feature(out[0]), x.replace_feature(out[1])
        return x.replace_feature(out)


# ----------------------------------------------------------------------------------------
# rows of one tensor at the rows of another (csrc/sparse_sets.hip, include/u3d.h section S1)
# ----------------------------------------------------------------------------------------
def _rows_check(t: torch.Tensor, what: str):
    refuse_rows_only(t, what)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise L.U3DError(f'{what}: features must be fp32 [n, C], got {t.dtype} {tuple(t.shape)} (fp32 rows under every operand format)')
    C = t.shape[1]
    if C % 4 or not 4 <= C <= 512:
        raise L.U3DError(f'{what}: {C} channels: the gfx950 kernels take a multiple of 4 in 4..512')
    if not t.is_cuda:
        raise L.U3DError(f'{what}: u3d kernels need CUDA (HIP) tensors: the product path has no CPU fallback')


def rows_take(x: torch.Tensor, rows: torch.Tensor, what: str = 'rows_take') -> torch.Tensor:
    """y[j] = x[rows[j]], bit for bit; a row value outside [0, len(x)) gives a row of +0.0 (u3d_rows_take: every element of y written
    once by the kernel).  No destination rows launches nothing; no source rows gives zeros without a launch."""
    _rows_check(x, what)
    n_out, (n_src, C) = rows.shape[0], x.shape
    if not (n_out and n_src):
        return torch.zeros(n_out, C, dtype=torch.float32, device=x.device)
    y = torch.empty(n_out, C, dtype=torch.float32, device=x.device)
    L.call('u3d_rows_take', L.ptr(x.contiguous()), L.ptr(rows), n_out, n_src, C, L.ptr(y), L.stream())
    return y


def rows_take2(a: torch.Tensor, rows_a: torch.Tensor, b: torch.Tensor, rows_b: torch.Tensor, what: str = 'rows_take2') -> torch.Tensor:
    """y[j] = a[rows_a[j]] + b[rows_b[j]] in one pass (u3d_rows_take2): the fp32 sum where both rows are present, the bits of the
    present one where one is, +0.0 where neither is.  Both operands have rows (an empty operand is the caller's case)."""
    _rows_check(a, what)
    _rows_check(b, what)
    n_out, C = rows_a.shape[0], a.shape[1]
    y = torch.empty(n_out, C, dtype=torch.float32, device=a.device)
    if n_out:
        L.call('u3d_rows_take2', L.ptr(a.contiguous()), L.ptr(rows_a), a.shape[0], L.ptr(b.contiguous()), L.ptr(rows_b), b.shape[0], n_out, C,
               L.ptr(y), L.stream())
    return y


class _JoinFn(torch.autograd.Function):
    """a and b on the union level ``lvl`` (``geometry.UnionLevel``).  The backward is two copies, da[i] = dy[union row of a's row i],
    each made only where its operand asks for it; an operand whose level IS the union takes dy itself."""

    @staticmethod
    def forward(ctx, a, b, lvl: UnionLevel):
        ctx.lvl = lvl
        return rows_take2(a, lvl.rows_a, b, lvl.rows_b, 'sparse_add')

    @staticmethod
    def backward(ctx, dy):
        lvl, dy = ctx.lvl, dy.contiguous()
        grads = [None, None]
        for i, which in enumerate('ab'):
            if ctx.needs_input_grad[i]:
                grads[i] = dy if lvl.same == which else rows_take(dy, lvl.into(which), 'sparse_add (backward)')
        return grads[0], grads[1], None


class _PruneFn(torch.autograd.Function):
    """the rows ``kept`` of x; backward dx[i] = dy[pos[i]], +0.0 for a dropped row (pos -1) -- every element written by the kernel"""

    @staticmethod
    def forward(ctx, x, kept, pos):
        ctx.save_for_backward(pos)
        return rows_take(x, kept, 'prune')

    @staticmethod
    def backward(ctx, dy):
        (pos,) = ctx.saved_tensors
        return rows_take(dy.contiguous(), pos, 'prune (backward)'), None, None


class _DenseFn(torch.autograd.Function):
    """the rows of ``x`` in a dense grid (u3d_dense_scatter: every element written once by the kernel, +0.0 in a cell without a row);
    backward the pure copy df[i] = d_dense[cell of row i] (u3d_dense_gather) -- autograd runs it only when the features ask for it"""

    @staticmethod
    def forward(ctx, f, x: 'SparseConvTensor', channels_first: bool):
        B, (X, Y, Z), (n, C) = x.batch_size, x.spatial_shape, f.shape
        ctx.geo = (x.indices, B, X, Y, Z, C, int(channels_first))
        y = torch.empty((B, C, X, Y, Z) if channels_first else (B, X, Y, Z, C), dtype=torch.float32, device=f.device)
        L.call('u3d_dense_scatter', L.ptr(f.contiguous()), n, C, *x.index.table(), B, X, Y, Z, int(channels_first), L.ptr(y), L.stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        coords, B, X, Y, Z, C, channels_first = ctx.geo
        df = torch.empty(coords.shape[0], C, dtype=torch.float32, device=dy.device)
        L.call('u3d_dense_gather', L.ptr(dy.contiguous()), B, X, Y, Z, C, channels_first, L.ptr(coords), coords.shape[0], L.ptr(df), L.stream())
        return df, None, None


class _FromDenseFn(torch.autograd.Function):
    """the active cells ``kept`` of a channels-last grid viewed as rows [n_cells, C]; backward dx[cell] = dy[pos[cell]], +0.0 for an
    inactive cell (pos -1) -- both directions are u3d_rows_take, every element written"""

    @staticmethod
    def forward(ctx, cells, kept, pos):
        ctx.save_for_backward(pos)
        return rows_take(cells, kept, 'from_dense')

    @staticmethod
    def backward(ctx, dy):
        (pos,) = ctx.saved_tensors
        return rows_take(dy.contiguous(), pos, 'from_dense (backward)'), None, None


def _plain(t: torch.Tensor) -> torch.Tensor:
    """the same values as a new tensor object: what a layer left on ``t`` for its reader (bf16 shadow, epilogue statistics, the
    ``_u3d_from_conv`` mark: attributes of the object) does not travel, as behind ``sparse_bias``"""
    return t.view(t.shape)


# ----------------------------------------------------------------------------------------
# SparseConvTensor + layers
# ----------------------------------------------------------------------------------------
class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size, indice_dict=None, index=None):
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(s) for s in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {} if indice_dict is None else indice_dict
        self._index = index
        self._scene = None

    def replace_feature(self, new_features):
        t = SparseConvTensor(new_features, self.indices, self.spatial_shape, self.batch_size, self.indice_dict, self._index)
        t._scene = self._scene                     # the result shares ``indices``: the same scene ranges
        return t

    def _scene_ranges(self):
        """offsets, order flag (device tensors) and whether the flag has been seen clear; built on first use, no host read"""
        if self._scene is None:
            offsets, flag = scene_offsets(self.indices, self.batch_size)
            self._scene = SimpleNamespace(offsets=offsets, flag=flag, checked=is_canonical(self.indices) or not self.indices.shape[0])
        return self._scene

    @property
    def scene_offsets(self) -> torch.Tensor:
        """int32 [batch_size + 1] on the device: scene b owns the rows offsets[b] .. offsets[b + 1] of the canonical order (empty scenes
        included).  Cached on the tensor; ``replace_feature`` carries it.  u3d_scene_offsets, no host read."""
        return self._scene_ranges().offsets

    @property
    def index(self) -> OccupancyIndex:
        if self._index is None:
            self._index = tensor_index(self.indice_dict, self.indices, self.batch_size, self.spatial_shape)
        return self._index

    def dense(self, channels_first: bool = True) -> torch.Tensor:
        """spconv's ``SparseConvTensor.dense``: a contiguous fp32 [B, C, X, Y, Z] -- [B, X, Y, Z, C] with ``channels_first=False`` -- whose
        axes follow ``spatial_shape``.  An active cell holds exactly the bits of its feature row (-0.0 stays -0.0, a NaN keeps its
        payload), every other cell +0.0; one kernel writes every element of the result once (u3d_dense_scatter: no memset, no
        ``torch.zeros`` of the result).  A tensor without rows gives zeros by one fill, a zero-size result launches nothing.  No host read.
        fp32 rows under every operand format, a multiple of 4 in 4..512 channels, fewer than 2^31 cells (B X Y Z; element offsets are
        64-bit); bf16 rows only are refused.  The result is a plain tensor: no shadow, no statistics, no marks.  Backward: the pure copy
        dfeatures[i] = d_dense[cell of row i] (u3d_dense_gather), run only when the features ask for a gradient.
        ``from_dense(t.dense(channels_first=False))`` holds exactly the rows of ``t`` that are not all-zero, in order."""
        f = self.features
        refuse_rows_only(f, 'dense')
        n_cells = dense_cells(self.batch_size, self.spatial_shape, 'dense')
        _rows_check(f, 'dense')
        if len(self.spatial_shape) != 3 or self.indices.shape[0] != f.shape[0]:
            raise L.U3DError(f'dense: {f.shape[0]} feature rows on {self.indices.shape[0]} coordinate rows of a grid {self.spatial_shape}: a '
                             'three-dimensional grid and one coordinate row per feature row are needed')
        B, (X, Y, Z), C = self.batch_size, self.spatial_shape, f.shape[1]
        shape = (B, C, X, Y, Z) if channels_first else (B, X, Y, Z, C)
        if not n_cells:
            return torch.empty(shape, dtype=torch.float32, device=f.device)
        if not f.shape[0]:
            return torch.zeros(shape, dtype=torch.float32, device=f.device)
        return _DenseFn.apply(f, self, bool(channels_first))

    @classmethod
    def from_dense(cls, x: torch.Tensor) -> 'SparseConvTensor':
        """spconv's ``SparseConvTensor.from_dense``: ``x`` is a contiguous fp32 [B, X, Y, Z, C] (channels last) on the device.  A cell is
        active iff any of its C values != 0: a NaN makes a cell active, a cell of only +0.0 / -0.0 is not.  Rows in canonical order
        (= ascending cell number ((b X + x) Y + y) Z + z), features bit copies, ``indices`` built on the device (u3d_dense_active,
        ``compact_mask``, u3d_cells_coords, u3d_rows_take); ``spatial_shape = [X, Y, Z]``, ``batch_size = B``, a fresh, empty
        ``indice_dict``; the occupancy index is built when a layer first asks for it.  One host read, the active count; no active cell
        gives an empty tensor.  A multiple of 4 in 4..512 channels, fewer than 2^31 cells.  Backward: dx[cell] = dfeatures[row] for an
        active cell, +0.0 elsewhere, every element written.
        ``from_dense(x).dense(channels_first=False)`` equals ``x`` bit for bit, except that a -0.0 in an inactive cell comes back +0.0."""
        if not isinstance(x, torch.Tensor) or x.dim() != 5 or x.dtype != torch.float32:
            raise L.U3DError(f'from_dense: the grid must be an fp32 tensor [B, X, Y, Z, C], got {getattr(x, "dtype", type(x).__name__)} '
                             f'{tuple(getattr(x, "shape", ()))}')
        B, X, Y, Z, C = x.shape
        if C % 4 or not 4 <= C <= 512:
            raise L.U3DError(f'from_dense: {C} channels: the gfx950 kernels take a multiple of 4 in 4..512')
        n_cells = dense_cells(B, (X, Y, Z), 'from_dense')
        if not x.is_contiguous():
            raise L.U3DError(f'from_dense: the grid must be contiguous [B, X, Y, Z, C] (channels last), got strides {tuple(x.stride())}')
        if not x.is_cuda:
            raise L.U3DError('from_dense: u3d kernels need CUDA (HIP) tensors: the product path has no CPU fallback')
        if not n_cells:
            return cls(x.view(0, C), torch.empty(0, 4, dtype=torch.int32, device=x.device), [X, Y, Z], B)
        kept, pos, _ = active_cells(x.detach())
        return cls(_FromDenseFn.apply(x.view(n_cells, C), kept, pos), cells_coords(kept, (X, Y, Z)), [X, Y, Z], B)


class SparseModule(nn.Module):
    pass


class SparseSequential(SparseModule):
    """spconv.SparseSequential: sparse layers see the tensor, dense layers its features;
    a BatchNorm directly followed by ReLU runs as one fused kernel."""

    def __init__(self, *args):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], dict):
            for k, m in args[0].items():
                self.add_module(k, m)
        else:
            for i, m in enumerate(args):
                self.add_module(str(i), m)

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def __len__(self):
        return len(self._modules)

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        mods = list(self._modules.values())
        if any(isinstance(m, ToDense) for m in mods[:-1]):
            raise L.U3DError('SparseSequential: ToDense must come last: what it returns is a dense tensor, no layer of this library reads one')
        for m in mods[:-1]:
            if getattr(m, 'returns_dense', False):
                raise L.U3DError(f'SparseSequential: {type(m).__name__} must come last: what it returns is a dense tensor [B, C], no layer of '
                                 'this library reads one')
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, SparseModule):
                x = m(x)
            elif isinstance(m, SparseBatchNorm):
                fuse = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                feeds_conv = fuse and i + 2 < len(mods) and isinstance(mods[i + 2], _ConvBase)      # only then a bf16 shadow of y is of use
                x = m.on(x, relu=fuse, feeds_conv=feeds_conv)
                i += 1 if fuse else 0
            elif isinstance(m, nn.Identity):
                pass
            elif isinstance(m, nn.ReLU):
                x = x.replace_feature(_relu(x.features))
            else:
                raise L.U3DError(f'SparseSequential: no gfx950 kernel for dense layer {type(m).__name__}')
            i += 1
        return x


class _ReLUFn(torch.autograd.Function):
    """y = x where x > 0, else +0.0 (u3d_relu_fwd); dx = dy where x > 0, else +0.0 (u3d_relu_bwd).  Flat buffers: any row count, zero
    included (no launch), any channel count."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        if x.numel():
            L.call('u3d_relu_fwd', L.ptr(x), x.numel(), L.ptr(y), L.stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        if x.numel():
            L.call('u3d_relu_bwd', L.ptr(x), L.ptr(dy), x.numel(), L.ptr(dx), L.stream())
        return dx


def _relu(f):
    """stand-alone ReLU (an nn.ReLU that no batch norm precedes): off the hot path, differentiable.  The result is a new tensor: what a
    layer left on ``f`` for its reader (bf16 shadow, epilogue statistics, the ``_u3d_from_conv`` mark) stays behind."""
    refuse_rows_only(f, 'ReLU')
    if f.dim() != 2 or f.dtype != torch.float32:
        raise L.U3DError(f'ReLU: features must be fp32 [n, C], got {f.dtype} {tuple(f.shape)}')
    if not f.is_cuda:
        raise L.U3DError('ReLU: u3d kernels need CUDA (HIP) tensors: the product path has no CPU fallback')
    return _ReLUFn.apply(f)


def _pad16(f):
    c = f.shape[1]
    return f if c % 16 == 0 else F.pad(f, (0, 16 - c % 16))


class _ConvBase(SparseModule):
    """Weight [C_out, k0, k1, k2, C_in] and the layer geometry (``conv_geometry``: each of kernel_size / stride / padding / dilation an int
    or a 3-sequence).  ``kernel_size`` keeps the int of a cubic kernel (a tuple otherwise); ``K`` is the number of offsets.
    ``bias=True`` (an fp32 ``bias`` [C_out], added to every output row after the convolution, ``sparse_bias``) is taken by the layer
    kinds that set ``_takes_bias``: ``SparseInverseConv3d`` and ``SparseConvTranspose3d``.  ``SubMConv3d`` and ``SparseConv3d`` refuse it as
    they always did."""
    _takes_bias = False

    def __init__(self, in_channels, out_channels, kernel_size, bias=False, indice_key=None, stride=1, padding=0, dilation=1):
        super().__init__()
        if bias and not self._takes_bias:
            raise L.U3DError(f'{type(self).__name__}: bias=True is not built for this layer kind (SparseInverseConv3d and '
                             f'SparseConvTranspose3d take one)')
        k = layer_geometry(self, conv_geometry(kernel_size, stride, padding, dilation))
        self.in_channels, self.out_channels, self.indice_key = in_channels, out_channels, indice_key
        self.weight = nn.Parameter(torch.empty(out_channels, *k, in_channels))
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)
        if bias:                # fp32 [C_out], uniform in +-1 / sqrt(K C_in) (the fan-in of the weight above)
            self.bias = nn.Parameter(torch.empty(out_channels))
            bound = 1.0 / (self.K * in_channels) ** 0.5
            nn.init.uniform_(self.bias, -bound, bound)
        else:
            self.register_parameter('bias', None)

    def _biased(self, y: torch.Tensor) -> torch.Tensor:
        """y + bias on every row of the layer's result, rows without a pair included (``sparse_bias``); y itself without a bias"""
        return y if self.bias is None else sparse_bias(y, self.bias)

    def _w16(self):
        c = self.in_channels
        return self.weight if c % 16 == 0 else F.pad(self.weight, (0, 16 - c % 16))

    def _conv(self, x: 'SparseConvTensor', rb: Rulebook, mode: str, addend=None) -> torch.Tensor:
        """pad -> sparse_conv -> result features; in training mode with the statistics for a norm behind this layer asked for.
        On the fused inference path (a ``FusionRun`` in the tensor's ``indice_dict`` that plans this layer, ``fusion_active``) the
        launch writes the result of the norm(s) behind this layer as well, and the result itself where the plan says.
        With a bias the result is (conv + addend) + bias, two fp32 roundings in that order; such a layer asks the launch for no
        statistics (the epilogue's would be those of the value before the bias) and is in no fusion plan (``spconv_unet.fusion_plan``)."""
        run = x.indice_dict.get(FUSE_KEY)
        cp = run.plan.convs.get(self) if run is not None else None
        if cp is not None and fusion_active(self, *(a[0] for a in cp.acts)):
            if self.bias is not None:
                raise L.U3DError(f'{type(self).__name__}: a layer with a bias has no fused-inference epilogue')
            return run.conv(self, cp, x, rb, mode, addend)
        return self._biased(sparse_conv(_pad16(x.features), self._w16(), rb, mode, addend, self.training and self.bias is None))


class SubMConv3d(_ConvBase):
    """Submanifold convolution: the output set is the input set.  Kernel extents 1 or 3 per axis (odd, as in spconv), any dilation;
    ``stride`` / ``padding`` are accepted and, as in spconv, without effect: the effective padding is d (k - 1) / 2.
    k = 3 with dilation 1 builds the hard-coded 27-neighbour rulebook (``build_subm_rulebook``), the all-ones kernel is a dense GEMM,
    everything else goes through the general builder."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=False, indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, bias, indice_key, stride, padding, dilation)
        k, d = self.geom[:3], self.geom[9:]
        if not all(a in (1, 3) for a in k):
            raise L.U3DError(f'SubMConv3d: kernel_size {k}: every kernel extent must be 1 or 3 (odd extents only, as in spconv)')
        self.general = not (k == (3, 3, 3) and d == (1, 1, 1))
        self._rb_geom = ('subm', k, d)
        self._subm_geom = (*k, 1, 1, 1, *[d[a] * (k[a] - 1) // 2 for a in range(3)], *d)

    def forward(self, x: SparseConvTensor, addend: Optional[torch.Tensor] = None) -> SparseConvTensor:
        if self.K == 1:
            # 1x1 skip convolution = [N, Cin] x [Cin, Cout] GEMM, no rulebook (K5): the decoder's fp32 MFMA GEMM kernels (the
            # library picked a 0.6 ms kernel for the level-1 weight gradient, a [64 x 356k] x [356k x 32] product)
            y = dense.linear(x.features, self.weight.view(self.out_channels, self.in_channels))
            return x.replace_feature(y if addend is None else y + addend)
        return x.replace_feature(self._conv(x, self.geometry(x), 'fwd', addend))

    def geometry(self, x: SparseConvTensor) -> Rulebook:
        def build():
            if self.general:
                return build_conv_rulebook(x.indices, x.index, x.batch_size, x.spatial_shape, self._subm_geom, subm=True)[3]
            return build_subm_rulebook(x.indices, x.index)
        return cached_level(x, 'subm', self, self._rb_geom, build)


class SparseConv3d(_ConvBase):
    """Regular sparse convolution: kernel extents 1..3, any stride / padding / dilation.  k = 2, s = 2, p = 0 (the U-Net's) builds the
    hard-coded parity rulebook (``build_down_rulebook``), everything else goes through the general builder."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=False, indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, bias, indice_key, stride, padding, dilation)
        self.general = self.geom != _DOWN_K2S2
        self._rb_geom = ('conv', *self.geom)

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        oc, oshape, ix2, rb = self.geometry(x)
        return SparseConvTensor(self._conv(x, rb, 'fwd'), oc, oshape, x.batch_size, x.indice_dict, ix2)

    def geometry(self, x: SparseConvTensor):
        """Output level + rulebook for this conv (``strided_geometry``)"""
        return strided_geometry(self, x)


class _PoolBase(SparseModule):
    """spconv's SparseMaxPool3d / SparseAvgPool3d: the geometry of a ``SparseConv3d`` with the same kernel_size / stride / padding /
    dilation (``strided_geometry``: same cache entries, so a convolution or a ``SparseInverseConv3d`` under the same ``indice_key``
    finds this layer's rulebook), ``stride=None`` meaning stride = kernel_size.  No parameters."""
    mode = None

    def __init__(self, kernel_size, stride=None, padding=0, dilation=1, indice_key=None, subm=False):
        super().__init__()
        if subm:
            raise L.U3DError(f'{type(self).__name__}: subm=True is not built')
        layer_geometry(self, conv_geometry(kernel_size, kernel_size if stride is None else stride, padding, dilation))
        self.indice_key = indice_key

    def geometry(self, x: SparseConvTensor):
        return strided_geometry(self, x)

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        _pool_width(x.features.shape[1])
        oc, oshape, ix2, rb = self.geometry(x)
        return SparseConvTensor(sparse_pool(x.features, rb, self.mode), oc, oshape, x.batch_size, x.indice_dict, ix2)


class SparseMaxPool3d(_PoolBase):
    """Maximum over the inputs present in each window (an absent cell is not a zero); the gradient goes to the first maximal element."""
    mode = 'max'


class SparseAvgPool3d(_PoolBase):
    """Sum over the inputs present in each window divided by their number."""
    mode = 'avg'


class SparseInverseConv3d(_ConvBase):
    """Undoes the ``SparseConv3d`` found under its ``indice_key``, whatever that layer's geometry: the saved pairs with the roles
    swapped (mode 'inv'), output on the strided convolution's input level.  ``kernel_size`` must be that layer's.  With ``bias=True`` the
    bias reaches every row of that level, a row without a pair included (a voxel beyond the last full window of a p = 0 layer)."""
    _takes_bias = True

    def __init__(self, in_channels, out_channels, kernel_size, indice_key=None, bias=False):
        super().__init__(in_channels, out_channels, kernel_size, bias, indice_key)

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        kind, entry = saved_under(x.indice_dict, self.indice_key)
        if kind is None:
            raise L.U3DError(f'SparseInverseConv3d: no rulebook saved under {self.indice_key!r}')
        if kind == 'subm':
            raise L.U3DError(f'SparseInverseConv3d: indice_key {self.indice_key!r} belongs to a SubMConv3d, not to a SparseConv3d')
        if kind == 'up':
            raise L.U3DError(f'SparseInverseConv3d: indice_key {self.indice_key!r} belongs to a SparseConvTranspose3d: inverting a '
                             f'transposed layer is not built')
        rb, idx, shape, index = entry
        if rb.geom is not None and tuple(rb.geom[1:4]) != self.geom[:3]:
            raise L.U3DError(f'SparseInverseConv3d: kernel_size {self.geom[:3]} differs from kernel_size {tuple(rb.geom[1:4])} of the '
                             f'SparseConv3d saved under {self.indice_key!r}')
        return SparseConvTensor(self._conv(x, rb, 'inv'), idx, shape, x.batch_size, x.indice_dict, index)


class SparseConvTranspose3d(_ConvBase):
    """Transposed sparse convolution: learned up-sampling into NEW voxels.  Input cell i and tap t reach output cell o = i s - p + t d
    (per axis, taps not flipped); the output set is every cell so reached inside the output grid, in canonical order, and
    y[o] = sum over the pairs (i, t) of W[:, t, :] x[i] -- ``F.conv_transpose3d(x, W.permute(4, 0, 1, 2, 3), stride=s, padding=p,
    output_padding=q, dilation=d)`` sampled at the active rows (the dense result is zero everywhere else).  Kernel extents 1..3.
    Output extent per axis: (in - 1) s - 2 p + d (k - 1) + q + 1, torch's rule.  spconv's own rule for this layer leaves the dilation out
    ((in - 1) s - 2 p + k + q); the two agree at dilation 1.  ``output_padding`` must be smaller than max(stride, dilation), as in torch.
    An input row whose taps all fall outside the grid (padding beyond the reach) contributes nothing; an empty output level gives an
    empty tensor.  The rulebook is cached under the layer's indice_key (``geometry.cached_level``) -- its own identity without a key; two transposed layers
    that share a key must share the geometry, output padding included.  Geometry and launch path: ``build_convt_rulebook``."""
    _takes_bias = True

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, output_padding=0, dilation=1, bias=False, indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, bias, indice_key, stride, padding, dilation)
        self.output_padding = output_padding_of(output_padding, self.geom)
        self.general = True                 # not the U-Net's own layer shapes: a fusion plan that meets it steps aside
        self._rb_geom = ('convt', *self.geom, *self.output_padding)

    def geometry(self, x: SparseConvTensor) -> UpLevel:
        """Output level + rulebook of this layer: (out_coords, out_shape, out_index, Rulebook), cached in ``indice_dict``"""
        return cached_level(x, 'up', self, self._rb_geom,
                            lambda: build_convt_rulebook(x.indices, x.batch_size, x.spatial_shape, self.geom, self.output_padding))

    def forward(self, x: SparseConvTensor) -> SparseConvTensor:
        oc, oshape, ix, rb = self.geometry(x)
        return SparseConvTensor(self._conv(x, rb, 'inv'), oc, oshape, x.batch_size, x.indice_dict, ix)


# ----------------------------------------------------------------------------------------
# tensors on different voxel sets: union add, pruning
# ----------------------------------------------------------------------------------------
def _join_check(a: 'SparseConvTensor', b: 'SparseConvTensor'):
    if a.batch_size != b.batch_size:
        raise L.U3DError(f'sparse_add: the operands differ in batch_size: {a.batch_size} and {b.batch_size}')
    if list(a.spatial_shape) != list(b.spatial_shape):
        raise L.U3DError(f'sparse_add: the operands differ in spatial_shape: {a.spatial_shape} and {b.spatial_shape}')
    fa, fb = a.features, b.features
    refuse_rows_only(fa, 'sparse_add')
    refuse_rows_only(fb, 'sparse_add')
    if fa.dim() != 2 or fb.dim() != 2 or fa.shape[1] != fb.shape[1]:
        raise L.U3DError(f'sparse_add: the operands differ in channel count: {tuple(fa.shape)} and {tuple(fb.shape)} features')


def sparse_add(a: 'SparseConvTensor', b: 'SparseConvTensor', *more: 'SparseConvTensor') -> 'SparseConvTensor':
    """a + b for tensors on DIFFERENT voxel sets of one grid (spconv's ``functional.sparse_add``, MinkowskiEngine's ``a + b``): the result
    lives on the union of the active sets, rows in canonical order.  Per row and channel: the fp32 sum (one rounding) where both operands
    have the voxel, exactly the bits of the one operand that has it otherwise.  More operands fold from the LEFT, ((a + b) + c) + ...:
    that order is part of the contract (fp32 addition is not associative).  The operands must agree in batch_size, spatial_shape and
    channel count.  fp32 rows under every operand format; the result hands no bf16 shadow, no epilogue statistics and no
    ``_u3d_from_conv`` mark to its reader.  Backward: pure copies, da[i] = dy[row of a's voxel i], made only for an operand that asks.
    Levels: a result on a NEW voxel set starts from a fresh, empty ``indice_dict`` (no rulebook of another row count can reach it); when
    the union has as many rows as an operand (the other set lies inside it) the result keeps that operand's ``indices``, index and
    ``indice_dict``; operands that share one ``indices`` tensor object build no geometry at all; an empty operand gives the other's level.
    One host read (the row count of the union)."""
    for other in (b, *more):                        # every operand, before the first launch: what must agree, then what the kernels take
        _join_check(a, other)
    for t in (a, b, *more):
        _rows_check(t.features, 'sparse_add')
        if t.features.device != a.features.device:
            raise L.U3DError(f'sparse_add: the operands live on different devices: {a.features.device} and {t.features.device}')
    if more:
        return sparse_add(sparse_add(a, b), *more)
    na, nb = a.features.shape[0], b.features.shape[0]
    if a.indices is b.indices:                      # one level: a plain feature add
        return a.replace_feature(a.features + b.features)
    if not nb:
        return a.replace_feature(_plain(a.features))
    if not na:
        return b.replace_feature(_plain(b.features))
    lvl = build_union_level(a.indices, a.index, b.indices, b.index, a.batch_size, a.spatial_shape)
    y = _JoinFn.apply(a.features, b.features, lvl)
    if lvl.same is not None:
        return (a if lvl.same == 'a' else b).replace_feature(y)
    return SparseConvTensor(y, lvl.coords, a.spatial_shape, a.batch_size, None, lvl.index)


def prune(x: 'SparseConvTensor', keep: torch.Tensor) -> 'SparseConvTensor':
    """The voxels of ``x`` whose ``keep`` bit is set (MinkowskiEngine's ``MinkowskiPruning``), rows in their old order -- a subset of a
    canonical order is canonical.  ``keep``: torch.bool [n] on the tensor's device, typically ``score > t`` or a scatter of top-k indices;
    it takes no gradient.  Backward: dx[i] = dy[position of i] for a kept row, +0.0 for a dropped one.  The result lives on a new voxel
    set and starts from a fresh, empty ``indice_dict`` -- unless every bit is set, then it keeps the level of ``x``; no bit set gives an
    empty tensor.  fp32 rows under every operand format, nothing handed to the reader (``sparse_add``).  One host read (the kept count)."""
    f = x.features
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool:
        raise L.U3DError(f'prune: the mask must be a torch.bool tensor, got {getattr(keep, "dtype", type(keep).__name__)}')
    if keep.dim() != 1 or keep.shape[0] != f.shape[0]:
        raise L.U3DError(f'prune: the mask must have one entry per row: {tuple(keep.shape)} for {f.shape[0]} rows')
    _rows_check(f, 'prune')
    if keep.device != f.device:
        raise L.U3DError(f'prune: the mask lives on {keep.device}, the tensor on {f.device}')
    kept, pos, n_keep = compact_mask(keep.contiguous())
    if n_keep == f.shape[0]:                        # every row kept: the level of x (same count as a superset = the same rows)
        return x.replace_feature(_plain(f))
    y = _PruneFn.apply(f, kept, pos)
    coords = rows_take(x.indices.view(torch.float32), kept, 'prune (coordinates)').view(torch.int32) if n_keep else x.indices[:0]
    return SparseConvTensor(y, coords, x.spatial_shape, x.batch_size)


class SparsePrune(SparseModule):
    """``prune`` as a module (``MinkowskiPruning``): ``forward(x, keep)``.  No parameters."""

    def forward(self, x: 'SparseConvTensor', keep: torch.Tensor) -> 'SparseConvTensor':
        return prune(x, keep)


# ----------------------------------------------------------------------------------------
# per-scene operations (csrc/sparse_scene.hip, include/u3d.h section S3): top-k pruning, global pooling
# ----------------------------------------------------------------------------------------
# The order flag of a tensor's scene ranges is read by the host at most once per voxel set, and never on its own where another value is
# read anyway: ``topk_mask`` / ``prune_topk`` read it in the same host read as the kept count.  ``global_pool`` reads no count, so it reads
# the flag only for a tensor whose coordinate rows this library did not write itself (``geometry.is_canonical``: rows from an index, from a
# dense grid, or a subset of checked rows are canonical by construction) -- once, on first use; ``replace_feature`` carries the verdict.
def _scene_order_seen(x: 'SparseConvTensor', flag: int, what: str):
    check_scene_order(flag, what, x.batch_size)
    x._scene_ranges().checked = True
    mark_canonical(x.indices)


def _topk_check(x: 'SparseConvTensor', scores, k, what: str):
    """the refusals of the top-k family, before any launch; returns (scores fp32 [n] contiguous, the B counts)"""
    f = x.features
    refuse_rows_only(f, what)
    n, B = f.shape[0], x.batch_size
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32:
        raise L.U3DError(f'{what}: the scores must be a torch.float32 tensor, got {getattr(scores, "dtype", type(scores).__name__)}')
    if tuple(scores.shape) not in ((n,), (n, 1)):
        raise L.U3DError(f'{what}: the scores must have one entry per row, [n] or [n, 1]: {tuple(scores.shape)} for {n} rows')
    if isinstance(k, int) and not isinstance(k, bool):
        ks = [int(k)] * B
    else:
        try:
            ks = list(k)
        except TypeError:
            ks = None
        if ks is None or isinstance(k, (str, torch.Tensor)) or any(isinstance(v, bool) or not isinstance(v, int) for v in ks):
            raise L.U3DError(f'{what}: k must be an int or a sequence of ints (host values), got {type(k).__name__}')
        if len(ks) != B:
            raise L.U3DError(f'{what}: k must have one entry per scene: {len(ks)} for batch_size {B}')
    if any(v < 0 for v in ks):
        raise L.U3DError(f'{what}: k must be >= 0, got {min(ks)}')
    if scores.device != f.device:
        raise L.U3DError(f'{what}: the scores live on {scores.device}, the tensor on {f.device}')
    _rows_check(f, what)
    return scores.detach().reshape(n).contiguous(), [min(v, 0x7fffffff) for v in ks]


def _scene_topk(x: 'SparseConvTensor', scores, k, largest, what: str):
    """(mask bool [n], kept int32 [n_keep], pos int32 [n], n_keep) of the top-k rows of every scene (u3d_scene_topk).  One host read:
    the kept count together with the order flag.  No rows: nothing launched, nothing read."""
    s, ks = _topk_check(x, scores, k, what)
    n, B, dev = s.shape[0], x.batch_size, s.device
    mask = torch.empty(n, dtype=torch.bool, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    if not n:
        return mask, kept, pos, 0
    sc = x._scene_ranges()
    result = torch.empty(2, dtype=torch.int32, device=dev)
    w = L.ws(L.lib().u3d_scene_topk_ws_bytes(n, B), dev)
    L.call('u3d_scene_topk', L.ptr(s), L.ptr(x.indices.contiguous()), L.ptr(sc.offsets), L.ptr(sc.flag), L.ptr(L.h2d(ks, torch.int32, dev)), n, B,
           1 if largest else 0, L.ptr(mask), L.ptr(kept), L.ptr(pos), L.ptr(result), L.ptr(w), L.stream())
    n_keep, flag = result.tolist()             # documented read-back (one host sync): the kept count and the order flag
    _scene_order_seen(x, flag, what)
    return mask, kept[:n_keep], pos, n_keep


def topk_mask(x: 'SparseConvTensor', scores: torch.Tensor, k, largest: bool = True) -> torch.Tensor:
    """torch.bool [n]: the mask of the ``k`` best-scored voxels of EVERY scene of ``x`` (the ``_prune`` step of FCAF3D / TR3D necks), for
    ``prune``.  ``scores``: fp32 [n] or [n, 1] on the tensor's device, no gradient.  ``k``: an int >= 0 or a sequence of batch_size such
    ints (host values).  Scene b keeps its first min(k_b, n_b) rows of this order -- that of a stable descending sort, defined here because
    ``torch.topk`` leaves ties unspecified: score descending, then row ascending; every NaN ranks above +inf and all NaNs are equal; -0.0
    equals +0.0; denormals keep their value (the comparison is on integer keys, nothing is flushed).  ``largest=False`` reverses the score
    order only: NaNs still rank first, ties still go to the lower row.  One chain of launches for the whole batch (u3d_scene_topk: radix
    select, integer only, deterministic) and ONE host read, the kept count together with the order flag of the scene ranges: a tensor
    whose batch indices descend or leave [0, batch_size) raises.  fp32 rows under every operand format; bf16 rows only are refused."""
    return _scene_topk(x, scores, k, largest, 'topk_mask')[0]


def prune_topk(x: 'SparseConvTensor', scores: torch.Tensor, k, largest: bool = True) -> 'SparseConvTensor':
    """``prune(x, topk_mask(x, scores, k, largest))`` in every bit and in what it does to levels, without the mask's round trip: the select
    writes the kept list and the positions itself.  A new voxel set starts from a fresh, empty ``indice_dict``; every row kept keeps the
    level of ``x``; nothing kept gives an empty tensor.  Backward as ``prune`` (``_PruneFn``).  One host read (the kept count, with the
    order flag)."""
    _, kept, pos, n_keep = _scene_topk(x, scores, k, largest, 'prune_topk')
    f = x.features
    if n_keep == f.shape[0]:
        return x.replace_feature(_plain(f))
    y = _PruneFn.apply(f, kept, pos)
    coords = rows_take(x.indices.view(torch.float32), kept, 'prune_topk (coordinates)').view(torch.int32) if n_keep else x.indices[:0]
    return SparseConvTensor(y, mark_canonical(coords), x.spatial_shape, x.batch_size)      # (rows of a checked order, taken in order)


class SparseTopKPrune(SparseModule):
    """``prune_topk`` as a module: ``SparseTopKPrune(k, largest=True)``, ``forward(x, scores)``.  No parameters."""

    def __init__(self, k, largest: bool = True):
        super().__init__()
        ok = isinstance(k, int) and not isinstance(k, bool) or (isinstance(k, (list, tuple)) and
                                                                  all(isinstance(v, int) and not isinstance(v, bool) for v in k))
        if not ok:
            raise L.U3DError(f'SparseTopKPrune: k must be an int or a sequence of ints (host values), got {type(k).__name__}')
        if (k if isinstance(k, int) else min(k, default=0)) < 0:
            raise L.U3DError(f'SparseTopKPrune: k must be >= 0, got {k if isinstance(k, int) else min(k)}')
        self.k, self.largest = (k if isinstance(k, int) else list(k)), bool(largest)

    def forward(self, x: 'SparseConvTensor', scores: torch.Tensor) -> 'SparseConvTensor':
        return prune_topk(x, scores, self.k, self.largest)


def _global_pool_check(x: 'SparseConvTensor', mode: str):
    if mode not in _POOL_MODES:
        raise L.U3DError(f"global_pool: mode must be 'max' or 'avg', got {mode!r}")
    _rows_check(x.features, 'global_pool')
    if x.indices.shape[0] != x.features.shape[0]:
        raise L.U3DError(f'global_pool: {x.features.shape[0]} feature rows on {x.indices.shape[0]} coordinate rows')


def global_pool_forward(f: torch.Tensor, x: 'SparseConvTensor', mode: str):
    """(y fp32 [B, C], arg) without autograd: arg is int32 [B, C], the winning row of every element (-1 for an empty scene), for 'max'
    and None for 'avg'.  No host read on rows this library wrote; see the rule above for others."""
    n, C = f.shape
    B, dev = x.batch_size, f.device
    sc = x._scene_ranges()
    if not sc.checked:
        _scene_order_seen(x, int(sc.flag.item()), 'global_pool')          # rows a caller handed in: the flag's own read, once per voxel set
    y = torch.empty(B, C, dtype=torch.float32, device=dev)
    arg = torch.empty(B, C, dtype=torch.int32, device=dev) if mode == 'max' else None
    w = L.ws(L.lib().u3d_scene_pool_ws_bytes(n, B, C), dev)
    L.call('u3d_scene_pool_fwd', L.ptr(f.contiguous()), L.ptr(sc.offsets), n, B, C, _POOL_MODES[mode], L.ptr(y), L.ptr(arg), L.ptr(w), L.stream())
    return y, arg


def global_pool_backward(dy: torch.Tensor, indices: torch.Tensor, offsets: torch.Tensor, mode: str, arg) -> torch.Tensor:
    """dx [n, C] from dy [B, C]: every element written by the kernel (u3d_scene_pool_bwd, gather form)"""
    n, (B, C) = indices.shape[0], dy.shape
    dx = torch.empty(n, C, dtype=torch.float32, device=dy.device)
    L.call('u3d_scene_pool_bwd', L.ptr(dy.contiguous()), L.ptr(indices.contiguous()), L.ptr(offsets), L.ptr(arg), n, B, C, _POOL_MODES[mode],
           L.ptr(dx), L.stream())
    return dx


class _GlobalPoolFn(torch.autograd.Function):
    """Saves the winning rows (max) or nothing (avg: the scene ranges suffice), and neither x nor y."""

    @staticmethod
    def forward(ctx, f, x: 'SparseConvTensor', mode: str):
        y, arg = global_pool_forward(f, x, mode)
        ctx.save_for_backward(*([arg] if arg is not None else []))
        ctx.geo = (x.indices, x.scene_offsets, mode)
        return y

    @staticmethod
    def backward(ctx, dy):
        indices, offsets, mode = ctx.geo
        arg = ctx.saved_tensors[0] if ctx.saved_tensors else None
        return global_pool_backward(dy, indices, offsets, mode, arg), None, None


def global_pool(x: 'SparseConvTensor', mode: str) -> torch.Tensor:
    """Global pooling of every scene of ``x`` (spconv's ``SparseGlobalMaxPool`` / ``SparseGlobalAvgPool``, MinkowskiEngine's global
    pooling): fp32 [batch_size, C], a plain dense tensor.  'max': the rule of the pooling layers -- a strictly larger value replaces the held
    one, a NaN replaces a number, ties and later NaNs keep the lower row; the gradient goes to the winning row alone.  'avg': the column
    sums of a scene in fp64 in a fixed order, y = (float)(sum / n_b), one rounding; the gradient is dy * (1.0f / n_b).  An empty scene
    gives a row of +0.0 and takes no gradient.  Several workgroups per scene, no atomics: bit-reproducible.  No host read (for coordinate
    rows handed in by the caller, the order flag is read once per voxel set).  A multiple of 4 in 4..512 channels, fp32 rows under every
    operand format; bf16 rows only are refused.  No rows gives zeros [batch_size, C] without a launch."""
    _global_pool_check(x, mode)
    f = x.features
    if not f.shape[0]:
        return torch.zeros(x.batch_size, f.shape[1], dtype=torch.float32, device=f.device)
    return _GlobalPoolFn.apply(f, x, mode)


class SparseGlobalMaxPool(SparseModule):
    """``global_pool(x, 'max')`` as a module (spconv's ``SparseGlobalMaxPool``).  No parameters.  In a ``SparseSequential`` it is the last
    module -- the sequence then returns the dense [B, C] tensor; a module behind it is refused."""
    returns_dense = True

    def forward(self, x: 'SparseConvTensor') -> torch.Tensor:
        return global_pool(x, 'max')


class SparseGlobalAvgPool(SparseModule):
    """``global_pool(x, 'avg')`` as a module (spconv's ``SparseGlobalAvgPool``); otherwise as ``SparseGlobalMaxPool``."""
    returns_dense = True

    def forward(self, x: 'SparseConvTensor') -> torch.Tensor:
        return global_pool(x, 'avg')


# ----------------------------------------------------------------------------------------
# dense interchange: the module form of ``SparseConvTensor.dense``
# ----------------------------------------------------------------------------------------
class ToDense(SparseModule):
    """spconv's ``ToDense``: ``forward(x) -> x.dense()``, fp32 [B, C, X, Y, Z].  No parameters.  In a ``SparseSequential`` it is the last
    module -- the sequence then returns the dense tensor; a module behind it is refused."""

    def forward(self, x: 'SparseConvTensor') -> torch.Tensor:
        return x.dense()
