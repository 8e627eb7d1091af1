"""Voxelisation and superpoint pooling through the C ABI (host side).

``voxelize``     replaces ME.utils.batch_sparse_collate + ME.TensorField(...).sparse()
                 + inverse_mapping                       (unidet3d/unidet3d.py:158-174)
``PoolPlan`` / ``superpoint_pool``   replace  scatter_mean(x.features[inverse_mapping], superpoints)
                                                          (unidet3d/unidet3d.py:130)
``superpoint_centers``               replaces scatter_mean(points, sp_pts_mask)   (:332-333, :446-447)
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import _lib as L
from .geometry import OccupancyIndex


@dataclass
class VoxelBatch:
    coords: torch.Tensor          # int32 [Nv, 4]  (b, x, y, z), canonical order
    feats: torch.Tensor           # f32   [Nv, 6]
    inverse: torch.Tensor         # int64 [Np]     point -> voxel row
    spatial_shape: List[int]
    index: OccupancyIndex
    vox_offsets: torch.Tensor     # int32 [Nv+1]   CSR of points per voxel
    vox_points: torch.Tensor      # int32 [Np]
    pt_offsets: torch.Tensor      # int64 [B+1] (device)
    stats: torch.Tensor           # f32 [B, 12] min, max, mean_xyz, pad
    points: torch.Tensor          # f32 [Np, 6] concatenated
    coord_src: Optional[torch.Tensor] = None      # f32 [Np, 3] elastic coordinates (voxel units) when the batch has them


def voxelize(points: List[torch.Tensor], voxel_size: float, min_spatial_shape: int,
             elastic_points: Optional[List[torch.Tensor]] = None, div_mode: int = 0) -> VoxelBatch:
    dev = points[0].device
    B = len(points)
    sizes = [int(p.shape[0]) for p in points]
    pts = torch.cat([p.to(torch.float32) for p in points]).contiguous() if B > 1 else points[0].to(torch.float32).contiguous()
    n_pts = pts.shape[0]
    offs_h = [0]
    for s in sizes:
        offs_h.append(offs_h[-1] + s)
    offs = torch.tensor(offs_h, dtype=torch.int64, device=dev)
    csrc = None
    vs = float(voxel_size)
    if elastic_points is not None:
        csrc = torch.cat([e.to(torch.float32) for e in elastic_points]).contiguous()
        vs = 1.0
    stats = torch.empty(B, 12, dtype=torch.float32, device=dev)
    gmax = torch.empty(3, dtype=torch.int32, device=dev)
    w = L.ws(L.lib().u3d_vox_scene_stats_ws_bytes(B), dev)
    L.call('u3d_vox_scene_stats', L.ptr(pts), L.ptr(csrc), L.ptr(offs), B, max(sizes), vs, div_mode,
           L.ptr(stats), L.ptr(gmax), L.ptr(w), L.stream())
    shape = [max(int(v) + 1, int(min_spatial_shape)) for v in gmax.tolist()]       # read-back #1
    pt_cell = torch.empty(n_pts, dtype=torch.int64, device=dev)

    def mark(bitmap):           # bitmap None = hashed index (large extent): cell ids only, then sort -> unique -> hash table (csrc/hashidx.hip)
        L.call('u3d_vox_mark', L.ptr(pts), L.ptr(csrc), L.ptr(offs), B, max(sizes), L.ptr(stats), vs, div_mode,
               *shape, L.ptr(bitmap), L.ptr(pt_cell), L.stream())
        return pt_cell
    index = OccupancyIndex.from_marks(B, shape, dev, mark)
    n_vox = index.count()                                                          # read-back #2
    coords = index.coords(n_vox)
    inverse = torch.empty(n_pts, dtype=torch.int64, device=dev)
    vox_offsets = torch.empty(n_vox + 1, dtype=torch.int32, device=dev)
    vox_points = torch.empty(n_pts, dtype=torch.int32, device=dev)
    feats = torch.empty(n_vox, 6, dtype=torch.float32, device=dev)
    w2 = L.ws(L.lib().u3d_vox_finalize_ws_bytes(n_pts, n_vox), dev)
    L.call('u3d_vox_finalize', L.ptr(pts), L.ptr(offs), B, n_pts, L.ptr(stats), L.ptr(pt_cell), *index.table(), n_vox, L.ptr(inverse), L.ptr(vox_offsets), L.ptr(vox_points), L.ptr(feats), 6,
           L.ptr(w2), L.stream())
    return VoxelBatch(coords, feats, inverse, shape, index, vox_offsets, vox_points, offs, stats, pts, csrc)


def csr_build(seg_ids: torch.Tensor, S: int):
    """offsets int32 [S+1], list int32 [L] of element ids grouped by segment."""
    Ln = seg_ids.shape[0]
    dev = seg_ids.device
    offsets = torch.empty(S + 1, dtype=torch.int32, device=dev)
    lst = torch.empty(Ln, dtype=torch.int32, device=dev)
    w = L.ws(L.lib().u3d_csr_build_ws_bytes(Ln, S), dev)
    L.call('u3d_csr_build', L.ptr(seg_ids.contiguous()), Ln, S, L.ptr(offsets), L.ptr(lst), L.ptr(w), L.stream())
    return offsets, lst


class PoolPlan:
    """Index structures of one batch for pooling voxel features into superpoints (built once,
    integer work only): CSR of points per superpoint composed with inverse_mapping (forward) and
    the voxelizer's CSR of points per voxel composed with the superpoint ids (backward)."""

    def __init__(self, vb: VoxelBatch, superpoints: torch.Tensor, n_superpoints: int):
        self.S = int(n_superpoints)
        self.n_vox = vb.coords.shape[0]
        sp = superpoints.contiguous()
        self.sp_offsets, self.sp_points = csr_build(sp, self.S)
        n = sp.shape[0]
        self.sp_vox = torch.empty(n, dtype=torch.int32, device=sp.device)
        L.call('u3d_gather_i64_to_i32', L.ptr(vb.inverse), L.ptr(self.sp_points), n, L.ptr(self.sp_vox), L.stream())
        self.vox_sp = torch.empty(n, dtype=torch.int32, device=sp.device)
        L.call('u3d_gather_i64_to_i32', L.ptr(sp), L.ptr(vb.vox_points), n, L.ptr(self.vox_sp), L.stream())
        self.vox_offsets = vb.vox_offsets


def _need_fp32(t: torch.Tensor, what: str):
    """the pooling kernel reads rows as float4 through the raw pointer: any other dtype would be reinterpreted, not converted"""
    if t.dtype != torch.float32:
        raise L.U3DError(f'superpoint_pool: {what} must be float32, got {t.dtype}')


class _PoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, plan: PoolPlan):
        _need_fp32(feats, 'feats')
        feats = feats.contiguous()
        C = feats.shape[1]
        out = torch.empty(plan.S, C, dtype=torch.float32, device=feats.device)
        L.call('u3d_segment_gather_sum', L.ptr(feats), L.ptr(plan.sp_vox), L.ptr(plan.sp_offsets), plan.S, C, 1,
               None, L.ptr(out), L.stream())
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, dout):
        plan = ctx.plan
        _need_fp32(dout, 'the gradient of the pooled tensor')
        dout = dout.contiguous()
        C = dout.shape[1]
        df = torch.empty(plan.n_vox, C, dtype=torch.float32, device=dout.device)
        L.call('u3d_segment_gather_sum', L.ptr(dout), L.ptr(plan.vox_sp), L.ptr(plan.vox_offsets), plan.n_vox, C, 0,
               L.ptr(plan.sp_offsets), L.ptr(df), L.stream())
        return df, None


def superpoint_pool(feats: torch.Tensor, plan: PoolPlan) -> torch.Tensor:
    return _PoolFn.apply(feats, plan)


def superpoint_centers(points: torch.Tensor, sp_offsets: torch.Tensor, sp_points: torch.Tensor, S: int,
                       stats: Optional[torch.Tensor] = None, pt_offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mean over each superpoint's points of (xyz - scene_min); ``stats`` = VoxelBatch.stats
    (row b starts with the scene's min xyz) or None for raw coordinates (predict path)."""
    out = torch.empty(S, 3, dtype=torch.float32, device=points.device)
    B = 0 if stats is None else stats.shape[0]
    L.call('u3d_segment_mean_xyz', L.ptr(points), points.stride(0), L.ptr(sp_points), L.ptr(sp_offsets), S,
           L.ptr(stats), 12, L.ptr(pt_offsets), B, L.ptr(out), L.stream())
    return out


def instance_boxes(vb: VoxelBatch, instance_ids: torch.Tensor, n_inst_total: int, voxel_size: Optional[float] = None) -> torch.Tensor:
    """[n_inst_total, 6] = (centre xyz, size xyz) of the axis-aligned box around each instance's points in the
    scene-shifted frame; ``instance_ids`` int64 [Np] are batch-global (-1 = no instance).  The frame is
    ``xyz - scene min`` (unidet3d.py:300-301) or, when the batch carries elastic coordinates,
    ``(elastic - scene min) * voxel_size`` (:296-297; scaling by a positive constant commutes with min / max, so it is
    applied to the result).  One pass over the batch instead of the reference's per-instance boolean masks (:220-256)."""
    dev = vb.points.device
    src = vb.points if vb.coord_src is None else vb.coord_src
    mm = torch.empty(n_inst_total, 6, dtype=torch.float32, device=dev)
    ws = L.scratch(n_inst_total * 24 + 64, dev)
    L.call('u3d_segment_minmax_xyz', L.ptr(src), src.stride(0), L.ptr(instance_ids.contiguous()), src.shape[0],
           n_inst_total, L.ptr(vb.stats), 12, L.ptr(vb.pt_offsets), vb.stats.shape[0], L.ptr(mm), L.ptr(ws), L.stream())
    if vb.coord_src is not None:
        mm = mm * float(voxel_size)
    lo, hi = mm[:, :3], mm[:, 3:]
    return torch.cat(((hi + lo) / 2, hi - lo), 1)


TARGETS_MAX_K = 16                         # csrc/targets.hip: topk + 1 values a lane keeps in registers


def targets_by_distance(centers: torch.Tensor, sp_offsets, box_centers: torch.Tensor, box_offsets, topk: int):
    """``UniDet3D.get_targets`` (unidet3d.py:371-409) for every scene of a batch in two launches (csrc/targets.hip).

    ``centers`` float32 [S_total, 3] batch-global superpoint centres, ``sp_offsets`` host ints [B+1]; ``box_centers`` float32
    [G_total, >=3] gravity centres in the training frame (a column view of wider rows is read in place: unit column stride, the
    row stride is passed on), ``box_offsets`` host ints [B+1].  Returns ``(packed, mask_off)``: one bool buffer holding scene b's
    [G_b, S_b] matrix row-major at ``mask_off[b]`` (host ints [B+1]); a scene without boxes owns an empty block."""
    if topk + 1 > TARGETS_MAX_K:
        raise L.U3DError(f'targets_by_distance: topk + 1 = {topk + 1} exceeds {TARGETS_MAX_K}')
    sp_offsets, box_offsets = [int(v) for v in sp_offsets], [int(v) for v in box_offsets]
    B = len(sp_offsets) - 1
    assert len(box_offsets) == B + 1 and B >= 0
    S = [sp_offsets[b + 1] - sp_offsets[b] for b in range(B)]
    G = [box_offsets[b + 1] - box_offsets[b] for b in range(B)]
    assert all(s >= 0 for s in S) and all(g >= 0 for g in G) and (not B or (sp_offsets[0] >= 0 and box_offsets[0] >= 0))
    mask_off = [0]
    for s, g in zip(S, G):
        mask_off.append(mask_off[-1] + s * g)
    dev = centers.device
    packed = torch.empty(mask_off[-1], dtype=torch.bool, device=dev)
    if not mask_off[-1]:
        return packed, mask_off
    assert centers.dtype == torch.float32 and centers.dim() == 2 and centers.shape[1] == 3 and sp_offsets[-1] <= centers.shape[0]
    assert box_centers.dtype == torch.float32 and box_centers.dim() == 2 and box_centers.shape[1] >= 3 and box_offsets[-1] <= box_centers.shape[0]
    if box_centers.stride(1) != 1 or box_centers.stride(0) < 3:
        box_centers = box_centers[:, :3].contiguous()
    if not box_centers.is_cuda:
        raise L.U3DError('u3d kernels need CUDA (HIP) tensors: the product path has no CPU fallback')
    d_sp, d_box, d_mask = L.h2d_pack([(sp_offsets, torch.int64), (box_offsets, torch.int64), (mask_off, torch.int64)], dev)
    ws = L.scratch(L.lib().u3d_targets_by_distance_ws_bytes(box_centers.shape[0]), dev)
    L.call('u3d_targets_by_distance', L.ptr(centers), centers.shape[0], L.ptr(d_sp), box_centers.data_ptr(), box_centers.stride(0),
           box_centers.shape[0], L.ptr(d_box), L.ptr(d_mask), mask_off[-1], B, max(G), max(S), int(topk), L.ptr(packed), L.ptr(ws), L.stream())
    return packed, mask_off


# ----------------------------------------------------------------------------------------
# inference post-processing
# ----------------------------------------------------------------------------------------
NMS_MAX, NMS_ROT_MAX = 4400, 3600          # csrc/postproc.hip: boxes one workgroup keeps in LDS


def nms_multiclass(bboxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, iou_thr: float, score_thr: float,
                   fast_nms: bool = True):
    """``UniDet3D._single_scene_multiclass_nms`` (unidet3d/unidet3d.py:595-650): class by class
    (ascending id), boxes above ``score_thr`` visited by descending score, greedy suppression by the BEV IoU
    (``fast_nms``: mmcv ``nms3d_normal``) or by the 3-D IoU of the corner boxes (mmdet3d ``aligned_3d_nms`` on
    ``_bbox_to_loss(boxes)``); 7-dof boxes go through mmcv ``nms3d`` (rotated BEV IoU) whatever ``fast_nms`` says.
    ``scores`` must already be sorted descending (they come from a sorted top-k).
    Returns (bboxes, scores, labels) in the reference's output order."""
    if bboxes.shape[1] not in (6, 7):
        raise ValueError('boxes must be (cx, cy, cz, dx, dy, dz[, heading])')
    sel = scores > score_thr
    bboxes, scores, labels = bboxes[sel], scores[sel], labels[sel]
    n = bboxes.shape[0]
    if n == 0:
        return bboxes.new_zeros((0, bboxes.shape[1])), bboxes.new_zeros((0,)), bboxes.new_zeros((0,))      # unidet3d.py:645-648: all three from `bboxes`
    order = torch.sort(labels, stable=True).indices            # (label asc, score desc)
    b = bboxes[order].contiguous().float()
    lab = labels[order].to(torch.int32).contiguous()
    keep = torch.empty(n, dtype=torch.uint8, device=b.device)
    if b.shape[1] == 7:                                           # with_yaw: mmcv nms3d on the rotated BEV rectangles (:625-626)
        fn, arg, limit = 'u3d_nms_rotated', b, NMS_ROT_MAX
    elif fast_nms:
        fn, arg, limit = 'u3d_nms_bev', b, NMS_MAX
    else:
        half = b[:, 3:] / 2                                      # _bbox_to_loss (criterion.py:180-198)
        fn, arg, limit = 'u3d_nms_aligned3d', torch.cat((b[:, :3] - half, b[:, :3] + half), dim=1).contiguous(), NMS_MAX
    # One workgroup holds a launch's boxes in LDS (4400 / 3600 boxes).  Suppression never crosses a class boundary, so a larger
    # set (test_cfg.topk_insts above the limit -- the reference accepts any) is cut at class boundaries into several launches;
    # only a SINGLE class with more boxes than the limit is refused.
    if n <= limit:
        L.call(fn, L.ptr(arg), L.ptr(lab), n, float(iou_thr), L.ptr(keep), L.stream())
    else:
        starts = torch.cat((lab.new_zeros(1), (lab[1:] != lab[:-1]).nonzero()[:, 0].to(torch.int32) + 1, lab.new_full((1,), n))).tolist()
        lo = 0
        while lo < n:
            hi = max([e for e in starts if lo < e <= lo + limit], default=None)
            if hi is None:
                raise L.U3DError(f'nms: one class holds more than {limit} boxes above the score threshold')
            L.call(fn, L.ptr(arg[lo:hi]), L.ptr(lab[lo:hi]), hi - lo, float(iou_thr), L.ptr(keep[lo:hi]), L.stream())
            lo = hi
    k = order[keep.bool()]
    out = bboxes[k]
    if fast_nms and out.shape[1] == 6:        # the reference appends a zero heading for nms3d_normal and returns those 7-column boxes (:629-638)
        out = torch.cat((out, torch.zeros_like(out[:, :1])), dim=1)
    return out, scores[k], labels[k]


def nms_bev_multiclass(bboxes, scores, labels, iou_thr, score_thr):
    return nms_multiclass(bboxes, scores, labels, iou_thr, score_thr, True)


def trim_boxes_by_superpoints(points: torch.Tensor, sp_offsets: torch.Tensor, sp_points: torch.Tensor, n_superpoints: int,
                              bboxes: torch.Tensor, low_sp_thr: float, up_sp_thr: float) -> torch.Tensor:
    """``UniDet3D.trim_bboxes_by_superpoints`` (unidet3d/unidet3d.py:540-593): [n,6] (centre, size) of the axis-aligned box
    around the points each box keeps after whole superpoints were deleted (< low) / added (> up).  ``bboxes`` [n,6] or [n,7]
    (heading: the inside test rotates the point shift by -yaw, ``get_face_distances`` :652-677).  ``(sp_offsets, sp_points)``
    is the CSR of point rows per superpoint (``csr_build`` / ``PoolPlan``)."""
    nb = bboxes.shape[0]
    mm = torch.empty(nb, 6, dtype=torch.float32, device=points.device)
    if nb:
        if bboxes.shape[1] == 7 and not bool((bboxes[:, 6] != 0).any()):
            bboxes = bboxes[:, :6]            # zero heading appended by the fast-NMS branch: the exact yaw-free path
        b = bboxes.contiguous().float()
        L.call('u3d_trim_boxes', L.ptr(points), points.stride(0), L.ptr(sp_points), L.ptr(sp_offsets), int(n_superpoints),
               L.ptr(b), nb, int(b.shape[1]), float(low_sp_thr), float(up_sp_thr), L.ptr(mm), L.stream())
    mn, mx = mm[:, :3], mm[:, 3:]
    return torch.cat(((mx + mn) / 2, mx - mn), dim=1)


# ----------------------------------------------------------------------------------------
# inference post-processing of a whole batch (u3d.h "batched"): softmax per dataset group, then one chain of kernels
# (segmented top-k -> ordering by class -> NMS per (scene, class) -> compaction -> superpoint trimming), one host read
# ----------------------------------------------------------------------------------------
PP_MAX_K = NMS_ROT_MAX          # csrc/postproc.hip PP_MAX_K: top-k candidates per scene the batched kernels take
PP_META, PP_FMETA = 8, 4        # include/u3d.h U3D_PP_META / U3D_PP_FMETA
NMS_MODE_BEV, NMS_MODE_ALIGNED3D, NMS_MODE_ROTATED = 0, 1, 2


def postproc_settings(test_cfg: dict, dataset_index: int, fast_nms, use_superpoints) -> dict:
    """The post-processing settings of a scene of dataset ``dataset_index`` (UniDet3D.predict_by_feat, unidet3d.py:498-538)."""
    return dict(topk=int(test_cfg['topk_insts']), score_thr=float(test_cfg['score_thr']), iou_thr=float(test_cfg['iou_thr'][dataset_index]),
                fast_nms=bool(fast_nms[dataset_index]), trim=bool(use_superpoints[dataset_index]),
                low_sp_thr=float(test_cfg['low_sp_thr']), up_sp_thr=float(test_cfg['up_sp_thr']))


def postproc_batched_ok(n_queries: int, n_classes: int, settings: dict) -> bool:
    """Whether a scene fits the batched kernels (top-k within the in-LDS sort, flat indices in 31 bits); the others take the
    per-scene path, which gives the same result."""
    return settings['topk'] <= PP_MAX_K and n_queries * n_classes < 2 ** 31


def postproc_scene_table(n_queries, n_classes, box_dims, settings):
    """Host side of the per-scene settings tables of u3d_topk_segmented / u3d_nms_batched / u3d_trim_boxes_batched:
    (meta int32 [B, 8], fmeta float32 [B, 4]).  A scene that does not fit the batched kernels gets topk = 0 and trim = 0 there
    (it has no candidates in the chain)."""
    import numpy as np
    B = len(settings)
    meta = np.zeros((B, PP_META), np.int32)
    fmeta = np.zeros((B, PP_FMETA), np.float32)
    for i, (n, c, bd, st) in enumerate(zip(n_queries, n_classes, box_dims, settings)):
        if bd not in (6, 7):
            raise ValueError('boxes must be (cx, cy, cz, dx, dy, dz[, heading])')
        ok = postproc_batched_ok(n, c, st)
        mode = NMS_MODE_ROTATED if bd == 7 else (NMS_MODE_BEV if st['fast_nms'] else NMS_MODE_ALIGNED3D)
        meta[i] = (n, c, c + 1, st['topk'] if ok else 0, bd, mode, int(st['trim'] and ok), 0)
        fmeta[i] = (st['score_thr'], st['iou_thr'], st['low_sp_thr'], st['up_sp_thr'])
    return meta, fmeta


def postproc_columns(box_dim: int, settings: dict, n_out: int) -> int:
    """Columns of a scene's output boxes, as the per-scene path returns them: trimmed boxes are (centre, size); untrimmed ones keep
    the heading of 7-dof boxes or get the zero heading the fast-NMS branch appends (unidet3d.py:629-638) -- except when nothing
    passed the score threshold, where nms_multiclass returns zeros of the input width (:645-648)."""
    if settings['trim']:
        return 6
    if n_out == 0:
        return box_dim
    return 7 if box_dim == 7 or settings['fast_nms'] else box_dim


def postprocess_scene(cls_pred: torch.Tensor, bbox: torch.Tensor, settings: dict, points: torch.Tensor, sp_offsets: torch.Tensor,
                      sp_points: torch.Tensor, n_superpoints: int, probs: Optional[torch.Tensor] = None):
    """One scene through the per-scene kernels (unidet3d.py:498-538): softmax -> torch top-k -> ``nms_multiclass`` ->
    ``trim_boxes_by_superpoints``.  ``sp_offsets`` starts at the scene's first superpoint.  Returns (boxes, labels, scores)."""
    import torch.nn.functional as F
    scores = (probs if probs is not None else F.softmax(cls_pred, dim=-1))[:, :-1]
    num_classes = scores.shape[1]
    scores, topk_idx = scores.flatten(0, 1).topk(min(settings['topk'], scores.numel()), sorted=True)
    labels = topk_idx % num_classes
    boxes = bbox[torch.div(topk_idx, num_classes, rounding_mode='floor')]
    boxes, scores, labels = nms_multiclass(boxes, scores, labels, settings['iou_thr'], settings['score_thr'], settings['fast_nms'])
    if settings['trim']:       # trimmed boxes are axis-aligned whatever went in (:585-592)
        boxes = trim_boxes_by_superpoints(points, sp_offsets, sp_points, n_superpoints, boxes, settings['low_sp_thr'], settings['up_sp_thr'])
    return boxes, labels, scores


def postprocess_batch(cls_preds, bboxes, settings, vb: VoxelBatch, plan: PoolPlan, batch_offsets):
    """Post-processing of every scene of a batch, each with its own settings (``postproc_settings``): ``cls_preds[i]`` [n_i, C_i + 1]
    logits and ``bboxes[i]`` [n_i, 6 | 7] boxes of the decoder, ``vb`` / ``plan`` / ``batch_offsets`` (superpoints of scene i:
    batch_offsets[i] .. batch_offsets[i + 1]) from the batch's front end.  Returns [(boxes [m_i, 6 | 7], labels, scores)] equal to
    ``postprocess_scene`` on each scene, except that exact score ties inside a top-k go to the lower flat index (the documented rule
    of oracle.postproc.topk_instances; torch.topk documents none).  The softmax runs once per group of scenes with the same class
    count (F.softmax: row by row, so the same bits as per scene); the rest is one chain of kernels with the [B] survivor counts as
    the only read back to the host.  Scenes outside the kernels' limits (``postproc_batched_ok``) take ``postprocess_scene``."""
    import torch.nn.functional as F
    B = len(settings)
    if B == 0:
        return []
    cls = [cls_preds[i] for i in range(B)]
    box = [bboxes[i].contiguous().float() for i in range(B)]
    dev = box[0].device
    n_q = [int(c.shape[0]) for c in cls]
    n_c = [int(c.shape[1]) - 1 for c in cls]
    bdim = [int(b.shape[1]) for b in box]
    meta, fmeta = postproc_scene_table(n_q, n_c, bdim, settings)
    groups = {}
    for i, c in enumerate(cls):
        if c.dtype != torch.float32:
            raise TypeError('postprocess_batch: class logits must be float32')
        groups.setdefault(n_c[i], []).append(i)
    probs, prob_ptr = [None] * B, [0] * B
    for g in groups.values():
        p = F.softmax(torch.cat([cls[i] for i in g]) if len(g) > 1 else cls[g[0]], dim=-1)
        r0 = 0
        for i in g:
            probs[i] = p[r0:r0 + n_q[i]]
            prob_ptr[i] = p.data_ptr() + r0 * p.shape[1] * p.element_size()
            r0 += n_q[i]
    takes = [min(int(meta[i, 3]), n_q[i] * n_c[i]) for i in range(B)]
    K = max(1, max(takes))
    C_max = max(1, max(n_c))
    d_ptr, d_meta, d_fmeta, d_sp = L.h2d_pack([(prob_ptr + [b.data_ptr() for b in box], torch.int64), (meta.tolist(), torch.int32),
                                               (fmeta.tolist(), torch.float32), ([int(v) for v in batch_offsets], torch.int32)], dev)
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    score, label, query = torch.empty(B * K, **f32), torch.empty(B * K, **i32), torch.empty(B * K, **i32)
    count, n_order = torch.empty(B, **i32), torch.empty(B, **i32)
    L.call('u3d_topk_segmented', L.ptr(d_ptr[:B]), L.ptr(d_meta), B, K, L.ptr(score), L.ptr(label), L.ptr(query), L.ptr(count), L.stream())
    order, keep, boxes_ord = torch.empty(B * K, **i32), torch.empty(B * K, dtype=torch.uint8, device=dev), torch.empty(B * K, 7, **f32)
    w = L.ws(L.lib().u3d_nms_batched_ws_bytes(B, C_max), dev)
    L.call('u3d_nms_batched', L.ptr(d_ptr[B:]), L.ptr(d_meta), L.ptr(d_fmeta), B, K, C_max, L.ptr(score), L.ptr(label), L.ptr(query),
           L.ptr(count), L.ptr(order), L.ptr(n_order), L.ptr(keep), L.ptr(boxes_ord), L.ptr(w), L.stream())
    out_b, out_s = torch.empty(B * K, 7, **f32), torch.empty(B * K, **f32)
    out_l, out_n, yaw = torch.empty(B * K, dtype=torch.int64, device=dev), torch.empty(B, **i32), torch.empty(B, **i32)
    minmax = torch.empty(B * K, 6, **f32)
    L.call('u3d_nms_compact', L.ptr(d_meta), B, K, L.ptr(score), L.ptr(label), L.ptr(order), L.ptr(n_order), L.ptr(keep), L.ptr(boxes_ord),
           L.ptr(out_b), L.ptr(out_s), L.ptr(out_l), L.ptr(out_n), L.ptr(yaw), L.ptr(minmax), L.stream())
    if bool(meta[:, 6].any()):
        L.call('u3d_trim_boxes_batched', L.ptr(vb.points), vb.points.stride(0), L.ptr(plan.sp_points), L.ptr(plan.sp_offsets), L.ptr(d_sp),
               B, plan.S, L.ptr(d_meta), L.ptr(d_fmeta), K, L.ptr(out_n), L.ptr(yaw), L.ptr(minmax), L.ptr(out_b), L.stream())
    counts = out_n.tolist()                                   # the one device -> host read of the batch
    res = []
    for i in range(B):
        st = settings[i]
        if not postproc_batched_ok(n_q[i], n_c[i], st):
            o0 = int(batch_offsets[i])
            res.append(postprocess_scene(cls[i], box[i], st, vb.points, plan.sp_offsets[o0:], plan.sp_points,
                                         int(batch_offsets[i + 1]) - o0, probs[i]))
            continue
        n, r0 = counts[i], i * K
        if n == 0:                          # nms_multiclass: all three outputs are zeros made from the boxes (unidet3d.py:645-648)
            res.append((box[i].new_zeros((0, postproc_columns(bdim[i], st, 0))), box[i].new_zeros((0,)), box[i].new_zeros((0,))))
            continue
        res.append((out_b[r0:r0 + n, :postproc_columns(bdim[i], st, n)], out_l[r0:r0 + n], out_s[r0:r0 + n]))
    return res


def cat_views(ts):
    """``torch.cat(ts)`` -- without the copy (and without the slice / cat nodes in the autograd graph) when ``ts`` are the consecutive row
    slices of ONE contiguous tensor that together cover it, which is how the per-scene lists of the reference's interface are made
    here (``pooled[o_i:o_{i+1}]``): the base tensor itself is returned.  Anything else is concatenated."""
    ts = list(ts)
    if len(ts) == 1:
        return ts[0]
    base = getattr(ts[0], '_base', None)
    if base is not None and base.is_contiguous() and base.dim() >= 1:
        off, ok = base.storage_offset(), True
        for t in ts:
            # (also the autograd state and dtype of the base: slices taken under no_grad of a differentiable base must not hand the
            # base -- and with it a gradient path torch.cat(ts) would not have -- to the caller)
            if t._base is not base or not t.is_contiguous() or t.dim() != base.dim() or t.shape[1:] != base.shape[1:] or t.storage_offset() != off \
                    or t.requires_grad != base.requires_grad or t.dtype != base.dtype:
                ok = False
                break
            off += t.numel()
        if ok and off == base.storage_offset() + base.numel():
            return base
    return torch.cat(ts)


def dropout_mask_attn(p: float, seed: int, offset: int, H: int, n_total: int, device='cuda') -> torch.Tensor:
    """uint8 [H, n_total, n_total], 1 = kept: the mask the attention kernels apply to the softmax probabilities of a packed matrix of
    ``n_total`` rows for the key ``(seed, offset)`` (``UniDet3DEncoder.dropout_key``); rows and columns are PACKED row indices, so
    scene b's block is ``[:, cu[b]:cu[b+1], cu[b]:cu[b+1]]``.  The kernels never store it -- this is the same device function, dumped."""
    mask = torch.empty(int(H), int(n_total), int(n_total), dtype=torch.uint8, device=device)
    L.call('u3d_dropout_mask_attn', float(p), int(seed), int(offset), int(H), int(n_total), L.ptr(mask), L.stream())
    return mask


def dropout_mask_rows(p: float, seed: int, offset: int, n: int, C: int, device='cuda') -> torch.Tensor:
    """uint8 [n, C], 1 = kept: the mask ``dense.dropout`` applies to an [n, C] tensor for the key ``(seed, offset)``"""
    mask = torch.empty(int(n), int(C), dtype=torch.uint8, device=device)
    L.call('u3d_dropout_mask_rows', float(p), int(seed), int(offset), int(n), int(C), L.ptr(mask), L.stream())
    return mask


def offset_ids(ids, biases, keep_negative: bool = False) -> torch.Tensor:
    """``torch.cat([ids[i] + biases[i] for i])`` for per-scene int64 id tensors (superpoint / instance ids made batch-global) in a handful
    of multi-tensor launches whatever the number of scenes.  ``keep_negative``: ids < 0 ("no instance") stay as they are:
    id + bias * min(max(id + 1, 0), 1)."""
    ids, biases = list(ids), [int(b) for b in biases]
    if keep_negative:
        live = torch._foreach_add(ids, 1)
        torch._foreach_clamp_min_(live, 0)
        torch._foreach_clamp_max_(live, 1)
        torch._foreach_mul_(live, biases)
        out = torch._foreach_add(live, ids)
    else:
        out = torch._foreach_add(ids, biases)
    return torch.cat(out) if len(out) > 1 else out[0]


# ----------------------------------------------------------------------------------------
# detection evaluation of a whole validation pass (csrc/evalmap.hip)
# ----------------------------------------------------------------------------------------
EVAL_MAX_CLASSES, EVAL_MAX_THR = 1024, 8    # include/u3d.h U3D_EVAL_MAX_CLASSES / U3D_EVAL_MAX_THR


def _eval_check(name, t, dtype, cols=None):
    if not t.is_cuda:
        raise L.U3DError('u3d kernels need CUDA (HIP) tensors: the product path has no CPU fallback')
    if t.dtype != dtype or not t.is_contiguous() or (cols is not None and (t.dim() != 2 or t.shape[1] != cols)):
        raise L.U3DError(f'eval: {name} must be a contiguous {dtype} tensor' + (f' [n, {cols}]' if cols else ''))


def eval_match(det_boxes, det_labels, det_off, gt_boxes, gt_labels, gt_off, n_classes: int, counts: Optional[torch.Tensor] = None):
    """Best same-class ground truth of every detection of a packed validation pass (``u3d_eval_match``): ``(iou_max float32 [D],
    jmax int32 [D], n_gt int32 [C], n_det int32 [C])``.  ``counts``: an int32 [2, C] buffer the two histograms are written to."""
    for name, t, dt, cols in (('det_boxes', det_boxes, torch.float32, 7), ('det_labels', det_labels, torch.int32, None),
                              ('det_off', det_off, torch.int32, None), ('gt_boxes', gt_boxes, torch.float32, 7),
                              ('gt_labels', gt_labels, torch.int32, None), ('gt_off', gt_off, torch.int32, None)):
        _eval_check(name, t, dt, cols)
    D, G, I, C = det_boxes.shape[0], gt_boxes.shape[0], det_off.numel() - 1, int(n_classes)
    if det_labels.numel() != D or gt_labels.numel() != G or gt_off.numel() != I + 1 or I < 0:
        raise L.U3DError('eval_match: labels / offsets do not fit the boxes')
    dev = det_boxes.device
    iou_max = torch.empty(D, dtype=torch.float32, device=dev)
    jmax = torch.empty(D, dtype=torch.int32, device=dev)
    if counts is None:
        counts = torch.empty((2, C), dtype=torch.int32, device=dev)
    _eval_check('counts', counts, torch.int32, C)
    L.call('u3d_eval_match', L.ptr(det_boxes), L.ptr(det_labels), L.ptr(det_off), L.ptr(gt_boxes), L.ptr(gt_labels), L.ptr(gt_off), D, G, I, C,
           L.ptr(iou_max), L.ptr(jmax), L.ptr(counts[0]), L.ptr(counts[1]), None, L.stream())
    return iou_max, jmax, counts[0], counts[1]


def eval_order(det_scores: torch.Tensor, det_labels: torch.Tensor, n_classes: int) -> torch.Tensor:
    """Evaluation order of the detections (``u3d_eval_order``): class ascending, score descending, ties by packed index.  int32 [D]."""
    _eval_check('det_scores', det_scores, torch.float32)
    _eval_check('det_labels', det_labels, torch.int32)
    D = det_scores.numel()
    perm = torch.empty(D, dtype=torch.int32, device=det_scores.device)
    ws = L.scratch(L.lib().u3d_eval_order_ws_bytes(D), det_scores.device)
    L.call('u3d_eval_order', L.ptr(det_scores), L.ptr(det_labels), D, int(n_classes), L.ptr(perm), L.ptr(ws), L.stream())
    return perm


def eval_sweep(iou_max, jmax, perm, n_gt, n_det, n_gts: int, thresholds, out: Optional[torch.Tensor] = None, with_flags: bool = False):
    """True-positive sweep and AP / last recall of every (threshold, class) (``u3d_eval_sweep``): ``(ap, rec)`` float32 [T, C];
    ``out``: a float32 [2, T, C] buffer they are written to.  ``with_flags``: also ``(tp_flag uint8 [T, D], tp_cum int32 [T, D])`` by
    sorted rank (zero where the kernel writes nothing)."""
    thresholds = [float(t) for t in thresholds]
    D, G, C, T = iou_max.numel(), int(n_gts), n_gt.numel(), len(thresholds)
    for name, t, dt in (('iou_max', iou_max, torch.float32), ('jmax', jmax, torch.int32), ('perm', perm, torch.int32),
                        ('n_gt', n_gt, torch.int32), ('n_det', n_det, torch.int32)):
        _eval_check(name, t, dt)
    dev = iou_max.device
    if out is None:
        out = torch.empty((2, T, C), dtype=torch.float32, device=dev)
    _eval_check('out', out, torch.float32)
    flag = torch.zeros((T, D), dtype=torch.uint8, device=dev) if with_flags else None
    cum = torch.zeros((T, D), dtype=torch.int32, device=dev) if with_flags else None
    ws = L.scratch(L.lib().u3d_eval_sweep_ws_bytes(D, G, T), dev)
    thr = (ctypes.c_float * max(T, 1))(*thresholds)
    L.call('u3d_eval_sweep', L.ptr(iou_max), L.ptr(jmax), L.ptr(perm), L.ptr(n_gt), L.ptr(n_det), thr, D, G, C, T, L.ptr(out[0]), L.ptr(out[1]),
           L.ptr(flag), L.ptr(cum), L.ptr(ws), L.stream())
    return (out[0], out[1], flag, cum) if with_flags else (out[0], out[1])
