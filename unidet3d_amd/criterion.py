"""Loss driver of the hot path (drives backward): matcher + per-layer CE + DIoU.

Same registry names, constructor arguments and call signatures as the reference
(unidet3d/criterion.py:7-178 ``UniDet3DCriterion``; :200-320 ``QueryClassificationCost``,
``BboxCostJointTraining``, ``UniMatcher``; unidet3d/axis_aligned_iou_loss.py:14-116
``UniDet3DAxisAlignedIoULoss``).  The tensors here are [n_queries, n_gt] -- tiny next to the
backbone -- so this stays on torch ops on the device, including the rotated
IoU / DIoU of ARKitScenes boxes (unidet3d/rotated_iou_loss.py; mmcv's polygon intersection as batched tensor ops).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from ._lib import h2d as _h2d
from ._lib import h2d_pack as _h2d_pack
from .ops import cat_views
from .registry import MODELS, TASK_UTILS
from .structures import InstanceData_


def _aligned_iou_3d(b1, b2, eps=1e-6):
    """mmdet3d AxisAlignedBboxOverlaps3D(is_aligned=True) on (x1,y1,z1,x2,y2,z2)."""
    d1 = b1[..., 3:] - b1[..., :3]
    d2 = b2[..., 3:] - b2[..., :3]
    wh = (torch.min(b1[..., 3:], b2[..., 3:]) - torch.max(b1[..., :3], b2[..., :3])).clamp(min=0)
    vol1 = d1[..., 0] * d1[..., 1] * d1[..., 2]          # explicit products: .prod()'s backward is a scan kernel
    vol2 = d2[..., 0] * d2[..., 1] * d2[..., 2]
    inter = wh[..., 0] * wh[..., 1] * wh[..., 2]
    union = torch.max(vol1 + vol2 - inter, inter.new_tensor([eps]))
    return inter / union


def axis_aligned_diou_loss(pred, target):
    """1 - IoU + centre_dist^2 / enclosing_diag^2 (axis_aligned_iou_loss.py:14-53), including
    the reference's ``[:, 0]`` indexing of the distance term (:51)."""
    iou_loss = 1 - _aligned_iou_3d(pred, target)
    pc = (pred[..., :3] + pred[..., 3:]) / 2
    tc = (target[..., :3] + target[..., 3:]) / 2
    r2 = ((pc - tc) ** 2).sum(-1, keepdim=True)
    lo = torch.minimum(pred[..., :3], target[..., :3])
    hi = torch.maximum(pred[..., 3:], target[..., 3:])
    c2 = ((lo - hi) ** 2).sum(-1, keepdim=True)
    return iou_loss + (r2 / c2)[:, 0]


@MODELS.register_module()
class UniDet3DAxisAlignedIoULoss(nn.Module):
    def __init__(self, mode='iou', reduction='mean', loss_weight=1.0):
        super().__init__()
        assert mode in ['iou', 'diou'] and reduction in ['none', 'sum', 'mean']
        self.mode, self.reduction, self.loss_weight = mode, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        reduction = reduction_override if reduction_override else self.reduction
        loss = axis_aligned_diou_loss(pred, target) if self.mode == 'diou' else 1 - _aligned_iou_3d(pred, target)
        if weight is not None:
            loss = loss * weight
        if reduction == 'mean':
            loss = loss.mean() if avg_factor is None else loss.sum() / avg_factor
        elif reduction == 'sum':
            loss = loss.sum()
        return loss * self.loss_weight


# ---- rotated boxes (ARKitScenes, angles=True): unidet3d/rotated_iou_loss.py -------------------------------------
# The BEV polygon intersection of mmcv.ops.diff_iou_rotated (box2corners, box_intersection, box1_in_box2,
# build_vertices, sort_indices + calculate_area) as batched tensor ops on whatever device the boxes live on: the 24
# candidate vertices are ordered by angle around their mean with one argsort (invalid candidates last, then overwritten
# by the first vertex so that they add nothing to the shoelace sum) instead of mmcv's per-box comparison-sort kernel.
def _box2corners(box):
    x, y, w, h, a = box.unbind(-1)
    x4 = torch.stack((0.5 * w, -0.5 * w, -0.5 * w, 0.5 * w), -1)
    y4 = torch.stack((0.5 * h, 0.5 * h, -0.5 * h, -0.5 * h), -1)
    c, s = torch.cos(a)[..., None], torch.sin(a)[..., None]
    return torch.stack((x4 * c - y4 * s + x[..., None], x4 * s + y4 * c + y[..., None]), -1)


def _corners_inside(c1, c2):
    a, b, d = c2[..., 0:1, :], c2[..., 1:2, :], c2[..., 3:4, :]
    ab, ad, am = b - a, d - a, c1 - a
    pab, pad = (ab * am).sum(-1) / (ab * ab).sum(-1), (ad * am).sum(-1) / (ad * ad).sum(-1)
    return (pab > -1e-6) & (pab < 1 + 1e-6) & (pad > -1e-6) & (pad < 1 + 1e-6)


def _oriented_box_intersection_2d(c1, c2):
    a1, a2 = c1[..., :, None, :], c1[..., [1, 2, 3, 0], :][..., :, None, :]
    b1, b2 = c2[..., None, :, :], c2[..., [1, 2, 3, 0], :][..., None, :, :]
    x1, y1, x2, y2 = a1[..., 0], a1[..., 1], a2[..., 0], a2[..., 1]
    x3, y3, x4, y4 = b1[..., 0], b1[..., 1], b2[..., 0], b2[..., 1]
    num = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4)
    den_t = (x1 - x3) * (y3 - y4) - (y1 - y3) * (x3 - x4)
    den_u = (x1 - x2) * (y1 - y3) - (y1 - y2) * (x1 - x3)
    par = num == 0
    safe = torch.where(par, torch.ones_like(num), num)
    t = torch.where(par, -torch.ones_like(num), den_t / safe)
    u = torch.where(par, -torch.ones_like(num), -den_u / safe)
    m_int = ((t > 0) & (t < 1) & (u > 0) & (u < 1)).flatten(-2, -1)
    t2 = den_t / (num + 1e-8)
    pts = torch.stack((x1 + t2 * (x2 - x1), y1 + t2 * (y2 - y1)), -1).flatten(-3, -2)
    verts = torch.cat((c1, c2, pts), -2)                                                    # (..., 24, 2)
    mask = torch.cat((_corners_inside(c1, c2), _corners_inside(c2, c1), m_int), -1)       # (..., 24)
    with torch.no_grad():
        # a candidate that repeats an earlier one (coincident boxes) is passed over, as mmcv's vertex sort does: the first copy stays
        same = ((verts[..., :, None, :] - verts[..., None, :, :]).abs() <= 1e-8).all(-1) & mask[..., None, :]
        mask = mask & ~torch.tril(same, -1).any(-1)
        nv = mask.sum(-1, keepdim=True).clamp(min=1)
        mean = (verts * mask[..., None]).sum(-2, keepdim=True) / nv[..., None]
        d = verts - mean
        ang = torch.where(mask, torch.atan2(d[..., 1], d[..., 0]), torch.full_like(d[..., 0], float('inf')))
        order = torch.argsort(ang, dim=-1)
    sv = torch.gather(verts, -2, order[..., None].expand(*order.shape, 2))
    sm = torch.gather(mask, -1, order)
    sv = torch.where(sm[..., None], sv, sv[..., :1, :])
    nx = torch.roll(sv, -1, -2)
    area = (sv[..., 0] * nx[..., 1] - sv[..., 1] * nx[..., 0]).sum(-1).abs() / 2
    return torch.where(mask.sum(-1) >= 3, area, torch.zeros_like(area))


def diff_iou_rotated_3d(box3d1, box3d2, diou: bool):
    """(..., 7) (x, y, z, w, h, l, alpha) pairs -> (...,) IoU, or DIoU as ``diff_diou_rotated_3d`` computes it
    (rotated_iou_loss.py:14-60; its centre term is over the first three entries of the BEV vectors, (dx, dy, dw), :58)."""
    box1, box2 = box3d1[..., [0, 1, 3, 4, 6]], box3d2[..., [0, 1, 3, 4, 6]]
    c1, c2 = _box2corners(box1), _box2corners(box2)
    inter = _oriented_box_intersection_2d(c1, c2)
    zmax1, zmin1 = box3d1[..., 2] + box3d1[..., 5] * 0.5, box3d1[..., 2] - box3d1[..., 5] * 0.5
    zmax2, zmin2 = box3d2[..., 2] + box3d2[..., 5] * 0.5, box3d2[..., 2] - box3d2[..., 5] * 0.5
    inter3d = inter * (torch.min(zmax1, zmax2) - torch.max(zmin1, zmin2)).clamp(min=0.)
    union3d = box3d1[..., 3] * box3d1[..., 4] * box3d1[..., 5] + box3d2[..., 3] * box3d2[..., 4] * box3d2[..., 5] - inter3d
    iou = inter3d / union3d
    if not diou:
        return iou
    x_max = torch.max(c1[..., 0].max(-1)[0], c2[..., 0].max(-1)[0]); x_min = torch.min(c1[..., 0].min(-1)[0], c2[..., 0].min(-1)[0])
    y_max = torch.max(c1[..., 1].max(-1)[0], c2[..., 1].max(-1)[0]); y_min = torch.min(c1[..., 1].min(-1)[0], c2[..., 1].min(-1)[0])
    z_max, z_min = torch.max(zmax1, zmax2), torch.min(zmin1, zmin2)
    r2 = ((box1[..., :3] - box2[..., :3]) ** 2).sum(-1)
    c2_ = (x_min - x_max) ** 2 + (y_min - y_max) ** 2 + (z_min - z_max) ** 2
    return iou - r2 / c2_


@MODELS.register_module()
class UniDet3DRotatedIoU3DLoss(nn.Module):
    """1 - IoU ('iou', mmdet3d ``rotated_iou_3d_loss``) or 1 - DIoU ('diou') of rotated boxes, with the weight / reduction
    handling of mmdet's ``weighted_loss`` (rotated_iou_loss.py:85-151)."""

    def __init__(self, mode='iou', reduction='mean', loss_weight=1.0):
        super().__init__()
        assert mode in ('iou', 'diou') and reduction in ('none', 'sum', 'mean')
        self.mode, self.reduction, self.loss_weight = mode, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        if weight is not None and not torch.any(weight > 0):
            return pred.sum() * weight.sum()
        reduction = reduction_override if reduction_override else self.reduction
        if weight is not None and weight.dim() > 1:
            weight = weight.mean(-1)
        loss = 1 - diff_iou_rotated_3d(pred, target, self.mode == 'diou')
        if weight is not None:
            loss = loss * weight
        if avg_factor is None:
            loss = loss.mean() if reduction == 'mean' else (loss.sum() if reduction == 'sum' else loss)
        elif reduction == 'mean':
            loss = loss.sum() / (avg_factor + torch.finfo(torch.float32).eps)
        elif reduction != 'none':
            raise ValueError('avg_factor can not be used with reduction="sum"')
        return loss * self.loss_weight


def _bbox_to_loss(bbox):                       # criterion.py:180-198
    if bbox.shape[-1] != 6:
        return bbox
    half = bbox[..., 3:] / 2
    return torch.cat((bbox[..., :3] - half, bbox[..., :3] + half), dim=-1)


@TASK_UTILS.register_module()
class QueryClassificationCost:
    def __init__(self, weight):
        self.weight = weight

    def __call__(self, pred_instances, gt_instances, **kwargs):
        return -pred_instances.scores.softmax(-1)[:, gt_instances.labels] * self.weight


@TASK_UTILS.register_module()
class BboxCostJointTraining:
    def __init__(self, weight, loss_simple, loss_rotated):
        self.weight = weight
        self.loss_simple = MODELS.build(loss_simple)
        self.loss_rotated = MODELS.build(loss_rotated)

    def __call__(self, pred_instances, gt_instances, **kwargs):
        n, g = pred_instances.bboxes.shape[0], gt_instances.bboxes.shape[0]
        assert gt_instances.bboxes.shape[1] == pred_instances.bboxes.shape[1]
        pb = pred_instances.bboxes.unsqueeze(1).expand(n, g, -1)
        gb = gt_instances.bboxes.unsqueeze(0).expand(n, g, -1)
        loss = self.loss_rotated if gt_instances.bboxes.shape[1] == 7 else self.loss_simple
        return loss(_bbox_to_loss(pb), _bbox_to_loss(gb)) * self.weight


@TASK_UTILS.register_module()
class UniMatcher:
    """Each GT keeps its ``topk`` cheapest queries among those its mask allows (criterion.py:272-320)."""

    def __init__(self, costs):
        self.costs = [TASK_UTILS.build(c) for c in costs]
        self.inf = 1e8

    @torch.no_grad()
    def __call__(self, pred_instances, gt_instances, topk, **kwargs):
        labels = gt_instances.labels
        if len(labels) == 0:
            return labels.new_empty((0,)), labels.new_empty((0,))
        cost = torch.stack([c(pred_instances, gt_instances) for c in self.costs]).sum(dim=0)
        cost = torch.where(gt_instances.query_masks.T, cost, cost.new_tensor(self.inf))
        kth = torch.topk(cost, topk + 1, dim=0, sorted=True, largest=False).values[-1:, :]
        ids = torch.argwhere(cost < kth)
        return ids[:, 0], ids[:, 1]


class _FusedCriterionFn(torch.autograd.Function):
    """include/u3d.h u3d_criterion_packed: the loss AND its gradients w.r.t. the stacked head outputs in five launches (six when a
    scene has more than 64 GTs)."""

    @staticmethod
    def forward(ctx, cls, box, g, consts):
        cls, box = cls.contiguous(), box.contiguous()
        Ln, n_tot, CU = cls.shape
        BD = box.shape[-1]
        dev = cls.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dcls, dbox = torch.empty_like(cls), torch.empty_like(box)
        ws = L.scratch(L.lib().u3d_criterion_ws_bytes_gt(Ln, g['B'], n_tot, g['G'], g['P'], g['max_gt']), dev)
        L.call('u3d_criterion_packed', L.ptr(cls), L.ptr(box), L.ptr(g['cu']), L.ptr(g['gt_off']), L.ptr(g['labels']), L.ptr(g['boxes']),
               L.ptr(g['qmask']), L.ptr(g['qm_off']), L.ptr(g['meta']), L.ptr(g['scene_w']), L.ptr(g['cidx']), Ln, g['B'], n_tot, CU, BD,
               g['G'], g['P'], g['max_gt'], g['slack'], *consts, L.ptr(loss), L.ptr(dcls), L.ptr(dbox), L.ptr(ws), L.stream())
        ctx.save_for_backward(dcls, dbox)
        return loss[0]

    @staticmethod
    def backward(ctx, go):
        dcls, dbox = ctx.saved_tensors
        return dcls * go, dbox * go, None, None


def _gt_boxes(b):
    rows = getattr(b, 'gt_rows', None)
    if rows is not None and rows.shape[0] == b.tensor.shape[0]:       # computed once for the whole batch (UniDet3D._prepare_train)
        return rows
    return torch.cat((b.gravity_center, b.tensor[:, 3:] if b.with_yaw else b.tensor[:, 3:6]), dim=1)


@MODELS.register_module()
class UniDet3DCriterion:
    def __init__(self, matcher, loss_weight, non_object_weight, iter_matcher, bbox_loss_simple, bbox_loss_rotated,
                 datasets, datasets_weights, topk):
        self.bbox_loss_simple = MODELS.build(bbox_loss_simple)
        self.bbox_loss_rotated = MODELS.build(bbox_loss_rotated)
        self.matcher = TASK_UTILS.build(matcher)
        self.non_object_weight = non_object_weight
        self.loss_weight = loss_weight
        self.iter_matcher = iter_matcher
        self.datasets = datasets
        self.datasets_weights = datasets_weights
        self.topk = topk

    def get_layer_loss(self, aux_outputs, insts, datasets_names, indices=None):
        cls_preds, pred_bboxes = aux_outputs['cls_preds'], aux_outputs['bboxes']
        if indices is None:
            indices = []
            for i, inst in enumerate(insts):
                idx = self.datasets.index(datasets_names[i])
                pred = InstanceData_(scores=cls_preds[i], bboxes=pred_bboxes[i])
                gt = InstanceData_(labels=inst.labels_3d, query_masks=inst.query_masks, bboxes=_gt_boxes(inst.bboxes_3d))
                indices.append(self.matcher(pred, gt, self.topk[idx]))
        cls_losses, bbox_losses = [], []
        for name, cls_pred, bbox, inst, (idx_q, idx_gt) in zip(datasets_names, cls_preds, pred_bboxes, insts, indices):
            weight = self.datasets_weights[self.datasets.index(name)]
            n_cls = cls_pred.shape[1] - 1
            target = cls_pred.new_full((len(cls_pred),), n_cls, dtype=torch.long)
            # a query matched by several GTs: the reference's index assignment keeps the LAST pair (criterion.py:98-99; on a GPU
            # the order of duplicate writes is undefined).  The matcher returns pairs sorted by (query, gt), so the last pair of
            # every run of equal query ids is the winner -- written through unique indices, deterministic on any device.
            if len(idx_q):
                last = torch.ones_like(idx_q, dtype=torch.bool)
                last[:-1] = idx_q[1:] != idx_q[:-1]
                target[idx_q[last]] = inst.labels_3d[idx_gt[last]]
            cw = cls_pred.new_ones(n_cls + 1)
            cw[-1] = self.non_object_weight
            cls_losses.append(weight * F.cross_entropy(cls_pred, target, cw))
            if len(inst) == 0 or len(idx_q) == 0:
                continue
            tgt = _gt_boxes(inst.bboxes_3d[idx_gt])
            loss_fn = self.bbox_loss_rotated if tgt.shape[1] == 7 else self.bbox_loss_simple
            bbox_losses.append(weight * loss_fn(_bbox_to_loss(bbox[idx_q]), _bbox_to_loss(tgt)).mean())
        cls_loss = torch.mean(torch.stack(cls_losses))
        # no match anywhere in the batch: the reference adds the Python int 0 (criterion.py:137-138).  Same value here, but
        # connected to the graph so that every parameter receives a gradient on every rank (the data-parallel bucket
        # schedule relies on it)
        # (b * 0 would turn an overflowed box parameter -- exp() of a large prediction -- into NaN where the reference returns 0)
        bbox_loss = torch.stack(bbox_losses).mean() if bbox_losses else sum(torch.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0).sum() for b in pred_bboxes) * 0
        return self.loss_weight[0] * cls_loss + self.loss_weight[1] * bbox_loss

    # ---- packed fast path ---------------------------------------------------------------------
    # Same arithmetic as get_layer_loss, but every scene of the batch goes through ONE set of
    # [B, n_max, g_max] tensor ops instead of a Python loop of ~70 small kernels per (layer, scene):
    # the reference's loop (criterion.py:79-134) costs thousands of launches per step on a GPU.
    def _matcher_ok(self):
        return (isinstance(self.matcher, UniMatcher) and len(self.matcher.costs) == 2 and
                isinstance(self.matcher.costs[0], QueryClassificationCost) and
                isinstance(self.matcher.costs[1], BboxCostJointTraining))

    def _can_pack(self, pred, insts, datasets_names):
        """single-dataset yaw-free batch with the decoder's packed head outputs: the batched tensor-op formulation applies"""
        if '_packed' not in pred or len(set(datasets_names)) != 1 or not self.iter_matcher or not self._matcher_ok():
            return False
        pk = pred['_packed']
        return pk.get('cidx') is None and all((not i.bboxes_3d.with_yaw) for i in insts) and pk['box'][0].shape[-1] == 6

    def _can_fuse(self, pred, insts, datasets_names):
        """what csrc/criterion.hip takes: the decoder's packed head outputs of ANY batch -- one dataset or several, 6-dof boxes
        or boxes with a heading -- under the reference configs' matcher and DIoU losses"""
        if '_packed' not in pred or not self.iter_matcher or not self.fused or not self._fusable():
            return False
        pk = pred['_packed']
        if not (pk['cls_stacked'] if 'cls_stacked' in pk else pk['cls'][0]).is_cuda:
            return False
        bd = (pk['box_stacked'] if 'box_stacked' in pk else pk['box'][0]).shape[-1]
        yaw = pk.get('yaw') or [bd == 7] * len(insts)
        return all(bool(i.bboxes_3d.with_yaw) == bool(y) or len(i) == 0 for i, y in zip(insts, yaw))

    def _pack_gt(self, insts, sizes, device):
        B, g_max, n_max = len(insts), max(max(len(i) for i in insts), 1), max(sizes)
        labels = torch.zeros(B, g_max, dtype=torch.long, device=device)
        boxes = torch.zeros(B, g_max, 6, device=device)
        boxes[..., 3:] = 1.0                                   # harmless unit boxes for the padding slots
        qmask = torch.zeros(B, g_max, n_max, dtype=torch.bool, device=device)
        for b, inst in enumerate(insts):
            g = len(inst)
            if g:
                labels[b, :g] = inst.labels_3d
                boxes[b, :g] = _gt_boxes(inst.bboxes_3d)
                qmask[b, :g, :sizes[b]] = inst.query_masks
        valid = torch.zeros(B, n_max, dtype=torch.bool, device=device)
        dest = []
        for b, n in enumerate(sizes):
            valid[b, :n] = True
            dest.append(torch.arange(b * n_max, b * n_max + n, device=device))
        rows = torch.cat(dest)                                  # packed row -> slot in the padded batch
        has_gt = _h2d([len(i) > 0 for i in insts], torch.bool, device)
        return dict(labels=labels, boxes=boxes, qmask=qmask.transpose(1, 2), rows=rows, valid=valid, has_gt=has_gt,
                    uniform=len(set(sizes)) == 1)

    def _loss_packed(self, cls, box, gt, name):
        """All decoder layers and all scenes at once: cls [L, sum n_i, C+1], box [L, sum n_i, 6] ->
        sum over layers of (w_cls * mean_scenes CE + w_box * mean_scenes DIoU) with per-layer re-matching."""
        idx = self.datasets.index(name)
        weight, topk = self.datasets_weights[idx], self.topk[idx]
        L = cls.shape[0]
        B, n = gt['valid'].shape
        if gt['uniform']:
            cls_b, box_b = cls.view(L, B, n, -1), box.view(L, B, n, 6)
        else:       # index_copy into the padded layout: its backward is an index_select (no scatter-add kernel)
            rows = (gt['rows'][None] + torch.arange(L, device=cls.device)[:, None] * (B * n)).reshape(-1)
            cls_b = cls.new_zeros(L * B * n, cls.shape[-1]).index_copy(0, rows, cls.reshape(-1, cls.shape[-1])).view(L, B, n, -1)
            pad_box = box.new_zeros(L * B * n, 6)
            pad_box[:, 3:] = 1.0
            box_b = pad_box.index_copy(0, rows, box.reshape(-1, 6)).view(L, B, n, 6)
        n_cls = cls_b.shape[-1] - 1
        g = gt['labels'].shape[1]
        labels = gt['labels'][None].expand(L, -1, -1)                              # [L,B,g]
        gtb = _bbox_to_loss(gt['boxes'])[None, :, None]                            # [1,B,1,g,6]
        pbx = _bbox_to_loss(box_b)[:, :, :, None]                                  # [L,B,n,1,6]

        def diou_terms(pb):
            iou_loss = 1 - _aligned_iou_3d(pb, gtb)                                # [L,B,n,g]
            pc, tc = (pb[..., :3] + pb[..., 3:]) / 2, (gtb[..., :3] + gtb[..., 3:]) / 2
            r2 = ((pc - tc) ** 2).sum(-1)
            c2 = ((torch.minimum(pb[..., :3], gtb[..., :3]) - torch.maximum(pb[..., 3:], gtb[..., 3:])) ** 2).sum(-1)
            return iou_loss, r2 / c2

        with torch.no_grad():                                                      # UniMatcher (criterion.py:286-320)
            prob = cls_b.softmax(-1)
            c_cls = -prob.gather(3, labels[:, :, None, :].expand(-1, -1, n, -1)) * self.matcher.costs[0].weight
            iou_loss, rc = diou_terms(pbx)
            c_box = (iou_loss + rc[..., :1]) * self.matcher.costs[1].weight        # the reference's [:, 0] term
            cost = torch.where(gt['qmask'][None], c_cls + c_box, cls_b.new_tensor(self.matcher.inf))
            kth = torch.topk(cost, topk + 1, dim=2, sorted=True, largest=False).values[:, :, -1:, :]
            matched = cost < kth                                                   # [L,B,n,g]
            last = (matched * torch.arange(1, g + 1, device=cls.device)).amax(3) - 1   # highest matched gt wins
            target = torch.where(last >= 0, labels.gather(2, last.clamp(min=0)), n_cls)
            cw = cls_b.new_ones(n_cls + 1)
            cw[-1] = self.non_object_weight
            w = cw[target] * gt['valid'][None]
        nll = -torch.log_softmax(cls_b, -1).gather(3, target[..., None])[..., 0]
        cls_loss = (weight * (nll * w).sum(2) / w.sum(2)).mean(1)                  # [L]
        iou_loss, rc = diou_terms(pbx)
        diou = iou_loss + rc
        cnt = matched.sum((2, 3))                                                  # [L,B]
        per_scene = (torch.where(matched, diou, diou.new_zeros(())).sum((2, 3)) / cnt.clamp(min=1)) * weight
        has = (cnt > 0) & gt['has_gt'][None]
        bbox_loss = (per_scene * has).sum(1) / has.sum(1).clamp(min=1)             # [L]
        return (self.loss_weight[0] * cls_loss + self.loss_weight[1] * bbox_loss).sum()

    # ---- fused device path (csrc/criterion.hip) ---------------------------------------------------
    def _flat_gt(self, insts, sizes, device, topks, weights, c1s, yaw, cidx, bd):
        """Ragged GT and per-scene dataset constants of the batch as flat device arrays for u3d_criterion_packed; None when the
        kernel's one condition does not hold (a scene with GT but fewer than topk + 1 queries -- left to the per-scene path, which
        raises like the reference).  The number of GTs of a scene is not limited: the kernel keeps ceil(max_gt / 64) mask words."""
        gs = [len(i) for i in insts]
        if any(g and n < k + 1 for g, n, k in zip(gs, sizes, topks)):
            return None
        for b, (n, g) in enumerate(zip(sizes, gs)):
            if n * g > 0x7fffffff:
                raise ValueError(f'criterion: scene {b} has {n} queries x {g} ground-truth boxes, beyond the 32-bit index range of the kernel')
        cu, go, qo = [0], [0], [0]
        for n, g in zip(sizes, gs):
            cu.append(cu[-1] + n); go.append(go[-1] + g); qo.append(qo[-1] + n * g)
        with_gt = [i for i in insts if len(i)]
        labels = torch.cat([i.labels_3d for i in with_gt]) if with_gt else None
        boxes = None
        if with_gt:
            rows = [_gt_boxes(i.bboxes_3d).float() for i in with_gt]
            rows = [r if r.shape[1] == bd else torch.nn.functional.pad(r, (0, bd - r.shape[1])) for r in rows]
            boxes = cat_views(rows).contiguous()           # row views of one cached tensor: no copy
        qmask = torch.cat([i.query_masks.reshape(-1) for i in with_gt]).contiguous().view(torch.uint8) if with_gt else None
        meta, coff, cflat = [], 0, []
        for b in range(len(insts)):
            meta.append([int(c1s[b]), int(topks[b]), int(bool(yaw[b])), coff])
            if cidx is not None:
                cflat.extend(int(c) for c in cidx[b])
                coff += len(cidx[b])
        # the six small host arrays travel in ONE pinned buffer / one H2D copy
        cu_d, go_d, qo_d, meta_d, w_d, cidx_d = _h2d_pack(
            [(cu, torch.int32), (go, torch.int32), (qo, torch.int64), (meta, torch.int32), ([float(w) for w in weights], torch.float32),
             (cflat if cidx is not None else [], torch.int32)], device)
        return dict(B=len(insts), G=go[-1], P=qo[-1], max_gt=max(gs, default=0),
                    slack=min([n - (k + 1) for g, n, k in zip(gs, sizes, topks) if g], default=0),
                    cu=cu_d, gt_off=go_d, qm_off=qo_d, meta=meta_d.view(-1, 4), scene_w=w_d,
                    cidx=cidx_d if cidx is not None else None,
                    labels=labels, boxes=boxes, qmask=qmask)

    @staticmethod
    def _stacked(pk):
        """[L, sum n_i, .] head outputs: the decoder's own stacked views when it evaluated the head once over all layers"""
        if 'cls_stacked' in pk:
            return pk['cls_stacked'], pk['box_stacked']
        return torch.stack(pk['cls']), torch.stack(pk['box'])

    def _loss_fused(self, pk, insts, names):
        """``names``: the dataset of every scene.  ``pk`` (UniDet3DEncoder): stacked logits [L, sum n_i, CU] and boxes [L, sum n_i, 6 | 7]
        plus, for a mixed batch, ``cidx`` (per scene: the columns of its dataset's classes, "no object" last) and ``yaw`` (per scene:
        its boxes carry a heading)."""
        cls, box = self._stacked(pk)
        B, bd = len(insts), box.shape[-1]
        idxs = [self.datasets.index(n) for n in names]
        cidx = pk.get('cidx')
        c1s = [len(c) for c in cidx] if cidx is not None else [cls.shape[-1]] * B
        yaw = pk.get('yaw') or [bd == 7] * B
        g = self._flat_gt(insts, pk['sizes'], cls.device, [self.topk[i] for i in idxs], [self.datasets_weights[i] for i in idxs], c1s, yaw,
                          cidx, bd)
        if g is None:
            return None
        consts = (float(self.matcher.costs[0].weight), float(self.matcher.costs[1].weight), float(self.non_object_weight),
                  float(self.loss_weight[0]), float(self.loss_weight[1]))
        return _FusedCriterionFn.apply(cls, box, g, consts)

    def _fusable(self):
        """The fused kernel hard-codes the ScanNet config's matcher (configs/unidet3d_1xb8_scannet.py:75-84): exactly
        [QueryClassificationCost, BboxCostJointTraining] in this order, DIoU with weight 1 and no reduction inside the cost."""
        costs = self.matcher.costs
        if len(costs) != 2 or not isinstance(costs[0], QueryClassificationCost) or not isinstance(costs[1], BboxCostJointTraining):
            return False
        c = costs[1]
        if getattr(c.loss_simple, 'reduction', None) != 'none':
            return False
        rot_ok = all(isinstance(r, UniDet3DRotatedIoU3DLoss) and r.mode == 'diou' and r.loss_weight == 1.0 and r.reduction == 'none'
                     for r in (c.loss_rotated, self.bbox_loss_rotated))
        return (rot_ok and isinstance(c.loss_simple, UniDet3DAxisAlignedIoULoss) and c.loss_simple.mode == 'diou' and c.loss_simple.loss_weight == 1.0 and
                isinstance(self.bbox_loss_simple, UniDet3DAxisAlignedIoULoss) and self.bbox_loss_simple.mode == 'diou' and
                self.bbox_loss_simple.loss_weight == 1.0 and self.bbox_loss_simple.reduction == 'none')

    fused = True        # device kernel (csrc/criterion.hip) for packed head outputs; False forces the tensor-op formulations (tests)

    def __call__(self, pred, insts, datasets_names):
        if self._can_fuse(pred, insts, datasets_names):
            loss = self._loss_fused(pred['_packed'], insts, datasets_names)
            if loss is not None:
                return {'det_loss': loss}
        if self._can_pack(pred, insts, datasets_names):
            pk = pred['_packed']
            gt = self._pack_gt(insts, pk['sizes'], pk['cls'][0].device)
            # final layer + the aux layers, each re-matched (iter_matcher), in one batched pass
            return {'det_loss': self._loss_packed(*self._stacked(pk), gt, datasets_names[0])}
        loss = self.get_layer_loss(pred, insts, datasets_names)
        if 'aux_outputs' in pred:
            indices = None        # iter_matcher=True re-matches per layer; the reference leaves `indices`
            if not self.iter_matcher:   # undefined otherwise (criterion.py:171-176) -- same requirement here
                raise NotImplementedError('iter_matcher=False is not exercised by the reference configs')
            for aux in pred['aux_outputs']:
                loss = loss + self.get_layer_loss(aux, insts, datasets_names, indices)
        return {'det_loss': loss}
