"""Shared inputs of the device-evaluation tests (tests/test_eval_cases_cpu.py, tests/test_gpu_eval_device.py): deterministic
validation passes whose every IoU is known in closed form, and a host restatement of the evaluation protocol with a STABLE order.

Boxes come from a lattice: ground truths of one size sit on sites 4 m apart, and a detection is its ground truth shifted by ``s`` of the
box's length along one of the box's OWN axes, so that IoU = (1 - s) / (1 + s): s in {0, 0.25, 0.5, 0.75, >= 1} gives {1, 0.6, 1/3, 1/7, 0},
each at least 0.08 from the thresholds 0.25 and 0.5.  The rotated variants use the same construction with a common non-zero heading
per image.  Nothing here touches a GPU."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np
import torch

THRESHOLDS = (0.25, 0.5)
SIZE = np.array([1.0, 0.8, 0.6])
PITCH = 4.0
IOU_OF_SHIFT = {0.0: 1.0, 0.25: 0.6, 0.5: 1 / 3, 0.75: 1 / 7, 1.5: 0.0}


@dataclass
class Case:
    name: str
    n_classes: int
    gt: List[tuple] = field(default_factory=list)        # per image (boxes float32 [n, 6 or 7], labels int64 [n])
    dt: List[tuple] = field(default_factory=list)        # per image (boxes float32 [n, 6 or 7], scores float32 [n], labels int64 [n])
    tied: bool = False                                   # scores tie inside a class: only the stable order is defined


def site(k: int) -> np.ndarray:
    """Bottom centre of lattice site k (a 16 x 16 x ... grid in x, y; z varies a little so that z_bottom is not always 0)."""
    return np.array([PITCH * (k % 16), PITCH * (k // 16 % 16), 0.25 * (k % 3)])


def box(k: int, shift: float = 0.0, axis: int = 0, heading: float = 0.0, cols: int = 7) -> np.ndarray:
    """The box of site k moved by ``shift`` of its extent along its own axis ``axis``."""
    c, s = np.cos(heading), np.sin(heading)
    ax = (np.array([c, s]), np.array([-s, c]))
    mv = ax[axis] * shift * SIZE[axis]
    p = site(k)
    row = [p[0] + mv[0], p[1] + mv[1], p[2], *SIZE, heading]
    return np.asarray(row[:cols], np.float32)


def _img(case: Case, gts, dts, gt_cols=7, dt_cols=7):
    """gts: [(box row, label)], dts: [(box row, score, label)]"""
    gb = np.stack([g[0] for g in gts]).astype(np.float32) if gts else np.zeros((0, gt_cols), np.float32)
    db = np.stack([d[0] for d in dts]).astype(np.float32) if dts else np.zeros((0, dt_cols), np.float32)
    case.gt.append((gb, np.asarray([g[1] for g in gts], np.int64)))
    case.dt.append((db, np.asarray([d[1] for d in dts], np.float32), np.asarray([d[2] for d in dts], np.int64)))


def _basic(name: str, h: float) -> Dict[str, Case]:
    out = {}
    # (a) two detections claim one ground truth: the higher score wins, the other is a false positive
    c = Case(f'a{name}', 2)
    _img(c, [(box(0, heading=h), 0), (box(1, heading=h), 1)],
         [(box(0, 0.0, heading=h), 0.9, 0), (box(0, 0.25, heading=h), 0.8, 0), (box(1, 0.25, 1, heading=h), 0.7, 1), (box(1, 0.0, heading=h), 0.6, 1)])
    out[c.name] = c
    # (b) the claim flips between thresholds: higher score at IoU 1/3, lower score at IoU 0.6
    c = Case(f'b{name}', 1)
    _img(c, [(box(2, heading=h), 0)], [(box(2, 0.5, heading=h), 0.9, 0), (box(2, 0.25, 1, heading=h), 0.8, 0)])
    out[c.name] = c
    # (c) best ground truth taken, second best free: a false positive all the same.  A at the site, B 0.75 lengths on; Y sits on A
    # (IoU 1 / 1/7), X 0.25 on (IoU 0.6 with A, 1/3 with B) and scores lower
    c = Case(f'c{name}', 1)
    _img(c, [(box(3, heading=h), 0), (box(3, 0.75, heading=h), 0)], [(box(3, 0.25, heading=h), 0.5, 0), (box(3, 0.0, heading=h), 0.9, 0)])
    out[c.name] = c
    # (d) two bit-identical ground truths: the first index wins, for both detections
    c = Case(f'd{name}', 2)
    _img(c, [(box(5, heading=h), 1), (box(4, heading=h), 0), (box(4, heading=h), 0)],
         [(box(4, 0.0, heading=h), 0.7, 0), (box(4, 0.25, heading=h), 0.6, 0), (box(5, 0.5, 1, heading=h), 0.4, 1)])
    out[c.name] = c
    # (h) tied scores within a class: the order is by packed index
    c = Case(f'h{name}', 2, tied=True)
    _img(c, [(box(6, heading=h), 0), (box(7, heading=h), 0), (box(8, heading=h), 1)],
         [(box(6, 0.25, heading=h), 0.5, 0), (box(6, 0.0, heading=h), 0.5, 0), (box(7, 0.5, heading=h), 0.5, 0), (box(8, 0.0, heading=h), 0.5, 1),
          (box(7, 0.25, 1, heading=h), 0.5, 0), (box(8, 0.25, heading=h), 0.5, 1), (box(6, 0.5, 1, heading=h), 0.75, 0)])
    _img(c, [(box(9, heading=h), 0)], [(box(9, 0.25, heading=h), 0.5, 0), (box(9, 0.0, heading=h), 0.5, 0), (box(9, 1.5, heading=h), 0.5, 1)])
    out[c.name] = c
    return out


def build_cases() -> Dict[str, Case]:
    cases = {}
    cases.update(_basic('', 0.0))
    cases.update(_basic('_rot', 0.4))
    # (e) empty images on either side; class 3: detections and no ground truth anywhere (NaN); class 4: ground truths and no
    # detections (0); class 5 absent from both (no key); class 0 ordinary
    c = Case('e', 7)
    _img(c, [(box(0), 0), (box(1), 4)], [])                                                     # no detections
    _img(c, [], [(box(2), 0.9, 0), (box(3), 0.8, 3)])                                           # no ground truths
    _img(c, [], [])
    _img(c, [(box(4), 0), (box(5), 4), (box(6), 6)], [(box(4, 0.25), 0.7, 0), (box(5, 0.0), 0.6, 3), (box(6, 0.5), 0.65, 6), (box(7), -0.5, 0)])
    cases[c.name] = c
    # (f) class 1 has 3000 detections over 40 images (longer than one workgroup's scan tile, and it starts at an odd rank behind
    # class 0's 37 detections); image 0 has 150 ground truths (more than one LDS chunk), its class-1 ones spread over all chunks
    c = Case('f', 3)
    rng = np.random.RandomState(7)
    shifts = np.array(sorted(IOU_OF_SHIFT))
    score1 = rng.permutation(3000).astype(np.float64) / 3000.0 - 0.1            # distinct, some negative
    score0 = rng.permutation(37).astype(np.float64) / 64.0 + 0.01
    n1 = n0 = 0
    for im in range(40):
        n_gt = 150 if im == 0 else 10
        gts = [(box(k), 1 if k % 3 else 0) for k in range(n_gt)]
        ones = [k for k in range(n_gt) if k % 3]
        dts = []
        for q in range(75):
            k = ones[int(rng.randint(len(ones)))]                                 # a class-1 site
            dts.append((box(k, float(shifts[rng.randint(5)]), int(rng.randint(2))), float(score1[n1]), 1))
            n1 += 1
        if im < 37:
            dts.insert(im, (box(3 * (im % 3), float(shifts[im % 5])), float(score0[n0]), 0))
            n0 += 1
        _img(c, gts, dts)
    cases[c.name] = c
    # (g) six- and seven-column inputs mixed between detections and ground truths
    c = Case('g', 2)
    _img(c, [(box(0), 0), (box(1), 1)], [(box(0, 0.25, cols=6), 0.9, 0), (box(1, 0.5, 1, cols=6), 0.8, 1), (box(0, 0.0, cols=6), 0.3, 0)], 7, 6)
    _img(c, [(box(2, cols=6), 0), (box(3, cols=6), 1)], [(box(2, 0.5), 0.85, 0), (box(3, 0.0), 0.6, 1), (box(3, 0.75, 1), 0.95, 1)], 6, 7)
    _img(c, [(box(4, heading=-1.1), 0)], [(box(4, 0.25, heading=-1.1), 0.4, 0), (box(4, 0.75, 1, heading=-1.1), 0.45, 0)])
    cases[c.name] = c
    return cases


def annos(case: Case, device='cpu', gt_device=None):
    """(gt_annos, dt_annos) as ``indoor_eval`` takes them; ground-truth labels as a list of int, like the reference's annotations."""
    gt = [dict(gt_bboxes_3d=torch.from_numpy(b).to(gt_device or 'cpu'), gt_labels_3d=[int(x) for x in l]) for b, l in case.gt]
    dt = [dict(bboxes_3d=torch.from_numpy(b).to(device), scores_3d=torch.from_numpy(s).to(device), labels_3d=torch.from_numpy(l).to(device))
          for b, s, l in case.dt]
    return gt, dt


def label2cat(case: Case):
    return [f'c{i}' for i in range(case.n_classes)]


def host_match(case: Case):
    """What ``indoor_eval`` derives per detection, in packed order, from the host ``boxes_iou_3d`` called per image as it calls it:
    label, score, iou_max (float32, -inf without a same-class ground truth), jmax (PACKED ground-truth index, -1), aligned (the
    image took the axis-aligned formula), pairs (all same-class IoUs of the detection, float32)."""
    from unidet3d_amd.evaluation import boxes_iou_3d
    lab, score, iou_max, jmax, aligned, pairs = [], [], [], [], [], []
    g0 = 0
    for (gb, gl), (db, ds, dl) in zip(case.gt, case.dt):
        iou = boxes_iou_3d(torch.from_numpy(db), torch.from_numpy(gb)).numpy() if len(dl) and len(gl) else np.zeros((len(dl), len(gl)), np.float32)
        al = not ((db.shape[1] == 7 and (db[:, 6] != 0).any()) or (gb.shape[1] == 7 and (gb[:, 6] != 0).any()))
        for d in range(len(dl)):
            sel = np.nonzero(gl == dl[d])[0]
            lab.append(int(dl[d])); score.append(ds[d]); aligned.append(al)
            if len(sel):
                sub = iou[d, sel]
                iou_max.append(sub.max()); jmax.append(g0 + int(sel[sub.argmax()])); pairs.append(sub.astype(np.float32))
            else:
                iou_max.append(-np.inf); jmax.append(-1); pairs.append(np.zeros(0, np.float32))
        g0 += len(gl)
    return dict(label=np.asarray(lab, np.int64), score=np.asarray(score, np.float32), iou_max=np.asarray(iou_max, np.float32),
                jmax=np.asarray(jmax, np.int64), aligned=np.asarray(aligned, bool), pairs=pairs, n_gts=g0)


def first_claimant(score: np.ndarray, iou_max: np.ndarray, jmax: np.ndarray, thr: float):
    """The parallel rule for one class: in STABLE descending-score order, a detection is a true positive iff iou_max > thr and it is
    the first among those with iou_max > thr that name the same ground truth.  Returns (order, tp bool in that order)."""
    order = np.argsort(-score, kind='stable')
    q = iou_max[order] > thr
    g = jmax[order]
    rank = np.arange(len(order))
    claim = np.full(int(g.max()) + 2 if len(g) else 1, len(order), np.int64)
    np.minimum.at(claim, g[q], rank[q])
    return order, q & (claim[g] == rank)


def curves(tp: np.ndarray, npos: int):
    """recall, precision (fp64) of a class from its true-positive flags in evaluation order, as ``eval_det_cls`` forms them."""
    tpc, fpc = np.cumsum(tp.astype(np.float64)), np.cumsum((~tp).astype(np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        recall = tpc / float(npos)
    return recall, tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)


def reference_eval(case: Case, thresholds=THRESHOLDS, m=None) -> dict:
    """The result dictionary of ``indoor_eval`` from the parallel rule with a stable order (the reference for tied scores, where the
    host's ``np.argsort`` is not stable by contract)."""
    from unidet3d_amd.evaluation import average_precision
    m = m or host_match(case)
    names = label2cat(case)
    gl = np.concatenate([l for _, l in case.gt]) if case.gt else np.zeros(0, np.int64)
    classes = sorted(set(m['label'].tolist()) | set(gl.tolist()))
    ret = {}
    for thr in thresholds:
        aps, recs = [], []
        for c in classes:
            sel = m['label'] == c
            npos = int((gl == c).sum())
            if sel.any():
                _, tp = first_claimant(m['score'][sel], m['iou_max'][sel], m['jmax'][sel], thr)
                recall, precision = curves(tp, npos)
                aps.append(average_precision(recall, precision)); recs.append(recall[-1])
            else:
                aps.append(np.zeros(1)); recs.append(0.0)
            ret[f'{names[c]}_AP_{thr:.2f}'] = float(aps[-1][0])
            ret[f'{names[c]}_rec_{thr:.2f}'] = float(recs[-1])
        with np.errstate(all='ignore'):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                ret[f'mAP_{thr:.2f}'] = float(np.nanmean(aps)) if aps else float('nan')
                ret[f'mAR_{thr:.2f}'] = float(np.nanmean(recs)) if recs else float('nan')
    return ret


def same_dict(a: dict, b: dict, tol: float = 1e-6):
    """Key sets identical, NaN in the same places, |delta| < tol.  Returns the list of offending keys (empty = equal)."""
    if set(a) != set(b):
        return sorted(set(a) ^ set(b))
    return [k for k in a if not ((np.isnan(a[k]) and np.isnan(b[k])) or abs(a[k] - b[k]) < tol)]


def iou64_of_best(case: Case, m: dict) -> np.ndarray:
    """fp64 evaluation of the rotated-IoU formula for every detection's best pair (NaN where there is none or the image is axis
    aligned): ``oracle.rotated_iou`` on double tensors for the BEV intersection, height overlap and volumes in fp64."""
    from oracle.rotated_iou import box2corners, oriented_box_intersection_2d
    gb = np.concatenate([np.pad(b, ((0, 0), (0, 7 - b.shape[1]))) for b, _ in case.gt]).astype(np.float64)
    db = np.concatenate([np.pad(b, ((0, 0), (0, 7 - b.shape[1]))) for b, _, _ in case.dt]).astype(np.float64)
    out = np.full(len(db), np.nan)
    sel = np.nonzero((m['jmax'] >= 0) & ~m['aligned'])[0]
    if len(sel):
        a, b = torch.from_numpy(db[sel]), torch.from_numpy(gb[m['jmax'][sel]])
        bev = oriented_box_intersection_2d(box2corners(a[:, [0, 1, 3, 4, 6]]), box2corners(b[:, [0, 1, 3, 4, 6]]))
        h = (torch.min(a[:, 2] + a[:, 5], b[:, 2] + b[:, 5]) - torch.max(a[:, 2], b[:, 2])).clamp(min=0)
        inter = bev * h
        out[sel] = (inter / (a[:, 3] * a[:, 4] * a[:, 5] + b[:, 3] * b[:, 4] * b[:, 5] - inter).clamp(min=1e-8)).numpy()
    return out
