"""Edge-case inputs of the fused criterion (unidet3d_amd/csrc/criterion.hip): cost ties, coinciding box faces, zero extents,
class bookkeeping, saturating logits, scattered class columns and rotated-box degeneracies.  Case builders only: plain CPU tensors,
no test functions, no device use.  tests/test_criterion_edges_cpu.py pins every case on the fp64 oracle, tests/test_gpu_criterion_edges.py
runs the kernel on it.

Rules that make every case decidable in fp32 and in fp64 alike:
  * every value that takes part in a constructed equality (box centres, sizes, GT boxes) is a multiple of 1/8 below 64, so
    ``c +- s/2``, the min / max and their differences are exact in both precisions;
  * cost ties come only from duplicating a query bit for bit (logit row, box row, mask column): ``dup`` lists those groups;
  * every other (query, GT) cost is clear of its column's (topk+1)-th value by 1e-4 * max(1, |kth|) in the fp64 oracle --
    ``build`` re-draws the random filler from a fixed seed sequence until that holds and asserts it;
  * all costs are finite (no pair whose enclosing box is a single point).
Most constructed pairs are matched through the GT's query mask: a GT that allows at most ``topk`` queries has the 1e8 sentinel as
its (topk+1)-th cost and therefore matches every allowed query, whatever the cost values are.

A case is a dict:
  name, crit ('scannet' | 'joint'), names [B], sizes [B], CU, BD, L,
  cls  [L] x float32 [sum n, CU]     packed logits (columns outside a scene's ``cidx`` hold random non-zero values),
  box  [L] x float32 [sum n, BD]     packed (centre, size[, heading]) rows,
  gt   [B] x dict(labels int64 [g], boxes float32 [g, 6 | 7], qmask bool [g, n]),
  cidx None | [B] column lists ("no object" last), yaw None | [B] bools,
  dup  [B] x list of groups of bit-identical queries (scene-local indices).
"""
import math

import torch

from oracle import criterion as oc

N_CLS = dict(scannet=18, s3dis=5, arkitscenes=17)
DATASETS = ['scannet', 's3dis', 'arkitscenes']
TOPK = dict(scannet=6, s3dis=4, arkitscenes=3)
WEIGHT = dict(scannet=1.0, s3dis=0.7, arkitscenes=2.5)
MARGIN = 1e-4
INF = 1e8
L = 2


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand_boxes(g, n, dof=6, lo=0.2):
    b = torch.cat((torch.rand(n, 3, generator=g) * 3, torch.rand(n, 3, generator=g) + lo), 1)
    if dof == 7:
        b = torch.cat((b, (torch.rand(n, 1, generator=g) - 0.5) * 2.4), 1)
    return b


def _near(g, gtb, n, p=0.5):
    """random boxes, about half of them close to a random GT (as the decoder's predictions are after a few steps)"""
    b = _rand_boxes(g, n, gtb.shape[1] if len(gtb) else 6)
    if len(gtb):
        near = gtb[torch.randint(0, len(gtb), (n,), generator=g)] + torch.randn(n, gtb.shape[1], generator=g) * 0.08
        near[:, 3:6] = near[:, 3:6].abs() + 0.05
        b = torch.where((torch.rand(n, generator=g) < p)[:, None], near, b)
    return b


def _scene(name, n, gt_labels, gt_boxes, qmask, cls, box, dup=()):
    """one scene: cls / box are [L] lists of [n, C1] / [n, dof]"""
    g = len(gt_labels)
    dof = 7 if name == 'arkitscenes' else 6
    return dict(name=name, n=n, labels=torch.as_tensor(gt_labels, dtype=torch.long).reshape(g),
                boxes=torch.as_tensor(gt_boxes, dtype=torch.float32).reshape(g, dof), qmask=torch.as_tensor(qmask, dtype=torch.bool).reshape(g, n),
                cls=cls, box=box, dup=[list(d) for d in dup])


def _random_scene(g, name, n, n_gt, p_mask=0.3, scale=1.5):
    dof = 7 if name == 'arkitscenes' else 6
    gtb = _rand_boxes(g, n_gt, dof, lo=0.3)
    qm = torch.rand(n_gt, n, generator=g) < p_mask
    labels = torch.randint(0, N_CLS[name], (n_gt,), generator=g)
    cls = [torch.randn(n, N_CLS[name] + 1, generator=g) * scale for _ in range(L)]
    box = [_near(g, gtb, n) if n_gt else _rand_boxes(g, n, dof) for _ in range(L)]
    return _scene(name, n, labels, gtb, qm, cls, box)


def _pack(name, crit, scenes, g, cidx=None, CU=None):
    """scenes -> the packed case dict.  A mixed batch gets ``cidx`` column lists in a CU-wide row and 7 box columns; the columns and the
    heading entries a scene does not own are filled with random non-zero values."""
    names = [s['name'] for s in scenes]
    mixed = cidx is not None
    if not mixed:
        assert len(set(names)) == 1
        CU = N_CLS[names[0]] + 1
    BD = 7 if (mixed or names[0] == 'arkitscenes') else 6
    cls, box = [], []
    for l in range(L):
        rows_c, rows_b = [], []
        for b, s in enumerate(scenes):
            c = torch.randn(s['n'], CU, generator=g) * 2 + 0.25
            c[c == 0] = 1.0
            cols = cidx[b] if mixed else list(range(CU))
            c[:, cols] = s['cls'][l]
            bx = torch.rand(s['n'], BD, generator=g) + 0.5
            bx[:, :s['box'][l].shape[1]] = s['box'][l]
            rows_c.append(c); rows_b.append(bx)
        cls.append(torch.cat(rows_c).contiguous()); box.append(torch.cat(rows_b).contiguous())
    return dict(name=name, crit=crit, names=names, sizes=[s['n'] for s in scenes], CU=CU, BD=BD, L=L, cls=cls, box=box,
                gt=[dict(labels=s['labels'], boxes=s['boxes'], qmask=s['qmask']) for s in scenes],
                cidx=[list(c) for c in cidx] if mixed else None, yaw=[n == 'arkitscenes' for n in names] if mixed else None,
                dup=[s['dup'] for s in scenes])


# ---------------------------------------------------------------------------------------------------------------- oracle helpers
def scene_views(case, cls, box):
    """packed [L] leaves -> per-layer, per-scene views in the scene's own columns (what the reference's dict contract carries)"""
    out_c, out_b = [], []
    for l in range(case['L']):
        cs, bs, o = [], [], 0
        for b, n in enumerate(case['sizes']):
            c, bx = cls[l][o:o + n], box[l][o:o + n]
            if case['cidx'] is not None:
                c = c[:, case['cidx'][b]]
                bx = bx if case['yaw'][b] else bx[:, :6]
            cs.append(c); bs.append(bx); o += n
        out_c.append(cs); out_b.append(bs)
    return out_c, out_b


def oracle_insts(case, dtype):
    out = []
    for name, gt in zip(case['names'], case['gt']):
        out.append(oc.OInst(labels_3d=gt['labels'], query_masks=gt['qmask'], bboxes_3d=oc.OBoxes(gt['boxes'].to(dtype), name == 'arkitscenes')))
    return out


def oracle_costs(scores, bboxes, labels, gtb, qm, w_cls=0.5, w_box=2.0):
    """the cost matrix of oracle.criterion.uni_matcher (its lines, up to the top-k) -> [n, g]"""
    n_gts = len(labels)
    c_cls = -scores.softmax(-1)[:, labels] * w_cls
    pb = bboxes.unsqueeze(1).repeat(1, n_gts, 1)
    gb = gtb.unsqueeze(0).repeat(bboxes.shape[0], 1, 1)
    c_box = oc.box_cost_loss(oc.bbox_to_loss(pb), oc.bbox_to_loss(gb)) * w_box
    return torch.where(qm.T, c_cls + c_box, torch.tensor(INF, dtype=c_cls.dtype))


def run_oracle(case, dtype=torch.float64):
    """oracle.criterion on the case in ``dtype`` -> dict(loss, dcls [L], dbox [L], matched [L][B] bool [n, g], cost, kth, target [L][B])"""
    cls = [c.detach().clone().to(dtype).requires_grad_() for c in case['cls']]
    box = [b.detach().clone().to(dtype).requires_grad_() for b in case['box']]
    vc, vb = scene_views(case, cls, box)
    insts = oracle_insts(case, dtype)
    topk = [TOPK[n] for n in case['names']]
    dw = [WEIGHT[n] if case['crit'] == 'joint' else 1.0 for n in case['names']]
    pred = dict(cls_preds=vc[0], bboxes=vb[0], aux_outputs=[dict(cls_preds=vc[l], bboxes=vb[l]) for l in range(1, case['L'])])
    loss = oc.criterion(pred, insts, topk=topk, dataset_weight=dw)
    loss.backward()
    matched, costs, kths, targets = [], [], [], []
    with torch.no_grad():
        for l in range(case['L']):
            ml, cl, kl, tl = [], [], [], []
            for b, inst in enumerate(insts):
                n, g = case['sizes'][b], len(inst)
                if g == 0:
                    ml.append(torch.zeros(n, 0, dtype=torch.bool)); cl.append(torch.zeros(n, 0, dtype=dtype)); kl.append(torch.zeros(0, dtype=dtype))
                    tl.append(torch.full((n,), N_CLS[case['names'][b]], dtype=torch.long))
                    continue
                cost = oracle_costs(vc[l][b], vb[l][b], inst.labels_3d, oc._gt_box_rows(inst.bboxes_3d), inst.query_masks)
                kth = torch.topk(cost, topk[b] + 1, dim=0, sorted=True, largest=False).values[-1]
                m = cost < kth[None]
                iq, ig = oc.uni_matcher(vc[l][b], vb[l][b], inst.labels_3d, oc._gt_box_rows(inst.bboxes_3d), inst.query_masks, topk[b])
                m2 = torch.zeros_like(m); m2[iq, ig] = True
                assert torch.equal(m, m2)
                last = (m * torch.arange(1, g + 1)).amax(1) - 1                      # the reference's index assignment keeps the last pair
                tl.append(torch.where(last >= 0, inst.labels_3d[last.clamp(min=0)], N_CLS[case['names'][b]]))
                ml.append(m); cl.append(cost); kl.append(kth)
            matched.append(ml); costs.append(cl); kths.append(kl); targets.append(tl)
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(loss=loss.detach(), dcls=[zero(c) for c in cls], dbox=[zero(b) for b in box], matched=matched, cost=costs, kth=kths, target=targets)


def margin_violations(case, ora):
    """(query, GT) costs that are NOT clear of their column's kth value and are not a constructed tie with it: the 1e8 sentinel of a
    forbidden pair (a constant in any precision) and the bit-identical duplicates of the kth query are the only admissible equalities"""
    bad = []
    for l in range(case['L']):
        for b in range(len(case['sizes'])):
            cost, kth = ora['cost'][l][b], ora['kth'][l][b]
            qm = case['gt'][b]['qmask']
            for j in range(cost.shape[1]):
                k = float(kth[j])
                if k == INF:
                    close = (cost[:, j] - k).abs() <= MARGIN * k
                    if not torch.equal(close, ~qm[j]):
                        bad.append((l, b, j, 'sentinel'))
                    continue
                close = ((cost[:, j] - k).abs() <= MARGIN * max(1.0, abs(k))).nonzero().flatten().tolist()
                groups = [d for d in case['dup'][b] if set(close) <= set(d)]
                if len(close) != 1 and not (groups and all(float(cost[q, j]) == k for q in close)):
                    bad.append((l, b, j, close))
    return bad


def all_finite(case, ora):
    ok = bool(torch.isfinite(ora['loss']))
    for l in range(case['L']):
        ok = ok and bool(torch.isfinite(ora['dcls'][l]).all()) and bool(torch.isfinite(ora['dbox'][l]).all())
        ok = ok and all(bool(torch.isfinite(c).all()) for c in ora['cost'][l])
    return ok


_ORACLE = {}


def build(name):
    """-> (case, fp64 oracle result).  Deterministic: filler seeds are tried in a fixed order until the kth-margin condition holds;
    the condition and the finiteness of every cost are asserted.  Cached: the oracle of a case is computed once per process."""
    if name not in _ORACLE:
        for attempt in range(50):
            case = BUILDERS[name](1000 * (1 + list(BUILDERS).index(name)) + attempt)
            ora = run_oracle(case, torch.float64)
            if not margin_violations(case, ora):
                break
        assert not margin_violations(case, ora), (name, margin_violations(case, ora))
        assert all_finite(case, ora), name
        _ORACLE[name] = (case, ora)
    return _ORACLE[name]


# ---------------------------------------------------------------------------------------------------------------- the cases
def _quiet_logits(g, n, C1):
    """near-uniform rows: the class cost is -0.5 / C1 +- a little, so the box cost orders the constructed queries"""
    return torch.randn(n, C1, generator=g) * 0.1


def _box(*v):
    return torch.tensor(v, dtype=torch.float32)


def tie_straddles_kth(seed):
    """ScanNet, topk = 6.  Scene 0, 40 queries, every GT restricted to its own query group by the masks:
      GT 0 (1,1,1; 1,1,1): queries 0-4 enlarge it along x by 1/8 .. 5/8 (IoU 0.89 .. 0.62), queries 5-7 are three bit-identical
            copies shifted by 1/2 (IoU 1/3), 8-10 are far away -> the copies hold ranks 6-8, the 7th value lies INSIDE the run and the
            whole run stays unmatched;
      GT 1 (3,1,1; 1,1,1): query 11 equals it, 12-14 are three copies (x size + 1/8) on ranks 2-4, 15-17 follow (+3/8 .. +5/8), 18-20 far
            -> kth is query 17's cost, the run is matched whole;
      GT 2 (1,3,1; 1,1,1): queries 21-28 are eight copies of the GT itself at the minimum, 29-31 far -> kth equals the minimum, NO match;
      GT 3: random, allowed on the filler queries 29-39.
    Scene 1: 300 random queries (more than one pass of the 256-thread statistics loop) and 3 GTs with random masks."""
    g = _gen(seed)
    n, C1 = 40, 19
    gtb = torch.stack([_box(1, 1, 1, 1, 1, 1), _box(3, 1, 1, 1, 1, 1), _box(1, 3, 1, 1, 1, 1), _box(3, 3, 2, 1.5, 1, 0.5)])
    qm = torch.zeros(4, n, dtype=torch.bool)
    qm[0, 0:11] = True; qm[1, 11:21] = True; qm[2, 21:32] = True; qm[3, 29:40] = True
    cls, box = [], []
    for l in range(L):
        c = _quiet_logits(g, n, C1)
        b = _rand_boxes(g, n)
        b[:, :3] += 6.0                                                     # filler and "far" queries: disjoint from GT 0-2
        b[32:] = _near(g, gtb[3:4], n - 32, p=0.7)
        for k in range(5):
            b[k] = _box(1, 1, 1, 1 + (k + 1) / 8, 1, 1)
        b[5:8] = _box(1.5, 1, 1, 1, 1, 1); c[5:8] = c[5]
        b[11] = gtb[1]
        b[12:15] = _box(3, 1, 1, 1.125, 1, 1); c[12:15] = c[12]
        for k in range(3):
            b[15 + k] = _box(3, 1, 1, 1 + (k + 3) / 8, 1, 1)
        b[21:29] = gtb[2]; c[21:29] = c[21]
        cls.append(c); box.append(b)
    s0 = _scene('scannet', n, [3, 11, 7, 5], gtb, qm, cls, box, dup=[range(5, 8), range(12, 15), range(21, 29)])
    return _pack('tie_straddles_kth', 'scannet', [s0, _random_scene(g, 'scannet', 300, 3)], g)


def pred_equals_gt(seed):
    """ScanNet.  Scene 0 (16 queries; GT 0 = GT 1 = [0.5, 1.5]^3 with different labels, GT 2 at (3,1,1), GT 3 at (1,3,1), unit cubes):
      q0 = GT 0 bit for bit (matched by GT 0 AND GT 1: every min / max of the pair is a tie);
      q1 / q2 / q3 share exactly one / two / three upper faces with GT 0 and lie inside it; q4 shares its three lower faces and is larger;
      q5 touches GT 2 from outside on its +x face (hi - lo == 0: empty intersection with a live clamp); q7 = GT 2;
      q6 is separated from GT 3 by a gap of 7.
    All these pairs are matched through the masks (<= topk allowed queries per GT).  Scene 1: random, with random masks."""
    g = _gen(seed)
    n, C1 = 16, 19
    gtb = torch.stack([_box(1, 1, 1, 1, 1, 1), _box(1, 1, 1, 1, 1, 1), _box(3, 1, 1, 1, 1, 1), _box(1, 3, 1, 1, 1, 1)])
    qm = torch.zeros(4, n, dtype=torch.bool)
    qm[0, [0, 1, 2, 3, 4]] = True; qm[1, [0, 1, 4]] = True; qm[2, [5, 7]] = True; qm[3, [6, 8, 9]] = True
    cls, box = [], []
    for l in range(L):
        b = _near(g, gtb, n)
        b[0] = gtb[0]
        b[1] = _box(1.25, 1, 1, 0.5, 0.5, 0.5)
        b[2] = _box(1.25, 1.25, 1, 0.5, 0.5, 0.5)
        b[3] = _box(1.25, 1.25, 1.25, 0.5, 0.5, 0.5)
        b[4] = _box(1.25, 1.25, 1.25, 1.5, 1.5, 1.5)
        b[5] = _box(4, 1, 1, 1, 1, 1)
        b[6] = _box(1, 10.5, 1, 1, 0.5, 1)
        b[7] = gtb[2]
        if l == 1:                                                          # the second layer: the same events on the lower faces / other axes
            b[1] = _box(1, 0.75, 1, 0.5, 0.5, 0.5)
            b[2] = _box(0.75, 1, 0.75, 0.5, 0.5, 0.5)
            b[5] = _box(3, 1, 0, 1, 1, 1)
        cls.append(torch.randn(n, C1, generator=g) * 1.5); box.append(b)
    s0 = _scene('scannet', n, [3, 11, 7, 5], gtb, qm, cls, box)
    return _pack('pred_equals_gt', 'scannet', [s0, _random_scene(g, 'scannet', 20, 3, p_mask=0.6)], g)


def flat_boxes(seed):
    """ScanNet.  Scene 0 (12 queries): GT 0 a unit cube, GT 1 with extent 0 along z, GT 2 with extent 0 along y and z (a segment);
      q0 has extent 0 along z and cuts GT 0 (zero volume, zero intersection, clamp(min=0) live at 0); q1 is a regular box around the
      flat GT 1; q2 a regular box around the segment GT 2; q5 = GT 2 bit for bit.
    Scene 1 (8 queries), kept apart because its gradients are of order 1 / 1e-6: GT 0 flat along z, q0 = GT 0 and q1 = GT 0 shifted by 1/2
      along x, both flat: the raw union is 0 < 1e-6, so the union clamp is live (the gradient does not reach the volumes)."""
    g = _gen(seed)
    n, C1 = 12, 19
    gtb = torch.stack([_box(1, 1, 1, 1, 1, 1), _box(3, 1, 1, 1, 1, 0), _box(1, 3, 1, 1, 0, 0)])
    qm = torch.zeros(3, n, dtype=torch.bool)
    qm[0, [0, 6, 7]] = True; qm[1, [1, 8]] = True; qm[2, [2, 5]] = True
    cls, box = [], []
    for l in range(L):
        b = _near(g, gtb[:1], n)
        b[0] = _box(1, 1, 1, 1, 1, 0) if l == 0 else _box(1, 1.25, 1, 1, 0, 1)
        b[1] = _box(3, 1, 1, 1, 1, 0.5)
        b[2] = _box(1, 3, 1, 0.5, 0.5, 0.5)
        b[5] = gtb[2]
        cls.append(torch.randn(n, C1, generator=g) * 1.5); box.append(b)
    s0 = _scene('scannet', n, [3, 11, 7], gtb, qm, cls, box)
    n1 = 8
    gt1 = torch.stack([_box(2, 2, 1, 1, 1, 0), _box(0.5, 0.5, 0.5, 0.5, 0.5, 0.5)])
    qm1 = torch.zeros(2, n1, dtype=torch.bool)
    qm1[0, [0, 1]] = True; qm1[1, [2, 3, 4]] = True
    cls1, box1 = [], []
    for l in range(L):
        b = _near(g, gt1[1:], n1)
        b[0] = gt1[0]
        b[1] = _box(2.5, 2, 1, 1, 1, 0)
        cls1.append(torch.randn(n1, C1, generator=g) * 1.5); box1.append(b)
    s1 = _scene('scannet', n1, [2, 9], gt1, qm1, cls1, box1)
    return _pack('flat_boxes', 'scannet', [s0, s1], g)


def _forbidden_scene(g, n, n_gt):
    s = _random_scene(g, 'scannet', n, n_gt)
    s['qmask'][:] = False
    return s


def class_bookkeeping(seed):
    """ScanNet, topk = 6.
      Scene 0 (20 queries): GT 0 / 1 / 2 with labels 3 / 11 / 7 all match query 0 -> its target is 7, the LAST matched GT's label.
      Scene 1: exactly topk + 1 = 7 queries, 2 GTs, every query allowed: kth is the column's maximum.
      Scene 2 (30 queries): 64 GTs; GT 0 (label 4) and GT 63 (label 13) both match query 5 -> bit 63 of the match mask, target 13.
      Scene 3: 3 GTs whose masks forbid every query: a scene with GT and no match at all."""
    g = _gen(seed)
    s0 = _random_scene(g, 'scannet', 20, 4)
    s0['labels'][:3] = torch.tensor([3, 11, 7])
    s0['qmask'][:3] = False
    s0['qmask'][0, [0, 1]] = True; s0['qmask'][1, [0, 2]] = True; s0['qmask'][2, [0, 3]] = True
    s1 = _random_scene(g, 'scannet', 7, 2, p_mask=2.0)
    s2 = _random_scene(g, 'scannet', 30, 64, p_mask=0.08)
    s2['labels'][0], s2['labels'][63] = 4, 13
    s2['qmask'][[0, 63]] = False
    s2['qmask'][0, [5, 6]] = True; s2['qmask'][63, [5, 7]] = True
    s2['qmask'][1:63, 5] = False                                           # nothing between GT 0 and GT 63 on query 5
    return _pack('class_bookkeeping', 'scannet', [s0, s1, s2, _forbidden_scene(g, 9, 3)], g)


def class_bookkeeping_no_match(seed):
    """ScanNet.  Every scene with GT forbids every query and one scene has no GT: no scene of the batch has a match, the number of
    scenes with matches is clamped to 1 and every box gradient is 0."""
    g = _gen(seed)
    return _pack('class_bookkeeping_no_match', 'scannet',
                 [_forbidden_scene(g, 9, 3), _random_scene(g, 'scannet', 12, 0), _forbidden_scene(g, 270, 12)], g)


def extreme_logits(seed):
    """ScanNet.  Scene 0 (16 queries, GT labels 2 / 5 / 9, matches forced by the masks):
      q0: +88 in column 2, -88 in column 5, matched by GT 0 and GT 1 -> target 5, the column at -88 (nll = 176);
      q1: every logit 60; q2: 1e4 in column 4, target 9 (nll = 1e4); q3: target 9 at the smallest logit (-30);
      q4: "no object" dominant (40) while matched; q5 / q6: +-88 in the "no object" column, unmatched;
      q7 / q8: 1e4 in the "no object" column / in column 3, unmatched.
    Scene 1: random, with saturated rows among them."""
    g = _gen(seed)
    n, C1 = 16, 19
    gtb = _rand_boxes(g, 3, lo=0.3)
    qm = torch.zeros(3, n, dtype=torch.bool)
    qm[0, [0, 1]] = True; qm[1, [0, 10]] = True; qm[2, [2, 3, 4]] = True
    cls, box = [], []
    for l in range(L):
        c = torch.randn(n, C1, generator=g) * 1.5
        c[0] = 0; c[0, 2] = 88; c[0, 5] = -88
        c[1] = 60
        c[2] = 0; c[2, 4] = 1e4
        c[3] = torch.rand(C1, generator=g) * 5; c[3, 9] = -30
        c[4, 18] = 40
        c[5, 18] = 88; c[6, 18] = -88
        c[7] = 0; c[7, 18] = 1e4
        c[8] = 0; c[8, 3] = 1e4
        if l == 1:
            c[0, 2], c[0, 5] = -88, 88
        cls.append(c); box.append(_near(g, gtb, n))
    s0 = _scene('scannet', n, [2, 5, 9], gtb, qm, cls, box)
    s1 = _random_scene(g, 'scannet', 40, 4, p_mask=0.5)
    for l in range(L):
        s1['cls'][l][3, 7] = 88; s1['cls'][l][5, 18] = 88; s1['cls'][l][9] = 60; s1['cls'][l][11, 2] = -88
    return _pack('extreme_logits', 'scannet', [s0, s1], g)


def scattered_columns(seed):
    """Joint config, mixed batch scannet / s3dis / arkitscenes / s3dis in a 30-column logit row: every dataset's class list is an
    interleaved, non-monotonic selection of columns 0..28 with "no object" at column 29 = CU - 1, as the decoder builds them from
    ``datasets_cls_idxs`` with its last entry -1.  The columns a scene does not own hold random non-zero logits."""
    g = _gen(seed)
    CU = 30
    cols = {}
    for k, name in enumerate(DATASETS):
        perm = torch.randperm(CU - 1, generator=_gen(77 + k))[:N_CLS[name]].tolist()
        assert perm != sorted(perm)
        cols[name] = perm + [CU - 1]
    names = ['scannet', 's3dis', 'arkitscenes', 's3dis']
    scenes = [_random_scene(g, nm, n, k, p_mask=0.4) for nm, n, k in zip(names, [60, 8, 33, 21], [5, 2, 4, 3])]
    return _pack('scattered_columns', 'joint', scenes, g, cidx=[cols[nm] for nm in names], CU=CU)


def rotated_edges(seed):
    """Joint config, two ARKitScenes scenes (7-dof boxes, topk = 3); constructed pairs are matched through the masks.
    Scene 0, every heading 0 (sin = 0, cos = 1 exactly; corners are dyadic):
      GT 0 (1,1,1; 1,1,1): q0 = GT 0; q1 = GT 0 shifted by 1/4 along x (parallel edges, num == 0, two of them collinear); q2 inside GT 0;
      GT 1 (4,1,1; 1,1,1): q3 touches it in one corner ((4.5, 1.5) of the GT = the lower corner of q3); q4 contains it;
      GT 2 (1,4,1; 0,1,1), w = 0: q5 is a regular box around it;
      GT 3: random heading, allowed on the random filler queries 8-15.
    Scene 1, headings 0 against pi/2 (cos(pi/2) is not 0 in either precision, so the edges are ALMOST parallel): values and gradients
    only -- the sizes differ, so no edge of one box is collinear with an edge of the other, and the masks decide the matches:
      GT 0 (1,1,1; 1,1,1; 0): q0 = (1,1,1; 1.5,0.5,1; pi/2), a cross; q1 = (1,1,1; 0.5,0.25,0.5; pi/2), inside;
      GT 1 (4,4,1; 2,0.5,1; pi/2): q2 = (4,4,1; 1,1,1; 0), crossing it; q3 = (4,4.5,1; 0.25,0.25,1; 0) inside it."""
    g = _gen(seed)
    n, C1 = 16, 18
    h = math.pi / 2
    gtb = torch.stack([_box(1, 1, 1, 1, 1, 1, 0), _box(4, 1, 1, 1, 1, 1, 0), _box(1, 4, 1, 0, 1, 1, 0),
                       torch.cat((_box(3, 3.5, 1.5, 1.25, 0.75, 1), (torch.rand(1, generator=g) - 0.5) * 2.4))])
    qm = torch.zeros(4, n, dtype=torch.bool)
    qm[0, [0, 1, 2]] = True; qm[1, [3, 4]] = True; qm[2, [5]] = True; qm[3, 8:] = True
    cls, box = [], []
    for l in range(L):
        b = _near(g, gtb[3:], n, p=0.7)
        b[0] = gtb[0]
        b[1] = _box(1.25, 1, 1, 1, 1, 1, 0) if l == 0 else _box(1, 0.75, 1.25, 1, 1, 1, 0)
        b[2] = _box(1, 1, 1, 0.5, 0.5, 0.5, 0) if l == 0 else _box(1.125, 0.875, 1, 0.5, 0.25, 2, 0)
        b[3] = _box(5, 2, 1, 1, 1, 1, 0) if l == 0 else _box(3, 2, 1, 1, 1, 1, 0)
        b[4] = _box(4, 1, 1, 2, 1.5, 1, 0)
        b[5] = _box(1, 4, 1, 0.5, 0.5, 0.5, 0)
        cls.append(torch.randn(n, C1, generator=g) * 1.5); box.append(b)
    s0 = _scene('arkitscenes', n, [3, 11, 7, 5], gtb, qm, cls, box)
    n1 = 8
    gt1 = torch.stack([_box(1, 1, 1, 1, 1, 1, 0), _box(4, 4, 1, 2, 0.5, 1, h)])
    qm1 = torch.zeros(2, n1, dtype=torch.bool)
    qm1[0, [0, 1]] = True; qm1[1, [2, 3]] = True
    cls1, box1 = [], []
    for l in range(L):
        b = _rand_boxes(g, n1, 7)
        b[0] = _box(1, 1, 1, 1.5, 0.5, 1, h)
        b[1] = _box(1, 1, 1, 0.5, 0.25, 0.5, h)
        b[2] = _box(4, 4, 1, 1, 1, 1, 0)
        b[3] = _box(4, 4.5, 1, 0.25, 0.25, 1, 0)
        cls1.append(torch.randn(n1, C1, generator=g) * 1.5); box1.append(b)
    s1 = _scene('arkitscenes', n1, [1, 16], gt1, qm1, cls1, box1)
    return _pack('rotated_edges', 'joint', [s0, s1], g)


BUILDERS = dict(tie_straddles_kth=tie_straddles_kth, pred_equals_gt=pred_equals_gt, flat_boxes=flat_boxes, class_bookkeeping=class_bookkeeping,
                class_bookkeeping_no_match=class_bookkeeping_no_match, extreme_logits=extreme_logits, scattered_columns=scattered_columns,
                rotated_edges=rotated_edges)
CASES = list(BUILDERS)
