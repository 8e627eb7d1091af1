"""GPU kernels that bound, order or select float values, on the values where such kernels go wrong: signed zeros, scenes entirely
at negative coordinates or 1000 m from the origin, points exactly on cell boundaries, exact zeros and subnormals, values that differ
only in their lowest byte, large tie groups, and degenerate box geometry (duplicates, zero sizes, touching and nested boxes).

Every expectation comes from the CPU oracle (oracle/postproc.py, oracle/sparse_ops.py) or from a plain float64 computation of the
same operation.  Exact operations (min, max, floor, selection, keep flags) must match bit for bit; signed zeros compare by value."""
import numpy as np
import pytest
import torch

from oracle import postproc as pp
from oracle import sparse_ops as so

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
LOW, UP = 0.18, 0.81


def _permute(canon: np.ndarray, axis: int) -> np.ndarray:
    """canonical columns (u, v, w) -> xyz with u on `axis`, v on axis + 1, w on axis + 2 (mod 3)"""
    out = np.empty_like(canon)
    for k in range(3):
        out[:, (axis + k) % 3] = canon[:, k]
    return out


# ============================================================================================================ 1. trimming, signed zeros
def _zero_scene(case: str, rule: str, axis: int, bd: int, rng):
    """Points, superpoint ids and one box whose kept superpoints reach -0.0 on `axis`.
    case 'max': the only kept superpoint has its largest coordinate exactly -0.0 (and no +0.0 anywhere);
    case 'min': one kept superpoint spans [-1, -0.5], another has its smallest coordinate exactly -0.0;
    case 'all': the kept superpoint is all -0.0 on the axis.
    rule 'add': 9 of a kept superpoint's 10 points are inside (ratio 0.9 > up: all its points count);
    rule 'inside': half of them are inside (low <= 0.5 <= up: only the inside points count) -- the outside ones sit at u = +5.
    Inside points lie within 1.7 of the box centre, the box is a cube of half size 2 (inside whatever the heading); outside points
    are 50 away.  Superpoint 2 is a far cluster the box deletes (ratio 0)."""
    nz = F32(-0.0)
    if case == 'max':
        kept = [np.array([-1.0, -0.875, -0.75, -0.5, -0.375, -0.25, -0.125, nz, nz], F32)]
    elif case == 'min':
        kept = [np.array([-1.0, -0.9, -0.8, -0.75, -0.7, -0.6, -0.55, -0.5, -0.5], F32),
                np.array([nz, 0.05, 0.1, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45], F32)]
    else:
        kept = [np.full(9, nz, F32)]
    rows, sp = [], []
    for s, us in enumerate(kept):
        n_in = len(us)
        vw = rng.uniform(-1, 1, (n_in, 2)).astype(F32)
        rows.append(np.concatenate([us[:, None], vw], 1))
        if rule == 'add':
            u_out = us[-1:].copy()                                   # within the superpoint's own range (-0.0 for 'max' / 'all')
        else:
            u_out = np.full(n_in, 5.0, F32)
        out = np.stack([u_out, np.full(len(u_out), 50.0, F32), rng.uniform(-1, 1, len(u_out)).astype(F32)], 1)
        rows.append(out)
        sp += [s] * (n_in + len(u_out))
    bg = rng.uniform(20, 21, (20, 3)).astype(F32)
    rows.append(bg)
    sp += [len(kept)] * len(bg)
    canon = np.concatenate(rows).astype(F32)
    xyz = _permute(canon, axis)
    pts = np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 3)).astype(F32)], 1)
    box = _permute(np.array([[-0.5, 0.0, 0.0], [4.0, 4.0, 4.0]], F32), axis).reshape(-1)
    if bd == 7:
        box = np.concatenate([box, np.array([0.4], F32)])
    return pts.astype(F32), np.asarray(sp, np.int64), box[None].astype(F32)


def _trim_gpu(pts, sp, boxes):
    from unidet3d_amd import ops
    n_sp = int(sp.max()) + 1
    off, lst = ops.csr_build(torch.from_numpy(sp).to(DEV), n_sp)
    return ops.trim_boxes_by_superpoints(torch.from_numpy(pts).to(DEV), off, lst, n_sp, torch.from_numpy(boxes).to(DEV), LOW, UP).cpu().numpy()


@pytest.mark.parametrize('bd', [6, 7])
@pytest.mark.parametrize('rule', ['add', 'inside'])
@pytest.mark.parametrize('case', ['max', 'min', 'all'])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_trim_signed_zero_extremes(axis, case, rule, bd):
    """u3d_trim_boxes: the box's min / max accumulators are float atomics on bit patterns; -0.0 must bound like 0.0."""
    rng = np.random.default_rng(100 * axis + 10 * ['max', 'min', 'all'].index(case) + bd)
    pts, sp, boxes = _zero_scene(case, rule, axis, bd, rng)
    want = pp.trim_boxes(pts, sp, boxes, LOW, UP)
    lo_u = {'max': -1.0, 'min': -1.0, 'all': 0.0}[case]
    hi_u = {'max': 0.0, 'min': 0.45, 'all': 0.0}[case]
    assert want[0, 3 + axis] == F32(hi_u) - F32(lo_u) and np.isfinite(want).all()       # the case is what it claims to be
    got = _trim_gpu(pts, sp, boxes)
    assert np.array_equal(got, want), (got, want)


def test_trim_signed_zero_mixed_with_ordinary_boxes():
    """Several boxes over one scene: the -0.0 box next to boxes whose extremes are ordinary numbers, a box holding every point and a
    box without any point (its (centre, size) is (nan, -inf) in the oracle and the kernel alike)."""
    rng = np.random.default_rng(7)
    pts, sp, box = _zero_scene('max', 'add', 0, 6, rng)
    extra = np.array([[20.5, 20.5, 20.5, 2.0, 2.0, 2.0], [0.0, 0.0, 0.0, 200.0, 200.0, 200.0], [-90.0, -90.0, -90.0, 1.0, 1.0, 1.0],
                      [-0.25, 0.0, 0.0, 1.0, 3.0, 3.0]], F32)
    boxes = np.concatenate([box, extra]).astype(F32)
    want = pp.trim_boxes(pts, sp, boxes, LOW, UP)
    assert np.array_equal(_trim_gpu(pts, sp, boxes), want, equal_nan=True)


def _softmax_oracle(cls_pred, bbox, st, points, superpoints):
    scores = torch.softmax(cls_pred, -1)[:, :-1].cpu().numpy()          # the product's F.softmax bits
    s, l, q = pp.topk_instances(scores, st['topk'])
    b = bbox.cpu().numpy().astype(F32)[q]
    nb, ns, nl = pp.multiclass_nms(b, s, l, st['iou_thr'], st['score_thr'], st['fast_nms'])
    if st['trim']:
        nb = pp.trim_boxes(points[:, :3], superpoints, nb, LOW, UP)
    return nb, nl, ns


def _assert_same(got, want, what):
    gb, gl, gs = got
    wb, wl, ws = want
    assert gl.cpu().numpy().tolist() == wl.tolist(), what
    assert np.array_equal(gs.cpu().numpy(), ws), what
    assert tuple(gb.shape) == wb.shape, (what, tuple(gb.shape), wb.shape)
    assert np.array_equal(gb.cpu().numpy(), wb, equal_nan=True), what


def _settings(trim, fast_nms=True, iou_thr=0.5, score_thr=0.0, topk=1000):
    return dict(topk=topk, score_thr=score_thr, iou_thr=iou_thr, fast_nms=fast_nms, trim=trim, low_sp_thr=LOW, up_sp_thr=UP)


@pytest.mark.parametrize('rule', ['add', 'inside'])
@pytest.mark.parametrize('case', ['max', 'min', 'all'])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_postprocess_batch_trims_signed_zero_extremes(axis, case, rule):
    """The batched chain (u3d_trim_boxes_batched): three scenes with the crafted box as top-1 of its decoder outputs -- 6 columns
    trimmed, 7 columns untrimmed (rotated NMS, heading kept), 7 columns trimmed (rotated inside test)."""
    from unidet3d_amd import ops
    rng = np.random.default_rng(1000 + 100 * axis + 10 * ['max', 'min', 'all'].index(case) + (rule == 'add'))
    specs = [(6, _settings(True)), (7, _settings(False)), (7, _settings(True))]
    scenes, cls, box = [], [], []
    n, C = 24, 4
    for bd, st in specs:
        pts, sp, crafted = _zero_scene(case, rule, axis, bd, rng)
        logits = rng.normal(0, 1, (n, C + 1)).astype(F32)
        logits[0, 0] = 12.0                                              # the crafted box is the batch's top-1: NMS keeps it
        c = rng.uniform(15, 26, (n, 3)); d = rng.uniform(0.5, 3.0, (n, 3))
        b = np.concatenate([c, d] + ([rng.uniform(-3.1, 3.1, (n, 1))] if bd == 7 else []), 1).astype(F32)
        b[0] = crafted[0]
        scenes.append((pts, sp)); cls.append(torch.from_numpy(logits).to(DEV)); box.append(torch.from_numpy(b).to(DEV))
    vb = ops.voxelize([torch.from_numpy(p).to(DEV) for p, _ in scenes], 0.5, 16)
    offs = [0]
    for _, sp in scenes:
        offs.append(offs[-1] + int(sp.max()) + 1)
    plan = ops.PoolPlan(vb, ops.offset_ids([torch.from_numpy(sp).to(DEV) for _, sp in scenes], offs[:-1]), offs[-1])
    sts = [st for _, st in specs]
    got = ops.postprocess_batch(cls, box, sts, vb, plan, offs)
    for i, ((pts, sp), st) in enumerate(zip(scenes, sts)):
        want = _softmax_oracle(cls[i], box[i], st, pts, sp)
        assert want[1][0] == 0 and np.isfinite(want[0][0]).all(), i     # the crafted box survived and has a finite trimmed box
        _assert_same(got[i], want, f'scene {i}')


# ============================================================================================================ 2. voxelisation values
def _f64_feats(pts_list, coords, inverse):
    """float64 voxel features: mean over the voxel of (rgb, xyz - scene mean of xyz)"""
    feats, cnt = np.zeros((len(coords), 6)), np.zeros(len(coords))
    inv = inverse.numpy()
    f = np.concatenate([np.concatenate([p[:, 3:], p[:, :3] - p[:, :3].mean(0)], 1) for p in (q.numpy().astype(np.float64) for q in pts_list)])
    np.add.at(feats, inv, f)
    np.add.at(cnt, inv, 1.0)
    return feats / cnt[:, None]


def _check_voxelize(pts_list, vs, min_shape=16, elastic=None):
    from unidet3d_amd import ops
    oc, _, oinv, oshape = so.voxelize(pts_list, vs, min_shape, elastic)
    vb = ops.voxelize([p.to(DEV) for p in pts_list], vs, min_shape, None if elastic is None else [e.to(DEV) for e in elastic])
    assert vb.spatial_shape == [int(s) for s in oshape]
    assert torch.equal(vb.coords.cpu(), oc)
    assert torch.equal(vb.inverse.cpu(), oinv)
    ref = _f64_feats(pts_list, oc, oinv)
    got = vb.feats.cpu().double().numpy()
    # a few ulps of the scene's largest coordinate: the fp32 scene mean and the fp32 difference x - mean each round once
    mag = np.array([float(p[:, :3].abs().max()) for p in pts_list])[oc[:, 0].numpy()]
    tol_xyz = 4 * np.spacing(mag.astype(F32)).astype(np.float64)
    assert (np.abs(got[:, 3:] - ref[:, 3:]) <= tol_xyz[:, None]).all(), np.abs(got[:, 3:] - ref[:, 3:]).max()
    assert (np.abs(got[:, :3] - ref[:, :3]) <= 2 * np.spacing(F32(1.0))).all()
    return vb


def _rgb(rng, n):
    return rng.uniform(0, 1, (n, 3)).astype(F32)


def _scene(rng, lo, hi, n=3000):
    xyz = rng.uniform(lo, hi, (n, 3)).astype(F32)
    return torch.from_numpy(np.concatenate([xyz, _rgb(rng, n)], 1))


def _straddling_scene(rng, n=3000):
    """x, y across zero with points at exactly +0.0 and -0.0; z >= 0 with the scene minimum z exactly -0.0"""
    xyz = rng.uniform(-1.5, 1.5, (n, 3)).astype(F32)
    xyz[:, 2] = np.abs(xyz[:, 2])
    xyz[:40, 0] = 0.0; xyz[40:80, 0] = -0.0; xyz[80:120, 1] = 0.0; xyz[120:160, 1] = -0.0
    xyz[160:200, 2] = -0.0; xyz[200:220, 2] = 0.0
    assert xyz[:, 2].min() == 0 and np.signbit(xyz[160, 2]) and (xyz[:, 2] > 0).any()
    return torch.from_numpy(np.concatenate([xyz, _rgb(rng, n)], 1))


def _boundary_scene(rng, vs, base, n_cells=40, n=3000):
    """points exactly on cell boundaries base + k * vs (rounded to fp32) and one ulp either side; `base` is the scene minimum"""
    k = rng.integers(0, n_cells, (n, 3))
    on = (F32(base) + (k * F32(vs)).astype(F32)).astype(F32)
    side = rng.integers(-1, 2, (n, 3))
    xyz = np.where(side < 0, np.nextafter(on, F32(-np.inf)), np.where(side > 0, np.nextafter(on, F32(np.inf)), on)).astype(F32)
    xyz = np.maximum(xyz, F32(base))
    xyz[0] = F32(base)
    return torch.from_numpy(np.concatenate([xyz, _rgb(rng, n)], 1))


@pytest.mark.parametrize('kind', ['negative', 'straddle', 'far_plus', 'far_minus'])
@pytest.mark.parametrize('vs', [0.02, 0.0625])
def test_voxelize_value_domain(kind, vs):
    rng = np.random.default_rng(['negative', 'straddle', 'far_plus', 'far_minus'].index(kind) * 10 + int(vs * 1000))
    if kind == 'negative':
        p = _scene(rng, -7.3, -3.1)
    elif kind == 'straddle':
        p = _straddling_scene(rng)
    elif kind == 'far_plus':
        p = _scene(rng, 1000.0, 1003.5)
    else:
        p = _scene(rng, -1003.5, -1000.0)
    _check_voxelize([p], vs)


@pytest.mark.parametrize('base', [0.0, -3.0, 1000.0, -1000.0])
@pytest.mark.parametrize('vs', [0.02, 0.0625])
def test_voxelize_points_on_cell_boundaries(base, vs):
    rng = np.random.default_rng(int(abs(base)) + int(vs * 1000))
    _check_voxelize([_boundary_scene(rng, vs, base)], vs)


def _elastic(rng, p, vs, shift):
    """elastic coordinates in voxel units, shifted to negative values"""
    e = p[:, :3].numpy().astype(np.float64) / vs + rng.normal(0, 0.7, (len(p), 3)) + shift
    return torch.from_numpy(e.astype(F32))


def test_voxelize_negative_elastic_coordinates():
    rng = np.random.default_rng(17)
    ps = [_scene(rng, -2.0, 2.0), _scene(rng, 1000.0, 1003.0, 2000)]
    el = [_elastic(rng, ps[0], 0.02, -500.0), _elastic(rng, ps[1], 0.02, -50_230.0)]
    el[0][:30, 1] = float(el[0][:, 1].min())                 # ties at the minimum
    assert float(torch.cat(el).max()) < 0
    _check_voxelize(ps, 0.02, elastic=el)


@pytest.mark.parametrize('vs', [0.02, 0.0625])
def test_voxelize_mixed_batch(vs):
    """all of the above in one batch: the per-scene statistics (min, mean) are indexed by scene"""
    rng = np.random.default_rng(23)
    ps = [_scene(rng, -7.3, -3.1, 1500), _straddling_scene(rng, 2500), _scene(rng, 1000.0, 1003.5, 2000), _boundary_scene(rng, vs, -3.0),
          torch.from_numpy(np.concatenate([np.full((1, 3), -1000.0, F32), _rgb(rng, 1)], 1)), _scene(rng, -1003.5, -1000.0, 1800),
          _boundary_scene(rng, vs, 1000.0, n=1200)]
    _check_voxelize(ps, vs)


# ============================================================================================================ 3. boxes from masks, centres
def _instance_batch(rng):
    """scenes: negative-only, 1000 m out, one with -0.0 extremes; instance ids batch-global, -1 interleaved, single-point instances"""
    ps = [_scene(rng, -6.0, -2.0, 2500), _scene(rng, 1000.0, 1004.0, 2500), _straddling_scene(rng, 2500), _scene(rng, -1004.0, -1000.0, 1500)]
    ids, base = [], 0
    for i, p in enumerate(ps):
        n = len(p)
        m = 9 + i
        lab = rng.integers(0, m, n).astype(np.int64)
        lab[rng.random(n) < 0.3] = -1                                # unlabelled points between the instances
        lab[lab == m - 1] = -1
        if i == 2:                                                   # instance 0: the points at z = +-0.0 (the scene minimum)
            lab[lab == 0] = -1
            lab[p[:, 2].numpy() == 0] = 0
        lab[n // 2] = m - 1                                          # a single-point instance
        ids.append(np.where(lab >= 0, lab + base, -1))
        base += m
    return ps, np.concatenate(ids), base


def _minmax_ref(src_list, ids, n_inst):
    """float64 scatter amin / amax of the fp32 (coord - scene min)"""
    shifted = torch.cat([(s - s.min(0)[0]) for s in src_list]).double()       # fp32 subtraction, then exact widening
    idx = torch.from_numpy(ids)
    keep = idx >= 0
    sh, ix = shifted[keep], idx[keep]
    lo = torch.full((n_inst, 3), float('inf'), dtype=torch.float64).scatter_reduce(0, ix[:, None].expand(-1, 3), sh, 'amin', include_self=False)
    hi = torch.full((n_inst, 3), float('-inf'), dtype=torch.float64).scatter_reduce(0, ix[:, None].expand(-1, 3), sh, 'amax', include_self=False)
    return torch.cat((lo, hi), 1)


def _gpu_minmax(vb, ids_d, n_inst):
    from unidet3d_amd import _lib as L
    src = vb.points if vb.coord_src is None else vb.coord_src
    mm = torch.empty(n_inst, 6, dtype=torch.float32, device=DEV)
    ws = L.scratch(n_inst * 24 + 64, DEV)
    L.call('u3d_segment_minmax_xyz', L.ptr(src), src.stride(0), L.ptr(ids_d), src.shape[0], n_inst, L.ptr(vb.stats), 12,
           L.ptr(vb.pt_offsets), vb.stats.shape[0], L.ptr(mm), L.ptr(ws), L.stream())
    return mm


@pytest.mark.parametrize('elastic', [False, True])
def test_instance_boxes_value_edges(elastic):
    from unidet3d_amd import ops
    rng = np.random.default_rng(31 + elastic)
    ps, ids, n_inst = _instance_batch(rng)
    vs = 0.05
    el = [_elastic(rng, p, vs, -300.0 * (i + 1)) for i, p in enumerate(ps)] if elastic else None
    vb = ops.voxelize([p.to(DEV) for p in ps], vs, 16, None if el is None else [e.to(DEV) for e in el])
    ids_d = torch.from_numpy(ids).to(DEV)
    src = el if elastic else [p[:, :3] for p in ps]
    ref = _minmax_ref(src, ids, n_inst)
    assert torch.isfinite(ref).all()                                          # every instance has a point
    mm = _gpu_minmax(vb, ids_d, n_inst)
    assert np.array_equal(mm.cpu().double().numpy(), ref.numpy())             # min / max exact (signed zeros by value)
    got = ops.instance_boxes(vb, ids_d, n_inst, vs if elastic else None).cpu()
    r32 = ref.float()
    if elastic:
        r32 = r32 * float(vs)
    lo, hi = r32[:, :3], r32[:, 3:]
    want = torch.cat(((hi + lo) / 2, hi - lo), 1)
    assert np.array_equal(got.numpy(), want.numpy())


@pytest.mark.parametrize('frame', ['raw', 'scene_min', 'elastic'])
def test_superpoint_centers_value_edges(frame):
    from unidet3d_amd import ops
    rng = np.random.default_rng(41 + ['raw', 'scene_min', 'elastic'].index(frame))
    ps, ids, _ = _instance_batch(rng)
    vs = 0.05
    el = [_elastic(rng, p, vs, -300.0 * (i + 1)) for i, p in enumerate(ps)] if frame == 'elastic' else None
    vb = ops.voxelize([p.to(DEV) for p in ps], vs, 16, None if el is None else [e.to(DEV) for e in el])
    # superpoints: ragged spatial groups per scene, a few single-point ones
    sps, base = [], 0
    for p in ps:
        n = len(p)
        s = rng.integers(0, 60, n).astype(np.int64)
        s[rng.integers(0, n, 3)] = [60, 61, 62]
        s[-1] = 62
        sps.append(s + base)
        base += 63
    sp = np.concatenate(sps)
    off, lst = ops.csr_build(torch.from_numpy(sp).to(DEV), base)
    if frame == 'raw':
        src, got = [p[:, :3] for p in ps], ops.superpoint_centers(vb.points, off, lst, base)
        frames = [s.double() for s in src]
    elif frame == 'scene_min':
        src, got = [p[:, :3] for p in ps], ops.superpoint_centers(vb.points, off, lst, base, vb.stats, vb.pt_offsets)
        frames = [(s - s.min(0)[0]).double() for s in src]
    else:
        src, got = el, ops.superpoint_centers(vb.coord_src, off, lst, base, vb.stats, vb.pt_offsets)
        frames = [(s - s.min(0)[0]).double() for s in src]
    f = torch.cat(frames)
    idx = torch.from_numpy(sp)
    cnt = torch.bincount(idx, minlength=base)
    assert bool((cnt > 0).all())
    ref = torch.zeros(base, 3, dtype=torch.float64).index_add_(0, idx, f) / cnt.double()[:, None]
    g = got.cpu()
    ulp = torch.from_numpy(np.maximum(np.spacing(np.abs(g.numpy())), np.spacing(np.abs(ref.float().numpy()))).astype(np.float64))
    assert ((g.double() - ref).abs() <= ulp).all(), float(((g.double() - ref).abs() / ulp).max())


# ============================================================================================================ 4. top-k selection values
def _topk_launch(mats, ks, K):
    from unidet3d_amd import _lib as L
    B = len(mats)
    meta = np.zeros((B, 8), np.int32)
    for i, (m, k) in enumerate(zip(mats, ks)):
        meta[i, :4] = (m.shape[0], m.shape[1] - 1, m.shape[1], k)
    d_ptr, d_meta = L.h2d_pack([([m.data_ptr() for m in mats], torch.int64), (meta.tolist(), torch.int32)], DEV)
    score = torch.empty(B * K, device=DEV)
    label, query = torch.empty(B * K, dtype=torch.int32, device=DEV), torch.empty(B * K, dtype=torch.int32, device=DEV)
    count = torch.empty(B, dtype=torch.int32, device=DEV)
    L.call('u3d_topk_segmented', L.ptr(d_ptr), L.ptr(d_meta), B, K, L.ptr(score), L.ptr(label), L.ptr(query), L.ptr(count), L.stream())
    return score.view(B, K), label.view(B, K), query.view(B, K), count


def _with_noobj(x):
    """[n, C] probabilities + a no-object column larger than all of them (it must never be read)"""
    return np.concatenate([x, np.full((x.shape[0], 1), 2.0, F32)], 1).astype(F32)


def _topk_cases():
    rng = np.random.default_rng(51)
    cases = []
    x = rng.random((800, 6)).astype(F32)                               # exact zeros (softmax underflow) and subnormals
    r = rng.random(x.shape)
    x[r < 0.4] = 0.0
    sub = (rng.integers(1, 2 ** 23, x.shape).astype(np.uint32)).view(F32)
    x = np.where((r >= 0.4) & (r < 0.7), sub, x).astype(F32)
    x[:5, :] = np.float32(1.4e-45)                                     # the smallest subnormal, repeated
    for k in (100, 1500, 2400, 3000, 4799):                            # k inside the normals, the subnormals and the zeros
        cases.append((x, min(k, 3600)))
    base = np.uint32(0x3e800000)                                       # 0.25: low byte 0, so a 256-long chain keeps the upper bytes
    chain = (base + np.arange(256, dtype=np.uint32)).view(F32)
    assert np.array_equal(chain[1:], np.nextafter(chain[:-1], F32(1)))
    y = np.concatenate([chain, chain, rng.random(1000).astype(F32) * F32(0.2)])       # every chain value twice
    y = y[rng.permutation(len(y))].reshape(-1, 4)
    for k in (1, 255, 256, 257, 300, 511, 512, 513):                   # cut across the chain and inside pairs of equal values
        cases.append((y, k))
    z = np.full((700, 5), F32(0.125))                                  # all equal
    for k in (1, 1000, 2345, 3499):
        cases.append((z, k))
    w = rng.random((300, 10)).astype(F32)                              # k == N > 1024, k == N - 1, k == 1
    w[::7] = F32(0.5)
    for k in (3000, 2999, 1):
        cases.append((w, k))
    c1 = rng.random((2000, 1)).astype(F32)                              # C == 1
    c1[::3] = c1[1]
    for k in (1, 999, 1999, 2000):
        cases.append((c1, k))
    t = rng.random((1000, 9)).astype(F32) * F32(0.5)                    # a tie group of 5000 at the k-th value
    flat = t.reshape(-1)
    perm = rng.permutation(flat.size)
    flat[perm[:500]] = F32(0.75) + rng.random(500).astype(F32) * F32(0.2)
    flat[perm[500:5500]] = F32(0.625)
    for k in (501, 1700, 2800, 3600):
        cases.append((t, k))
    return cases


def test_topk_selection_value_edges():
    cases = _topk_cases()
    mats = [torch.from_numpy(_with_noobj(x)).to(DEV) for x, _ in cases]
    ks = [k for _, k in cases]
    score, label, query, count = _topk_launch(mats, ks, max(ks))
    for i, (x, k) in enumerate(cases):
        ws, wl, wq = pp.topk_instances(x, k)
        c = int(count[i])
        assert c == len(ws) == min(k, x.size), i
        assert np.array_equal(score[i, :c].cpu().numpy().view(np.uint32), ws.view(np.uint32)), i      # the bits
        assert label[i, :c].cpu().numpy().tolist() == wl.tolist(), i
        assert query[i, :c].cpu().numpy().tolist() == wq.tolist(), i


# ============================================================================================================ 5. degenerate NMS geometry
def _degenerate_set(bd):
    """(boxes, labels) of crafted classes:
    0: 100 exact duplicates (more than one wave of 64) and 5 other boxes around them;
    1: zero size in one dimension and in all, 10 duplicates each, inside a unit box;
    2: a 3 x 3 x 2 grid of unit cubes touching along faces and edges, and two cubes touching at one corner;
    3: nested boxes (2 / 1 / 0.5 cubes, one inner cube touching the outer face, BEV IoU 1/4 and 3-D IoU 1/8 exactly);
    4 (7 columns): boxes at heading 0, +-pi/2 (sizes swapped) and pi coinciding with the same rectangle."""
    rows = []
    a = [1.5, -2.0, 0.5, 1.0, 1.0, 1.0]
    rows += [(a, 0)] * 100
    rows += [([1.5 + dx, -2.0, 0.5, 1.0, 1.2, 1.0], 0) for dx in (0.3, -0.6, 1.0, 2.5, 0.5)]
    rows += [([10.0, 10.0, 0.0, 1.0, 1.0, 1.0], 1)]
    rows += [([10.0, 10.0, 0.0, 0.0, 0.5, 0.5], 1)] * 10 + [([10.2, 10.0, 0.0, 0.5, 0.0, 0.5], 1)] * 3 + [([10.0, 10.2, 0.1, 0.5, 0.5, 0.0], 1)] * 3
    rows += [([10.0, 10.0, 0.0, 0.0, 0.0, 0.0], 1)] * 10 + [([12.0, 12.0, 0.0, 0.0, 0.0, 0.0], 1)]
    rows += [([-10.0 + i, 5.0 + j, 1.0 + k, 1.0, 1.0, 1.0], 2) for i in range(3) for j in range(3) for k in range(2)]
    rows += [([-20.0, 5.0, 1.0, 1.0, 1.0, 1.0], 2), ([-19.0, 6.0, 2.0, 1.0, 1.0, 1.0], 2)]
    rows += [([0.0, 20.0, 0.0, 2.0, 2.0, 2.0], 3), ([0.0, 20.0, 0.0, 1.0, 1.0, 1.0], 3), ([0.0, 20.0, 0.0, 0.5, 0.5, 0.5], 3),
             ([0.5, 20.5, 0.5, 1.0, 1.0, 1.0], 3), ([-0.75, 20.0, 0.0, 0.5, 0.5, 0.5], 3)]
    if bd == 7:
        rows = [(r + [0.0], c) for r, c in rows]
        rows += [([5.0, -5.0, 0.0, 2.0, 1.0, 1.0, 0.0], 4), ([5.0, -5.0, 0.0, 1.0, 2.0, 1.0, float(np.pi / 2)], 4),
                 ([5.0, -5.0, 0.0, 1.0, 2.0, 1.0, float(-np.pi / 2)], 4), ([5.0, -5.0, 0.0, 2.0, 1.0, 1.0, float(np.pi)], 4),
                 ([5.0, -5.0, 0.0, 2.0, 1.0, 1.0, 0.0], 4), ([8.0, -5.0, 0.0, 2.0, 1.0, 1.0, float(np.pi / 2)], 4),
                 ([8.0, -3.5, 0.0, 1.0, 2.0, 1.0, 0.0], 4)]
    boxes = np.array([r for r, _ in rows], F32)
    labels = np.array([c for _, c in rows], np.int64)
    return boxes, labels


def _rot_pairs_clear_of(boxes, labels, thr):
    """the rotated-IoU policy of test_gpu_postproc: no pair of a class within 1e-4 of the threshold (fp32 edges vs fp64 polygons)"""
    from oracle import rotated_iou as ri
    b5 = torch.from_numpy(boxes[:, [0, 1, 3, 4, 6]]).double()
    cor = ri.box2corners(b5)
    ar = (b5[:, 2] * b5[:, 3]).numpy()
    for c in np.unique(labels):
        idx = np.nonzero(labels == c)[0]
        if len(idx) < 2:
            continue
        ii, jj = np.triu_indices(len(idx), 1)
        inter = ri.oriented_box_intersection_2d(cor[idx[ii]], cor[idx[jj]]).numpy()
        iou = inter / np.maximum(ar[idx[ii]] + ar[idx[jj]] - inter, 1e-8)
        assert not (np.abs(iou - thr) < 1e-4).any(), (c, thr)


def _scored(boxes, labels, seed):
    rng = np.random.default_rng(seed)
    scores = np.sort(rng.uniform(0.05, 1.0, len(boxes)).astype(F32))[::-1].copy()
    assert len(np.unique(scores)) == len(scores)
    perm = rng.permutation(len(boxes))
    return boxes[perm], scores, labels[perm]


@pytest.mark.parametrize('bd,fast,thr', [(6, True, 0.25), (6, True, 0.5), (6, False, 0.125), (6, False, 0.5),
                                         (7, True, 0.3), (7, True, 0.5)])
def test_nms_degenerate_geometry(bd, fast, thr):
    """per-scene kernels (u3d_nms_bev / u3d_nms_aligned3d / u3d_nms_rotated) vs the oracle.  Thresholds 0.25 (BEV) and 0.125
    (3-D) sit exactly on the nested boxes' IoU: both sides compute it exactly and keep the box (suppression needs iou > thr)."""
    from unidet3d_amd import ops
    boxes, labels = _degenerate_set(bd)
    boxes, scores, labels = _scored(boxes, labels, 61 + bd)
    if bd == 7:
        _rot_pairs_clear_of(boxes, labels, thr)
    ob, os_, ol = pp.multiclass_nms(boxes, scores, labels, thr, 0.0, fast)
    gb, gs, gl = ops.nms_multiclass(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV),
                                    thr, 0.0, fast)
    assert gl.cpu().numpy().tolist() == ol.tolist()
    assert np.array_equal(gs.cpu().numpy(), os_) and np.array_equal(gb.cpu().numpy(), ob)
    n_dup = int(((ob[:, :6] == np.array([1.5, -2.0, 0.5, 1.0, 1.0, 1.0], F32)).all(1) & (ol == 0)).sum())
    assert n_dup == 1                                                       # one of the 100 duplicates survives


def test_rotated_touching_boxes_do_not_overlap():
    """Two rectangles that share only an edge have an empty intersection, whichever side of the kept box the other lies on (the
    kernel sums clipped edges relative to the kept box's first corner, so a shared edge counted from one outline alone gives area
    unless that corner lies on it), and a box of zero size has none either."""
    from unidet3d_amd import ops
    a = [0.5, 0.5, 0.0, 1.0, 1.0, 1.0, 0.0]
    others = [[1.5, 0.5, 0.0, 1.0, 1.0, 1.0, 0.0], [-0.5, 0.5, 0.0, 1.0, 1.0, 1.0, 0.0], [0.5, 1.5, 0.0, 1.0, 1.0, 1.0, 0.0],
              [0.5, -0.5, 0.0, 1.0, 1.0, 1.0, 0.0], [-0.5, -0.5, 0.0, 1.0, 1.0, 1.0, 0.0], [0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0],
              [0.5, 0.5, 0.0, 0.0, 0.6, 1.0, 0.0]]
    for o in others:
        boxes = np.array([a, o], F32)
        scores = np.array([0.9, 0.8], F32)
        labels = np.zeros(2, np.int64)
        ob, _, _ = pp.multiclass_nms(boxes, scores, labels, 0.05, 0.0)
        assert len(ob) == 2, o                                             # the oracle's fp64 polygons: no overlap
        gb, _, _ = ops.nms_multiclass(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV),
                                      0.05, 0.0)
        assert np.array_equal(gb.cpu().numpy(), ob), o


@pytest.mark.parametrize('thr', [0.3, 0.5])
def test_nms_batched_degenerate_geometry(thr):
    """u3d_nms_batched keep flags (through postprocess_batch, untrimmed): BEV, aligned 3-D and rotated scenes of the crafted boxes
    in one batch, against the oracle's top-k + NMS on the same probabilities."""
    from unidet3d_amd import ops
    specs = [(6, True), (6, False), (7, True)]
    cls, box, sts = [], [], []
    C = 5
    for i, (bd, fast) in enumerate(specs):
        boxes, labels = _degenerate_set(bd)
        rng = np.random.default_rng(71 + i)
        if bd == 7:
            _rot_pairs_clear_of(boxes, labels, thr)
        logits = np.zeros((len(boxes), C + 1), F32)
        logits[np.arange(len(boxes)), labels] = 5.0 + rng.random(len(boxes)).astype(F32)     # distinct scores, one class per query
        cls.append(torch.from_numpy(logits).to(DEV)); box.append(torch.from_numpy(boxes).to(DEV))
        sts.append(_settings(False, fast_nms=fast, iou_thr=thr, score_thr=0.05))
    got = ops.postprocess_batch(cls, box, sts, None, None, [0] * (len(specs) + 1))
    for i in range(len(specs)):
        want = _softmax_oracle(cls[i], box[i], sts[i], None, None)
        _assert_same(got[i], want, f'scene {i}')
