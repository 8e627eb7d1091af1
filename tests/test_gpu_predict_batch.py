"""Batched inference post-processing on the device: ``UniDet3D.predict`` returns results for EVERY scene of a batch (mixed-dataset
batches included, each scene with its own dataset's settings), through one chain of kernels (u3d_topk_segmented -> u3d_nms_batched
-> u3d_nms_compact -> u3d_trim_boxes_batched) with the survivor counts as the only read back to the host.

Expectations come from oracle/postproc.py on each scene's own decoder outputs: torch.softmax (the product keeps F.softmax, so its
scores are those bits) -> topk_instances (ties: lower flat index first) -> multiclass_nms -> trim_boxes, bit-exact."""
import warnings

import numpy as np
import pytest
import torch

from _detw import fill_state_dict
from oracle import postproc as pp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32


def _settings(topk=1000, score_thr=0.0, iou_thr=0.5, fast_nms=True, trim=True):
    return dict(topk=topk, score_thr=score_thr, iou_thr=iou_thr, fast_nms=fast_nms, trim=trim, low_sp_thr=0.18, up_sp_thr=0.81)


def _oracle(cls_pred, bbox, st, points, superpoints):
    """(boxes, labels, scores) of one scene: oracle pipeline on the scene's own logits / boxes."""
    scores = torch.softmax(cls_pred, -1)[:, :-1].cpu().numpy()
    s, l, q = pp.topk_instances(scores, st['topk'])
    b = bbox.cpu().numpy().astype(F32)[q]
    nb, ns, nl = pp.multiclass_nms(b, s, l, st['iou_thr'], st['score_thr'], st['fast_nms'])
    if st['trim']:
        nb = pp.trim_boxes(points[:, :3], superpoints, nb, st['low_sp_thr'], st['up_sp_thr'])
    return nb, nl, ns


def _assert_same(got, want, what):
    gb, gl, gs = got
    wb, wl, ws = want
    assert gl.cpu().numpy().tolist() == wl.tolist(), what
    assert np.array_equal(gs.cpu().numpy(), ws), what
    assert tuple(gb.shape) == wb.shape, (what, tuple(gb.shape), wb.shape)
    assert np.array_equal(gb.cpu().numpy(), wb, equal_nan=True), what


def _capture(model):
    seen, orig = {}, model.predict_by_feat
    model.predict_by_feat = lambda out, *a, **k: (seen.update(out=out), orig(out, *a, **k))[1]
    return seen


def _check_predicted(res, want, bd7_expected=None):
    wb, wl, ws = want
    assert res.labels_3d.cpu().numpy().tolist() == wl.tolist()
    assert np.array_equal(res.scores_3d.cpu().numpy(), ws)
    wb = wb.copy()
    wb[:, 2] += wb[:, 5] * F32(-0.5)                 # DepthInstance3DBoxes(origin=(0.5, 0.5, 0.5)) stores the bottom centre
    assert res.bboxes_3d.tensor.shape[1] == wb.shape[1]
    assert res.bboxes_3d.with_yaw == (wb.shape[1] == 7)
    assert np.array_equal(res.bboxes_3d.tensor.cpu().numpy(), wb, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ 1. ScanNet batch
def test_predict_every_scene_of_a_scannet_batch():
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd.config import build_model, scannet_model_cfg
    from unidet3d_amd.data import make_batch_inputs
    from unidet3d_amd.synthetic import make_scene
    cfg = scannet_model_cfg()
    cfg['decoder']['num_layers'] = 2
    model = fill_state_dict(build_model(cfg), tag0=3000, scale=0.06).to(DEV).eval()
    model.voxel_size = 0.05
    scenes = [make_scene(s, n_points=20_000) for s in (11, 12, 13, 14)]
    inputs, samples = make_batch_inputs(scenes, DEV)
    seen = _capture(model)
    with torch.no_grad():
        out_samples = model.predict(inputs, samples)
    out = seen['out']
    st = _settings()
    for i, sc in enumerate(scenes):
        assert hasattr(out_samples[i], 'pred_instances_3d'), f'scene {i} has no prediction'
        res = out_samples[i].pred_instances_3d
        assert res.points is inputs['points'][i]
        want = _oracle(out['cls_preds'][i], out['bboxes'][i], st, sc.points, sc.superpoints)
        assert len(want[1]) > 0
        _check_predicted(res, want)


# ------------------------------------------------------------------------------------------------------------ 2. mixed joint batch
def test_predict_mixed_joint_batch_each_scene_its_own_branch():
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd.config import build_model, joint_model_cfg
    from unidet3d_amd.data import make_batch_inputs
    from unidet3d_amd.synthetic import make_scene
    cfg = joint_model_cfg()
    cfg['decoder']['num_layers'] = 2
    model = fill_state_dict(build_model(cfg), tag0=3000, scale=0.06).to(DEV).eval()
    model.voxel_size = 0.05
    names = ['scannet', 's3dis', 'arkitscenes', '3rscan', 'scannetpp']
    ds = [model.decoder.datasets.index(n) for n in names]
    scenes = [make_scene(31, n_points=20_000, dataset=n, n_classes=len(cfg['decoder']['datasets_classes'][d])) for n, d in zip(names, ds)]
    inputs, samples = make_batch_inputs(scenes, DEV)
    seen = _capture(model)
    with torch.no_grad():
        out_samples = model.predict(inputs, samples)
    out = seen['out']
    for i, (name, d, sc) in enumerate(zip(names, ds, scenes)):
        st = _settings(iou_thr=cfg['test_cfg']['iou_thr'][d], fast_nms=bool(cfg['fast_nms'][d]), trim=bool(cfg['use_superpoints'][d]))
        bbox = out['bboxes'][i]
        if name == 'arkitscenes':
            assert bbox.shape[1] == 7 and not st['trim']          # rotated NMS, 7-dof boxes, no trimming
        elif name == 's3dis':
            assert not st['fast_nms'] and st['trim']               # aligned_3d_nms + trimming
        elif name == '3rscan' or name == 'scannetpp':
            assert st['fast_nms'] and not st['trim']               # BEV NMS, no trimming: 7 columns with a zero heading
        else:
            assert st['fast_nms'] and st['trim']
        want = _oracle(out['cls_preds'][i], bbox, st, sc.points, sc.superpoints)
        assert len(want[1]) > 0, name
        res = out_samples[i].pred_instances_3d
        _check_predicted(res, want)
        assert res.bboxes_3d.tensor.shape[1] == (6 if st['trim'] else 7), name
        assert res.bboxes_3d.with_yaw == (not st['trim']), name
        if name in ('3rscan', 'scannetpp'):
            assert bool((res.bboxes_3d.tensor[:, 6] == 0).all())


# ------------------------------------------------------------------------------------------------------------ 3. postprocess_batch
def _geometry(scenes):
    from unidet3d_amd import ops
    pts = [torch.from_numpy(sc.points).to(DEV) for sc in scenes]
    vb = ops.voxelize(pts, 0.05, 128)
    offs = [0]
    for sc in scenes:
        offs.append(offs[-1] + int(sc.superpoints.max()) + 1)
    sps = [torch.from_numpy(sc.superpoints).to(DEV) for sc in scenes]
    plan = ops.PoolPlan(vb, ops.offset_ids(sps, offs[:-1]), offs[-1])
    return vb, plan, offs


def _decoder_like(rng, n, C, scene, bd=6, dup=False, one_class=None):
    logits = rng.normal(0, 2.0, (n, C + 1)).astype(F32)
    if one_class is not None:
        logits[:, one_class] += 12.0
    lo, hi = scene.points[:, :3].min(0), scene.points[:, :3].max(0)
    c = rng.uniform(lo, hi, (n, 3)); d = rng.uniform(0.05, 0.8, (n, 3))
    boxes = np.concatenate([c, d] + ([rng.uniform(-3.1, 3.1, (n, 1))] if bd == 7 else []), 1).astype(F32)
    if dup and n > 20:
        logits[n // 2:] = logits[:n - n // 2]                     # duplicated query rows: exact score ties across queries
        boxes[n // 2:] = boxes[:n - n // 2]
    return torch.from_numpy(logits).to(DEV), torch.from_numpy(boxes).to(DEV)


def test_postprocess_batch_synthetic_cases_match_oracle():
    from unidet3d_amd import ops
    from unidet3d_amd.synthetic import make_scene
    rng = np.random.default_rng(5)
    cases = [  # (n queries, classes, settings, decoder kwargs)
        (0, 18, _settings(), {}),                                            # empty scene
        (1, 18, _settings(), {}),                                            # one query
        (3000, 18, _settings(), {}),
        (3000, 200, _settings(iou_thr=0.3), {}),                             # 600 000 candidates
        (10, 5, _settings(topk=1000), {}),                                   # k > n C
        (500, 18, _settings(score_thr=2.0), {}),                             # score_thr removes everything
        (400, 18, _settings(trim=False), dict(dup=True)),                    # exact ties (BEV, 7 columns out)
        (300, 18, _settings(score_thr=0.5, fast_nms=False), dict(one_class=3)),    # one class only, aligned_3d_nms
        (500, 18, _settings(score_thr=2.0, trim=False), {}),                 # nothing left, untrimmed: 6 columns
        (800, 5, _settings(fast_nms=False, trim=False, topk=300), {}),       # aligned_3d_nms, untrimmed
    ]
    scenes = [make_scene(40 + i, n_points=8_000) for i in range(len(cases))]
    vb, plan, offs = _geometry(scenes)
    cls, box, sts = [], [], []
    for (n, C, st, kw), sc in zip(cases, scenes):
        c, b = _decoder_like(rng, n, C, sc, **kw)
        cls.append(c); box.append(b); sts.append(st)
    got = ops.postprocess_batch(cls, box, sts, vb, plan, offs)
    assert len(got) == len(cases)
    for i, ((n, C, st, kw), sc) in enumerate(zip(cases, scenes)):
        _assert_same(got[i], _oracle(cls[i], box[i], st, sc.points, sc.superpoints), f'case {i}')
        if not kw.get('dup'):                                        # without ties: the per-scene path agrees as well
            o0 = offs[i]
            ref = ops.postprocess_scene(cls[i], box[i], st, vb.points, plan.sp_offsets[o0:], plan.sp_points, offs[i + 1] - o0)
            gb, gl, gs = got[i]
            rb, rl, rs = ref
            assert gl.dtype == rl.dtype and gs.dtype == rs.dtype and tuple(gb.shape) == tuple(rb.shape), f'case {i}'
            assert torch.equal(gl, rl) and torch.equal(gs, rs), f'case {i}'
            assert np.array_equal(gb.cpu().numpy(), rb.cpu().numpy(), equal_nan=True), f'case {i}'


def test_postprocess_batch_rotated_and_trimmed_rotated_match_per_scene_path():
    """7-dof boxes: rotated NMS (untrimmed: 7 columns) and, with trimming, the rotated inside test -- the same kernels' arithmetic
    as the per-scene path (the oracle's fp64 polygons may flip a pair that sits on the threshold, test_gpu_postproc nudges those)."""
    from unidet3d_amd import ops
    from unidet3d_amd.synthetic import make_scene
    rng = np.random.default_rng(9)
    sts = [_settings(trim=False, iou_thr=0.55), _settings(trim=True, iou_thr=0.55), _settings(trim=True)]
    scenes = [make_scene(60 + i, n_points=8_000) for i in range(3)]
    vb, plan, offs = _geometry(scenes)
    cls, box = [], []
    for i, sc in enumerate(scenes):
        c, b = _decoder_like(rng, 600, 17, sc, bd=7)
        if i == 2:
            b[:, 6] = 0                                               # all headings zero: the yaw-free trimming path
        cls.append(c); box.append(b)
    got = ops.postprocess_batch(cls, box, sts, vb, plan, offs)
    for i in range(3):
        o0 = offs[i]
        rb, rl, rs = ops.postprocess_scene(cls[i], box[i], sts[i], vb.points, plan.sp_offsets[o0:], plan.sp_points, offs[i + 1] - o0)
        gb, gl, gs = got[i]
        assert len(rl) > 0 and tuple(gb.shape) == tuple(rb.shape) and gb.shape[1] == (6 if sts[i]['trim'] else 7)
        assert torch.equal(gl, rl) and torch.equal(gs, rs), i
        assert np.array_equal(gb.cpu().numpy(), rb.cpu().numpy(), equal_nan=True), i


# ------------------------------------------------------------------------------------------------------------ 4. kernel level
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


def test_topk_segmented_matches_stable_argsort():
    rng = np.random.default_rng(3)
    shapes = [(0, 18), (1, 18), (3000, 18), (10, 5), (5000, 200), (700, 84), (2000, 18), (3000, 18)]
    ks = [1000, 1000, 1000, 1000, 3600, 2500, 1000, 3600]
    mats = []
    for i, (n, C) in enumerate(shapes):
        x = rng.random((n, C + 1)).astype(F32)
        if i >= 6:
            x = (np.floor(x * 16) / 16).astype(F32)                 # quantised: thousands of exact ties
        mats.append(torch.from_numpy(x).to(DEV))
    score, label, query, count = _topk_launch(mats, ks, 3600)
    for i, (m, k) in enumerate(zip(mats, ks)):
        x = m.cpu().numpy()[:, :-1]                                 # the last column (no-object) is never read
        ws, wl, wq = pp.topk_instances(x, k)
        c = int(count[i])
        assert c == len(ws), i
        assert np.array_equal(score[i, :c].cpu().numpy(), ws), i
        assert label[i, :c].cpu().numpy().tolist() == wl.tolist(), i
        assert query[i, :c].cpu().numpy().tolist() == wq.tolist(), i


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_nms_batched_keep_flags_match_per_scene_kernels(mode):
    from unidet3d_amd import _lib as L
    rng = np.random.default_rng(11 + mode)
    bd = 7 if mode == 2 else 6
    shapes = [(300, 18), (1, 5), (2000, 18), (0, 18), (900, 3)]
    B, K = len(shapes), 1000
    mats, boxes = [], []
    for n, C in shapes:
        mats.append(torch.from_numpy(rng.random((n, C + 1)).astype(F32)).to(DEV))
        c = rng.uniform(-3, 3, (n, 3)); d = rng.uniform(0.2, 2.5, (n, 3))
        b = np.concatenate([c, d] + ([rng.uniform(-3.1, 3.1, (n, 1))] if bd == 7 else []), 1).astype(F32)
        if n > 10:
            b[5] = b[4]
        boxes.append(torch.from_numpy(b).to(DEV))
    ks = [K] * B
    score, label, query, count = _topk_launch(mats, ks, K)
    meta = np.zeros((B, 8), np.int32)
    fmeta = np.zeros((B, 4), np.float32)
    for i, (n, C) in enumerate(shapes):
        meta[i] = (n, C, C + 1, K, bd, mode, 0, 0)
        fmeta[i] = (0.2 if i == 2 else 0.0, 0.5, 0.18, 0.81)
    d_ptr, d_meta, d_fmeta = L.h2d_pack([([b.data_ptr() for b in boxes], torch.int64), (meta.tolist(), torch.int32),
                                         (fmeta.tolist(), torch.float32)], DEV)
    order = torch.empty(B * K, dtype=torch.int32, device=DEV)
    n_order = torch.empty(B, dtype=torch.int32, device=DEV)
    keep = torch.empty(B * K, dtype=torch.uint8, device=DEV)
    boxes_ord = torch.empty(B * K, 7, device=DEV)
    w = L.ws(L.lib().u3d_nms_batched_ws_bytes(B, 18), DEV)
    L.call('u3d_nms_batched', L.ptr(d_ptr), L.ptr(d_meta), L.ptr(d_fmeta), B, K, 18, L.ptr(score), L.ptr(label), L.ptr(query),
           L.ptr(count), L.ptr(order), L.ptr(n_order), L.ptr(keep), L.ptr(boxes_ord), L.ptr(w), L.stream())
    fn = ['u3d_nms_bev', 'u3d_nms_aligned3d', 'u3d_nms_rotated'][mode]
    for i in range(B):
        c, s, lab, q = int(count[i]), score[i, :count[i]], label[i, :count[i]].long(), query[i, :count[i]].long()
        sel = s > float(fmeta[i, 0])
        ranks = torch.nonzero(sel)[:, 0]
        o = ranks[torch.sort(lab[sel], stable=True).indices]           # ops.nms_multiclass's order
        n = int(n_order[i])
        assert n == len(o) and torch.equal(order[i * K:i * K + n].long(), o), i
        if n == 0:
            continue
        b = boxes[i][q[o]].contiguous()
        assert torch.equal(boxes_ord[i * K:i * K + n, :bd], b)
        arg = b
        if mode == 1:
            half = b[:, 3:] / 2
            arg = torch.cat((b[:, :3] - half, b[:, :3] + half), dim=1).contiguous()
        want = torch.empty(n, dtype=torch.uint8, device=DEV)
        L.call(fn, L.ptr(arg), L.ptr(lab[o].to(torch.int32).contiguous()), n, 0.5, L.ptr(want), L.stream())
        assert torch.equal(keep[i * K:i * K + n], want), i


# ------------------------------------------------------------------------------------------------------------ 5. fallback
def test_topk_above_the_kernel_limit_takes_the_per_scene_path():
    from unidet3d_amd import ops
    from unidet3d_amd.synthetic import make_scene
    rng = np.random.default_rng(21)
    scenes = [make_scene(70 + i, n_points=8_000) for i in range(3)]
    vb, plan, offs = _geometry(scenes)
    sts = [_settings(topk=ops.PP_MAX_K + 400), _settings(), _settings(topk=ops.PP_MAX_K + 400, trim=False)]
    cls, box = [], []
    for sc in scenes:
        c, b = _decoder_like(rng, 400, 18, sc)
        cls.append(c); box.append(b)
    assert not ops.postproc_batched_ok(400, 18, sts[0]) and ops.postproc_batched_ok(400, 18, sts[1])
    got = ops.postprocess_batch(cls, box, sts, vb, plan, offs)
    for i in range(3):
        o0 = offs[i]
        rb, rl, rs = ops.postprocess_scene(cls[i], box[i], sts[i], vb.points, plan.sp_offsets[o0:], plan.sp_points, offs[i + 1] - o0)
        gb, gl, gs = got[i]
        assert torch.equal(gl, rl) and torch.equal(gs, rs) and tuple(gb.shape) == tuple(rb.shape), i
        assert np.array_equal(gb.cpu().numpy(), rb.cpu().numpy(), equal_nan=True), i
        _assert_same(got[i], _oracle(cls[i], box[i], sts[i], scenes[i].points, scenes[i].superpoints), f'scene {i}')


# ------------------------------------------------------------------------------------------------------------ 6. synchronisations
def test_postprocess_batch_of_eight_reads_the_device_once():
    from unidet3d_amd import ops
    from unidet3d_amd.synthetic import make_scene
    rng = np.random.default_rng(31)
    scenes = [make_scene(80 + i, n_points=8_000) for i in range(8)]
    vb, plan, offs = _geometry(scenes)
    sts = [_settings(fast_nms=i % 3 != 1, trim=i % 2 == 0) for i in range(8)]
    cls, box = [], []
    for sc in scenes:
        c, b = _decoder_like(rng, 1000, 18, sc)
        cls.append(c); box.append(b)
    ops.postprocess_batch(cls, box, sts, vb, plan, offs)           # warm: library, workspaces, pinned staging
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('warn')
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            got = ops.postprocess_batch(cls, box, sts, vb, plan, offs)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in rec if 'synchroniz' in str(w.message).lower()]
    assert len(syncs) == 1, syncs                                  # the [B] count vector, nothing else
    assert len(got) == 8 and all(len(r[1]) > 0 for r in got)
