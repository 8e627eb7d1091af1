"""Device augmentation of box-annotated scenes (u3d_aug_boxes, u3d_aug_points_dn, DeviceAugment on a box cache,
MixedDeviceAugment) on the MI355X against the host pipeline (unidet3d_amd/transforms.py) with the same draws, and the joint model
on a mixed batch.  Nothing here is compared with the code under test."""
import copy
import json
import os
import warnings

import numpy as np
import pytest
import torch

from _detw import fill_state_dict
from test_augment_boxes_cpu import ARKIT_TRAIN, MULTISCAN_TRAIN
from test_augment_cpu import SCANNET_TRAIN
from test_gpu_augment import _affine_np, _synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
VOXEL = 0.05                                     # small scenes: 3 000 points, 5 cm voxels


def _at_voxel(pipeline, num_points=None):
    out = []
    for s in pipeline:
        s = dict(s)
        if s['type'] == 'ElasticTransfrom':
            s['voxel_size'] = VOXEL
        if s['type'] == 'PointSample_' and num_points is not None:
            s['num_points'] = num_points
        out.append(s)
    return out


# ---------------------------------------------------------------------------------------------------------------- kernels
def _boxes_kernel(boxes, flips, angles, scales, trans):
    """u3d_aug_boxes called directly on a cache-shaped [G, 7] array; returns the [G, 7] output"""
    from unidet3d_amd import _lib as L
    from unidet3d_amd.augment import compose_affine
    B = len(boxes)
    n = [len(b) for b in boxes]
    off = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    src = np.stack([off[:-1], n], 1).astype(np.int64)
    rows = np.concatenate([np.concatenate((b, np.zeros((len(b), 7 - b.shape[1]), F32)), 1) for b in boxes]).astype(F32)
    A = compose_affine([f[0] for f in flips], [f[1] for f in flips], angles, scales, trans)
    scal = np.stack([[float(f[0]) for f in flips], [float(f[1]) for f in flips], angles, scales], 1).astype(np.float64)
    d_rows = torch.from_numpy(rows).to(DEV)
    d_src, d_off, d_aff, d_scal, d_wy = L.h2d_pack([(src.tolist(), torch.int64), (off.tolist(), torch.int64), (A.tolist(), torch.float32),
                                                    (scal.tolist(), torch.float64), ([int(b.shape[1] == 7) for b in boxes], torch.uint8)], DEV)
    out = torch.full((int(off[-1]), 7), 123.0, dtype=torch.float32, device=DEV)
    L.call('u3d_aug_boxes', L.ptr(d_rows), d_rows.shape[0], L.ptr(d_src), L.ptr(d_off), B, int(off[-1]), L.ptr(d_aff), L.ptr(d_scal), L.ptr(d_wy),
           L.ptr(out), L.stream())
    return out.cpu().numpy(), off


@pytest.mark.parametrize('shift', [0, 1])
def test_box_kernel_equals_host_twin_bit_for_bit(shift):
    """4 scenes of 0, 1, 3 and 65 boxes (more than one wave); the 3-box scene has six columns and no rotation.  Two assignments of the
    four flip combinations, so that each one meets boxes."""
    from unidet3d_amd import transforms as X
    rng = np.random.RandomState(17)
    G, dof = [0, 1, 3, 65], [7, 7, 6, 7]
    boxes = [np.concatenate([rng.uniform(-4, 4, (g, 3)), rng.uniform(0.1, 3, (g, 3)), rng.uniform(-3.2, 3.2, (g, 1))], 1).astype(F32)[:, :d]
             for g, d in zip(G, dof)]
    combos = [(False, False), (True, False), (False, True), (True, True)]
    flips = combos[shift:] + combos[:shift]
    angles = np.array([0.5, -0.5, 0.0, 0.5] if shift == 0 else [-0.5, 0.5, 0.0, -0.5])
    scales, trans = rng.uniform(0.9, 1.1, 4), rng.randn(4, 3) * 0.1
    got, off = _boxes_kernel(boxes, flips, angles, scales, trans)
    for b in range(4):
        want = X.transform_boxes(boxes[b], flips[b][0], flips[b][1], angles[b], scales[b], trans[b])
        g = got[off[b]:off[b + 1]]
        assert np.array_equal(g[:, :dof[b]].view(np.uint32), want.view(np.uint32)), b
        if dof[b] == 6:
            assert not g[:, 6].any()                                         # six-column scenes keep yaw 0


def test_denormalising_point_kernel():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import transforms as X
    from unidet3d_amd.augment import compose_affine
    import ctypes as C
    rng = np.random.RandomState(23)
    n = [0, 1, 1000]
    off = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    pts = np.concatenate([rng.randn(off[-1], 3), rng.rand(off[-1], 3)], 1).astype(F32)
    pts[:4, 3:] = [[0, 1 / 255, 0.5], [1.0, 0.5, 0], [1 / 255, 1.0, 1.0], [0.5, 0, 1 / 255]]
    A = compose_affine([False, True, False], [False, False, True], [0.0, 0.3, -0.2], [1.0, 1.05, 0.95], rng.randn(3, 3) * 0.1)
    d_pts = torch.from_numpy(pts).to(DEV)
    d_src, d_off, d_aff = L.h2d_pack([(np.stack([off[:-1], n], 1).tolist(), torch.int64), (off.tolist(), torch.int64), (A.tolist(), torch.float32)], DEV)
    f3 = C.c_float * 3

    def run(name, *denorm):
        out = torch.empty((int(off[-1]), 6), dtype=torch.float32, device=DEV)
        coords = torch.empty((int(off[-1]), 3), dtype=torch.float32, device=DEV)
        L.call(name, L.ptr(d_pts), d_pts.shape[0], None, L.ptr(d_src), L.ptr(d_off), 3, int(off[-1]), L.ptr(d_aff), f3(127.5, 127.5, 127.5),
               f3(127.5, 127.5, 127.5), *denorm, VOXEL, L.ptr(out), L.ptr(coords), L.stream())
        return out.cpu().numpy(), coords.cpu().numpy()
    got, coords = run('u3d_aug_points_dn', f3(0, 0, 0), f3(255, 255, 255))
    host = X.NormalizePointsColor_([127.5] * 3)(X.DenormalizePointsColor([0, 0, 0], [255, 255, 255])(dict(points=pts.copy())))['points']
    assert np.array_equal(got[:, 3:].view(np.uint32), host[:, 3:].view(np.uint32))
    assert got[0, 3] == -1.0 and got[1, 3] == 1.0 and got[0, 5] == 0.0           # 0 -> -1, 1 -> 1, 0.5 -> 0
    for b in range(3):
        xyz = _affine_np(A[b], pts[off[b]:off[b + 1], :3])
        assert np.array_equal(got[off[b]:off[b + 1], :3], xyz) and np.array_equal(coords[off[b]:off[b + 1]], xyz / F32(VOXEL))
    # mean only / std only
    only_std, _ = run('u3d_aug_points_dn', None, f3(255, 255, 255))
    assert np.array_equal(only_std, got)                                         # + 0 changes no bit of a non-negative product
    only_mean, _ = run('u3d_aug_points_dn', f3(10, 20, 30), None)
    want = ((pts[:, 3:] + np.asarray([10, 20, 30], F32)) - F32(127.5)) / F32(127.5)
    assert np.array_equal(only_mean[:, 3:].view(np.uint32), want.view(np.uint32))
    plain, pc = run('u3d_aug_points')
    none, nc = run('u3d_aug_points_dn', None, None)
    assert plain.tobytes() == none.tobytes() and pc.tobytes() == nc.tobytes()     # both denorm pointers null: u3d_aug_points' bits


# ---------------------------------------------------------------------------------------------------------------- scenes
def _box_dict(idx, name, n=3000, yaw=False, n_classes=17, empty=False):
    """a box-annotated raw scene in its dataset's storage convention: ARKitScenes keeps colours in 0..1, the others in 0..255"""
    from unidet3d_amd.data import scene_boxes
    from unidet3d_amd.synthetic import make_scene
    sc = make_scene(idx, n_points=n, n_classes=n_classes, dataset=name)
    b, keep = scene_boxes(sc)
    lab = sc.labels[keep].astype(np.int64)
    if yaw:
        b = np.concatenate((b, np.random.RandomState(idx).uniform(-0.6, 0.6, (len(b), 1)).astype(F32)), 1)
    if empty:
        b, lab = b[:0], lab[:0]
    pts = sc.points.copy()
    pts[:, 3:] = (pts[:, 3:] + 1) / 2 if name == 'arkitscenes' else np.round((pts[:, 3:] + 1) * 127.5)
    return dict(points=pts.astype(F32), sp_pts_mask=sc.superpoints.astype(np.int64), gt_bboxes_3d=b.astype(F32), gt_labels_3d=lab,
                lidar_path=f'data/{name}/points/syn{idx}.bin')


def _box_draws(B, seed, rot):
    from unidet3d_amd import AugmentDraws
    r = np.random.RandomState(seed)
    return AugmentDraws(flip_h=r.rand(B) < 0.5, flip_v=r.rand(B) < 0.5, angle=r.uniform(-0.5, 0.5, B) if rot else np.zeros(B),
                        scale=r.uniform(0.9, 1.1, B), trans=r.randn(B, 3) * 0.1, elastic_gate=np.zeros(B, bool))


def _host_box_pipeline(dicts, draws, seeds, pipeline):
    """transforms.py on every scene with the same draws: PointSample_ from numpy's generator (the indices the device gets injected),
    the colour steps, the affine on points and boxes, ElasticTransfrom(p=-1)"""
    from unidet3d_amd import transforms as X
    from unidet3d_amd.augment import compose_affine
    from unidet3d_amd.registry import TRANSFORMS
    A = compose_affine(draws.flip_h, draws.flip_v, draws.angle, draws.scale, draws.trans)
    steps = {s['type']: s for s in pipeline}
    out, indices = [], []
    for b, d in enumerate(dicts):
        n = len(d['points'])
        np.random.seed(seeds[b])
        indices.append(np.random.choice(range(n), min(steps['PointSample_']['num_points'], n)))
        np.random.seed(seeds[b])
        h = X.PointSample_(steps['PointSample_']['num_points'])({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()})
        for t in ('DenormalizePointsColor', 'NormalizePointsColor_'):
            if t in steps:
                h = TRANSFORMS.build(dict(steps[t]))(h)
        h['points'] = np.concatenate([_affine_np(A[b], h['points'][:, :3]), h['points'][:, 3:]], 1)
        h['gt_bboxes_3d'] = X.transform_boxes(d['gt_bboxes_3d'], draws.flip_h[b], draws.flip_v[b], draws.angle[b], draws.scale[b], draws.trans[b])
        h = X.ElasticTransfrom([6, 20], [40, 160], VOXEL, -1)(h)
        out.append(h)
    return out, indices


def _same_box_batch(inputs, samples, winputs, wsamples):
    for k in ('points', 'elastic_coords'):
        assert len(inputs[k]) == len(winputs[k])
        for g, w in zip(inputs[k], winputs[k]):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), k
    for g, w in zip(samples, wsamples):
        assert torch.equal(g.gt_pts_seg.sp_pts_mask.cpu(), w.gt_pts_seg.sp_pts_mask) and g.n_superpoints == w.n_superpoints
        assert g.lidar_path == w.lidar_path
        if hasattr(w.gt_instances_3d, 'bboxes_3d'):
            gb, wb = g.gt_instances_3d.bboxes_3d, w.gt_instances_3d.bboxes_3d
            assert g.gt_pts_seg.pts_instance_mask is None
            assert gb.with_yaw == wb.with_yaw and gb.box_dim == wb.box_dim and gb.tensor.shape == wb.tensor.shape
            assert gb.tensor.dtype == torch.float32 and torch.equal(gb.tensor.cpu(), wb.tensor)
            assert g.gt_instances_3d.labels_3d.dtype == torch.int64 and torch.equal(g.gt_instances_3d.labels_3d.cpu(), w.gt_instances_3d.labels_3d)
        else:
            assert torch.equal(g.gt_pts_seg.pts_instance_mask.cpu(), w.gt_pts_seg.pts_instance_mask)
            assert torch.equal(g.gt_instances_3d.labels_3d.cpu(), w.gt_instances_3d.labels_3d)
            assert torch.equal(g.gt_instances_3d.sp_masks.cpu(), w.gt_instances_3d.sp_masks)


def test_arkitscenes_pipeline_equals_host_pipeline_and_reads():
    """ARKitScenes' list (PointSample_, DenormalizePointsColor, NormalizePointsColor_, flip, rotation / scale / translation,
    ElasticTransfrom p=-1) with injected draws: one scene is smaller than num_points, one has no box."""
    from unidet3d_amd import DeviceAugment, DeviceSceneCache
    from unidet3d_amd import transforms as X
    pipeline = _at_voxel(ARKIT_TRAIN, num_points=2500)
    dicts = [_box_dict(400, 'arkitscenes', 3000, yaw=True), _box_dict(401, 'arkitscenes', 1800, yaw=True),
             _box_dict(402, 'arkitscenes', 3000, yaw=True, empty=True)]
    cache = DeviceSceneCache.from_scene_dicts(dicts, DEV)
    aug = DeviceAugment.from_pipeline(pipeline, VOXEL)
    d = _box_draws(3, 71, rot=True)
    d.flip_h[:] = [True, False, True]; d.flip_v[:] = [False, True, True]
    host, d.indices = _host_box_pipeline(dicts, d, [81, 82, 83], pipeline)
    winputs, wsamples = X.to_batch_inputs(host, 'cpu')
    inputs, samples = aug(cache, [0, 1, 2], d)
    assert aug.last_host_reads == 1 and aug.last_launches == 7                  # point map, superpoint relabel (5), boxes
    # host reads counted by torch on a call that draws for itself (injected indices are uploaded from pageable memory, a wait of the test's own)
    g = torch.Generator(DEV)
    g.manual_seed(7)
    aug(cache, [0, 1, 2], generator=g)                                          # warm: allocator, pinned staging
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('warn')
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            aug(cache, [0, 1, 2], generator=g)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [str(w.message) for w in rec if 'synchroniz' in str(w.message).lower()]
    print('host reads:', len(syncs), 'reported', aug.last_host_reads, 'launches', aug.last_launches)
    assert len(syncs) <= 2 and len(syncs) == aug.last_host_reads == 1, syncs     # the superpoint counts; no elastic pass
    assert [len(p) for p in inputs['points']] == [2500, 1800, 2500] and 'ready_event' in inputs
    _same_box_batch(inputs, samples, winputs, wsamples)
    assert len(samples[0].gt_instances_3d.labels_3d) > 2 and samples[2].gt_instances_3d.bboxes_3d.tensor.shape == (0, 7)
    assert samples[0].gt_instances_3d.bboxes_3d.with_yaw and samples[0].n_superpoints <= int(dicts[0]['sp_pts_mask'].max()) + 1
    col = inputs['points'][0][:, 3:].cpu().numpy()
    assert col.min() >= -1.0 and col.max() <= 1.0 and col.std() > 0.1           # 0..1 colours came out in [-1, 1]
    for b in range(3):                                                          # p = -1: elastic_coords = x / voxel_size
        assert np.array_equal(inputs['elastic_coords'][b].cpu().numpy(), inputs['points'][b][:, :3].cpu().numpy() / F32(VOXEL))


# ---------------------------------------------------------------------------------------------------------------- joint model
def _joint_model():
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd.config import build_model
    cfg = json.load(open(os.path.join(GOLD, 'ref_joint_model_cfg.json')))
    cfg['voxel_size'] = VOXEL
    cfg['decoder']['num_layers'] = 2
    return fill_state_dict(build_model(cfg), tag0=3600, scale=0.06).to(DEV).train()


def _to_dev(inputs, samples):
    inputs = {k: [t.to(DEV) for t in v] for k, v in inputs.items()}
    for s in samples:
        for obj in (s.gt_pts_seg, s.gt_instances_3d):
            for k, v in list(vars(obj).items()):
                if torch.is_tensor(v) or hasattr(v, 'gravity_center'):
                    setattr(obj, k, v.to(DEV))
    return inputs, samples


@pytest.fixture(scope='module')
def mixed():
    """one ScanNet-style mask scene, one MultiScan scene (six-column boxes), one ARKitScenes scene (seven columns) and an ARKitScenes
    scene WITHOUT boxes placed last; the device-built batch and the host-built one from the same draws"""
    from unidet3d_amd import DeviceAugment, DeviceSceneCache, MixedDeviceAugment
    from unidet3d_amd import transforms as X
    from unidet3d_amd.augment import compose_affine
    sn_pl, ms_pl, ak_pl = _at_voxel(SCANNET_TRAIN), _at_voxel(MULTISCAN_TRAIN), _at_voxel(ARKIT_TRAIN)
    sn, ms = [_synthetic(410, 3000)], [_box_dict(411, 'multiscan', 3000)]
    ak = [_box_dict(412, 'arkitscenes', 3000, yaw=True), _box_dict(413, 'arkitscenes', 3000, yaw=True, empty=True)]
    mixer = MixedDeviceAugment(dict(scannet=(DeviceAugment.from_pipeline(sn_pl, VOXEL), DeviceSceneCache.from_scene_dicts(sn, DEV)),
                                    multiscan=(DeviceAugment.from_pipeline(ms_pl, VOXEL), DeviceSceneCache.from_scene_dicts(ms, DEV)),
                                    arkitscenes=(DeviceAugment.from_pipeline(ak_pl, VOXEL), DeviceSceneCache.from_scene_dicts(ak, DEV))))
    draws = dict(scannet=_box_draws(1, 91, rot=True), multiscan=_box_draws(1, 92, rot=False), arkitscenes=_box_draws(2, 93, rot=True))
    h_ms, draws['multiscan'].indices = _host_box_pipeline(ms, draws['multiscan'], [101], ms_pl)
    h_ak, draws['arkitscenes'].indices = _host_box_pipeline(ak, draws['arkitscenes'], [102, 103], ak_pl)
    ds = draws['scannet']
    A = compose_affine(ds.flip_h, ds.flip_v, ds.angle, ds.scale, ds.trans)
    h = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sn[0].items()}
    h['points'] = np.concatenate([_affine_np(A[0], h['points'][:, :3]), h['points'][:, 3:]], 1)
    for t in (X.NormalizePointsColor_([127.5] * 3), X.PointDetClassMappingScanNet(20, [0, 1]), X.ElasticTransfrom([6, 20], [40, 160], VOXEL, -1)):
        h = t(h)
    order = [('scannet', 0), ('multiscan', 0), ('arkitscenes', 0), ('arkitscenes', 1)]
    host = X.to_batch_inputs([h, h_ms[0], h_ak[0], h_ak[1]], 'cpu')
    return mixer, order, draws, host


def test_mixed_batch_equals_host_batch_and_loss_bits(mixed):
    mixer, order, draws, (winputs, wsamples) = mixed
    inputs, samples = mixer(order, draws=draws)
    assert mixer.last_host_reads == 3 and mixer.last_launches >= 3 * 7          # ScanNet: instance counts; the box datasets: superpoint counts
    assert [s.lidar_path.split('/')[1] for s in samples] == [n for n, _ in order] and 'ready_event' in inputs
    _same_box_batch(inputs, samples, winputs, wsamples)
    model = _joint_model()
    torch.manual_seed(0)
    a = model.loss(inputs, samples)['det_loss']
    hin, hsm = _to_dev(copy.copy(winputs), copy.deepcopy(wsamples))
    torch.manual_seed(0)
    b = model.loss(hin, hsm)['det_loss']
    print('joint loss on the device-built batch', float(a), 'on the host-built batch', float(b))
    assert torch.isfinite(a) and torch.equal(a, b)


def test_prepare_train_targets_equal_per_scene_get_targets(mixed):
    from unidet3d_amd import ops
    mixer, order, draws, _ = mixed
    inputs, samples = mixer(order, draws=draws)
    assert samples[1].gt_pts_seg.pts_instance_mask is None                       # accepted for datasets whose boxes come with the sample
    model = _joint_model()
    prep = model._prepare_train(inputs, samples)
    insts, topk = prep['sp_gt_instances'], model.train_cfg['topk']
    for i in (1, 2):
        want = model.get_targets(insts[i].sp_centers, insts[i].bboxes_3d, topk)
        assert insts[i].sp_masks.dtype == torch.bool and insts[i].sp_masks.shape == want.shape and want.shape[0] > 2
        assert torch.equal(insts[i].sp_masks, want) and want.any()
    assert insts[3].sp_masks.shape == (0, samples[3].n_superpoints) and insts[3].sp_masks.dtype == torch.bool
    assert insts[0].sp_masks.shape[0] == len(insts[0].labels_3d)                 # the mask scene keeps the masks of its pipeline
    # the same kernel on the third scene that has boxes (ScanNet's come from its instance masks), read in place from the cached rows
    b0 = insts[0].bboxes_3d
    off = prep['batch_offsets']
    packed, mo = ops.targets_by_distance(model._centers, off, b0.gravity_center, [0] + [len(b0)] * 4, topk)
    assert mo[1] == len(b0) * off[1] and mo[4] == mo[1]
    assert torch.equal(packed[:mo[1]].view(len(b0), off[1]), model.get_targets(insts[0].sp_centers, b0, topk))


def test_train_step_through_prefetch_step_on_a_mixed_batch(mixed):
    mixer, order, draws, _ = mixed

    class OptimWrapper:
        def __init__(self, params):
            self.opt = torch.optim.AdamW(params, lr=1e-3)
            self.finite = None

        def update_params(self, loss):
            loss.backward()
            self.finite = all(bool(torch.isfinite(p.grad).all()) for p in self.opt.param_groups[0]['params'] if p.grad is not None)
            self.opt.step(); self.opt.zero_grad()
    model = _joint_model()
    ow = OptimWrapper(list(model.parameters()))
    batch = dict(zip(('inputs', 'data_samples'), mixer(order, draws=draws)))
    model.prefetch_step(batch)
    assert model._staged is not None and model._prefetched is not None
    log = model.train_step(batch, ow)
    torch.cuda.synchronize()
    assert ow.finite and np.isfinite(float(log['loss'].detach()))
