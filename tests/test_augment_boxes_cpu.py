"""Host-side logic of the device augmentation for box-annotated datasets (unidet3d_amd/augment.py, transforms.transform_boxes) and
the C ABI of the new entry points.  No GPU needed; the kernels are checked in tests/test_gpu_augment_boxes.py / test_gpu_targets.py."""
import re
import os

import numpy as np
import pytest
import torch

VOXEL = 0.02
_LOAD = [dict(type='LoadPointsFromFile', coord_type='DEPTH', shift_height=False, use_color=True, load_dim=6, use_dim=[0, 1, 2, 3, 4, 5]),
         dict(type='LoadAnnotations3D_', with_label_3d=True, with_bbox_3d=True, with_sp_mask_3d=True)]
_PACK = [dict(type='Pack3DDetInputs_', keys=['points', 'elastic_coords', 'gt_bboxes_3d', 'gt_labels_3d', 'sp_pts_mask'])]


def _six_dof(num_points):
    return _LOAD + [
        dict(type='PointSample_', num_points=num_points),
        dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
        dict(type='GlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[0.9, 1.1], translation_std=[0.1, 0.1, 0.1], shift_height=False),
        dict(type='NormalizePointsColor_', color_mean=[127.5, 127.5, 127.5]),
        dict(type='ElasticTransfrom', gran=[6, 20], mag=[40, 160], voxel_size=VOXEL, p=-1)] + _PACK


# the four box pipelines of the reference's joint config (configs/unidet3d_1xb8_scannet_s3dis_multiscan_3rscan_scannetpp_arkitscenes.py
# :291-329, :365-403, :440-478, :512-553) as plain dicts
MULTISCAN_TRAIN, RSCAN_TRAIN, SCANNETPP_TRAIN = _six_dof(100000), _six_dof(100000), _six_dof(200000)
ARKIT_TRAIN = _LOAD + [
    dict(type='PointSample_', num_points=100000),
    dict(type='DenormalizePointsColor', color_mean=[0, 0, 0], color_std=[255, 255, 255]),
    dict(type='NormalizePointsColor_', color_mean=[127.5, 127.5, 127.5]),
    dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
    dict(type='GlobalRotScaleTrans', rot_range=[-0.5, 0.5], scale_ratio_range=[0.9, 1.1], translation_std=[0.1, 0.1, 0.1], shift_height=False),
    dict(type='ElasticTransfrom', gran=[6, 20], mag=[40, 160], voxel_size=VOXEL, p=-1)] + _PACK


def _box_scene(n=8, g=2, dof=7, name='arkitscenes'):
    rng = np.random.RandomState(n + g)
    b = np.concatenate([rng.randn(g, 3), rng.rand(g, 3) + 0.2, rng.uniform(-1, 1, (g, 1))], 1).astype(np.float32)[:, :dof]
    return dict(points=rng.rand(n, 6).astype(np.float32), sp_pts_mask=np.arange(n) % 3, gt_bboxes_3d=b, gt_labels_3d=np.arange(g) % 5,
                lidar_path=f'data/{name}/points/s{n}.bin')


def _mask_scene(n=6):
    return dict(points=np.zeros((n, 6), np.float32), sp_pts_mask=np.zeros(n, np.int64), pts_instance_mask=np.zeros(n, np.int64),
                pts_semantic_mask=np.zeros(n, np.int64))


def test_new_entry_points_symbols_arity_and_empty_calls():
    from unidet3d_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'u3d.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    l = _lib.lib()
    for name, n_args in (('u3d_aug_points_dn', 16), ('u3d_aug_boxes', 11), ('u3d_targets_by_distance', 16), ('u3d_targets_by_distance_ws_bytes', 1)):
        assert name in _lib.PROTOTYPES and hasattr(l, name)
        m = re.search(r'\b' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S)
        assert m and len(m.group(1).split(',')) == n_args == len(_lib.PROTOTYPES[name][1]), name
    assert len(_lib.PROTOTYPES['u3d_aug_points'][1]) == 14                        # the existing entry point keeps its argument list
    # zero points / boxes / scenes launch nothing and succeed (no GPU needed); bad sizes are a clean error code
    assert l.u3d_aug_points_dn(None, 0, None, None, None, 0, 0, None, None, None, None, None, 0.02, None, None, None) == 0
    assert l.u3d_aug_points_dn(None, 0, None, None, None, 0, 5, None, None, None, None, None, 0.02, None, None, None) == -1
    assert l.u3d_aug_boxes(None, 0, None, None, 0, 0, None, None, None, None, None) == 0
    assert l.u3d_aug_boxes(None, 0, None, None, 0, -1, None, None, None, None, None) == -1
    assert l.u3d_aug_boxes(None, 0, None, None, 2, 3, None, None, None, None, None) == -1
    assert l.u3d_targets_by_distance(None, 0, None, None, 3, 0, None, None, 0, 0, 0, 0, 6, None, None, None) == 0
    assert l.u3d_targets_by_distance(None, 0, None, None, 3, 0, None, None, 0, 4, 0, 100, 6, None, None, None) == 0      # no box anywhere
    assert l.u3d_targets_by_distance(None, 10, None, None, 3, 2, None, None, 20, 1, 2, 10, 6, None, None, None) == -1    # null pointers
    assert l.u3d_targets_by_distance(None, 0, None, None, 3, 0, None, None, 0, 0, 0, 0, 16, None, None, None) == -3      # topk + 1 > 16
    assert b'topk' in l.u3d_last_error()
    assert l.u3d_targets_by_distance_ws_bytes(100) >= 400 and l.u3d_targets_by_distance_ws_bytes(0) == 0
    assert l.u3d_targets_by_distance_ws_bytes(-1) < 0


def test_from_pipeline_parses_the_four_box_pipelines():
    from unidet3d_amd import DeviceAugment
    for pl, n in ((MULTISCAN_TRAIN, 100000), (RSCAN_TRAIN, 100000), (SCANNETPP_TRAIN, 200000)):
        a = DeviceAugment.from_pipeline(pl, VOXEL)
        assert a.kind == 'box' and a.mapping is None and a.num_points == n and a.rot_range == (0.0, 0.0) and a.scale_range == (0.9, 1.1)
        assert a.denorm_mean is None and a.denorm_std is None and a.color_mean.tolist() == [127.5] * 3 and a.elastic['p'] == -1
    k = DeviceAugment.from_pipeline(ARKIT_TRAIN, VOXEL)
    assert k.kind == 'box' and k.rot_range == (-0.5, 0.5) and k.num_points == 100000
    assert k.denorm_mean.tolist() == [0.0] * 3 and k.denorm_std.tolist() == [255.0] * 3 and k.denorm_std.dtype == np.float32
    assert k.color_mean.tolist() == [127.5] * 3 and k.color_std.tolist() == [127.5] * 3
    from test_augment_cpu import SCANNET_TRAIN
    assert DeviceAugment.from_pipeline(SCANNET_TRAIN, VOXEL).kind == 'mask'
    with pytest.raises(NotImplementedError, match='DenormalizePointsColor'):       # the step must precede the normalisation
        DeviceAugment.from_pipeline([ARKIT_TRAIN[4], ARKIT_TRAIN[3]], VOXEL)


def test_box_scene_cache_and_refusals():
    from unidet3d_amd import DeviceSceneCache
    ds = [_box_scene(8, 2, 7), _box_scene(5, 0, 7), _box_scene(9, 3, 6, 'multiscan')]
    c = DeviceSceneCache.from_scene_dicts(ds, 'cpu')
    assert c.kind == 'box' and c.box_offsets == [0, 2, 2, 5] and c.scene_with_yaw == [True, True, False] and c.offsets == [0, 8, 13, 22]
    assert c.boxes.shape == (5, 7) and c.boxes.dtype == torch.float32 and c.box_labels.dtype == torch.int64 and c.with_yaw.tolist() == [1, 1, 0]
    assert np.array_equal(c.boxes[:2].numpy(), ds[0]['gt_bboxes_3d']) and np.array_equal(c.boxes[2:, :6].numpy(), ds[2]['gt_bboxes_3d'])
    assert not c.boxes[2:, 6].any() and c.pts_instance_mask is None and c.pts_semantic_mask is None and c.max_sp == [2, 2, 2]
    assert DeviceSceneCache.from_scene_dicts([_mask_scene()], 'cpu').kind == 'mask'
    with pytest.raises(ValueError, match='one cache'):
        DeviceSceneCache.from_scene_dicts([_box_scene(), _mask_scene()], 'cpu')
    with pytest.raises(NotImplementedError, match='box'):                          # masks and boxes in one dict stay refused
        DeviceSceneCache.from_scene_dicts([dict(_mask_scene(), gt_bboxes_3d=np.zeros((1, 7), np.float32), gt_labels_3d=np.zeros(1))], 'cpu')
    with pytest.raises(NotImplementedError, match='axis_align_matrix'):
        DeviceSceneCache.from_scene_dicts([dict(_box_scene(), axis_align_matrix=np.eye(4))], 'cpu')
    with pytest.raises(NotImplementedError, match='gt_bboxes_3d'):
        DeviceSceneCache.from_scene_dicts([dict(points=np.zeros((2, 6), np.float32), sp_pts_mask=np.zeros(2, np.int64), ann_info={})], 'cpu')


def test_kind_mismatch_and_rotation_of_yaw_free_boxes_are_refused():
    """the checks run before any kernel is touched, so CPU-resident caches show them"""
    from unidet3d_amd import DeviceAugment, DeviceSceneCache, MixedDeviceAugment
    from test_augment_cpu import SCANNET_TRAIN
    boxes = DeviceSceneCache.from_scene_dicts([_box_scene(8, 2, 7), _box_scene(9, 3, 6, 'multiscan')], 'cpu')
    masks = DeviceSceneCache.from_scene_dicts([_mask_scene()], 'cpu')
    with pytest.raises(ValueError, match='box-annotated pipeline'):
        DeviceAugment.from_pipeline(MULTISCAN_TRAIN, VOXEL)(masks, [0])
    with pytest.raises(ValueError, match='mask-annotated pipeline'):
        DeviceAugment.from_pipeline(SCANNET_TRAIN, VOXEL)(boxes, [0])
    with pytest.raises(NotImplementedError, match='rotation'):                      # ARKitScenes' rot_range on a six-column scene
        DeviceAugment.from_pipeline(ARKIT_TRAIN, VOXEL)(boxes, [0, 1])
    with pytest.raises(ValueError, match='multiscan'):
        MixedDeviceAugment(dict(multiscan=(DeviceAugment.from_pipeline(MULTISCAN_TRAIN, VOXEL), masks)))
    with pytest.raises(KeyError):
        MixedDeviceAugment(dict(multiscan=(DeviceAugment.from_pipeline(MULTISCAN_TRAIN, VOXEL), boxes)))([('s3dis', 0)])


def test_denormalize_points_color_host_step():
    from unidet3d_amd import transforms as X
    from unidet3d_amd.registry import TRANSFORMS
    pts = np.concatenate([np.zeros((4, 3)), np.array([[0, 1 / 255, 0.5], [1.0, 0.25, 0.75], [0.1, 0.2, 0.3], [1, 1, 1]])], 1).astype(np.float32)
    step = TRANSFORMS.build(dict(type='DenormalizePointsColor', color_mean=[0, 0, 0], color_std=[255, 255, 255]))
    out = step(dict(points=pts.copy()))['points']
    assert out.dtype == np.float32 and np.array_equal(out[:, 3:], pts[:, 3:] * np.float32(255) + np.float32(0)) and np.array_equal(out[:, :3], pts[:, :3])
    assert out[0, 4] == 1.0 and out[3, 3] == 255.0
    two = X.NormalizePointsColor_([127.5] * 3)(dict(points=out))['points']
    assert np.array_equal(two[:, 3:], (out[:, 3:] - np.float32(127.5)) / np.float32(127.5))


def _local(points_xy, box):
    """box-local BEV coordinates of points with the counter-clockwise heading convention of criterion._box2corners:
    world = centre + R(yaw) local, so local = R(-yaw) (world - centre)"""
    c, s = np.cos(box[6]), np.sin(box[6])
    d = points_xy - box[None, :2]
    return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], 1)


CASES = [(False, False, 0.0), (True, False, 0.5), (False, True, -0.5), (True, True, 0.5), (True, False, 0.0), (False, True, 0.37), (False, False, -0.5)]


def test_transform_boxes_moves_boxes_with_the_points():
    """Points placed at known box-local coordinates, transformed with the points' affine, sit at scale x the same local coordinates
    of the transformed box (local y mirrored under a single flip); z and the sizes scale.  float32 results against float64
    expectations: coordinates below 8 carry errors of a few 1e-7, against local extents of order 1 -> 1e-5 of the largest extent."""
    from unidet3d_amd import criterion as pc
    from unidet3d_amd import transforms as X
    from unidet3d_amd.augment import compose_affine
    rng = np.random.RandomState(7)
    # the convention the helper above assumes is criterion._box2corners': corner 0 = centre + R(yaw) (+w/2, +h/2)
    probe = np.array([0.3, -0.2, 2.0, 1.0, 0.7])
    c0 = pc._box2corners(torch.from_numpy(probe))[0].numpy()
    assert np.allclose(_local(c0[None], np.array([0.3, -0.2, 0, 0, 0, 0, 0.7]))[0], [1.0, 0.5], atol=1e-12)
    worst = 0.0
    for k, (fh, fv, th) in enumerate(CASES):
        G = 9
        boxes = np.concatenate([rng.uniform(-3, 3, (G, 3)), rng.uniform(0.3, 2.0, (G, 3)), rng.uniform(-3.1, 3.1, (G, 1))], 1).astype(np.float32)
        scale, trans = rng.uniform(0.9, 1.1), rng.randn(3) * 0.1
        out = X.transform_boxes(boxes, fh, fv, th, scale, trans)
        assert out.dtype == np.float32 and out.shape == boxes.shape
        A = compose_affine([fh], [fv], [th], [scale], [trans])[0]
        for g in range(G):
            b64 = boxes[g].astype(np.float64)
            local = rng.uniform(-1, 1, (12, 3)) * b64[3:6] / 2
            c, s = np.cos(b64[6]), np.sin(b64[6])
            world = np.stack([b64[0] + c * local[:, 0] - s * local[:, 1], b64[1] + s * local[:, 0] + c * local[:, 1], b64[2] + local[:, 2]], 1).astype(np.float32)
            x, y, z = world[:, 0], world[:, 1], world[:, 2]
            moved = np.stack([((A[r, 0] * x + A[r, 1] * y) + A[r, 2] * z) + A[r, 3] for r in range(3)], 1)
            assert moved.dtype == np.float32
            o64 = out[g].astype(np.float64)
            got = np.concatenate([_local(moved[:, :2].astype(np.float64), o64), moved[:, 2:3].astype(np.float64) - o64[2]], 1)
            want = scale * local * np.array([1.0, -1.0 if fh != fv else 1.0, 1.0])
            worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
            assert np.abs(o64[3:6] - scale * b64[3:6]).max() <= 1e-5 * np.abs(b64[3:6]).max()
    print('box-local coordinates after the transform: worst relative deviation', worst)
    assert worst <= 1e-5


def _iou3d(b1, b2):
    """rotated 3-D IoU from the oracle's BEV polygon intersection"""
    from oracle import rotated_iou as R
    b1, b2 = torch.from_numpy(b1).double(), torch.from_numpy(b2).double()
    inter = R.oriented_box_intersection_2d(R.box2corners(b1[:, [0, 1, 3, 4, 6]]), R.box2corners(b2[:, [0, 1, 3, 4, 6]]))
    zo = (torch.min(b1[:, 2] + b1[:, 5] / 2, b2[:, 2] + b2[:, 5] / 2) - torch.max(b1[:, 2] - b1[:, 5] / 2, b2[:, 2] - b2[:, 5] / 2)).clamp(min=0)
    i3 = inter * zo
    return (i3 / (b1[:, 3:6].prod(1) + b2[:, 3:6].prod(1) - i3)).numpy()


def test_transform_boxes_preserves_rotated_iou():
    """IoU is invariant under rigid motion, mirroring and uniform scale"""
    from unidet3d_amd import transforms as X
    rng = np.random.RandomState(11)
    G = 12
    b1 = np.concatenate([rng.uniform(-2, 2, (G, 3)), rng.uniform(0.8, 2.0, (G, 3)), rng.uniform(-3.1, 3.1, (G, 1))], 1).astype(np.float32)
    b2 = b1.copy()
    b2[:, :3] += rng.uniform(-0.4, 0.4, (G, 3)).astype(np.float32)
    b2[:, 3:6] *= rng.uniform(0.8, 1.2, (G, 3)).astype(np.float32)
    b2[:, 6] += rng.uniform(-0.6, 0.6, G).astype(np.float32)
    before = _iou3d(b1, b2)
    assert (before > 0.05).all() and (before < 0.95).all()
    for fh, fv, th in CASES:
        scale, trans = rng.uniform(0.9, 1.1), rng.randn(3) * 0.1
        after = _iou3d(X.transform_boxes(b1, fh, fv, th, scale, trans), X.transform_boxes(b2, fh, fv, th, scale, trans))
        assert np.abs(after - before).max() <= 1e-5, (fh, fv, th, np.abs(after - before).max())


def test_transform_boxes_six_columns_and_yaw_arithmetic():
    from unidet3d_amd import transforms as X
    b6 = np.array([[1.0, 2.0, 3.0, 0.5, 0.6, 0.7]], np.float32)
    out = X.transform_boxes(b6, True, True, 0.0, 1.1, [0.1, 0.2, 0.3])
    assert out.shape == (1, 6) and np.array_equal(out[0, 3:], b6[0, 3:] * np.float32(1.1))
    assert np.allclose(out[0, :3], [-1.1 + 0.1, -2.2 + 0.2, 3.3 + 0.3], atol=1e-6)
    with pytest.raises(NotImplementedError):
        X.transform_boxes(b6, False, False, 0.3, 1.0, [0, 0, 0])
    assert X.transform_boxes(np.zeros((0, 7), np.float32), True, False, 0.2, 1.0, [0, 0, 0]).shape == (0, 7)
    b7 = np.array([[0, 0, 0, 1, 1, 1, 0.25]], np.float32)
    yaw = np.float64(b7[0, 6])
    assert X.transform_boxes(b7, True, False, 0.5, 1.0, [0, 0, 0])[0, 6] == np.float32(np.pi - yaw + 0.5)       # float64, rounded once
    assert X.transform_boxes(b7, False, True, -0.5, 1.0, [0, 0, 0])[0, 6] == np.float32(-yaw - 0.5)
    assert X.transform_boxes(b7, True, True, 0.5, 1.0, [0, 0, 0])[0, 6] == np.float32(-(np.pi - yaw) + 0.5)      # no period wrapping
    assert np.array_equal(X.transform_boxes(b7, False, False, 0.0, 1.0, [0, 0, 0]), b7)


def test_to_batch_inputs_packs_box_scenes():
    from unidet3d_amd import transforms as X
    d = _box_scene(8, 2, 7)
    d['elastic_coords'] = d['points'][:, :3] / np.float32(VOXEL)
    z = dict(_box_scene(5, 0, 6, 'multiscan'))
    z['elastic_coords'] = z['points'][:, :3] / np.float32(VOXEL)
    inputs, samples = X.to_batch_inputs([d, z], 'cpu')
    assert len(inputs['points']) == 2 and len(inputs['elastic_coords']) == 2
    s = samples[0]
    assert s.gt_pts_seg.pts_instance_mask is None and torch.equal(s.gt_pts_seg.sp_pts_mask, torch.from_numpy(d['sp_pts_mask']))
    b = s.gt_instances_3d.bboxes_3d
    assert b.with_yaw and b.box_dim == 7 and \
        torch.allclose(b.gravity_center, torch.from_numpy(d['gt_bboxes_3d'][:, :3].copy()), atol=1e-6)
    assert s.gt_instances_3d.labels_3d.dtype == torch.int64 and s.n_superpoints == 3 and 'arkitscenes' in s.lidar_path.split('/')
    e = samples[1].gt_instances_3d
    assert not e.bboxes_3d.with_yaw and e.bboxes_3d.tensor.shape == (0, 6) and e.labels_3d.shape == (0,)
