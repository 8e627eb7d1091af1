"""Host-side logic of the device augmentation (unidet3d_amd/augment.py): pipeline parsing, the affine convention and the draws.
No GPU needed; the kernels are checked in tests/test_gpu_augment.py."""
import numpy as np
import pytest
import torch

VOXEL = 0.02

# the reference's train pipelines (configs/unidet3d_1xb8_scannet.py:111-158, :200-247) as plain dicts
SCANNET_TRAIN = [
    dict(type='LoadPointsFromFile', coord_type='DEPTH', shift_height=False, use_color=True, load_dim=6, use_dim=[0, 1, 2, 3, 4, 5]),
    dict(type='LoadAnnotations3D_', with_bbox_3d=False, with_label_3d=False, with_mask_3d=True, with_seg_3d=True, with_sp_mask_3d=True),
    dict(type='GlobalAlignment', rotation_axis=2),
    dict(type='PointSegClassMapping'),
    dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
    dict(type='GlobalRotScaleTrans', rot_range=[-3.14, 3.14], scale_ratio_range=[0.8, 1.2], translation_std=[0.1, 0.1, 0.1], shift_height=False),
    dict(type='NormalizePointsColor_', color_mean=[127.5, 127.5, 127.5]),
    dict(type='PointDetClassMappingScanNet', num_classes=20, stuff_classes=[0, 1]),
    dict(type='ElasticTransfrom', gran=[6, 20], mag=[40, 160], voxel_size=VOXEL, p=0.5),
    dict(type='Pack3DDetInputs_', keys=['points', 'gt_labels_3d', 'pts_semantic_mask', 'pts_instance_mask', 'sp_pts_mask', 'gt_sp_masks',
                                        'elastic_coords']),
]
S3DIS_TRAIN = [
    dict(type='LoadPointsFromFile', coord_type='DEPTH', shift_height=False, use_color=True, load_dim=6, use_dim=[0, 1, 2, 3, 4, 5]),
    dict(type='LoadAnnotations3D_', with_label_3d=False, with_bbox_3d=False, with_mask_3d=True, with_seg_3d=True, with_sp_mask_3d=True),
    dict(type='PointSample_', num_points=180000),
    dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
    dict(type='GlobalRotScaleTrans', rot_range=[0.0, 0.0], scale_ratio_range=[0.9, 1.1], translation_std=[.1, .1, .1], shift_height=False),
    dict(type='PointDetClassMappingS3DIS', classes=[7, 8, 9, 10, 11]),
    dict(type='NormalizePointsColor_', color_mean=[127.5, 127.5, 127.5]),
    dict(type='ElasticTransfrom', gran=[6, 20], mag=[40, 160], voxel_size=VOXEL, p=-1),
    dict(type='Pack3DDetInputs_', keys=['points', 'elastic_coords', 'gt_labels_3d', 'sp_pts_mask', 'gt_sp_masks', 'pts_semantic_mask',
                                        'pts_instance_mask']),
]


def test_from_pipeline_parses_the_reference_train_pipelines():
    from unidet3d_amd import DeviceAugment
    a = DeviceAugment.from_pipeline(SCANNET_TRAIN, VOXEL)
    assert a.num_points is None and (a.flip_ratio_h, a.flip_ratio_v) == (0.5, 0.5)
    assert a.rot_range == (-3.14, 3.14) and a.scale_range == (0.8, 1.2) and a.translation_std == (0.1, 0.1, 0.1)
    assert a.color_mean.tolist() == [127.5] * 3 and a.color_std.tolist() == [127.5] * 3 and a.color_mean.dtype == np.float32
    assert a.mapping == ('scannet', 20, [0, 1])
    assert a.elastic == dict(gran=[6, 20], mag=[40, 160], p=0.5) and a.voxel_size == VOXEL
    s = DeviceAugment.from_pipeline(S3DIS_TRAIN, VOXEL)
    assert s.num_points == 180000 and s.rot_range == (0.0, 0.0) and s.scale_range == (0.9, 1.1)
    assert s.mapping == ('s3dis', [7, 8, 9, 10, 11]) and s.elastic['p'] == -1


def test_load_time_steps_are_recorded_for_the_cache_check():
    from unidet3d_amd import DeviceAugment, DeviceSceneCache
    assert DeviceAugment.from_pipeline(SCANNET_TRAIN, VOXEL).load_time_steps == ('GlobalAlignment', 'PointSegClassMapping')
    assert DeviceAugment.from_pipeline(S3DIS_TRAIN, VOXEL).load_time_steps == ()
    d = dict(points=np.zeros((4, 6), np.float32), sp_pts_mask=np.zeros(4, np.int64), pts_instance_mask=np.zeros(4, np.int64),
             pts_semantic_mask=np.zeros(4, np.int64))
    c = DeviceSceneCache.from_scene_dicts([d], 'cpu')
    assert not c.has_alignment and not c.has_seg_mapping
    c = DeviceSceneCache.from_scene_dicts([dict(d, axis_align_matrix=np.eye(4))], 'cpu', seg_label_mapping=np.arange(3))
    assert c.has_alignment and c.has_seg_mapping


def test_from_pipeline_refuses_what_it_does_not_implement():
    from unidet3d_amd import DeviceAugment
    with pytest.raises(NotImplementedError, match='RandomDropPointsColor'):
        DeviceAugment.from_pipeline(SCANNET_TRAIN[:5] + [dict(type='RandomDropPointsColor', drop_ratio=0.2)], VOXEL)
    with pytest.raises(NotImplementedError, match='MultiScaleFlipAug3D'):            # test-time wrapper: this is the training path
        DeviceAugment.from_pipeline([dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=1, flip=False, transforms=[])], VOXEL)
    with pytest.raises(NotImplementedError, match='PointSample_'):                   # sampling after the GT masks were built
        DeviceAugment.from_pipeline([S3DIS_TRAIN[5], S3DIS_TRAIN[2]], VOXEL)


def test_box_annotated_scenes_are_refused():
    from unidet3d_amd import DeviceSceneCache
    d = dict(points=np.zeros((4, 6), np.float32), sp_pts_mask=np.zeros(4, np.int64), pts_instance_mask=np.zeros(4, np.int64),
             pts_semantic_mask=np.zeros(4, np.int64), gt_bboxes_3d=np.zeros((1, 7), np.float32))
    with pytest.raises(NotImplementedError, match='box'):
        DeviceSceneCache.from_scene_dicts([d], 'cpu')


def test_scene_cache_records_offsets_and_maxima():
    from unidet3d_amd import DeviceSceneCache
    ds = [dict(points=np.ones((n, 6), np.float32), sp_pts_mask=np.arange(n) % 3, pts_instance_mask=np.arange(n) % 5 - 1,
               pts_semantic_mask=np.arange(n) % 7, lidar_path=f'data/scannet/points/s{n}.bin') for n in (10, 0, 4)]
    c = DeviceSceneCache.from_scene_dicts(ds, 'cpu')
    assert c.offsets == [0, 10, 10, 14] and c.max_inst == [3, -1, 2] and c.max_sp == [2, -1, 2] and len(c) == 3
    assert c.points.shape == (14, 6) and c.pts_instance_mask.dtype == torch.int64 and c.lidar_paths[2].endswith('s4.bin')


def test_affine_is_flip_then_rotation_then_scale_then_translation():
    from unidet3d_amd.augment import compose_affine
    th, sc, t = 0.3, 1.1, np.array([0.1, -0.2, 0.05])
    A = compose_affine([True, False, False], [False, True, False], [th, th, 0.0], [sc, sc, 1.0], [t, t, np.zeros(3)])
    assert A.dtype == np.float32 and A.shape == (3, 3, 4)
    c, s = np.cos(th), np.sin(th)
    p = np.array([1.0, 2.0, 3.0])
    for b, f in ((0, np.array([-1.0, 2.0, 3.0])), (1, np.array([1.0, -2.0, 3.0]))):        # horizontal: x -> -x, vertical: y -> -y
        want = sc * np.array([f[0] * c - f[1] * s, f[0] * s + f[1] * c, f[2]]) + t
        assert np.allclose(A[b, :, :3].astype(np.float64) @ p + A[b, :, 3], want, atol=1e-6)
    assert np.array_equal(A[2], np.eye(3, 4, dtype=np.float32))                             # no draw: identity, exactly
    want64 = np.zeros((3, 4))
    want64[:, :3] = sc * (np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.diag([-1.0, 1.0, 1.0]))
    want64[:, 3] = t
    assert np.array_equal(A[0], want64.astype(np.float32))                                  # composed in float64, rounded once
    al = np.eye(4); al[:3, 3] = [1.0, 2.0, 3.0]                                             # axis_align_matrix is applied first
    B = compose_affine([False], [False], [0.0], [2.0], [np.zeros(3)], [al])
    assert np.array_equal(B[0], np.array([[2, 0, 0, 2], [0, 2, 0, 4], [0, 0, 2, 6]], dtype=np.float32))


def test_equal_seeds_give_equal_draws():
    from unidet3d_amd import DeviceAugment
    a = DeviceAugment.from_pipeline(SCANNET_TRAIN, VOXEL)
    d = [a.draw(8, torch.Generator().manual_seed(s)) for s in (5, 5, 6)]
    for k in ('flip_h', 'flip_v', 'angle', 'scale', 'trans', 'elastic_gate'):
        assert np.array_equal(getattr(d[0], k), getattr(d[1], k)), k
    assert d[0].device_seed == d[1].device_seed and d[0].device_seed != d[2].device_seed
    assert not np.array_equal(d[0].angle, d[2].angle)
    assert (np.abs(d[0].angle) <= 3.14).all() and ((d[0].scale >= 0.8) & (d[0].scale <= 1.2)).all() and d[0].trans.shape == (8, 3)
    g = torch.Generator().manual_seed(5)                       # one generator, two batches: the state moves on
    assert not np.array_equal(a.draw(8, g).angle, a.draw(8, g).angle)
    s = DeviceAugment.from_pipeline(S3DIS_TRAIN, VOXEL).draw(64, torch.Generator().manual_seed(1))
    assert not s.elastic_gate.any() and not s.angle.any()      # p = -1 never fires; rot_range [0, 0]


def test_abi_version_and_symbols():
    import re, os
    from unidet3d_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'u3d.h')).read()
    assert int(re.search(r'#define\s+U3D_ABI_VERSION\s+(\d+)', hdr).group(1)) == _lib.ABI_VERSION == 117
    l = _lib.lib()
    for name in ('u3d_aug_points', 'u3d_aug_extent_f32', 'u3d_aug_extent_f64', 'u3d_aug_noise_blur', 'u3d_aug_elastic', 'u3d_relabel_ids',
                 'u3d_aug_remap_ids', 'u3d_aug_sp_masks'):
        assert name in _lib.PROTOTYPES and hasattr(l, name) and re.search(r'\b' + name + r'\s*\(', hdr)
    assert l.u3d_aug_noise_blur_ws_bytes(1000) >= 2 * 3 * 1000 * 4 and l.u3d_relabel_ids_ws_bytes(100) >= 3 * 100 * 4
    assert l.u3d_aug_sp_masks_ws_bytes(50, 10) >= 60 * 4 and l.u3d_aug_noise_blur_ws_bytes(-1) < 0
    # zero points / zero scenes are valid calls that launch nothing (no GPU needed); a bad size is a clean EINVAL
    assert l.u3d_aug_points(None, 0, None, None, None, 0, 0, None, None, None, 0.02, None, None, None) == 0
    assert l.u3d_aug_extent_f32(None, None, 0, 0, None, None) == 0 and l.u3d_aug_noise_blur(None, None, None, 0, 0, None, None, None) == 0
    assert l.u3d_aug_elastic(None, 0, None, 1, None, 0, 0, None, None, None, None, 6.0, 40.0, None) == 0
    assert l.u3d_relabel_ids(None, 0, None, None, None, 0, 0, None, 0, 1, None, None, 0, None, None, None, None, None, None) == 0
    assert l.u3d_aug_sp_masks(None, None, None, 0, None, 0, 0, None, None, None, 0, 0, None, None, None) == 0
    assert l.u3d_aug_points(None, 0, None, None, None, 0, -1, None, None, None, 0.02, None, None, None) == -1
    assert l.u3d_aug_points(None, 0, None, None, None, 0, 5, None, None, None, 0.02, None, None, None) == -1
