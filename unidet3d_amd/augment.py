"""Training-input augmentation on the device: the reference's ScanNet / S3DIS train pipelines after file loading, for every scene of
a batch in one chain of HIP launches (csrc/augment.hip), fed from a device-resident scene cache.

``transforms.py`` (host, numpy) stays the oracle: what ``DeviceAugment.__call__`` returns is what ``transforms.to_batch_inputs``
returns for the same scenes and the same random draws, so ``UniDet3D.loss`` / ``prefetch`` / ``prefetch_step`` / ``train_step``
take it unchanged (``train_step(dict(inputs=..., data_samples=...))``).

Data flow of one call (B scenes, N' points after sampling):

  host    draws (flip flags, angle, scale, translation, elastic gate), the float64 affine rounded to float32, table sizes from the
          cache's per-scene maximum ids -> one pinned upload
  device  u3d_aug_points      gather + affine + colour + voxel-unit coords            1 launch
          u3d_aug_extent_f32  max |coord| per scene (elastic batches)                 2
          u3d_relabel_ids     instance ids (stuff classes -> -1, dense, first index)  5
          u3d_relabel_ids     superpoint ids (sampled pipelines only)                 5
          u3d_aug_remap_ids   S3DIS class filter (after [n_inst]-sized torch ops)     1
  read 1  distinct-id counts + pass-1 extents, one device-to-host copy
  device  u3d_aug_sp_masks    (instance, superpoint) histograms -> gt_sp_masks         3
          u3d_aug_noise_blur, u3d_aug_elastic  pass 1                                  6 + 1
          u3d_aug_extent_f64                                                           2
  read 2  pass-2 extents
  device  u3d_aug_noise_blur, u3d_aug_elastic  pass 2                                  6 + 1

Box-annotated scenes (MultiScan, 3RScan, ScanNet++, ARKitScenes: ``gt_bboxes_3d`` / ``gt_labels_3d`` and no per-point masks) go
through the same chain without the instance steps: ``u3d_aug_points_dn`` when the pipeline holds ``DenormalizePointsColor``, the
superpoint relabel of a sampled pipeline (its counts are the one read) and ``u3d_aug_boxes``, one launch for all boxes of the batch.
``MixedDeviceAugment`` serves a batch drawn from several datasets, one ``DeviceAugment`` call per dataset present.

Random draws are separated from arithmetic (``AugmentDraws``): a test injects every draw, a training loop lets
``DeviceAugment.draw`` take the scalars from a host generator and the per-point / per-cell draws (sample indices, noise) from torch
on the device.  The same generator state gives the same bits twice.

Affine convention.  Horizontal flip negates x, vertical flip negates y: mmdet3d's rule for the depth frame as its documentation
states it.  mmdet3d is not a dependency of this package, so the rule is not checked against its code here.  Then a rotation about z by theta, x' = x cos(theta) - y sin(theta), y' = x sin(theta) + y cos(theta); then the scale s;
then the translation t ~ N(0, std).  The host composes the matrix in float64 and rounds it to float32; the kernel evaluates
x' = ((a00 x + a01 y) + a02 z) + t0 in float32.  The reference's angle ranges are symmetric ([-3.14, 3.14], [0, 0]), so the sign
convention of the rotation does not change the distribution of the augmented scenes.

Boxes follow the points: the gravity centre goes through the same float32 expression, the size is multiplied by float32(s), and the
heading -- measured counter-clockwise from +x, as ``criterion._box2corners`` reads it -- becomes pi - yaw under the horizontal flip,
-yaw under the vertical one, then + theta, in float64, rounded once, without period wrapping (``transforms.transform_boxes`` is the
host twin).  A rotation of boxes without a heading would need mmdet3d's enclosing-box rule, which cannot be checked here: refused.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import warnings
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .structures import DepthInstance3DBoxes, InstanceData_, PointSegData

__all__ = ['DeviceSceneCache', 'DeviceAugment', 'MixedDeviceAugment', 'AugmentDraws', 'compose_affine', 'blur_noise_grids']

_LOADERS = ('LoadPointsFromFile', 'LoadAnnotations3D_', 'LoadAnnotations3D')
_PACKERS = ('Pack3DDetInputs_', 'Pack3DDetInputs')
_LOAD_TIME = ('GlobalAlignment', 'PointSegClassMapping')
_BOX_KEYS = ('gt_bboxes_3d', 'gt_bboxes', 'ann_info')
_MASK_KEYS = ('pts_instance_mask', 'pts_semantic_mask')


class DeviceSceneCache:
    """Pre-processed scenes (the output of ``transforms.load_scene_bins``) concatenated on the device: ``points`` float32 [N, 6],
    ``sp_pts_mask`` / ``pts_instance_mask`` / ``pts_semantic_mask`` int64 [N], host-side point offsets, ``lidar_path`` s and the
    per-scene maximum ids (read once here, on the host; they size the relabel tables).

    A cache holds scenes of one ``kind``.  'mask': the per-point instance / semantic ids above.  'box': no per-point ids but
    ``boxes`` float32 [G, 7] = (gravity centre, size, yaw; yaw 0 for scenes whose boxes have six columns), ``box_labels`` int64 [G]
    and ``with_yaw`` uint8 [n_scenes] on the device, ``box_offsets`` / ``scene_with_yaw`` on the host."""

    def __init__(self, points, sp, inst, sem, offsets, lidar_paths, max_inst, max_sp, align):
        self.points, self.sp_pts_mask, self.pts_instance_mask, self.pts_semantic_mask = points, sp, inst, sem
        self.offsets, self.lidar_paths, self.max_inst, self.max_sp, self.align = offsets, lidar_paths, max_inst, max_sp, align
        self.has_alignment = self.has_seg_mapping = False      # set by from_scene_dicts: what the load-time steps were given
        self.kind = 'mask'
        self.boxes = self.box_labels = self.with_yaw = None
        self.box_offsets, self.scene_with_yaw = [0], []

    @property
    def device(self):
        return self.points.device

    def __len__(self):
        return len(self.lidar_paths)

    @classmethod
    def from_scene_dicts(cls, dicts: Sequence[dict], device, seg_label_mapping=None) -> 'DeviceSceneCache':
        """``seg_label_mapping`` (optional int array): mmdet3d's ``PointSegClassMapping`` table, applied to the semantic ids here,
        once.  A scene dict may carry ``axis_align_matrix`` [4, 4] (``GlobalAlignment``); it is composed into every affine.

        A dict with ``gt_bboxes_3d`` float [G, 6 | 7] (gravity centre, size[, yaw]: the reference's dataset classes build their boxes
        with ``origin=(0.5, 0.5, 0.5)``) and ``gt_labels_3d`` int [G] (G may be 0) and NO instance / semantic mask is a box-annotated
        scene.  Box keys next to masks, other box forms and ``axis_align_matrix`` on a box scene (no reference box pipeline has
        ``GlobalAlignment``) raise ``NotImplementedError``; mask and box scenes in one call raise ``ValueError``."""
        pts, sp, inst, sem, offs, paths, mi, ms, al = [], [], [], [], [0], [], [], [], []
        boxes, blabels, boffs, wyaw = [], [], [0], []
        kinds = set()
        for i, d in enumerate(dicts):
            boxed = any(k in d for k in _BOX_KEYS)
            if boxed and any(k in d for k in _MASK_KEYS):
                raise NotImplementedError(f'scene {i}: box annotations next to instance / semantic masks are not transformed on the device '
                                          '(a box-annotated scene carries no per-point masks)')
            if boxed and ('gt_bboxes_3d' not in d or 'gt_labels_3d' not in d):
                raise NotImplementedError(f"scene {i}: box annotations are expected as 'gt_bboxes_3d' [G, 6 | 7] and 'gt_labels_3d' [G]")
            if boxed and 'axis_align_matrix' in d:
                raise NotImplementedError(f'scene {i}: axis_align_matrix on a box-annotated scene (no box pipeline of the reference has '
                                          'GlobalAlignment)')
            kinds.add('box' if boxed else 'mask')
            if len(kinds) > 1:
                raise ValueError(f'scene {i}: mask-annotated and box-annotated scenes in one cache; build one cache per kind')
            p = np.ascontiguousarray(np.asarray(d['points'], dtype=np.float32))
            assert p.ndim == 2 and p.shape[1] == 6, 'points: float32 [N, 6] (xyz, rgb 0..255) expected'
            ids = []
            for key in ('sp_pts_mask',) if boxed else ('sp_pts_mask', 'pts_instance_mask', 'pts_semantic_mask'):
                a = np.asarray(d[key]).astype(np.int64)
                assert a.shape == (len(p),), f'{key}: one id per point expected'
                assert not len(a) or a.min() >= -1, f'{key}: ids below -1'
                ids.append(a)
            if seg_label_mapping is not None and not boxed:
                ids[2] = np.asarray(seg_label_mapping, dtype=np.int64)[ids[2]]
            assert not len(p) or ids[0].min() >= 0, 'sp_pts_mask: superpoint ids must be non-negative'
            pts.append(p); sp.append(ids[0])
            if boxed:
                gb = d['gt_bboxes_3d']
                gb = np.asarray(gb.detach().cpu() if torch.is_tensor(gb) else gb, dtype=np.float32)
                gb = gb.reshape(-1, gb.shape[-1] if gb.ndim == 2 else 7)
                assert gb.shape[1] in (6, 7), 'gt_bboxes_3d: [G, 6] or [G, 7] (gravity centre, size[, yaw]) expected'
                gl = d['gt_labels_3d']
                gl = np.asarray(gl.detach().cpu() if torch.is_tensor(gl) else gl).astype(np.int64).reshape(-1)
                assert len(gl) == len(gb), 'gt_labels_3d: one label per box expected'
                wyaw.append(gb.shape[1] == 7)
                boxes.append(np.concatenate((gb, np.zeros((len(gb), 7 - gb.shape[1]), np.float32)), 1))
                blabels.append(gl)
                boffs.append(boffs[-1] + len(gb))
            else:
                inst.append(ids[1]); sem.append(ids[2])
            offs.append(offs[-1] + len(p))
            paths.append(str(d.get('lidar_path', 'data/scannet/points/scene.bin')))
            mi.append(int(ids[1].max()) if len(p) and not boxed else -1)
            ms.append(int(ids[0].max()) if len(p) else -1)
            al.append(np.asarray(d.get('axis_align_matrix', np.eye(4)), dtype=np.float64).reshape(4, 4))
        dev = torch.device(device)

        def up(parts, dtype, tail):
            a = np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)
            return torch.from_numpy(a).to(dev)
        box = kinds == {'box'}
        cache = cls(up(pts, np.float32, (6,)), up(sp, np.int64, ()), None if box else up(inst, np.int64, ()),
                    None if box else up(sem, np.int64, ()), offs, paths, mi, ms, al)
        cache.has_alignment = any('axis_align_matrix' in d for d in dicts)
        cache.has_seg_mapping = seg_label_mapping is not None
        if box:
            cache.kind = 'box'
            cache.boxes, cache.box_labels = up(boxes, np.float32, (7,)), up(blabels, np.int64, ())
            cache.with_yaw = torch.from_numpy(np.asarray(wyaw, dtype=np.uint8)).to(dev)
            cache.box_offsets, cache.scene_with_yaw = boffs, wyaw
        return cache


@dataclass
class AugmentDraws:
    """Every random draw of one batch.  ``indices`` (per-scene int64 sample indices) and ``noise`` (``noise(scene, pass_index, dims)
    -> float32 [3, d0, d1, d2]``) may be None: they are then drawn by torch on the device."""
    flip_h: np.ndarray
    flip_v: np.ndarray
    angle: np.ndarray
    scale: np.ndarray
    trans: np.ndarray
    elastic_gate: np.ndarray
    indices: Optional[Sequence] = None
    noise: Optional[Callable] = None
    device_seed: Optional[int] = None


def compose_affine(flip_h, flip_v, angle, scale, trans, align=None) -> np.ndarray:
    """float32 [B, 3, 4]: flip (x -> -x horizontal, y -> -y vertical), rotation about z, scale, translation, composed in float64 (after
    the optional per-scene ``axis_align_matrix``) and rounded once."""
    B = len(angle)
    out = np.zeros((B, 3, 4), dtype=np.float64)
    for b in range(B):
        c, s = np.cos(np.float64(angle[b])), np.sin(np.float64(angle[b]))
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        F = np.diag([-1.0 if flip_h[b] else 1.0, -1.0 if flip_v[b] else 1.0, 1.0])
        M = np.float64(scale[b]) * (R @ F)
        t = np.asarray(trans[b], dtype=np.float64)
        if align is not None:
            A = np.asarray(align[b], dtype=np.float64)
            M, t = M @ A[:3, :3], M @ A[:3, 3] + t
        out[b, :, :3], out[b, :, 3] = M, t
    return out.astype(np.float32)


def blur_noise_grids(noise: torch.Tensor, dims, device):
    """``transforms.elastic_noise_grids``' six blur sweeps for every scene of a batch in six launches.  ``noise``: the scenes'
    [3, d0, d1, d2] float32 grids, flattened and concatenated on the device; ``dims`` int [B, 3] (zero rows: no grid).  Returns
    (grids float32 [cells, 4] -- channels 0..2 of cell (i0 d1 + i1) d2 + i2 of scene b at row offsets[b] + cell --, dims int32 [B, 3]
    and offsets int64 [B + 1] on the device)."""
    dims = np.asarray(dims, dtype=np.int64).reshape(-1, 3)
    goff = np.concatenate(([0], np.cumsum(dims.prod(1)))).astype(np.int64)
    total = int(goff[-1])
    assert noise.numel() == 3 * total and noise.dtype == torch.float32
    d_dims, d_goff = L.h2d_pack([(dims.tolist(), torch.int32), (goff.tolist(), torch.int64)], device)
    grids = torch.empty((total, 4), dtype=torch.float32, device=device)
    ws = L.ws(L.lib().u3d_aug_noise_blur_ws_bytes(total), device)
    L.call('u3d_aug_noise_blur', L.ptr(noise), L.ptr(d_dims), L.ptr(d_goff), len(dims), total, L.ptr(grids), L.ptr(ws), L.stream())
    return grids, d_dims, d_goff


def _split_generator(generator, device):
    """(host generator, device generator or None).  A CPU generator is used as it is for the host scalars and seeds a device
    generator when one is needed; a device generator is used for the device draws and its state seeds the host generator."""
    if generator is None:
        if torch.device(device).type == 'cuda':
            idx = torch.device(device).index
            generator = torch.cuda.default_generators[torch.cuda.current_device() if idx is None else idx]
        else:
            generator = torch.default_generator
    if generator.device.type == 'cpu':
        return generator, None
    seed = int.from_bytes(hashlib.sha256(generator.get_state().numpy().tobytes()).digest()[:7], 'little')
    torch.randint(0, 2, (1,), generator=generator, device=generator.device)      # advance it even when the batch draws nothing on the device
    return torch.Generator().manual_seed(seed), generator


class DeviceAugment:
    """The train pipeline of a ScanNet- or S3DIS-style dataset on the device.

    ``from_pipeline`` reads the reference's list of step dicts.  The loaders (``LoadPointsFromFile``, ``LoadAnnotations3D_``) and
    the packer (``Pack3DDetInputs_``) are skipped: the cache holds what the former produce, ``__call__`` returns what the latter
    and the data preprocessor produce.  ``GlobalAlignment`` and ``PointSegClassMapping`` carry no randomness and depend on
    annotation metadata only: they are accepted and belong to cache construction (``DeviceSceneCache.from_scene_dicts``: a scene's
    ``axis_align_matrix`` is composed into the affine, ``seg_label_mapping`` is applied to the semantic ids once).  The test-time
    wrappers (``MultiScaleFlipAug3D``) and every other step type raise ``NotImplementedError``: this is the training path.
    Implemented: ``PointSample_``, ``RandomFlip3D``, ``GlobalRotScaleTrans``, ``NormalizePointsColor_``,
    ``PointDetClassMappingScanNet``, ``PointDetClassMappingS3DIS``, ``ElasticTransfrom``, ``DenormalizePointsColor``.  Geometry,
    colour and label steps act on disjoint columns, so their relative order is free; ``PointSample_`` must precede the class mapping,
    ``DenormalizePointsColor`` must precede ``NormalizePointsColor_`` and ``ElasticTransfrom`` must follow the geometric steps, as in
    the reference's lists.

    A list without a ``PointDetClassMapping*`` step is the pipeline of a box-annotated dataset (``kind == 'box'``; the reference's
    MultiScan / 3RScan / ScanNet++ / ARKitScenes lists); calling it on a mask-annotated cache, or a mask pipeline on a box cache,
    raises ``ValueError``.  An instance built through the constructor has ``kind = None`` and takes the cache's kind."""

    def __init__(self, voxel_size, num_points=None, flip_ratio_h=0.0, flip_ratio_v=0.0, rot_range=(0.0, 0.0), scale_range=(1.0, 1.0),
                 translation_std=(0.0, 0.0, 0.0), color_mean=None, color_std=None, mapping=None, elastic=None, denorm_mean=None,
                 denorm_std=None, kind=None):
        self.voxel_size = float(voxel_size)
        self.num_points = None if num_points is None else int(num_points)
        self.flip_ratio_h, self.flip_ratio_v = float(flip_ratio_h), float(flip_ratio_v)
        self.rot_range = tuple(float(r) for r in (rot_range if isinstance(rot_range, (list, tuple)) else (-rot_range, rot_range)))
        self.scale_range = tuple(float(s) for s in scale_range)
        self.translation_std = tuple(float(t) for t in (translation_std if isinstance(translation_std, (list, tuple))
                                                        else (translation_std,) * 3))
        self.color_mean = None if color_mean is None else np.broadcast_to(np.asarray(color_mean, dtype=np.float32), (3,)).copy()
        self.color_std = None if color_std is None else np.broadcast_to(np.asarray(color_std, dtype=np.float32), (3,)).copy()
        # DenormalizePointsColor in front of the normalisation: c * denorm_std + denorm_mean (unidet3d/loading.py:123-143)
        self.denorm_mean = None if denorm_mean is None else np.broadcast_to(np.asarray(denorm_mean, dtype=np.float32), (3,)).copy()
        self.denorm_std = None if denorm_std is None else np.broadcast_to(np.asarray(denorm_std, dtype=np.float32), (3,)).copy()
        self.kind = kind                  # None | 'mask' | 'box': the cache kind this pipeline is for (from_pipeline sets it)
        self.mapping = mapping            # None | ('scannet', num_classes, stuff_classes) | ('s3dis', classes)
        self.elastic = elastic            # None | dict(gran=[g0, g1], mag=[m0, m1], p=float)
        self._warned = set()
        self.load_time_steps = ()         # from_pipeline: the GlobalAlignment / PointSegClassMapping steps the list held
        # launches (kernels + memsets) the LIBRARY issued in the last call, summed from each entry point's documented count; the torch
        # ops of the path come on top: the randint / randn draws, sem[first], the cat of the read and, for S3DIS, the isin / cumsum /
        # where / scatter chain on [n_inst]-sized tables (a kernel trace of tools/augment_time.py counts everything)
        self.last_launches = 0
        self.last_host_reads = 0          # device-to-host reads of the last call

    @classmethod
    def from_pipeline(cls, pipeline_list, voxel_size) -> 'DeviceAugment':
        kw, seen, load_time = {}, [], []
        for step in pipeline_list:
            t = step['type']
            if t in _LOAD_TIME:
                load_time.append(t)
            if t in _LOADERS or t in _PACKERS or t in _LOAD_TIME:
                continue
            if t == 'PointSample_':
                if any(s.startswith('PointDetClassMapping') for s in seen):
                    raise NotImplementedError('PointSample_ after a PointDetClassMapping step')
                kw['num_points'] = step['num_points']
            elif t == 'RandomFlip3D':
                kw['flip_ratio_h'] = step.get('flip_ratio_bev_horizontal', 0.0)
                kw['flip_ratio_v'] = step.get('flip_ratio_bev_vertical', 0.0)
            elif t == 'GlobalRotScaleTrans':
                kw['rot_range'] = step.get('rot_range', [-0.78539816, 0.78539816])
                kw['scale_range'] = step.get('scale_ratio_range', [0.95, 1.05])
                kw['translation_std'] = step.get('translation_std', [0, 0, 0])
            elif t == 'NormalizePointsColor_':
                kw['color_mean'], kw['color_std'] = step['color_mean'], step.get('color_std', 127.5)
            elif t == 'DenormalizePointsColor':
                if 'NormalizePointsColor_' in seen:
                    raise NotImplementedError('DenormalizePointsColor after NormalizePointsColor_')
                kw['denorm_mean'], kw['denorm_std'] = step['color_mean'], step['color_std']
            elif t == 'PointDetClassMappingScanNet':
                kw['mapping'] = ('scannet', int(step['num_classes']), list(step['stuff_classes']))
            elif t == 'PointDetClassMappingS3DIS':
                kw['mapping'] = ('s3dis', list(step['classes']))
            elif t == 'ElasticTransfrom':
                assert float(step['voxel_size']) == float(voxel_size), 'ElasticTransfrom.voxel_size differs from the model voxel size'
                kw['elastic'] = dict(gran=list(step['gran']), mag=list(step['mag']), p=step.get('p', 1.0))
            else:
                raise NotImplementedError(f'pipeline step {t!r} is not implemented on the device')
            if t in ('RandomFlip3D', 'GlobalRotScaleTrans', 'PointSample_') and 'ElasticTransfrom' in seen:
                raise NotImplementedError(f'{t} after ElasticTransfrom')
            seen.append(t)
        aug = cls(voxel_size, kind='box' if kw.get('mapping') is None else 'mask', **kw)
        aug.load_time_steps = tuple(load_time)
        return aug

    # ------------------------------------------------------------------ draws
    def draw(self, B: int, generator=None, device='cpu') -> AugmentDraws:
        """The host scalars of one batch from ``generator`` (see ``_split_generator``); sample indices and noise stay with the device."""
        host, dgen = _split_generator(generator, device)
        return self._draw_host(B, host, dgen is None)

    def _draw_host(self, B, host, need_seed):
        u = torch.rand(B, 5, generator=host, dtype=torch.float64).numpy()
        g = torch.randn(B, 3, generator=host, dtype=torch.float64).numpy()
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=host)) if need_seed else None
        lo, hi = self.rot_range
        s0, s1 = self.scale_range
        p = -1.0 if self.elastic is None else float(self.elastic['p'])
        return AugmentDraws(flip_h=u[:, 0] < self.flip_ratio_h, flip_v=u[:, 1] < self.flip_ratio_v, angle=lo + (hi - lo) * u[:, 2],
                            scale=s0 + (s1 - s0) * u[:, 3], trans=g * np.asarray(self.translation_std, dtype=np.float64)[None],
                            elastic_gate=u[:, 4] < p, device_seed=seed)

    # ------------------------------------------------------------------ the batch
    def __call__(self, cache: DeviceSceneCache, scene_ids, draws: Optional[AugmentDraws] = None, generator=None):
        """``(batch_inputs_dict, batch_data_samples)`` of the scenes ``scene_ids`` of ``cache``: ``points`` / ``elastic_coords`` lists
        and ``ready_event``; per sample ``gt_pts_seg.sp_pts_mask`` / ``pts_instance_mask`` (/ ``pts_semantic_mask``),
        ``gt_instances_3d.labels_3d`` / ``sp_masks``, ``n_superpoints``, ``lidar_path`` -- dtypes and shapes of
        ``transforms.to_batch_inputs``; the per-scene tensors are views of batch buffers.  A box-annotated cache gives
        ``gt_pts_seg.sp_pts_mask`` alone and ``gt_instances_3d.labels_3d`` / ``bboxes_3d`` (``DepthInstance3DBoxes``, 6 or 7 columns)."""
        from .structures import Det3DDataSample
        dev = cache.device
        B = len(scene_ids)
        if B == 0:
            raise ValueError('DeviceAugment: empty batch')
        boxed = cache.kind == 'box'
        if self.kind is not None and self.kind != cache.kind:
            raise ValueError(f'DeviceAugment: a {self.kind}-annotated pipeline was called on a {cache.kind}-annotated scene cache')
        if boxed and self.mapping is not None:
            raise ValueError('DeviceAugment: a PointDetClassMapping step needs instance masks, the scene cache holds box annotations')
        if boxed and self.rot_range != (0.0, 0.0) and not all(cache.scene_with_yaw[s] for s in scene_ids):
            raise NotImplementedError('DeviceAugment: a rotation range on boxes without a heading (mmdet3d encloses the rotated box; '
                                      'that rule cannot be checked here and no reference config uses it)')
        st = L.stream()
        self.last_launches = self.last_host_reads = 0
        for step, given, how in (('GlobalAlignment', cache.has_alignment, "no scene dict carried 'axis_align_matrix'"),
                                 ('PointSegClassMapping', cache.has_seg_mapping, 'from_scene_dicts got no seg_label_mapping')):
            if step in self.load_time_steps and not given and (step, id(cache)) not in self._warned:
                self._warned.add((step, id(cache)))
                warnings.warn(f'the pipeline holds {step}, which belongs to cache construction, but {how}: the step is not applied')
        dgen = None
        if draws is None:
            host_gen, dgen = _split_generator(generator, dev)
            draws = self._draw_host(B, host_gen, dgen is None)
        if dgen is None and (draws.noise is None or draws.indices is None) and dev.type == 'cuda':
            dgen = torch.Generator(dev).manual_seed(0 if draws.device_seed is None else draws.device_seed)
        n_src = [cache.offsets[s + 1] - cache.offsets[s] for s in scene_ids]
        sampled = self.num_points is not None
        m = [min(self.num_points, n) for n in n_src] if sampled else list(n_src)
        off = np.concatenate(([0], np.cumsum(m))).astype(np.int64)
        N = int(off[-1])
        gate = np.asarray(draws.elastic_gate, dtype=bool) & np.asarray(m, dtype=bool) if self.elastic is not None else np.zeros(B, dtype=bool)
        affine = compose_affine(draws.flip_h, draws.flip_v, draws.angle, draws.scale, draws.trans, [cache.align[s] for s in scene_ids])
        need_inst = (sampled or self.mapping is not None) and not boxed
        t_inst = np.concatenate(([0], np.cumsum([cache.max_inst[s] + 2 for s in scene_ids]))).astype(np.int64)
        t_sp = np.concatenate(([0], np.cumsum([cache.max_sp[s] + 2 for s in scene_ids]))).astype(np.int64)
        tab_scene = np.repeat(np.arange(B), np.diff(t_inst))
        tab_local = np.arange(t_inst[-1]) - t_inst[:-1][tab_scene]
        drop = np.zeros(1, dtype=np.uint8)
        if self.mapping is not None and self.mapping[0] == 'scannet':
            cl = [self.mapping[1]] + list(self.mapping[2])
            drop = np.zeros(max(cl) + 1, dtype=np.uint8)
            drop[cl] = 1
        src = np.stack([[cache.offsets[s] for s in scene_ids], n_src], axis=1).astype(np.int64)
        specs = [(off.tolist(), torch.int64), (src.tolist(), torch.int64), (affine.tolist(), torch.float32), (t_inst.tolist(), torch.int64),
                 (t_sp.tolist(), torch.int64), (gate.astype(np.uint8).tolist(), torch.uint8), (tab_scene.tolist(), torch.int64),
                 (tab_local.tolist(), torch.int64), (drop.tolist(), torch.uint8)]
        if boxed:
            # the boxes ride in the same upload: (first row, count) per scene, batch offsets, (flip_h, flip_v, angle, scale) in float64
            # and the constant that turns gravity centres into DepthInstance3DBoxes' bottom centres
            n_box = [cache.box_offsets[s + 1] - cache.box_offsets[s] for s in scene_ids]
            b_off = np.concatenate(([0], np.cumsum(n_box))).astype(np.int64)
            b_src = np.stack([[cache.box_offsets[s] for s in scene_ids], n_box], axis=1).astype(np.int64)
            scal = np.stack([np.asarray(draws.flip_h, dtype=np.float64), np.asarray(draws.flip_v, dtype=np.float64),
                             np.asarray(draws.angle, dtype=np.float64), np.asarray(draws.scale, dtype=np.float64)], axis=1)
            specs += [(b_src.tolist(), torch.int64), (b_off.tolist(), torch.int64), (scal.tolist(), torch.float64),
                      ([int(cache.scene_with_yaw[s]) for s in scene_ids], torch.uint8), ([0.0, 0.0, -0.5], torch.float32)]
        packed = L.h2d_pack(specs, dev)
        d_off, d_src, d_aff, d_tinst, d_tsp, d_gate, d_tscene, d_tlocal, d_drop = packed[:9]
        gather = None
        if sampled and N:
            if draws.indices is not None:
                idx = [np.asarray(torch.as_tensor(i).cpu() if torch.is_tensor(i) else i, dtype=np.int64) for i in draws.indices]
                assert [len(i) for i in idx] == m, 'draws.indices: min(num_points, scene size) indices per scene expected'
                assert all(not len(i) or (i.min() >= 0 and i.max() < n) for i, n in zip(idx, n_src)), 'draws.indices out of range'
                gather = torch.from_numpy(np.concatenate(idx)).to(dev)
            else:
                gather = torch.randint(0, 2 ** 62, (N,), generator=dgen, device=dev, dtype=torch.int64)    # reduced mod scene size by the kernels
        rows = cache.points.shape[0]
        f3 = C.c_float * 3
        mean = None if self.color_mean is None else f3(*self.color_mean.tolist())
        std = None if self.color_std is None else f3(*self.color_std.tolist())
        pts = torch.empty((N, 6), dtype=torch.float32, device=dev)
        coords = torch.empty((N, 3), dtype=torch.float32, device=dev) if self.elastic is not None else None
        if self.denorm_mean is None and self.denorm_std is None:
            L.call('u3d_aug_points', L.ptr(cache.points), rows, L.ptr(gather), L.ptr(d_src), L.ptr(d_off), B, N, L.ptr(d_aff), mean, std,
                   self.voxel_size, L.ptr(pts), L.ptr(coords), st)
        else:
            dmean = None if self.denorm_mean is None else f3(*self.denorm_mean.tolist())
            dstd = None if self.denorm_std is None else f3(*self.denorm_std.tolist())
            L.call('u3d_aug_points_dn', L.ptr(cache.points), rows, L.ptr(gather), L.ptr(d_src), L.ptr(d_off), B, N, L.ptr(d_aff), mean, std,
                   dmean, dstd, self.voxel_size, L.ptr(pts), L.ptr(coords), st)
        self.last_launches += 1 if N else 0
        box_objs = box_labels = None
        if boxed:
            d_bsrc, d_boff, d_scal, d_wyaw, d_shift = packed[9:]
            G = int(b_off[-1])
            bx = torch.empty((G, 7), dtype=torch.float32, device=dev)
            L.call('u3d_aug_boxes', L.ptr(cache.boxes), cache.boxes.shape[0], L.ptr(d_bsrc), L.ptr(d_boff), B, G, L.ptr(d_aff), L.ptr(d_scal),
                   L.ptr(d_wyaw), L.ptr(bx), st)
            self.last_launches += 1 if G else 0
            # DepthInstance3DBoxes(gravity rows, origin=(0.5, 0.5, 0.5)) for the whole batch: its constructor's arithmetic with the
            # constant from the upload (the constructor itself would copy two host tuples per scene and wait for each)
            bx[:, :3] += bx[:, 3:6] * d_shift
            box_objs, box_labels = [], []
            for b, s in enumerate(scene_ids):
                lo, hi = int(b_off[b]), int(b_off[b + 1])
                o = DepthInstance3DBoxes.__new__(DepthInstance3DBoxes)
                o.with_yaw = bool(cache.scene_with_yaw[s])
                o.box_dim = 7 if o.with_yaw else 6
                o.tensor = bx[lo:hi] if o.with_yaw else bx[lo:hi, :6]
                o.gt_rows = None
                box_objs.append(o)
                box_labels.append(cache.box_labels[cache.box_offsets[s]:cache.box_offsets[s + 1]])
        read = []
        ext1 = None
        if gate.any():
            ext1 = torch.empty((B, 3), dtype=torch.float32, device=dev)
            L.call('u3d_aug_extent_f32', L.ptr(coords), L.ptr(d_off), B, max(m), L.ptr(ext1), st)
            self.last_launches += 2
            read.append(ext1.view(torch.int32).reshape(-1))
        inst = sem = first = cnt_inst = sp = cnt_sp = None
        if need_inst:
            T = int(t_inst[-1])
            inst = torch.empty(N, dtype=torch.int64, device=dev)
            sem = torch.empty(N, dtype=torch.int64, device=dev)
            cnt_inst = torch.empty(B, dtype=torch.int32, device=dev)
            first = torch.empty(T, dtype=torch.int64, device=dev) if self.mapping is not None else None
            ws = L.ws(L.lib().u3d_relabel_ids_ws_bytes(T), dev)
            use_drop = self.mapping is not None and self.mapping[0] == 'scannet'
            L.call('u3d_relabel_ids', L.ptr(cache.pts_instance_mask), rows, L.ptr(gather), L.ptr(d_src), L.ptr(d_off), B, N, L.ptr(d_tinst), T, 1,
                   L.ptr(cache.pts_semantic_mask), L.ptr(d_drop) if use_drop else None, len(drop) if use_drop else 0, L.ptr(inst), L.ptr(sem),
                   L.ptr(cnt_inst), L.ptr(first), L.ptr(ws), st)
            self.last_launches += 5
        if sampled:
            T = int(t_sp[-1])
            sp = torch.empty(N, dtype=torch.int64, device=dev)
            cnt_sp = torch.empty(B, dtype=torch.int32, device=dev)
            ws = L.ws(L.lib().u3d_relabel_ids_ws_bytes(T), dev)
            L.call('u3d_relabel_ids', L.ptr(cache.sp_pts_mask), rows, L.ptr(gather), L.ptr(d_src), L.ptr(d_off), B, N, L.ptr(d_tsp), T, 0,
                   None, None, 0, L.ptr(sp), None, L.ptr(cnt_sp), None, L.ptr(ws), st)
            self.last_launches += 5
            read.append(cnt_sp)
        labels_pad = keep = cs = None
        if self.mapping is not None and self.mapping[0] == 'scannet':
            labels_pad = sem[first] - len(self.mapping[2]) if N else torch.zeros_like(first)     # label of each instance's first point
            read.append(cnt_inst)
        elif self.mapping is not None:
            # [n_inst]-sized arrays (padded to the table size, `valid` marks the real entries): label filter, remap table, class index
            classes = self.mapping[1]
            lut = torch.zeros(max(classes) + 1, dtype=torch.int64)
            lut[torch.as_tensor(classes)] = torch.arange(len(classes))
            d_classes, d_lut = L.h2d_pack([(list(classes), torch.int64), (lut.tolist(), torch.int64)], dev)
            lab = sem[first] if N else torch.zeros_like(first)
            valid = d_tlocal < cnt_inst.long()[d_tscene]
            keep = valid & torch.isin(lab, d_classes)
            cs = torch.cumsum(keep.long(), 0)
            csx = torch.cat((cs.new_zeros(1), cs))
            start = csx[d_tinst[:-1]]
            remap = torch.where(keep, cs - 1 - start[d_tscene], cs.new_full((), -1))
            labels_pad = d_lut[lab.clamp(0, len(lut) - 1)]
            L.call('u3d_aug_remap_ids', L.ptr(inst), L.ptr(d_off), B, N, L.ptr(remap), L.ptr(d_tinst), st)
            self.last_launches += 1 if N else 0
            read.append((csx[d_tinst[1:]] - start).int())
        host = None
        if read:
            host = torch.cat(read).cpu().numpy()          # the one read of the counts (and of the pass-1 extents)
            self.last_host_reads += 1
        pos = 0
        ext_host = None
        if ext1 is not None:
            ext_host = host[:3 * B].view(np.float32).reshape(B, 3)
            pos = 3 * B
        S = [cache.max_sp[s] + 1 for s in scene_ids]
        if sampled:
            S = host[pos:pos + B].tolist()
            pos += B
        n_inst = host[pos:pos + B].tolist() if self.mapping is not None else [0] * B
        masks = labels = None
        if self.mapping is not None:
            sp_off = np.concatenate(([0], np.cumsum(S))).astype(np.int64)
            mask_off = np.concatenate(([0], np.cumsum(np.asarray(n_inst, dtype=np.int64) * np.asarray(S, dtype=np.int64)))).astype(np.int64)
            i_off = np.concatenate(([0], np.cumsum(n_inst))).astype(np.int64)
            total = int(mask_off[-1])
            masks = torch.empty(total, dtype=torch.bool, device=dev)
            if total:
                d_ninst, d_spoff, d_moff = L.h2d_pack([(n_inst, torch.int32), (sp_off.tolist(), torch.int64), (mask_off.tolist(), torch.int64)], dev)
                ws = L.ws(L.lib().u3d_aug_sp_masks_ws_bytes(total, int(sp_off[-1])), dev)
                L.call('u3d_aug_sp_masks', L.ptr(inst), L.ptr(sp if sampled else cache.sp_pts_mask), None if sampled else L.ptr(d_src), rows,
                       L.ptr(d_off), B, N, L.ptr(d_ninst), L.ptr(d_spoff), L.ptr(d_moff), total, int(sp_off[-1]), L.ptr(masks), L.ptr(ws), st)
                self.last_launches += 3
            if self.mapping[0] == 'scannet':
                labels = [labels_pad[int(t_inst[b]):int(t_inst[b]) + n_inst[b]] for b in range(B)]
            else:
                comp = labels_pad.new_empty(int(i_off[-1]) + 1)
                comp.scatter_(0, torch.where(keep, cs - 1, cs.new_full((), int(i_off[-1]))), labels_pad)
                labels = [comp[int(i_off[b]):int(i_off[b + 1])] for b in range(B)]
        elastic = None
        if self.elastic is not None:
            elastic = self._elastic(coords, d_off, d_gate, gate, m, ext_host, draws, dgen, dev, st) if gate.any() else coords
        inputs = dict(points=[pts[off[b]:off[b + 1]] for b in range(B)])
        if elastic is not None:
            inputs['elastic_coords'] = [elastic[off[b]:off[b + 1]] for b in range(B)]
        samples = []
        for b, s in enumerate(scene_ids):
            lo, hi = int(off[b]), int(off[b + 1])
            c0 = cache.offsets[s]
            if boxed:
                seg = PointSegData(sp_pts_mask=sp[lo:hi] if sampled else cache.sp_pts_mask[c0:c0 + n_src[b]])
            else:
                seg = PointSegData(pts_instance_mask=inst[lo:hi] if need_inst else cache.pts_instance_mask[c0:c0 + n_src[b]],
                                   sp_pts_mask=sp[lo:hi] if sampled else cache.sp_pts_mask[c0:c0 + n_src[b]],
                                   pts_semantic_mask=sem[lo:hi] if need_inst else cache.pts_semantic_mask[c0:c0 + n_src[b]])
            gi = InstanceData_(labels_3d=box_labels[b], bboxes_3d=box_objs[b]) if boxed else InstanceData_()
            if self.mapping is not None:
                gi = InstanceData_(labels_3d=labels[b], sp_masks=masks[int(mask_off[b]):int(mask_off[b + 1])].view(n_inst[b], int(S[b])))
            ds = Det3DDataSample(cache.lidar_paths[s], seg, gi)
            ds.n_superpoints = int(S[b])
            samples.append(ds)
        if dev.type == 'cuda':
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            inputs['ready_event'] = ev
        return inputs, samples

    def _elastic(self, coords, d_off, d_gate, gate, m, ext_host, draws, dgen, dev, st):
        """The two elastic passes of the gated scenes: noise-grid dimensions on the host as numpy computes them
        (``int32(extent) // gran + 3``), noise, six blur sweeps, float64 lookup.  Pass 1: float32 -> float64, pass 2: float64 -> float32."""
        B, N = len(m), coords.shape[0]
        x = coords
        for p in (0, 1):
            gran, mag = self.elastic['gran'][p], self.elastic['mag'][p]
            if p == 1:
                ext = torch.empty((B, 3), dtype=torch.float64, device=dev)
                L.call('u3d_aug_extent_f64', L.ptr(x), L.ptr(d_off), B, max(m), L.ptr(ext), st)
                self.last_launches += 2
                ext_host = ext.cpu().numpy()
                self.last_host_reads += 1
            dims = np.zeros((B, 3), dtype=np.int64)
            for b in range(B):
                if gate[b]:
                    dims[b] = np.asarray(np.abs(ext_host[b]).astype(np.int32) // gran + 3, dtype=np.int64)
            cells = dims.prod(1)
            goff = np.concatenate(([0], np.cumsum(cells))).astype(np.int64)
            total = int(goff[-1])
            if draws.noise is not None:
                parts = []
                for b in range(B):
                    if gate[b]:
                        g = np.asarray(draws.noise(b, p, tuple(int(d) for d in dims[b])), dtype=np.float32)
                        assert g.shape == (3,) + tuple(dims[b]), 'noise: [3, d0, d1, d2] expected'
                        parts.append(g.reshape(-1))
                noise = torch.from_numpy(np.concatenate(parts)).to(dev)
            else:
                noise = torch.randn(3 * total, generator=dgen, device=dev, dtype=torch.float32)
            grids, d_dims, d_goff = blur_noise_grids(noise, dims, dev)
            out = torch.empty((N, 3), dtype=torch.float64 if p == 0 else torch.float32, device=dev)
            L.call('u3d_aug_elastic', L.ptr(x), p, L.ptr(out), 1 - p, L.ptr(d_off), B, N, L.ptr(grids), L.ptr(d_goff), L.ptr(d_dims),
                   L.ptr(d_gate), float(gran), float(mag), st)
            self.last_launches += 7
            x = out
        return x


class MixedDeviceAugment:
    """A batch drawn from several datasets (the joint config's ``ConcatDataset``): ``pipelines`` maps a dataset name to its
    ``(DeviceAugment, DeviceSceneCache)``.  The pipelines differ in sampling size, ranges, colour steps and elastic ``p``, so a call
    runs one ``DeviceAugment`` call per dataset PRESENT in the batch (not per scene) and returns the scenes in the requested order."""

    def __init__(self, pipelines: dict):
        self.pipelines = dict(pipelines)
        for name, (aug, cache) in self.pipelines.items():
            if aug.kind is not None and aug.kind != cache.kind:
                raise ValueError(f'{name}: a {aug.kind}-annotated pipeline with a {cache.kind}-annotated scene cache')
        self.last_launches = 0          # sums over the groups of the last call
        self.last_host_reads = 0

    def __call__(self, scenes, generator=None, draws: Optional[dict] = None):
        """``scenes``: [(dataset name, scene id), ...].  ``draws`` (optional, for tests): {dataset name: AugmentDraws} for that
        dataset's scenes in their order of appearance.  One ``ready_event`` is recorded after the last group."""
        if not len(scenes):
            raise ValueError('MixedDeviceAugment: empty batch')
        groups = {}
        for pos, (name, sid) in enumerate(scenes):
            if name not in self.pipelines:
                raise KeyError(f'MixedDeviceAugment: no pipeline for dataset {name!r}')
            groups.setdefault(name, []).append((pos, sid))
        self.last_launches = self.last_host_reads = 0
        points, elastic, samples = [None] * len(scenes), [None] * len(scenes), [None] * len(scenes)
        dev = None
        for name, members in groups.items():
            aug, cache = self.pipelines[name]
            dev = cache.device
            inputs, smp = aug(cache, [sid for _, sid in members], None if draws is None else draws.get(name), generator=generator)
            self.last_launches += aug.last_launches
            self.last_host_reads += aug.last_host_reads
            for k, (pos, _) in enumerate(members):
                points[pos], samples[pos] = inputs['points'][k], smp[k]
                elastic[pos] = inputs['elastic_coords'][k] if 'elastic_coords' in inputs else None
        out = dict(points=points)
        if all(e is not None for e in elastic):
            out['elastic_coords'] = elastic
        elif any(e is not None for e in elastic):
            raise ValueError('MixedDeviceAugment: some pipelines of the batch hold ElasticTransfrom and some do not')
        if dev.type == 'cuda':
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            out['ready_event'] = ev
        return out, samples
