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

Random draws are separated from arithmetic (``AugmentDraws``): a test injects every draw, a training loop lets
``DeviceAugment.draw`` take the scalars from a host generator and the per-point / per-cell draws (sample indices, noise) from torch
on the device.  The same generator state gives the same bits twice.

Affine convention.  Horizontal flip negates x, vertical flip negates y: mmdet3d's rule for the depth frame as its documentation
states it.  mmdet3d is not a dependency of this package, so the rule is not checked against its code here.  Then a rotation about z by theta, x' = x cos(theta) - y sin(theta), y' = x sin(theta) + y cos(theta); then the scale s;
then the translation t ~ N(0, std).  The host composes the matrix in float64 and rounds it to float32; the kernel evaluates
x' = ((a00 x + a01 y) + a02 z) + t0 in float32.  The reference's angle ranges are symmetric ([-3.14, 3.14], [0, 0]), so the sign
convention of the rotation does not change the distribution of the augmented scenes.
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
from .structures import InstanceData_, PointSegData

__all__ = ['DeviceSceneCache', 'DeviceAugment', 'AugmentDraws', 'compose_affine', 'blur_noise_grids']

_LOADERS = ('LoadPointsFromFile', 'LoadAnnotations3D_', 'LoadAnnotations3D')
_PACKERS = ('Pack3DDetInputs_', 'Pack3DDetInputs')
_LOAD_TIME = ('GlobalAlignment', 'PointSegClassMapping')
_BOX_KEYS = ('gt_bboxes_3d', 'gt_bboxes', 'ann_info')


class DeviceSceneCache:
    """Pre-processed scenes (the output of ``transforms.load_scene_bins``) concatenated on the device: ``points`` float32 [N, 6],
    ``sp_pts_mask`` / ``pts_instance_mask`` / ``pts_semantic_mask`` int64 [N], host-side point offsets, ``lidar_path`` s and the
    per-scene maximum ids (read once here, on the host; they size the relabel tables)."""

    def __init__(self, points, sp, inst, sem, offsets, lidar_paths, max_inst, max_sp, align):
        self.points, self.sp_pts_mask, self.pts_instance_mask, self.pts_semantic_mask = points, sp, inst, sem
        self.offsets, self.lidar_paths, self.max_inst, self.max_sp, self.align = offsets, lidar_paths, max_inst, max_sp, align
        self.has_alignment = self.has_seg_mapping = False      # set by from_scene_dicts: what the load-time steps were given

    @property
    def device(self):
        return self.points.device

    def __len__(self):
        return len(self.lidar_paths)

    @classmethod
    def from_scene_dicts(cls, dicts: Sequence[dict], device, seg_label_mapping=None) -> 'DeviceSceneCache':
        """``seg_label_mapping`` (optional int array): mmdet3d's ``PointSegClassMapping`` table, applied to the semantic ids here,
        once.  A scene dict may carry ``axis_align_matrix`` [4, 4] (``GlobalAlignment``); it is composed into every affine."""
        pts, sp, inst, sem, offs, paths, mi, ms, al = [], [], [], [], [0], [], [], [], []
        for i, d in enumerate(dicts):
            if any(k in d for k in _BOX_KEYS):
                raise NotImplementedError(f'scene {i}: box annotations are not transformed on the device (box-annotated datasets are out of scope)')
            p = np.ascontiguousarray(np.asarray(d['points'], dtype=np.float32))
            assert p.ndim == 2 and p.shape[1] == 6, 'points: float32 [N, 6] (xyz, rgb 0..255) expected'
            ids = []
            for key in ('sp_pts_mask', 'pts_instance_mask', 'pts_semantic_mask'):
                a = np.asarray(d[key]).astype(np.int64)
                assert a.shape == (len(p),), f'{key}: one id per point expected'
                assert not len(a) or a.min() >= -1, f'{key}: ids below -1'
                ids.append(a)
            if seg_label_mapping is not None:
                ids[2] = np.asarray(seg_label_mapping, dtype=np.int64)[ids[2]]
            assert not len(p) or ids[0].min() >= 0, 'sp_pts_mask: superpoint ids must be non-negative'
            pts.append(p); sp.append(ids[0]); inst.append(ids[1]); sem.append(ids[2])
            offs.append(offs[-1] + len(p))
            paths.append(str(d.get('lidar_path', 'data/scannet/points/scene.bin')))
            mi.append(int(ids[1].max()) if len(p) else -1)
            ms.append(int(ids[0].max()) if len(p) else -1)
            al.append(np.asarray(d.get('axis_align_matrix', np.eye(4)), dtype=np.float64).reshape(4, 4))
        dev = torch.device(device)

        def up(parts, dtype, tail):
            a = np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)
            return torch.from_numpy(a).to(dev)
        cache = cls(up(pts, np.float32, (6,)), up(sp, np.int64, ()), up(inst, np.int64, ()), up(sem, np.int64, ()), offs, paths, mi, ms, al)
        cache.has_alignment = any('axis_align_matrix' in d for d in dicts)
        cache.has_seg_mapping = seg_label_mapping is not None
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
    ``PointDetClassMappingScanNet``, ``PointDetClassMappingS3DIS``, ``ElasticTransfrom``.  Geometry, colour and label steps act on
    disjoint columns, so their relative order is free; ``PointSample_`` must precede the class mapping and ``ElasticTransfrom``
    must follow the geometric steps, as in the reference's lists."""

    def __init__(self, voxel_size, num_points=None, flip_ratio_h=0.0, flip_ratio_v=0.0, rot_range=(0.0, 0.0), scale_range=(1.0, 1.0),
                 translation_std=(0.0, 0.0, 0.0), color_mean=None, color_std=None, mapping=None, elastic=None):
        self.voxel_size = float(voxel_size)
        self.num_points = None if num_points is None else int(num_points)
        self.flip_ratio_h, self.flip_ratio_v = float(flip_ratio_h), float(flip_ratio_v)
        self.rot_range = tuple(float(r) for r in (rot_range if isinstance(rot_range, (list, tuple)) else (-rot_range, rot_range)))
        self.scale_range = tuple(float(s) for s in scale_range)
        self.translation_std = tuple(float(t) for t in (translation_std if isinstance(translation_std, (list, tuple))
                                                        else (translation_std,) * 3))
        self.color_mean = None if color_mean is None else np.broadcast_to(np.asarray(color_mean, dtype=np.float32), (3,)).copy()
        self.color_std = None if color_std is None else np.broadcast_to(np.asarray(color_std, dtype=np.float32), (3,)).copy()
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
        aug = cls(voxel_size, **kw)
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
        ``transforms.to_batch_inputs``; the per-scene tensors are views of batch buffers."""
        from .structures import Det3DDataSample
        dev = cache.device
        B = len(scene_ids)
        if B == 0:
            raise ValueError('DeviceAugment: empty batch')
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
        need_inst = sampled or self.mapping is not None
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
        d_off, d_src, d_aff, d_tinst, d_tsp, d_gate, d_tscene, d_tlocal, d_drop = L.h2d_pack(
            [(off.tolist(), torch.int64), (src.tolist(), torch.int64), (affine.tolist(), torch.float32), (t_inst.tolist(), torch.int64),
             (t_sp.tolist(), torch.int64), (gate.astype(np.uint8).tolist(), torch.uint8), (tab_scene.tolist(), torch.int64),
             (tab_local.tolist(), torch.int64), (drop.tolist(), torch.uint8)], dev)
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
        L.call('u3d_aug_points', L.ptr(cache.points), rows, L.ptr(gather), L.ptr(d_src), L.ptr(d_off), B, N, L.ptr(d_aff), mean, std,
               self.voxel_size, L.ptr(pts), L.ptr(coords), st)
        self.last_launches += 1 if N else 0
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
            seg = PointSegData(pts_instance_mask=inst[lo:hi] if need_inst else cache.pts_instance_mask[c0:c0 + n_src[b]],
                               sp_pts_mask=sp[lo:hi] if sampled else cache.sp_pts_mask[c0:c0 + n_src[b]],
                               pts_semantic_mask=sem[lo:hi] if need_inst else cache.pts_semantic_mask[c0:c0 + n_src[b]])
            gi = InstanceData_()
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
