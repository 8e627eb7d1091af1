"""Rate of the training-input pipeline: host (unidet3d_amd/transforms.py, one process) against device (unidet3d_amd/augment.py).

    python tools/augment_time.py [--batch 8] [--points 100000] [--reps 20] [--steps 6] [--no-train]
    python tools/augment_time.py --joint [--points 100000] [--reps 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/augment_time.py --trace-calls N

For B synthetic ScanNet-shape scenes it prints one JSON line with
  host_ms_per_scene      flip / rotation / scale / translation, NormalizePointsColor_, PointDetClassMappingScanNet, ElasticTransfrom
                         (gate on) and to_batch_inputs onto CPU tensors (no upload, no device wait), numpy in one process, mean over
                         the batch of the second of two runs;
  device_ms_per_batch    DeviceAugment on the batch, every scene taking both elastic passes (the most a batch can cost), HIP events
                         around the call, median of --reps repetitions after warm-up; device_ms_gate_off: no scene takes them;
  launches, host_reads   launches the library issues (kernels + memsets; the torch ops of the path -- random draws, a few ops on
                         [n_inst]-sized tables -- come on top, a kernel trace of this tool counts them) and device-to-host reads;
  step_ms_fixed_batch / step_ms_device_producer
                         train_step + prefetch_step on one resident batch, and with DeviceAugment (p = 0.5, on its own stream)
                         producing a fresh batch for every prefetch_step.
--joint times a MIXED batch of the joint config instead: eight scenes (ScanNet with instance masks; ARKitScenes, MultiScan, 3RScan and
ScanNet++ with boxes) through MixedDeviceAugment, one DeviceAugment call per dataset present: joint_device_ms_per_batch, launches and
host reads summed over the five calls, and prepare_train_ms, the joint model's batch-only preparation (voxelisation, boxes, distance
targets, rulebooks) of that batch, host wall time with a device wait, median.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIPELINE = [
    dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
    dict(type='GlobalRotScaleTrans', rot_range=[-3.14, 3.14], scale_ratio_range=[0.8, 1.2], translation_std=[0.1, 0.1, 0.1], shift_height=False),
    dict(type='NormalizePointsColor_', color_mean=[127.5, 127.5, 127.5]),
    dict(type='PointDetClassMappingScanNet', num_classes=20, stuff_classes=[0, 1]),
    dict(type='ElasticTransfrom', gran=[6, 20], mag=[40, 160], voxel_size=0.02, p=0.5),
]


def raw_scene(idx, n):
    """A synthetic scene in the on-disk form: rgb 0..255, semantic ids 0 / 1 = stuff, 2.. = things."""
    from unidet3d_amd.synthetic import make_scene
    sc = make_scene(idx, n_points=n)
    sem = np.where(sc.instance_mask >= 0, sc.labels[np.maximum(sc.instance_mask, 0)] + 2, np.arange(n) % 2).astype(np.int64)
    pts = sc.points.copy()
    pts[:, 3:] = np.round((pts[:, 3:] + 1) * 127.5)
    return dict(points=pts.astype(np.float32), sp_pts_mask=sc.superpoints.astype(np.int64), pts_instance_mask=sc.instance_mask.astype(np.int64),
                pts_semantic_mask=sem, lidar_path=f'data/scannet/points/syn{idx}.bin')


JOINT_ORDER = ['scannet', 'arkitscenes', 'multiscan', '3rscan', 'scannetpp', 'scannet', 'arkitscenes', 'multiscan']


def box_pipeline(num_points, arkit=False):
    """the reference's train list of a box-annotated dataset (joint config :291-329, :512-553) after the loaders"""
    colour = [dict(type='NormalizePointsColor_', color_mean=[127.5, 127.5, 127.5])]
    if arkit:
        colour.insert(0, dict(type='DenormalizePointsColor', color_mean=[0, 0, 0], color_std=[255, 255, 255]))
    return [dict(type='PointSample_', num_points=num_points)] + colour + [
        dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
        dict(type='GlobalRotScaleTrans', rot_range=[-0.5, 0.5] if arkit else [0, 0], scale_ratio_range=[0.9, 1.1], translation_std=[0.1, 0.1, 0.1],
             shift_height=False),
        dict(type='ElasticTransfrom', gran=[6, 20], mag=[40, 160], voxel_size=0.02, p=-1)]


def raw_box_scene(idx, n, name, n_classes):
    """A synthetic box-annotated scene in the on-disk form: boxes (gravity centre, size[, yaw]) and labels, no per-point masks;
    ARKitScenes stores colours in 0..1 and boxes with a heading."""
    from unidet3d_amd.data import scene_boxes
    from unidet3d_amd.synthetic import make_scene
    sc = make_scene(idx, n_points=n, n_classes=n_classes, dataset=name)
    b, keep = scene_boxes(sc)
    if name == 'arkitscenes':
        b = np.concatenate((b, np.random.RandomState(idx).uniform(-0.6, 0.6, (len(b), 1)).astype(np.float32)), 1)
    pts = sc.points.copy()
    pts[:, 3:] = (pts[:, 3:] + 1) / 2 if name == 'arkitscenes' else np.round((pts[:, 3:] + 1) * 127.5)
    return dict(points=pts.astype(np.float32), sp_pts_mask=sc.superpoints.astype(np.int64), gt_bboxes_3d=b, gt_labels_3d=sc.labels[keep],
                lidar_path=f'data/{name}/points/syn{idx}.bin')


def joint(args, dev):
    from unidet3d_amd import DeviceAugment, DeviceSceneCache, MixedDeviceAugment
    from unidet3d_amd.config import build_model, joint_model_cfg
    cfg = joint_model_cfg()
    dec = cfg['decoder']
    per, order = {}, []
    for i, name in enumerate(JOINT_ORDER):
        n_cls = len(dec['datasets_classes'][dec['datasets'].index(name)])
        per.setdefault(name, []).append(raw_scene(500 + i, args.points) if name == 'scannet' else raw_box_scene(500 + i, args.points, name, n_cls))
        order.append((name, len(per[name]) - 1))
    pipes = {}
    for name, dicts in per.items():
        pl = PIPELINE if name == 'scannet' else box_pipeline(200_000 if name == 'scannetpp' else 100_000, name == 'arkitscenes')
        pipes[name] = (DeviceAugment.from_pipeline(pl, 0.02), DeviceSceneCache.from_scene_dicts(dicts, dev))
    mixer = MixedDeviceAugment(pipes)
    g = torch.Generator(dev)
    g.manual_seed(1)
    res = dict(joint=True, scenes=len(order), points=args.points, datasets=len(per))
    times = []
    for r in range(3 + max(args.reps, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        inputs, samples = mixer(order, generator=g)
        e1.record()
        e1.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1))
    res.update(joint_device_ms_per_batch=round(statistics.median(times), 3), launches=mixer.last_launches, host_reads=mixer.last_host_reads)
    if not args.no_train:
        model = build_model(cfg).to(dev).train()
        times = []
        for r in range(3 + max(args.reps, 20)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            model._prepare_train(inputs, samples)
            torch.cuda.synchronize()
            if r >= 3:
                times.append((time.perf_counter() - t) * 1e3)
        res['prepare_train_ms'] = round(statistics.median(times), 3)
    print(json.dumps(res))


def host_pipeline(dicts, aug, dev):
    from unidet3d_amd import transforms as X
    from unidet3d_amd.augment import compose_affine
    d = aug.draw(len(dicts), torch.Generator().manual_seed(0))
    A = compose_affine(d.flip_h, d.flip_v, d.angle, d.scale, d.trans)
    out = []
    for b, sc in enumerate(dicts):
        sc = dict(sc)
        x, y, z = sc['points'][:, 0], sc['points'][:, 1], sc['points'][:, 2]
        xyz = np.stack([((A[b, r, 0] * x + A[b, r, 1] * y) + A[b, r, 2] * z) + A[b, r, 3] for r in range(3)], 1)
        sc['points'] = np.concatenate([xyz, sc['points'][:, 3:]], 1)
        for t in (X.NormalizePointsColor_([127.5] * 3), X.PointDetClassMappingScanNet(20, [0, 1]), X.ElasticTransfrom([6, 20], [40, 160], 0.02, 1.0)):
            sc = t(sc)
        out.append(sc)
    return X.to_batch_inputs(out, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--points', type=int, default=100_000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--no-train', action='store_true')
    ap.add_argument('--trace-calls', type=int, default=0, help='run only this many device calls (every scene elastic) and exit: for `rocprofv3 --kernel-trace --stats`')
    ap.add_argument('--joint', action='store_true', help='time a mixed batch of the joint config through MixedDeviceAugment instead')
    args = ap.parse_args()
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd import DeviceAugment, DeviceSceneCache
    dev = torch.device('cuda:0')
    if args.joint:
        joint(args, dev)
        return
    dicts = [raw_scene(i, args.points) for i in range(args.batch)]
    ids = list(range(args.batch))
    aug = DeviceAugment.from_pipeline(PIPELINE, 0.02)
    res = dict(batch=args.batch, points=args.points)

    if args.trace_calls:                                 # nothing but N gate-on calls: two kernel traces with different N give the launches of one call
        cache = DeviceSceneCache.from_scene_dicts(dicts, dev)
        g = torch.Generator(dev)
        g.manual_seed(1)
        aug.elastic['p'] = 1.0
        for _ in range(args.trace_calls):
            aug(cache, ids, generator=g)
        torch.cuda.synchronize()
        print(json.dumps(dict(res, trace_calls=args.trace_calls, launches=aug.last_launches)))
        return

    for _ in range(2):                                  # the first run warms numpy's allocator and the page cache
        t0 = time.perf_counter()
        host_pipeline(dicts, aug, 'cpu')
        res['host_ms_per_scene'] = round((time.perf_counter() - t0) * 1e3 / args.batch, 2)

    cache = DeviceSceneCache.from_scene_dicts(dicts, dev)
    g = torch.Generator(dev)
    g.manual_seed(1)
    for key, p in (('device_ms_per_batch', 1.0), ('device_ms_gate_off', 0.0)):
        aug.elastic['p'] = p
        times = []
        for r in range(3 + max(args.reps, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            aug(cache, ids, generator=g)
            e1.record()
            e1.synchronize()
            if r >= 3:
                times.append(e0.elapsed_time(e1))
        res[key] = round(statistics.median(times), 3)
        res[key.replace('ms', 'launches')] = aug.last_launches
        res[key.replace('ms', 'host_reads')] = aug.last_host_reads
    aug.elastic['p'] = 0.5

    if not args.no_train:
        from unidet3d_amd.config import build_model, scannet_model_cfg
        model = build_model(scannet_model_cfg(voxel_size=0.02)).to(dev).train()

        class OptimWrapper:
            def __init__(self, params):
                self.opt = torch.optim.AdamW(params, lr=2e-4, weight_decay=0.05, fused=True)

            def update_params(self, loss):
                loss.backward(); self.opt.step(); self.opt.zero_grad(set_to_none=True)
        ow = OptimWrapper([p for p in model.parameters() if p.requires_grad])
        producer = torch.cuda.Stream(dev)

        def produce():
            with torch.cuda.stream(producer):           # its host reads wait for this stream only, not for the step in flight
                return dict(zip(('inputs', 'data_samples'), aug(cache, ids, generator=g)))

        def loop(fresh):
            batch = produce()
            producer.synchronize()
            model.prefetch_step(batch)
            times, losses = [], []
            for it in range(3 + args.steps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                log = model.train_step(batch, ow)
                if fresh:
                    batch = produce()
                model.prefetch_step(batch)
                torch.cuda.synchronize()
                if it >= 3:
                    times.append((time.perf_counter() - t) * 1e3)
                losses.append(round(float(log['loss'].detach()), 4))
            return round(statistics.median(times), 2), losses
        res['step_ms_fixed_batch'], res['losses_fixed_batch'] = loop(False)
        res['step_ms_device_producer'], res['losses_device_producer'] = loop(True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
