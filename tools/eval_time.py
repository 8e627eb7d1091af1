"""Time the evaluation of one ScanNet-shaped validation pass: host ``indoor_eval`` against ``indoor_eval_device`` in the same process.

The pass is synthetic: 312 images, 18 classes, axis-aligned boxes.  The number of detections per image is what ``predict`` returns
under the reference's test settings (topk_insts = 1000, score_thr = 0) on ``synthetic.make_scene`` scenes -- measured here by a
``predict`` run, not assumed; the ground truths per image are those scenes' mean count.  Detections are noisy copies of the image's
ground truths (so every IoU range and both outcomes of the greedy match occur) with uniform random scores.

  host    ``indoor_eval`` on host tensors (what ``IndoorMetric`` hands it after its per-scene ``.cpu()``), wall clock
  device  ``indoor_eval_device`` on device detections and host annotations: packing, upload, launch chain and the one read, wall clock
  kernels HIP events around the three entry points on the packed arrays

Median of ``--reps`` (5) after one warm-up, min and max alongside.  Host reads are counted by wrapping the tensor methods that read.

    python tools/eval_time.py [--images 312] [--reps 5] [--out profiles/eval_time.txt]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))


def detections_per_image(dev):
    """(detections, ground truths) per image: a ``predict`` run of an untrained model on three synthetic scenes, reference test settings"""
    import _parity as PA
    from unidet3d_amd.config import build_model, scannet_model_cfg
    from unidet3d_amd.data import make_batch_inputs
    from unidet3d_amd.synthetic import make_scene
    torch.manual_seed(0)
    cfg = scannet_model_cfg(voxel_size=0.05)
    cfg['decoder']['num_layers'] = 3
    model = build_model(cfg).to(dev).eval()
    assert model.test_cfg['topk_insts'] == 1000 and model.test_cfg['score_thr'] == 0
    scenes = [make_scene(300 + i, n_points=12_000) for i in range(3)]
    inputs, samples = make_batch_inputs(scenes, dev)
    with torch.no_grad():
        res = model.predict(inputs, samples)
    n_det = [len(r.pred_instances_3d.scores_3d) for r in res]
    n_gt = [len(PA.scene_boxes(sc)[0]) for sc in scenes]
    return n_det, n_gt


def make_pass(n_img, n_det, n_gt, n_cls, seed=0):
    rng = np.random.RandomState(seed)
    gt, dt = [], []
    for _ in range(n_img):
        c = rng.uniform([0, 0, 0], [8, 8, 2], (n_gt, 3))
        s = rng.uniform(0.3, 1.5, (n_gt, 3))
        gb = np.concatenate((c, s), 1).astype(np.float32)
        gl = rng.randint(n_cls, size=n_gt)
        src = rng.randint(n_gt, size=n_det)
        noise = rng.standard_normal((n_det, 6)) * np.array([0.15, 0.15, 0.1, 0.1, 0.1, 0.1])
        db = (gb[src] + noise * rng.uniform(0, 2, (n_det, 1))).astype(np.float32)
        db[:, 3:] = np.abs(db[:, 3:]) + 0.05
        dl = np.where(rng.uniform(size=n_det) < 0.7, gl[src], rng.randint(n_cls, size=n_det))
        gt.append(dict(gt_bboxes_3d=torch.from_numpy(gb), gt_labels_3d=[int(x) for x in gl]))
        dt.append(dict(bboxes_3d=torch.from_numpy(db), scores_3d=torch.from_numpy(rng.uniform(size=n_det).astype(np.float32)),
                       labels_3d=torch.from_numpy(dl.astype(np.int64))))
    return gt, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=312)
    ap.add_argument('--classes', type=int, default=18)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_time.py measures on the GPU: no device, no number')
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd import ops
    from unidet3d_amd.evaluation import indoor_eval, indoor_eval_device, pack_annotations
    dev = torch.device('cuda:0')
    per_det, per_gt = detections_per_image(dev)
    n_det, n_gt = int(round(statistics.mean(per_det))), max(1, int(round(statistics.mean(per_gt))))
    gt, dt = make_pass(args.images, n_det, n_gt, args.classes)
    dt_dev = [{k: v.to(dev) for k, v in d.items()} for d in dt]
    names = [f'c{i}' for i in range(args.classes)]
    thr = [0.25, 0.5]

    reads = [0]
    wrapped = {}
    for meth in ('cpu', 'item', 'tolist', 'numpy'):
        real = getattr(torch.Tensor, meth)
        wrapped[meth] = real

        def counting(self, *a, _real=real, **k):
            if self.is_cuda:
                reads[0] += 1
            return _real(self, *a, **k)
        setattr(torch.Tensor, meth, counting)

    def timed(fn):
        out, ts, n_reads = None, [], 0
        for it in range(args.reps + 1):
            torch.cuda.synchronize()
            reads[0] = 0
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if it:
                ts.append((time.perf_counter() - t0) * 1e3)
            n_reads = reads[0]
        return out, ts, n_reads

    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        host, t_host, r_host = timed(lambda: indoor_eval(gt, dt, thr, names))
    devr, t_dev, r_dev = timed(lambda: indoor_eval_device(gt, dt_dev, thr, names))
    for meth, real in wrapped.items():
        setattr(torch.Tensor, meth, real)
    assert set(host) == set(devr)
    diff = max((abs(host[k] - devr[k]) for k in host if not (np.isnan(host[k]) and np.isnan(devr[k]))), default=0.0)
    nan_same = all(np.isnan(host[k]) == np.isnan(devr[k]) for k in host)

    p = pack_annotations(gt, dt_dev)
    G = p['gt_boxes'].shape[0]
    state = {}

    def k_match():
        state['m'] = ops.eval_match(p['det_boxes'], p['det_labels'], p['det_off'], p['gt_boxes'], p['gt_labels'], p['gt_off'], args.classes)

    def k_order():
        state['perm'] = ops.eval_order(p['det_scores'], p['det_labels'], args.classes)

    def k_sweep():
        iou_max, jmax, c_gt, c_det = state['m']
        ops.eval_sweep(iou_max, jmax, state['perm'], c_gt, c_det, G, thr)
    kernel_ms = {}
    for name, fn in (('u3d_eval_match', k_match), ('u3d_eval_order', k_order), ('u3d_eval_sweep', k_sweep)):
        ts = []
        for it in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it:
                ts.append(e0.elapsed_time(e1))
        kernel_ms[name] = ts

    def fmt(ts):
        return f'{statistics.median(ts):10.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})'
    D = sum(len(d['scores_3d']) for d in dt)
    lines = [f'evaluation of one validation pass; {torch.cuda.get_device_name(0)}; {args.images} images, {args.classes} classes, thresholds {thr}',
             f'predict on 3 synthetic scenes (12k points, reference test settings) returned {per_det} detections, scenes hold {per_gt} ground truths '
             f'-> {n_det} detections and {n_gt} ground truths per image: D = {D}, G = {G}',
             f'median of {args.reps} after one warm-up', '',
             f'host   indoor_eval (host tensors)              {fmt(t_host)}   reads of device tensors: {r_host}',
             f'device indoor_eval_device (pack + chain + read) {fmt(t_dev)}   reads of device tensors: {r_dev}',
             f'ratio host / device (medians): {statistics.median(t_host) / statistics.median(t_dev):.1f}',
             f'results: {len(host)} keys, max |host - device| = {diff:.3e}, NaN in the same places: {nan_same}', '',
             'HIP events around each entry point on the packed arrays:']
    lines += [f'  {name:<16} {fmt(ts)}' for name, ts in kernel_ms.items()]
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
