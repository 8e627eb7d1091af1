"""Inference throughput of UniDet3D.predict (forward + top-k + NMS + superpoint trimming) on batches of synthetic scenes.

    python tools/predict_time.py [--batch 1,8] [--points 100000] [--steps 20] [--warmup 3]

Prints one JSON line: for every batch size, ``predict`` scenes/s (device-synchronised host clock, warm-up excluded), and the
post-processing alone on the same decoder outputs -- ``ops.postprocess_batch`` (the batched kernels) against the per-scene loop
``ops.postprocess_scene`` -- alternated in this process (median ms over the steps)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unidet3d_amd import ops  # noqa: E402
from unidet3d_amd.config import build_model, scannet_model_cfg  # noqa: E402
from unidet3d_amd.data import make_batch_inputs  # noqa: E402
from unidet3d_amd.synthetic import make_scene  # noqa: E402


def _sync_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', default='1,8')
    ap.add_argument('--points', type=int, default=100_000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev = 'cuda:0'
    torch.manual_seed(0)
    model = build_model(scannet_model_cfg()).to(dev).eval()
    rec = dict(points=a.points, steps=a.steps, warmup=a.warmup)
    for B in [int(x) for x in a.batch.split(',')]:
        inputs, samples = make_batch_inputs([make_scene(3 + i, n_points=a.points) for i in range(B)], dev)
        seen, orig = {}, model.predict_by_feat
        model.predict_by_feat = lambda out, *x, **k: (seen.update(args=(out,) + x), orig(out, *x, **k))[1]
        with torch.no_grad():
            for _ in range(a.warmup):
                res = model.predict(inputs, samples)
            model.predict_by_feat = orig
            dt = [_sync_time(lambda: model.predict(inputs, samples)) for _ in range(a.steps)]
            res = model.predict(inputs, samples)
            out, plan, vb, offs, names = seen['args']
            cls = [out['cls_preds'][i] for i in range(B)]
            box = [out['bboxes'][i] for i in range(B)]
            sts = model.postproc_settings(names)

            def batched():
                ops.postprocess_batch(cls, box, sts, vb, plan, offs)

            def per_scene():
                for i in range(B):
                    ops.postprocess_scene(cls[i], box[i], sts[i], vb.points, plan.sp_offsets[offs[i]:], plan.sp_points, offs[i + 1] - offs[i])

            for _ in range(a.warmup):
                batched(); per_scene()
            tb, tl = [], []
            for _ in range(a.steps):                              # alternated, same decoder outputs
                tb.append(_sync_time(batched))
                tl.append(_sync_time(per_scene))
        total = sum(dt)
        rec[f'b{B}'] = dict(predict_scenes_per_s=round(B * len(dt) / total, 2), predict_ms_per_batch=round(1e3 * statistics.median(dt), 3),
                            postproc_batched_ms=round(1e3 * statistics.median(tb), 3), postproc_per_scene_loop_ms=round(1e3 * statistics.median(tl), 3),
                            boxes=[len(s.pred_instances_3d.labels_3d) for s in res], voxels=int(model._vb.coords.shape[0]))
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
