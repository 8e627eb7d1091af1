"""Time of ``UniDet3DCriterion.__call__`` forward + backward on a cfg4-shaped batch with one crowded scene (HIP events, after
warm-up): 8 scenes over the six datasets of the joint config, 7 decoder heads, the joint config's query counts (superpoint datasets
~1 500 queries, voxel-query datasets capped at ``query_thr`` = 3 000), 20 GTs per scene except the ScanNet++ scene, which holds
``--crowded G`` of them.

    python tools/criterion_time.py --crowded 64 65 128 256 [--tree OTHER_CHECKOUT] [--repeats 5] [--iters 10]

``--tree`` imports ``unidet3d_amd`` from another checkout (A/B against another commit: before the multi-word match masks a batch with
more than 64 GTs in a scene took the per-scene tensor-op loop).  ``U3D_CRITERION_COST=query|pair`` forces one of the two cost
kernels of csrc/criterion.hip for an A/B of the dispatch.  One line per G: median and range over the repeats, ms per call."""
import argparse
import os
import statistics
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--crowded', type=int, nargs='+', default=[64, 65, 128, 256])
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--warmup', type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

from unidet3d_amd.config import joint_model_cfg  # noqa: E402
from unidet3d_amd.registry import MODELS  # noqa: E402
from unidet3d_amd.structures import DepthInstance3DBoxes, InstanceData_  # noqa: E402

DEV = 'cuda:0'
SCENES = [('scannet', 1500), ('arkitscenes', 3000), ('s3dis', 1500), ('multiscan', 1500), ('3rscan', 3000), ('scannetpp', 3000),
          ('scannet', 1500), ('arkitscenes', 3000)]
CROWDED = 5
L_HEADS = 7


def make_batch(cfg, G):
    gen = torch.Generator().manual_seed(1234)
    dec = cfg['decoder']
    n_cls = {n: len(c) for n, c in zip(dec['datasets'], dec['datasets_classes'])}
    CU = 128
    cols = {n: torch.randperm(CU - 1, generator=torch.Generator().manual_seed(50 + k))[:n_cls[n]].tolist() + [CU - 1]
            for k, n in enumerate(dec['datasets'])}
    names, sizes = [s[0] for s in SCENES], [s[1] for s in SCENES]
    cidx, yaw = [cols[n] for n in names], [n == 'arkitscenes' for n in names]
    insts, gts = [], []
    for b, (name, n) in enumerate(SCENES):
        g = G if b == CROWDED else 20
        dof = 7 if yaw[b] else 6
        boxes = torch.cat((torch.rand(g, 3, generator=gen) * 6, torch.rand(g, 3, generator=gen) + 0.3), 1)
        if dof == 7:
            boxes = torch.cat((boxes, (torch.rand(g, 1, generator=gen) - 0.5) * 2.4), 1)
        owner = torch.randint(0, 4 * g, (n,), generator=gen)                       # a superpoint belongs to at most one GT
        qmask = owner[None, :] == torch.arange(g)[:, None]
        insts.append(InstanceData_(labels_3d=torch.randint(0, n_cls[name], (g,), generator=gen).to(DEV), query_masks=qmask.to(DEV),
                                   bboxes_3d=DepthInstance3DBoxes(boxes, with_yaw=yaw[b], box_dim=dof, origin=(0.5, 0.5, 0.5)).to(DEV)))
        gts.append(boxes)
    n_tot = sum(sizes)
    cls = [(torch.randn(n_tot, CU, generator=gen) * 1.5).to(DEV).requires_grad_() for _ in range(L_HEADS)]
    box = []
    for _ in range(L_HEADS):
        rows = []
        for b, n in enumerate(sizes):
            near = gts[b][torch.randint(0, len(gts[b]), (n,), generator=gen)]
            r = torch.zeros(n, 7)
            r[:, :near.shape[1]] = near
            r[:, :6] += torch.randn(n, 6, generator=gen) * 0.08
            r[:, 3:6] = r[:, 3:6].abs() + 0.05
            rows.append(r)
        box.append(torch.cat(rows).to(DEV).requires_grad_())

    def views(l):
        cs, bs, o = [], [], 0
        for b, n in enumerate(sizes):
            cs.append(cls[l][o:o + n][:, cidx[b]])
            bs.append(box[l][o:o + n] if yaw[b] else box[l][o:o + n][:, :6])
            o += n
        return dict(cls_preds=cs, bboxes=bs)
    pred = dict(views(0), aux_outputs=[views(l) for l in range(1, L_HEADS)],
                _packed=dict(cls=cls, box=box, sizes=sizes, cidx=cidx, yaw=yaw))
    return pred, insts, names, cls + box


def main():
    cfg = joint_model_cfg()
    crit = MODELS.build(cfg['criterion'])
    try:
        rev = subprocess.run(['git', '-C', args.tree, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
    except OSError:
        rev = ''
    print(f'tree {os.path.abspath(args.tree)} {rev} U3D_CRITERION_COST={os.environ.get("U3D_CRITERION_COST", "")}', flush=True)
    for G in args.crowded:
        pred, insts, names, leaves = make_batch(cfg, G)
        fused = crit._can_fuse(pred, insts, names) and crit._loss_fused(pred['_packed'], insts, names) is not None

        def step():
            for t in leaves:
                t.grad = None
            # the per-scene views of the dict contract are built once, as the decoder hands them over: keep their graph across calls
            crit(pred, insts, names)['det_loss'].backward(retain_graph=True)
        for _ in range(args.warmup):
            step()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.iters)
        print(f'G={G:4d} path={"fused kernel" if fused else "tensor-op fallback"} median {statistics.median(ms):9.3f} ms  '
              f'min {min(ms):9.3f}  max {max(ms):9.3f}  spread {(max(ms) - min(ms)) / statistics.median(ms) * 100:5.1f} %  repeats {ms}', flush=True)


if __name__ == '__main__':
    main()
