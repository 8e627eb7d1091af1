"""Build time of a general SparseConv3d(k=3, s=2, p=1) level (u3d_conv_mark + index rank + coordinates + u3d_conv_rulebook) next to the
hard-coded SparseConv3d(k=2, s=2) level (u3d_index_mark + ... + u3d_down_rulebook) on the same level-1 rows of a cfg2 batch (8
synthetic ScanNet-shape scenes x 100k points, 0.02 m voxels).  HIP events around the whole build, warm-up first, median of the repeats.
Both builds contain the one host read-back of the output row count.  Prints the pair counts too: 27 / 8 offsets is the expected order
of magnitude of the ratio.    python tools/prof_conv_general.py [--repeats 20]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    args = ap.parse_args()
    from unidet3d_amd import ops, sparse as S
    from unidet3d_amd.synthetic import make_scene
    dev = torch.device('cuda:0')
    scenes = [make_scene(i, n_points=100_000) for i in range(args.batch)]
    vb = ops.voxelize([torch.from_numpy(sc.points).to(dev) for sc in scenes], 0.02, 128)
    coords, shape, B, index = vb.coords, vb.spatial_shape, args.batch, vb.index
    geom = S.conv_geometry(3, 2, 1, 1)

    def timed(fn):
        for _ in range(args.warmup):
            out = fn()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return out, statistics.median(ms), min(ms), max(ms)
    down, t_down, lo_d, hi_d = timed(lambda: S.build_down_rulebook(coords, B, shape))
    gen, t_gen, lo_g, hi_g = timed(lambda: S.build_conv_rulebook(coords, index, B, shape, geom))
    p_down, p_gen = int(down[3].counts.sum()), int(gen[3].counts.sum())
    print(f'level-1 rows {coords.shape[0]}, grid {B} x {shape}, {args.repeats} repeats after {args.warmup} warm-up builds (HIP events, median [min, max])')
    print(f'k=2 s=2 p=0  (u3d_index_mark + u3d_down_rulebook): {t_down:.3f} ms [{lo_d:.3f}, {hi_d:.3f}]  out rows {down[3].n_out}  pairs {p_down}  K 8')
    print(f'k=3 s=2 p=1  (u3d_conv_mark + u3d_conv_rulebook):  {t_gen:.3f} ms [{lo_g:.3f}, {hi_g:.3f}]  out rows {gen[3].n_out}  pairs {p_gen}  K 27')
    print(f'time ratio {t_gen / t_down:.2f}; offsets 27 / 8 = {27 / 8:.2f}; pairs ratio {p_gen / max(p_down, 1):.2f}')


if __name__ == '__main__':
    main()
