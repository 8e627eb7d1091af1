"""Time of the per-scene operations (csrc/sparse_scene.hip) on the level-1 rows of a cfg2 batch (8 synthetic ScanNet-shape scenes x 100k
points, 0.02 m voxels) and of the cfg5 room (B = 1, one S3DIS-shape room of 1 M points).  HIP events around each call, warm-up first,
median of the repeats with min / max; the two sides of a pair are taken ALTERNATELY, call by call, in one session.
  prune_topk (k = 1000 and k = n_b / 2, 32 channels) against what users write today, which runs identically on the parent commit: a
  per-scene ``torch.topk`` + scatter loop over the scene ranges (one host wait per scene), then ``prune``.  Both include their host reads.
  The composition's own run-to-run spread, (max - min) / median of its repeats, is printed next to the ratio.
  global_pool ('max' / 'avg', 32 and 128 channels) against the per-scene ``amax(0)`` / ``mean(0)`` torch loop over host-known ranges, and
  against the streaming bound n C 4 bytes / 6.3 TB/s (the achievable HBM rate of the MI355X; 8 TB/s is the specification).  The working
  sets sit in the 256 MB Infinity Cache when a call repeats.
    python tools/scene_ops_time.py [--repeats 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from unidet3d_amd import geometry as G
    from unidet3d_amd import ops, sparse as S
    from unidet3d_amd.synthetic import make_scene
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def timed(*fns):
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        ms = [[] for _ in fns]
        for _ in range(args.repeats):
            for i, fn in enumerate(fns):
                ms[i].append(once(fn))
        return [(statistics.median(m), min(m), max(m)) for m in ms]

    def fmt(t):
        return f'{t[0] * 1e3:8.1f} [{t[1] * 1e3:.1f}, {t[2] * 1e3:.1f}]'

    say(f'{args.repeats} repeats after {args.warmup} warm-up calls, HIP events, median [min, max] in microseconds; device {torch.cuda.get_device_name(0)}')
    workloads = (('cfg2 level 1, B = 8', [make_scene(i, n_points=100_000) for i in range(8)]),
                 ('cfg5 room, B = 1', [make_scene(500, n_points=1_000_000, area_scale=10.0, n_furniture=40)]))
    for name, scenes in workloads:
        B = len(scenes)
        vb = ops.voxelize([torch.from_numpy(sc.points).to(dev) for sc in scenes], 0.02, 128)
        coords, shape = G.mark_canonical(vb.coords), vb.spatial_shape
        n = coords.shape[0]
        g = torch.Generator(device=dev).manual_seed(1)
        off = G.scene_offsets(coords, B)[0].tolist()
        sizes = [off[b + 1] - off[b] for b in range(B)]
        say()
        say(f'{name}: {n} rows, scenes of {sizes} rows')

        # ---- prune_topk against the per-scene torch.topk + scatter loop and prune
        x = S.SparseConvTensor(torch.randn(n, 32, device=dev, generator=g), coords, shape, B)
        scores = torch.rand(n, device=dev, generator=g)

        def composed(k):
            keep = torch.zeros(n, dtype=torch.bool, device=dev)
            o = off                                                        # (users hold the scene ranges on the host)
            for b in range(B):
                if o[b + 1] > o[b]:
                    kb = min(k if isinstance(k, int) else k[b], o[b + 1] - o[b])
                    keep[o[b] + torch.topk(scores[o[b]:o[b + 1]], kb).indices] = True
                    keep[o[b]].item()                                      # the host wait of a mask built scene by scene
            return S.prune(x, keep)
        for label, k in (('k = 1000', 1000), ('k = n_b / 2', [s // 2 for s in sizes])):
            ours, theirs = S.prune_topk(x, scores, k), composed(k)
            same = bool(torch.equal(ours.features, theirs.features) and torch.equal(ours.indices, theirs.indices))
            t_o, t_c = timed(lambda: S.prune_topk(x, scores, k), lambda: composed(k))
            say(f'  prune_topk {label}: {fmt(t_o)} | topk + scatter loop + prune {fmt(t_c)} | loop / HIP {t_c[0] / t_o[0]:5.2f}x | '
                f"the loop's spread {(t_c[2] - t_c[1]) / t_c[0]:.2f} | same rows {same}")

        # ---- global pooling against the per-scene torch loop and the streaming bound
        for C in (32, 128):
            f = torch.randn(n, C, device=dev, generator=g)
            xc = S.SparseConvTensor(f, coords, shape, B)
            bound = n * C * 4 / HBM * 1e6
            for mode, loop in (('max', lambda: torch.stack([f[off[b]:off[b + 1]].amax(0) for b in range(B)])),
                               ('avg', lambda: torch.stack([f[off[b]:off[b + 1]].mean(0) for b in range(B)]))):
                err = float((S.global_pool(xc, mode) - loop()).abs().max())
                t_o, t_c = timed(lambda: S.global_pool(xc, mode), loop)
                say(f'  global_pool {mode} C = {C:3d}: {fmt(t_o)} | torch loop {fmt(t_c)} | loop / HIP {t_c[0] / t_o[0]:5.2f}x | streaming bound '
                    f'{bound:6.1f} us ({n * C * 4 / 1e6:.1f} MB): HIP / bound {t_o[0] * 1e3 / bound:5.2f}x | max |difference| {err:.1e}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
