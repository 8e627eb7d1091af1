"""Time of the transposed-convolution geometry and of the two bias kernels (csrc/rulebook.hip convt_mark_k, csrc/sparse_bias.hip) on a
cfg2 batch (8 synthetic ScanNet-shape scenes x 100k points, 0.02 m voxels).  HIP events around each call, warm-up first, median of the
repeats.
Geometry: ``build_convt_rulebook`` (k3 s2 p1 q1) from the level-2 rows, next to ``build_conv_rulebook`` (k3 s2 p1) going the other way
from the level it made.  The two are NOT the same work: the forward layer's output set from the fine level is larger than the level-2
rows the transposed layer started from (every coarse cell a fine row reaches, not only the original ones), so it makes more pairs and
marks over the fine level's rows.  Each line therefore carries its own rows and pairs and the time per million pairs; no ratio is
formed.  Both builds include their one host read (``count()``).
Bias: u3d_bias_add / u3d_bias_grad at level 1 (32 channels) and level 3 (96), next to the torch operations they replace on the same
tensors, ``y.add_(b)`` and ``dy.sum(0)``.  Algorithmic bytes: add reads and writes every row, grad reads every row.  These working sets
(45 MB at level 1) sit in the 256 MB Infinity Cache when a call repeats: the rates are cache rates, not HBM rates.
    python tools/convt_time.py [--repeats 30] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from unidet3d_amd import _lib as L
    from unidet3d_amd import ops, sparse as S
    from unidet3d_amd.synthetic import make_scene
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    def fmt(t):
        return f'{t[0] * 1e3:8.1f} [{t[1] * 1e3:.1f}, {t[2] * 1e3:.1f}]'

    scenes = [make_scene(i, n_points=100_000) for i in range(args.batch)]
    vb = ops.voxelize([torch.from_numpy(sc.points).to(dev) for sc in scenes], 0.02, 128)
    B = args.batch
    c1, s1 = vb.coords, vb.spatial_shape
    c2, s2, i2, _ = S.build_down_rulebook(c1, B, s1)
    c3, s3, i3, _ = S.build_down_rulebook(c2, B, s2)
    say(f'{args.repeats} repeats after {args.warmup} warm-up calls, HIP events, median [min, max] in microseconds; device {torch.cuda.get_device_name(0)}')

    # ---- geometry
    geom, q = S.conv_geometry(3, 2, 1, 1), (1, 1, 1)
    cn, sn, ixn, rbt = S.build_convt_rulebook(c2, B, s2, geom, q)
    oc, oshape, _, rbf = S.build_conv_rulebook(cn, ixn, B, sn, geom)
    say()
    say(f'geometry, k3 s2 p1 (q1): level 2 = {c2.shape[0]} rows {list(s2)} -> new level {cn.shape[0]} rows {list(sn)}; '
        f'{int(rbt.counts.sum())} pairs transposed, {int(rbf.counts.sum())} pairs the other way ({oc.shape[0]} rows {list(oshape)})')
    t_t = timed(lambda: S.build_convt_rulebook(c2, B, s2, geom, q))
    t_f = timed(lambda: S.build_conv_rulebook(cn, ixn, B, sn, geom))
    pt, pf = int(rbt.counts.sum()), int(rbf.counts.sum())
    say(f'  build_convt_rulebook ({c2.shape[0]} -> {cn.shape[0]} rows, {pt} pairs):  {fmt(t_t)}   {t_t[0] * 1e3 / (pt / 1e6):6.1f} us per million pairs')
    say(f'  build_conv_rulebook  ({cn.shape[0]} -> {oc.shape[0]} rows, {pf} pairs):  {fmt(t_f)}   {t_f[0] * 1e3 / (pf / 1e6):6.1f} us per million pairs')

    # ---- bias
    for level, n, C in (('level 1', c1.shape[0], 32), ('level 3', c3.shape[0], 96)):
        g = torch.Generator(device=dev).manual_seed(1)
        y = torch.randn(n, C, device=dev, generator=g)
        b = torch.randn(C, device=dev, generator=g)
        db = torch.empty(C, device=dev)
        ws = L.ws(L.lib().u3d_bias_grad_ws_bytes(n, C), dev)
        ref_add, ref_sum = y + b, y.double().sum(0)
        S.bias_add_(y_hip := y.clone(), b)
        e_add = float((y_hip - ref_add).abs().max())
        e_sum = float((S.bias_grad(y).double() - ref_sum).abs().max())
        nbytes = 4.0 * n * C
        say()
        say(f'{level}: {n} rows x {C} channels ({nbytes / 1e6:.1f} MB)')
        for what, hip, ref, moved, err in (
                ('bias_add ', lambda: L.call('u3d_bias_add', L.ptr(y), L.ptr(b), n, C, L.stream()), lambda: y.add_(b), 2 * nbytes, e_add),
                ('bias_grad', lambda: L.call('u3d_bias_grad', L.ptr(y), n, C, L.ptr(db), L.ptr(ws), L.stream()), lambda: y.sum(0), nbytes, e_sum)):
            t_hip, t_ref = timed(hip), timed(ref)
            y.copy_(ref_add)                   # (the repeated in-place adds grow y: back to bounded values for the next measurement)
            say(f'  {what}: HIP {fmt(t_hip)}  {moved / (t_hip[0] * 1e-3) / 1e9:7.0f} GB/s | torch {fmt(t_ref)}  {moved / (t_ref[0] * 1e-3) / 1e9:7.0f} GB/s | '
                f'torch / HIP {t_ref[0] / t_hip[0]:5.2f}x | max |HIP - reference| {err:.2e}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
