"""Time of the union-add and pruning pieces (csrc/sparse_sets.hip, geometry.build_union_level / compact_mask) on a cfg2 batch (8 synthetic
ScanNet-shape scenes x 100k points, 0.02 m voxels): the level-1 rows x 32 channels and the level-3 rows x 96 channels.  HIP events around
each call, warm-up first, median of the repeats with min / max.
Geometry: ``build_union_level`` of a level against its own random half (the union IS the level: the shortcut), and of two random
three-quarter subsets (a new level: coordinate rows written too); ``compact_mask`` at p = 0.5.  Each includes its one host read.
Rows: u3d_rows_take2 (the join forward of the two three-quarter subsets) next to the torch composition a user writes today -- ``zeros``,
``index_copy_`` of a's rows, ``index_add_`` of b's -- and u3d_rows_take by the kept list next to ``index_select``.  A pair is taken
ALTERNATELY, call by call, in one session.  Algorithmic bytes next to each figure: the fused join reads both operands and both maps and
writes y once; the composition writes y three times (zeros, copy, add) and reads it once more.  These working sets sit in the 256 MB
Infinity Cache when a call repeats: the rates are cache rates, not HBM rates.
    python tools/sparse_sets_time.py [--repeats 30] [--out FILE]"""
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
        """the functions called alternately: (median, min, max) in ms of each"""
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

    def rate(nbytes, t):
        return f'{nbytes / 1e6:6.1f} MB {nbytes / (t[0] * 1e-3) / 1e9:6.0f} GB/s'

    scenes = [make_scene(i, n_points=100_000) for i in range(args.batch)]
    vb = ops.voxelize([torch.from_numpy(sc.points).to(dev) for sc in scenes], 0.02, 128)
    B = args.batch
    c1, s1 = vb.coords, vb.spatial_shape
    c2, s2, _, _ = S.build_down_rulebook(c1, B, s1)
    c3, s3, _, _ = S.build_down_rulebook(c2, B, s2)
    say(f'{args.repeats} repeats after {args.warmup} warm-up calls, HIP events, median [min, max] in microseconds; device {torch.cuda.get_device_name(0)}')

    for level, coords, shape, C in (('level 1', c1, s1, 32), ('level 3', c3, s3, 96)):
        n = coords.shape[0]
        g = torch.Generator(device=dev).manual_seed(1)
        full_ix = G.OccupancyIndex.from_coords(coords, B, shape)
        half = coords[torch.rand(n, device=dev, generator=g) < 0.5].contiguous()
        half_ix = G.OccupancyIndex.from_coords(half, B, shape)
        ca = coords[torch.rand(n, device=dev, generator=g) < 0.75].contiguous()
        cb = coords[torch.rand(n, device=dev, generator=g) < 0.75].contiguous()
        ia, ib = G.OccupancyIndex.from_coords(ca, B, shape), G.OccupancyIndex.from_coords(cb, B, shape)
        keep = torch.rand(n, device=dev, generator=g) < 0.5
        say()
        say(f'{level}: {n} rows x {C} channels, grid {list(shape)}')
        t_half, t_new, t_mask = timed(lambda: G.build_union_level(coords, full_ix, half, half_ix, B, shape),
                                      lambda: G.build_union_level(ca, ia, cb, ib, B, shape), lambda: G.compact_mask(keep))
        lvl = G.build_union_level(ca, ia, cb, ib, B, shape)
        say(f'  build_union_level, the level ({n} rows) and its random half ({half.shape[0]}): union = the level:  {fmt(t_half)}')
        say(f'  build_union_level, two 3/4 subsets ({ca.shape[0]}, {cb.shape[0]} rows) -> new level of {lvl.n} rows:  {fmt(t_new)}')
        say(f'  compact_mask at p = 0.5 ({int(keep.sum())} of {n} kept):  {fmt(t_mask)}')

        # ---- the join forward against the torch composition
        a = torch.randn(ca.shape[0], C, device=dev, generator=g)
        b = torch.randn(cb.shape[0], C, device=dev, generator=g)
        into_a, into_b = lvl.into('a').long(), lvl.into('b').long()
        y = torch.empty(lvl.n, C, device=dev)

        def fused():
            L.call('u3d_rows_take2', L.ptr(a), L.ptr(lvl.rows_a), a.shape[0], L.ptr(b), L.ptr(lvl.rows_b), b.shape[0], lvl.n, C, L.ptr(y), L.stream())

        def composed():
            z = torch.zeros(lvl.n, C, device=dev)
            z.index_copy_(0, into_a, a)
            z.index_add_(0, into_b, b)
            return z
        fused()
        err = float((y - composed()).abs().max())
        row = 4.0 * C
        b_fused = row * (a.shape[0] + b.shape[0] + lvl.n) + 8.0 * lvl.n
        b_comp = row * (lvl.n + 2 * a.shape[0] + 3 * b.shape[0]) + 8.0 * (a.shape[0] + b.shape[0])
        t_f, t_c = timed(fused, composed)
        say(f'  join forward: u3d_rows_take2 {fmt(t_f)} {rate(b_fused, t_f)} | zeros + index_copy_ + index_add_ {fmt(t_c)} {rate(b_comp, t_c)} | '
            f'torch / HIP {t_c[0] / t_f[0]:5.2f}x | max |difference| {err:.1e}')

        # ---- the gather by the kept list against index_select
        x = torch.randn(n, C, device=dev, generator=g)
        kept, pos, nk = G.compact_mask(keep)
        kept = kept.contiguous()
        kept64 = kept.long()
        yk = torch.empty(nk, C, device=dev)

        def take():
            L.call('u3d_rows_take', L.ptr(x), L.ptr(kept), nk, n, C, L.ptr(yk), L.stream())
        take()
        same = bool(torch.equal(yk, x.index_select(0, kept64)))
        t_t, t_s = timed(take, lambda: x.index_select(0, kept64))
        say(f'  gather of the kept rows: u3d_rows_take {fmt(t_t)} {rate(2 * row * nk + 4.0 * nk, t_t)} | index_select {fmt(t_s)} '
            f'{rate(2 * row * nk + 8.0 * nk, t_s)} | torch / HIP {t_s[0] / t_t[0]:5.2f}x | bit-equal {same}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
