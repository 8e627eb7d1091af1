"""Time of the sparse pooling kernels (csrc/sparse_pool.hip) next to the same four operations as a composition of torch ops on the same
tensors: per offset one ``index_select`` and one ``scatter_reduce_`` ('amax' / 'sum').  Two levels of a cfg2 batch (8 synthetic
ScanNet-shape scenes x 100k points, 0.02 m voxels): level 1 (about 350k rows) at 32 channels and level 3 (two k2 s2 steps down) at 96;
two layer geometries, k2 s2 p0 and k3 s2 p1; max and avg, forward and backward.  HIP events around each call, warm-up first, median of
the repeats.  Algorithmic bytes = present rows read + rows written + the neighbour table (4 K n); the fraction is of the 8 TB/s HBM peak
(about 6.3 TB/s is what streaming kernels reach).  The table build (u3d_pair_table, once per level and role) is timed on its own and
added to the operation that needs it for the verdict.    python tools/sparse_pool_time.py [--repeats 30] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
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

    scenes = [make_scene(i, n_points=100_000) for i in range(args.batch)]
    vb = ops.voxelize([torch.from_numpy(sc.points).to(dev) for sc in scenes], 0.02, 128)
    B = args.batch
    c1, s1, i1 = vb.coords, vb.spatial_shape, vb.index
    c2, s2, i2, _ = S.build_down_rulebook(c1, B, s1)
    c3, s3, i3, _ = S.build_down_rulebook(c2, B, s2)
    say(f'{args.repeats} repeats after {args.warmup} warm-up calls, HIP events, median [min, max] in microseconds; device {torch.cuda.get_device_name(0)}')
    slower = []
    for level, coords, shape, index, C in (('level 1', c1, s1, i1, 32), ('level 3', c3, s3, i3, 96)):
        for gname, geom in (('k2 s2 p0', S.conv_geometry(2, 2, 0, 1)), ('k3 s2 p1', S.conv_geometry(3, 2, 1, 1))):
            rb = S.build_conv_rulebook(coords, index, B, shape, geom)[3]
            n_in, n_out, K = rb.n_in, rb.n_out, rb.K
            cnt = rb.counts.cpu().tolist()
            P = sum(cnt)
            say()
            say(f'{level}, {gname}: {n_in} -> {n_out} rows x {C} channels, K = {K}, {P} pairs ({P / n_out:.2f} per output row)')
            g = torch.Generator(device=dev).manual_seed(1)
            x = torch.randn(n_in, C, device=dev, generator=g)
            dy = torch.randn(n_out, C, device=dev, generator=g)
            t_tab = {}
            for role in ('out', 'in'):
                def build(role=role):
                    rb._nbr.pop(role, None)
                    rb.neighbours(role)
                t_tab[role] = timed(build)
                say(f'  u3d_pair_table {role:3s}: {t_tab[role][0] * 1e3:8.1f} [{t_tab[role][1] * 1e3:.1f}, {t_tab[role][2] * 1e3:.1f}]   ({4 * K * (n_out if role == "out" else n_in) / 1e6:.1f} MB)')
            # the torch composition's index lists, converted once outside the timed region
            pin = [rb.pair_in[k, :cnt[k]].long() for k in range(K)]
            pout = [rb.pair_out[k, :cnt[k]].long() for k in range(K)]
            pin_e = [p[:, None].expand(-1, C) for p in pin]
            pout_e = [p[:, None].expand(-1, C) for p in pout]
            aux = {m: S.sparse_pool_forward(x, rb, m)[1] for m in ('max', 'avg')}
            count_f = aux['avg'].float()[:, None]

            def torch_fwd(mode):
                if mode == 'max':
                    y = torch.full((n_out, C), float('-inf'), device=dev)
                    for k in range(K):
                        if cnt[k]:
                            y.scatter_reduce_(0, pout_e[k], x.index_select(0, pin[k]), 'amax', include_self=True)
                    return y
                y = torch.zeros(n_out, C, device=dev)
                for k in range(K):
                    if cnt[k]:
                        y.scatter_reduce_(0, pout_e[k], x.index_select(0, pin[k]), 'sum', include_self=True)
                return y / count_f

            def torch_bwd(mode):
                dx = torch.zeros(n_in, C, device=dev)
                src = dy if mode == 'max' else dy / count_f
                for k in range(K):
                    if cnt[k]:
                        t = src.index_select(0, pout[k])
                        if mode == 'max':
                            t = t * (aux['max'].index_select(0, pout[k]) == k)
                        dx.scatter_reduce_(0, pin_e[k], t, 'sum', include_self=True)
                return dx

            for mode in ('max', 'avg'):
                # same results first (the yardstick computes what the kernels compute)
                y_hip, dx_hip = S.sparse_pool_forward(x, rb, mode)[0], S.sparse_pool_backward(dy, rb, mode, aux[mode])
                ey, ed = float((y_hip - torch_fwd(mode)).abs().max()), float((dx_hip - torch_bwd(mode)).abs().max())
                for direction, n_dst, role, hip, ref, err in (
                        ('fwd', n_out, 'out', lambda: S.sparse_pool_forward(x, rb, mode), lambda: torch_fwd(mode), ey),
                        ('bwd', n_in, 'in', lambda: S.sparse_pool_backward(dy, rb, mode, aux[mode]), lambda: torch_bwd(mode), ed)):
                    t_hip, t_ref = timed(hip), timed(ref)
                    nbytes = 4.0 * C * (P + n_dst) + 4.0 * K * n_dst
                    with_tab = t_hip[0] + t_tab[role][0]
                    say(f'  {mode} {direction}: HIP {t_hip[0] * 1e3:8.1f} [{t_hip[1] * 1e3:.1f}, {t_hip[2] * 1e3:.1f}]   {nbytes / 1e6:7.1f} MB  '
                        f'{nbytes / (t_hip[0] * 1e-3) / 1e12:5.2f} TB/s = {nbytes / (t_hip[0] * 1e-3) / HBM_PEAK * 100:4.1f} % of HBM peak | '
                        f'torch {t_ref[0] * 1e3:8.1f} [{t_ref[1] * 1e3:.1f}, {t_ref[2] * 1e3:.1f}] | torch / HIP {t_ref[0] / t_hip[0]:5.1f}x, '
                        f'with the table build {t_ref[0] / with_tab:5.1f}x | max |HIP - torch| {err:.2e}')
                    if with_tab > t_ref[0]:
                        slower.append(f'{level} {gname} {mode} {direction}')
    say()
    say('every HIP operation, its table build included, is at least as fast as the torch composition' if not slower
        else 'SLOWER than the torch composition (table build included): ' + '; '.join(slower))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
