"""Time of the sparse-convolution forward, input gradient and weight gradient at wide layer shapes, next to the nearest shapes of the
32-channel five-level U-Net, on tools/prof_conv.py's level geometry (8 scenes x 100 k points, 2 cm voxels; level L = L - 1 strided
steps down).  Shapes alternate inside each round, so every line of the table comes from the same call and the same clocks.
usage: python tools/wide_channels_time.py [iters] [rounds] [fp32|bf16]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidet3d_amd import ops, precision as P, sparse  # noqa: E402
from unidet3d_amd.synthetic import make_scene  # noqa: E402

# (cin, cout, level): the level at which the 64-channel five-level / 32-channel seven-level net has the layer; * = a shape of the
# 32-channel five-level net (its own kernels), the neighbour the wide shape is read against
SHAPES = [(64, 64, 1, '*'), (128, 128, 2, '*'), (160, 160, 5, '*'), (320, 320, 5, ''), (256, 128, 4, '*'), (512, 256, 4, ''), (224, 224, 7, ''),
          (192, 192, 6, ''), (384, 192, 3, '')]


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    mode = sys.argv[3] if len(sys.argv) > 3 else 'fp32'
    dev = torch.device('cuda:0')
    vb = ops.voxelize([torch.from_numpy(make_scene(i).points).to(dev) for i in range(8)], 0.02, 128)
    coords, shape, index = vb.coords, vb.spatial_shape, vb.index
    levels = {}
    for lvl in range(1, 8):
        levels[lvl] = sparse.build_subm_rulebook(coords, index)
        coords, shape, index, _rb = sparse.build_down_rulebook(coords, 8, shape)
    cases = []
    for cin, cout, lvl, mark in SHAPES:
        rb = levels[lvl]
        n = rb.n_out
        g = torch.Generator(device=dev).manual_seed(cin * 1000 + cout)
        cases.append(dict(cin=cin, cout=cout, lvl=lvl, mark=mark, rb=rb, n=n, pairs=rb.total_pairs,
                          x=torch.randn(n, cin, device=dev, generator=g), w=(torch.randn(cout, 3, 3, 3, cin, device=dev, generator=g) * 0.05).requires_grad_(),
                          go=torch.randn(n, cout, device=dev, generator=g), t=dict(fwd=[], dgrad=[], wgrad=[])))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3            # us

    def fwd(c):
        with torch.no_grad():
            sparse.sparse_conv(c['x'], c['w'], c['rb'])

    def dgrad(c):                                            # the input-gradient launch of _SparseConvFn.backward, alone
        rb = c['rb']
        g, s, role, n_dst = sparse._roles(rb, 'fwd', transposed=True)
        sparse._gmm(c['go'], c['w'].detach().reshape(c['cout'], rb.K, c['cin']), True, rb, g, s, role, n_dst, None, 0.0, P.conv_format())

    def wgrad(c):                                            # x does not ask for a gradient: the backward is the weight gradient alone
        y = sparse.sparse_conv(c['x'], c['w'], c['rb'])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y.backward(c['go'])
        e1.record()
        c['w'].grad = None
        return e0, e1

    with P.operands('bf16' if mode == 'bf16' else 'fp32'):
        for c in cases:                                      # warm-up: weight packs, tile lists, workspaces
            fwd(c); dgrad(c); wgrad(c)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for c in cases:
                c['t']['fwd'].append(timed(lambda: fwd(c)))
                c['t']['dgrad'].append(timed(lambda: dgrad(c)))
                evs = [wgrad(c) for _ in range(iters)]
                torch.cuda.synchronize()
                c['t']['wgrad'].append(sum(a.elapsed_time(b) for a, b in evs) / iters * 1e3)
    print(f'# {mode} flow ({P.get_fp32_math()} fp32 math), {iters} iterations x {rounds} alternating rounds, best round; * = shape of the 32-channel five-level net')
    print('# cin->cout level rows pairs | fwd us TF/s | dgrad us TF/s | wgrad us TF/s')
    for c in cases:
        fl = 2.0 * c['pairs'] * c['cin'] * c['cout']
        cols = ' | '.join(f"{min(c['t'][k]):8.1f} {fl / (min(c['t'][k]) * 1e-6) / 1e12:6.2f}" for k in ('fwd', 'dgrad', 'wgrad'))
        print(f"{c['cin']:>3}->{c['cout']:<3}{c['mark']:1} L{c['lvl']} {c['n']:>7} {c['pairs']:>9} | {cols}")


if __name__ == '__main__':
    main()
