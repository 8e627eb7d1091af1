"""Time the dense interchange of sparse tensors (``SparseConvTensor.dense`` in both layouts, its backward, ``from_dense``) against the
torch composition each replaces and against a ``torch.zeros`` fill of the same byte count, the streaming-write yardstick:

  dense, channels first    torch.zeros + index assignment + permute().contiguous()
  dense, channels last     torch.zeros + index assignment
  dense backward           the dense gradient indexed at the coordinates (through a permute view for channels first)
  from_dense               (x != 0).any(-1) + nonzero() + x[mask]

Random voxel sets at the given occupancies on one grid that does not fit the 256 MB cache, random features.  torch gets its index
tensors (int64 columns of the coordinates) built outside the timed region.  Device time: HIP events around one call, the variants
alternating inside every round (other work shares the host; a difference is read against the spread of the same variant).  ``from_dense``
and its composition both end in a host read of the count, inside the window.  Needs no reference tree and no network.

    python tools/dense_time.py [--reps 20] [--warmup 3] [--grid 2,200,176,40] [--out profiles/dense_time.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--grid', default='2,200,176,40')
    ap.add_argument('--channels', default='64,128')
    ap.add_argument('--occupancy', default='0.03,0.30')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dense_time.py measures on the GPU: no device, no number')
    from unidet3d_amd import sparse as S
    dev = torch.device('cuda:0')
    B, X, Y, Z = [int(v) for v in args.grid.split(',')]
    n_cells = B * X * Y * Z
    lines = [f'dense interchange on a grid {B} x ({X}, {Y}, {Z}) = {n_cells} cells; {torch.cuda.get_device_name(0)}; {args.warmup} warm-up + '
             f'{args.reps} timed rounds, variants alternating inside a round; command: python tools/dense_time.py ' + ' '.join(sys.argv[1:]),
             'device ms between HIP events around one call (median | p10 | p90); GB/s = bytes of the dense tensor / median; '
             'of fill = that rate over the torch.zeros fill\'s', '']
    ok = True
    for C in [int(v) for v in args.channels.split(',')]:
        nbytes = n_cells * C * 4
        for occ in [float(v) for v in args.occupancy.split(',')]:
            rng = np.random.RandomState(int(occ * 1000) + C)
            cells = np.flatnonzero(rng.rand(n_cells) < occ)
            coords = torch.tensor(np.stack(np.unravel_index(cells, (B, X, Y, Z)), 1).astype(np.int32)).to(dev)
            n = coords.shape[0]
            idx = tuple(coords[:, a].long() for a in range(4))
            f = torch.randn(n, C, device=dev)
            t = S.SparseConvTensor(f, coords, [X, Y, Z], B)
            t.index                                           # the level's index exists behind any layer: not part of dense()
            d_first = torch.randn(B, C, X, Y, Z, device=dev)
            d_last = d_first.permute(0, 2, 3, 4, 1).contiguous()
            x_last = t.dense(channels_first=False)

            def torch_first():
                d = torch.zeros(B, X, Y, Z, C, device=dev)
                d[idx] = f
                return d.permute(0, 4, 1, 2, 3).contiguous()

            def torch_last():
                d = torch.zeros(B, X, Y, Z, C, device=dev)
                d[idx] = f
                return d

            def torch_from_dense():
                mask = (x_last != 0).any(-1)
                return mask.nonzero().int(), x_last[mask]

            def gather(d, cf):
                y = torch.empty(n, C, device=dev)
                S.L.call('u3d_dense_gather', S.L.ptr(d), B, X, Y, Z, C, int(cf), S.L.ptr(coords), n, S.L.ptr(y), S.L.stream())
                return y

            variants = [
                ('fill: torch.zeros', None, lambda: torch.zeros(B, X, Y, Z, C, device=dev)),
                ('dense channels first: u3d', 'first', lambda: t.dense()),
                ('dense channels first: torch', 'first', torch_first),
                ('dense channels last: u3d', 'last', lambda: t.dense(channels_first=False)),
                ('dense channels last: torch', 'last', torch_last),
                ('backward channels first: u3d', 'bfirst', lambda: gather(d_first, True)),
                ('backward channels first: torch', 'bfirst', lambda: d_first.permute(0, 2, 3, 4, 1)[idx]),
                ('backward channels last: u3d', 'blast', lambda: gather(d_last, False)),
                ('backward channels last: torch', 'blast', lambda: d_last[idx]),
                ('from_dense: u3d', 'from', lambda: S.SparseConvTensor.from_dense(x_last)),
                ('from_dense: torch', 'from', torch_from_dense),
            ]
            # the compared pairs compute the same thing
            assert torch.equal(t.dense(), torch_first()) and torch.equal(x_last, torch_last())
            assert torch.equal(gather(d_first, True), d_first.permute(0, 2, 3, 4, 1)[idx]) and torch.equal(gather(d_last, False), d_last[idx])
            back = S.SparseConvTensor.from_dense(x_last)
            ri, rf = torch_from_dense()
            assert torch.equal(back.indices, ri) and torch.equal(back.features, rf)
            del back, ri, rf
            ms = {name: [] for name, _, _ in variants}
            for it in range(args.warmup + args.reps):
                for name, _, fn in variants:
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    del out
                    if it >= args.warmup:
                        ms[name].append(e0.elapsed_time(e1))

            def q(xs, p):
                xs = sorted(xs)
                return xs[min(len(xs) - 1, int(p * len(xs)))]
            med = {name: statistics.median(v) for name, v in ms.items()}
            fill = med['fill: torch.zeros']
            lines.append(f'C = {C}, occupancy {occ:.2f}: {n} rows, dense tensor {nbytes / 1e6:.0f} MB')
            for name, pair, _ in variants:
                v = ms[name]
                note = ''
                if name.endswith('u3d'):
                    other = med[name[:-3] + 'torch']
                    note = f'   {other / med[name]:.2f}x the torch composition'
                    if not pair.startswith('b') and med[name] > other:
                        ok = False
                        note += '   SLOWER'
                lines.append(f'  {name:<34} {med[name]:8.3f} | {q(v, 0.1):8.3f} | {q(v, 0.9):8.3f} ms   {nbytes / med[name] / 1e6:8.1f} GB/s   '
                             f'{fill / med[name]:5.2f} of fill{note}')
            lines.append('')
            del t, f, d_first, d_last, x_last
            torch.cuda.empty_cache()
    lines.append('every forward path at least as fast as its torch composition: ' + ('yes' if ok else 'NO'))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
