"""Time the varlen flash attention, forward and backward, at head_dim 32 and 64 on the same packed tensor, in the three data flows:

  fp32      fp32 tensors, three bf16 planes per operand (the default fp32 math)        u3d_attn_varlen_fwd / _bwd
  bf16 ops  fp32 tensors, bf16 operands (precision.operands('bf16'))                  u3d_attn_varlen_fwd_bf16 / _bwd_bf16
  bf16      bf16 tensors (what precision.bf16_act() hands the kernels)                u3d_attn_varlen_fwd_b16 / _bwd_b16

Workload: B scenes x n queries at width D (default 8 x 3000 x 256, the training cut).  The algorithmic work -- 4 n^2 D flops forward,
10 n^2 D backward, per scene -- does not depend on how D is split into heads, so (H, hd) = (D / 32, 32) of the same run is the yardstick
inside the library; torch's scaled_dot_product_attention per scene on the same box (fp32 beside the fp32 path, bf16 beside the bf16-tensor
path) is the one outside it.

Device time between HIP events around one forward / one backward call (the backward is delta + dQ + dK/dV), each issued behind a queued
4096^3 GEMM so that the host runs ahead of the GPU, after warm-up, the variants alternating inside every round; median | p10 | p90 over the rounds.  Per-kernel times come from a kernel trace of this script in a run
of its own (--no-sdpa --reps 5 under rocprofv3 --kernel-trace --stats).

--dropout P adds, in the same run and alternating with the others, the `_drop` kernels (dropout with probability P on the
softmax probabilities, mask regenerated in the kernels) beside the p = 0 ones, gives torch's per-scene call dropout_p = P -- what a user
without these kernels would run -- and prints the ratios `_drop` / p = 0 and `_drop` / torch.

--waves 4,8 (DESIGN 4.2 "tile waves") adds, alternating with the others, the same calls with that many waves per workgroup forced
(precision.attn_tile_waves) beside the launch plan's choice, and prints each forced form over the first one listed.

    python tools/attn_time.py [--reps 30] [--warmup 5] [--dropout 0.1] [--waves 4,8] [--out profiles/attn_hd64_time.txt]
"""
import argparse
import contextlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


_SPIN = None


def _timed(fn):
    """device ms of what fn() enqueues: the events go behind a queued GEMM, so the host has issued fn()'s launches before the GPU reaches
    them and the interval holds their execution, not their issue"""
    global _SPIN
    if _SPIN is None:
        _SPIN = torch.randn(4096, 4096, device='cuda:0')
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    _SPIN @ _SPIN
    e0.record()
    r = fn()
    e1.record()
    return r, (e0, e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--scenes', type=int, default=8)
    ap.add_argument('--queries', type=int, default=3000)
    ap.add_argument('--d', type=int, default=256)
    ap.add_argument('--no-sdpa', action='store_true')
    ap.add_argument('--dropout', type=float, default=0.0)
    ap.add_argument('--waves', default='', help='comma-separated tile waves to force beside the plan, e.g. 4,8')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('attn_time.py measures on the GPU: no device, no number')
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd import precision as P
    from unidet3d_amd.encoder import attention_varlen
    dev = torch.device('cuda:0')
    B, n, D = args.scenes, args.queries, args.d
    gen = torch.Generator(device=dev).manual_seed(0)
    qkv32 = torch.randn(B * n, 3 * D, device=dev, generator=gen)
    go32 = torch.randn(B * n, D, device=dev, generator=gen)
    cu = torch.arange(B + 1, device=dev, dtype=torch.int32) * n
    splits = [(D // 32, 32), (D // 64, 64)]
    flows = [('fp32', torch.float32, contextlib.nullcontext), ('bf16 ops', torch.float32, lambda: P.operands('bf16')),
             ('bf16', torch.bfloat16, contextlib.nullcontext)]

    waves = [int(w) for w in args.waves.split(',') if w]

    def lib_variant(flow, dtype, ctx, H, p=0.0, nw=None):
        x = qkv32.clone().to(dtype).requires_grad_()
        go = go32.to(dtype)

        def run():
            with ctx(), (P.attn_tile_waves(nw) if nw is not None else contextlib.nullcontext()):
                x.grad = None
                out, ef = _timed(lambda: attention_varlen(x, cu, n, H, 0, p, (1234, 5)))
                _, eb = _timed(lambda: out.backward(go))
            return ef, eb
        return run

    def sdpa_variant(dtype, H):
        hd = D // H
        q, k, v = [t.reshape(B, n, H, hd).transpose(1, 2).contiguous().to(dtype).requires_grad_() for t in qkv32.clone().chunk(3, -1)]
        go = go32.reshape(B, n, H, hd).transpose(1, 2).contiguous().to(dtype)

        def run():          # per scene, as a user without a varlen kernel would call it
            q.grad = k.grad = v.grad = None
            outs, ef = _timed(lambda: [torch.nn.functional.scaled_dot_product_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], dropout_p=args.dropout)
                                       for b in range(B)])
            _, eb = _timed(lambda: torch.autograd.backward(outs, [go[b:b + 1] for b in range(B)]))
            return ef, eb
        return run

    variants = []
    for flow, dtype, ctx in flows:
        for H, hd in splits:
            variants.append((f'library  {flow:<8} H={H} hd={hd}', flow, hd, lib_variant(flow, dtype, ctx, H)))
    if args.dropout:
        for flow, dtype, ctx in flows:
            for H, hd in splits:
                variants.append((f'library  {flow:<8} H={H} hd={hd} dropout {args.dropout}', flow + ' drop', hd, lib_variant(flow, dtype, ctx, H, args.dropout)))
    for nw in waves:
        for flow, dtype, ctx in flows:
            for H, hd in splits:
                variants.append((f'library  {flow:<8} H={H} hd={hd} waves {nw}', f'{flow} waves {nw}', hd, lib_variant(flow, dtype, ctx, H, 0.0, nw)))
                if args.dropout:
                    variants.append((f'library  {flow:<8} H={H} hd={hd} dropout {args.dropout} waves {nw}', f'{flow} drop waves {nw}', hd,
                                     lib_variant(flow, dtype, ctx, H, args.dropout, nw)))
    sdpa_tag = f' dropout {args.dropout}' if args.dropout else ''
    if not args.no_sdpa:
        for flow, dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
            for H, hd in splits:
                variants.append((f'torch sdpa per scene {flow:<4} H={H} hd={hd}{sdpa_tag}', 'sdpa ' + flow, hd, sdpa_variant(dtype, H)))
    fwd = {v[0]: [] for v in variants}
    bwd = {v[0]: [] for v in variants}
    for it in range(args.warmup + args.reps):
        for name, _, _, run in variants:
            ef, eb = run()
            torch.cuda.synchronize()
            if it >= args.warmup:
                fwd[name].append(ef[0].elapsed_time(ef[1]))
                bwd[name].append(eb[0].elapsed_time(eb[1]))

    def q(xs, f):
        xs = sorted(xs)
        return xs[min(len(xs) - 1, int(f * len(xs)))]

    def cell(xs, flops):
        m = statistics.median(xs)
        return f'{m:8.4f} | {q(xs, 0.1):8.4f} | {q(xs, 0.9):8.4f} ms  {flops / m * 1e-9:7.1f} TFLOP/s'
    ff, fb = 4.0 * B * n * n * D, 10.0 * B * n * n * D
    lines = [f'varlen attention, {B} scenes x {n} queries, D = {D}: {ff * 1e-9:.1f} GFLOP forward, {fb * 1e-9:.1f} GFLOP backward (algorithmic, the same for every head split); '
             f'{torch.cuda.get_device_name(0)}; {args.warmup} warm-up + {args.reps} timed rounds, variants alternating inside a round',
             'device ms between HIP events around one call (issued behind a queued GEMM: execution, not issue): median | p10 | p90, algorithmic TFLOP/s at the median', '']
    for name, _, _, _ in variants:
        lines.append(f'{name:<52} fwd {cell(fwd[name], ff)}   bwd {cell(bwd[name], fb)}')
    lines.append('')
    lines.append('head_dim 64 over head_dim 32 of the same flow (medians; p90 / p10 of each variant above is the noise to read it against)')
    by = {}
    for name, flow, hd, _ in variants:
        by.setdefault(flow, {})[hd] = name
    for flow, d in by.items():
        lines.append(f'{flow:<10} fwd {statistics.median(fwd[d[64]]) / statistics.median(fwd[d[32]]):.3f}   bwd {statistics.median(bwd[d[64]]) / statistics.median(bwd[d[32]]):.3f}')
    if args.dropout:
        med = statistics.median
        lines += ['', f'dropout {args.dropout}: the `_drop` kernels over the p = 0 kernels of the same flow and head dim | over torch sdpa per scene with dropout_p = '
                      f'{args.dropout} (fp32 and bf16 ops beside torch fp32, bf16 beside torch bf16); medians']
        for flow, _, _ in flows:
            for _, hd in splits:
                d, z = by[flow + ' drop'][hd], by[flow][hd]
                line = f'{flow:<10} hd={hd}  fwd {med(fwd[d]) / med(fwd[z]):.3f}   bwd {med(bwd[d]) / med(bwd[z]):.3f}'
                s = by.get('sdpa ' + ('bf16' if flow == 'bf16' else 'fp32'))
                if s:
                    line += f'   | over torch  fwd {med(fwd[d]) / med(fwd[s[hd]]):.3f}   bwd {med(bwd[d]) / med(bwd[s[hd]]):.3f}'
                lines.append(line)
    if len(waves) > 1:
        med = statistics.median
        lines += ['', f'tile waves: each forced form over waves {waves[0]} of the same flow and head dim (medians, with the (max - min) / median of the '
                      f'waves {waves[0]} samples: a form is ahead only by more than that)']
        for tag in [f for f, _, _ in flows] + ([f + ' drop' for f, _, _ in flows] if args.dropout else []):
            for _, hd in splits:
                z = by[f'{tag} waves {waves[0]}'][hd]
                line = f'{tag:<14} hd={hd}  spread fwd {(max(fwd[z]) - min(fwd[z])) / med(fwd[z]):.3f} bwd {(max(bwd[z]) - min(bwd[z])) / med(bwd[z]):.3f}'
                for nw in waves[1:]:
                    d = by[f'{tag} waves {nw}'][hd]
                    line += f'   | waves {nw}: fwd {med(fwd[d]) / med(fwd[z]):.3f}  bwd {med(bwd[d]) / med(bwd[z]):.3f}'
                lines.append(line)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
