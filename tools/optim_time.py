"""Time the optimizer tail of a training step on the cfg2 model's real parameter list, random gradients:

  (a) the torch tail of bench.py's step: FlatGradBucket.pack() + clip_grad_norm_(10) + torch.optim.AdamW(fused=True).step()
  (b) FlatGradBucket.pack() + FlatAdamW.step()          (gradients are views of the flat buffer: what an N-GPU loop has after the all-reduce)
  (c) FlatAdamW.step() on the fresh gradient tensors     (a one-GPU loop: no pack())

Every variant owns a copy of the parameters and sees the same gradient tensors, re-attached before every repetition the way a backward
pass leaves them (fresh tensors).  Device time: HIP events around one tail that is issued while the GPU still works on two queued GEMMs
(the bench step's host runs ahead of its GPU, so what a tail costs there is its execution, not its issue), the variants alternating inside every round (other work
shares the host; a difference is read against the spread of the same variant); host time: wall clock of issuing the tail.  Native
launches are counted from the ``_lib.call`` log; torch's own launches are not visible there (DESIGN.md 4.20 cites the kernel trace).

    python tools/optim_time.py [--reps 200] [--warmup 20] [--out profiles/optim_step_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('optim_time.py measures on the GPU: no device, no number')
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd import FlatAdamW
    from unidet3d_amd import _lib as L
    from unidet3d_amd.config import build_model, scannet_model_cfg
    from unidet3d_amd.dist import FlatGradBucket
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = build_model(scannet_model_cfg()).to(dev)
    base = [p.detach() for p in model.parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(p.shape, device=dev, generator=gen) * 0.01 for p in base]
    n_el = sum(p.numel() for p in base)

    spin = torch.randn(4096, 4096, device=dev)

    def copies():
        return [torch.nn.Parameter(p.clone()) for p in base]

    log, real = [], L.call

    def call(name, *a):
        log.append(name)
        return real(name, *a)
    L.call = call

    pa, pb, pc = copies(), copies(), copies()
    ba, bb = FlatGradBucket(pa, attach=False), FlatGradBucket(pb, attach=False)
    oa = torch.optim.AdamW(pa, lr=2e-4, weight_decay=0.05, fused=True)
    ob = FlatAdamW(pb, lr=2e-4, weight_decay=0.05, max_norm=10.0, bucket=bb)
    oc = FlatAdamW(pc, lr=2e-4, weight_decay=0.05, max_norm=10.0)

    def attach(params):
        for p, g in zip(params, grads):
            p.grad = g

    def tail_a():
        ba.pack()
        ba.clip_grad_norm_(10.0)
        oa.step()

    def tail_b():
        bb.pack()
        ob.step()

    def tail_c():
        oc.step()

    variants = [('(a) pack + clip_grad_norm_ + AdamW(fused=True)', pa, tail_a), ('(b) pack + FlatAdamW.step()', pb, tail_b),
                ('(c) FlatAdamW.step(), fresh gradients', pc, tail_c)]
    dev_ms = {name: [] for name, _, _ in variants}
    host_ms = {name: [] for name, _, _ in variants}
    calls = {}
    for it in range(args.warmup + args.reps):
        for name, params, tail in variants:
            attach(params)
            torch.cuda.synchronize()
            del log[:]
            spin @ spin                      # ~1 ms of queued work: the tail is issued while the GPU is busy, as in the bench step
            spin @ spin
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            tail()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if it >= args.warmup:
                dev_ms[name].append(e0.elapsed_time(e1))
                host_ms[name].append((t1 - t0) * 1e3)
                calls[name] = list(log)

    def q(xs, f):
        xs = sorted(xs)
        return xs[min(len(xs) - 1, int(f * len(xs)))]
    lines = [f'optimizer tail, cfg2 model: {len(base)} parameter tensors, {n_el} elements; {torch.cuda.get_device_name(0)}; '
             f'{args.warmup} warm-up + {args.reps} timed rounds, variants alternating inside a round, each tail issued behind two queued 4096^3 GEMMs (the host runs ahead, as in the bench step)',
             'device ms between HIP events around one tail (median | p10 | p90), host ms to issue it (median), native launches (_lib.call log), table uploads',
             '']
    for name, _, _ in variants:
        d, h = dev_ms[name], host_ms[name]
        up = {'(a)': '-', '(b)': str(ob.uploads), '(c)': str(oc.uploads)}[name[:3]]
        lines.append(f'{name:<50} device {statistics.median(d):.4f} | {q(d, 0.1):.4f} | {q(d, 0.9):.4f}   host {statistics.median(h):.4f}   '
                     f'native launches {len(calls[name])} {sorted(set(calls[name]))}   uploads {up}')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
