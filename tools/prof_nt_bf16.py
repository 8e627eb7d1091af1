"""Kernel time of the fp32-tensor bf16-operand NT route (dense.BF16.nt: u3d_linear_act with U3D_BF16_OPERANDS) next to a control that
no change of that route touches (dense16.gemm_nt on the same fp32 tensors: gemm_nt_b16_k on its own tile), per decoder shape.
A product of a few microseconds is launch-bound when it is timed from the host, and the host's cost per launch differs from process to
process, so an A/B of two builds needs the kernels' own durations:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/prof_nt_bf16.py [M ...]
    python tools/prof_nt_bf16.py --parse DIR/**/*kernel_trace.csv        (needs no GPU)
The run launches, per (M, N, K) in a fixed order, WARM + REPS times the route and then WARM + REPS times the control; --parse takes the
gemm_nt_* dispatches of the trace in that order and prints the median duration of each group's last REPS.  Without rocprofv3 the run
still prints event times of both columns (launch-bound below ~10 us: compare the route MINUS the control of the same process)."""
import csv
import os
import statistics
import sys

SHAPES = [(256, 256), (768, 256), (1024, 256), (256, 1024), (256, 32)]
MS = [24600, 2048]
WARM, REPS = 3, 50


def groups(ms):
    return [(M, N, K, col) for M in ms for (N, K) in SHAPES for col in ('route', 'control')]


def parse(paths, ms):
    rows = []
    for p in paths:
        with open(p, newline='') as f:
            for r in csv.DictReader(f):
                if 'gemm_nt_' in r['Kernel_Name']:
                    rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    rows.sort()
    per = WARM + REPS
    want = groups(ms)
    assert len(rows) == per * len(want), f'{len(rows)} gemm_nt dispatches in the trace, expected {per * len(want)}'
    for i, (M, N, K, col) in enumerate(want):
        g = rows[i * per + WARM:(i + 1) * per]
        assert len({n for _, _, n in g}) == 1, 'a group of launches ran more than one kernel'
        d = [(e - s) * 1e-3 for s, e, _ in g]
        print(f'M={M} N={N} K={K} {col} {statistics.median(d):.2f} us  {g[0][2].split("(")[0][:70]}')


def run(ms):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from unidet3d_amd import dense16 as D16
    from unidet3d_amd import precision as P
    from unidet3d_amd.dense import BF16
    dev = torch.device('cuda:0')
    for M in ms:
        for (N, K) in SHAPES:
            a = torch.randn(M, K, device=dev); w = torch.randn(N, K, device=dev); b = torch.randn(N, device=dev)
            out = []
            for f in (lambda: BF16.nt(a, w, b), lambda: D16.gemm_nt(a, w, b)):
                with P.operands('bf16'):
                    for _ in range(WARM):
                        f()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(REPS):
                        f()
                    e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) * 1e3 / REPS)
            print(f'M={M} N={N} K={K} event us per launch: route {out[0]:.1f} control {out[1]:.1f}', flush=True)


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--parse':
        paths = [a for a in args[1:] if not a.isdigit()]
        parse(paths, [int(a) for a in args[1:] if a.isdigit()] or MS)
    else:
        run([int(a) for a in args] or MS)
