"""Bit fingerprints of the fp32-tensor bf16-operand GEMM routes (dense.BF16): one sha256 per result, from inputs a CPU generator with
fixed seeds makes.  Run it before and after a change that must not move a bit and compare the outputs line for line.
    python tools/gemm_bits.py
Covered: BF16.nt with the bias, addend, ReLU-mask and GELU-mask (u3d_linear_dact) epilogues, BF16.relu_nt, BF16.ffn with GELU (the
GELU epilogue with its pre-activation), BF16.tn with and without the column sums (row splits S > 1 at these M)."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unidet3d_amd import dense as D                      # noqa: E402
from unidet3d_amd import precision as P                  # noqa: E402

DEV = torch.device('cuda:0')
SHAPES = [(333, 256, 32, 256), (1000, 768, 256, 768), (4097, 256, 1024, 256), (2500, 32, 256, 19)]      # M, N, K, live rows of W (N = 19 padded to 32)


def sha(t):
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    for M, N, K, live in SHAPES:
        g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) * 0.1
        b = torch.randn(N, generator=g)
        w2 = torch.randn(K, N, generator=g) * 0.1
        b2 = torch.randn(K, generator=g)
        aux = torch.randn(M, N, generator=g)
        dy = torch.randn(M, N, generator=g)
        w[live:] = 0; b[live:] = 0; w2[:, live:] = 0; dy[:, live:] = 0
        x, w, b, w2, b2, aux, dy = [t.to(DEV) for t in (x, w, b, w2, b2, aux, dy)]
        out = {}
        with P.operands('bf16'):
            F = D.BF16
            out['nt bias'] = F.nt(x, w, b)
            out['nt add'] = F.nt(x, w, None, D.EPI_ADD, aux)
            out['nt relu-mask'] = F.nt(x, w, None, D.EPI_RELU_MASK, torch.relu(aux))
            out['nt gelu-mask'] = F.nt(x, w, None, D.EPI_GELU_MASK, aux)
            out['relu_nt'] = F.relu_nt(x, w, b)
            h, a, z = F.ffn(x, w, b, w2, b2, D.ACT_GELU, None, None)
            out['ffn gelu pre'], out['ffn gelu act'], out['ffn gelu out'] = h, a, z
            dw, db = F.tn(dy, x, True)
            out['tn dw'], out['tn colsum'] = dw, db
            out['tn dw (no colsum)'] = F.tn(dy, x, False)[0]
        torch.cuda.synchronize()
        for k, v in out.items():
            print(f'M={M} N={N} K={K} {k}: {sha(v)}', flush=True)


if __name__ == '__main__':
    main()
