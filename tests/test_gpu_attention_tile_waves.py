"""Tile waves of the plane attention kernels (csrc/attn_x3.hip, DESIGN 4.2 "tile waves"): NW waves of 16 query (dK / dV: key) rows share a
workgroup and every 64-row tile it stages.  A wave runs the same program whatever NW is, so the forms forced through
precision.attn_tile_waves must agree BIT FOR BIT with NW = 4 -- out, lse and dqkv, in the three data flows, with and without dropout -- at the
scene lengths where a wave of a wide tile has no rows, a tile is exactly full, one row spills into a new tile and a scene is empty.  Beside
that: each forced form against float64 attention at the bounds of tests/test_gpu_attention_heads.py, and scene isolation per form."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H = 2
FORMS = (8,)            # the wide forms csrc/attn_x3.hip instantiates (attn_x3_by_waves; a six-wave form measured slower and was removed); 4 is
                        # the form they are compared with
# 64-row edges | 96-row edges (a 128-row tile whose last two waves have no rows, then one row) | 128-row edges (NW = 8) | edges of both at the second tile | empty scenes, eleven key tiles | short scenes
LAYOUTS = ((1, 63, 64, 65), (95, 96, 97), (127, 128, 129), (191, 192, 193), (0, 5, 0, 700), (48, 17))
FLOWS = ('fp32', 'bf16_operands', 'bf16_tensors')
KEY = (1234, 5)


@functools.lru_cache(maxsize=None)
def _inputs(lens, D, bf16_values):
    n = sum(lens)
    g = torch.Generator().manual_seed(n + (1 if bf16_values else 0))
    qkv = torch.randn(n, 3 * D, generator=g) * (1.0 if bf16_values else 1.5)
    go = torch.randn(n, D, generator=g)
    if bf16_values:
        qkv, go = qkv.to(torch.bfloat16).float(), go.to(torch.bfloat16).float()
    return qkv, go


@functools.lru_cache(maxsize=None)
def _ref64(lens, hd, bf16_values):
    """float64 softmax attention per scene and its autograd: (out, dqkv)"""
    qkv, go = _inputs(lens, H * hd, bf16_values)
    ref_in = qkv.clone().double().requires_grad_()
    outs, o = [], 0
    for ln in lens:
        x = ref_in[o:o + ln]; o += ln
        q, k, v = [t.view(ln, H, hd).transpose(0, 1) for t in x.chunk(3, -1)]
        a = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), -1)
        outs.append((a @ v).transpose(0, 1).reshape(ln, H * hd))
    ref = torch.cat(outs); ref.backward(go.double())
    return ref.detach(), ref_in.grad


def _run(qkv, go, lens, flow, p, nw):
    """forward + backward of the product's attention with the form `nw` forced: (out, lse, dqkv)"""
    from unidet3d_amd import precision as P
    from unidet3d_amd.encoder import attention_varlen
    dtype = torch.bfloat16 if flow == 'bf16_tensors' else torch.float32
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    x = qkv.clone().to(dtype).to(DEV).requires_grad_()
    with P.attn_tile_waves(nw), (P.operands('bf16') if flow == 'bf16_operands' else contextlib.nullcontext()):
        out = attention_varlen(x, cu, max(lens), H, 0, p, KEY)
        lse = out.grad_fn.saved_tensors[2]
        out.backward(go.to(dtype).to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), lse.detach().cpu(), x.grad.cpu()


@functools.lru_cache(maxsize=None)
def _result(lens, hd, flow, p, nw):
    qkv, go = _inputs(lens, H * hd, flow != 'fp32')
    return _run(qkv, go, lens, flow, p, nw)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12)) if a.numel() else 0.0


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('flow', FLOWS)
@pytest.mark.parametrize('nw', FORMS)
def test_wide_forms_give_the_bits_of_four_waves(nw, flow, hd, p):
    for lens in LAYOUTS:
        base, wide = _result(lens, hd, flow, p, 4), _result(lens, hd, flow, p, nw)
        assert torch.isfinite(base[0].float()).all() and torch.isfinite(base[2].float()).all(), lens
        for name, a, b in zip(('out', 'lse', 'dqkv'), wide, base):
            assert _same_bits(a, b), f'{name} of NW = {nw} differs from NW = 4 at lens = {lens}'


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('nw', (4,) + FORMS)
def test_forced_form_fp32_against_float64(nw, hd):
    for lens in LAYOUTS:
        ref, dref = _ref64(lens, hd, False)
        out, _, dqkv = _result(lens, hd, 'fp32', 0.0, nw)
        e = _rel(out, ref), _rel(dqkv, dref)
        print(f'attention NW = {nw} hd = {hd} lens = {lens}: rel err out / dqkv vs float64', e)
        assert e[0] < 5e-6 and e[1] < 2e-5, (lens, e)


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('flow', FLOWS[1:])
@pytest.mark.parametrize('nw', (4,) + FORMS)
def test_forced_form_bf16_against_float64(nw, flow, hd):
    for lens in LAYOUTS:
        ref, dref = _ref64(lens, hd, True)
        out, _, dqkv = _result(lens, hd, flow, 0.0, nw)
        e = _rel(out.float(), ref), _rel(dqkv.float(), dref)
        print(f'attention NW = {nw} {flow} hd = {hd} lens = {lens}: rel err out / dqkv vs float64', e)
        assert e[0] < 2e-2 and e[1] < 3e-2, (lens, e)


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('flow', FLOWS)
@pytest.mark.parametrize('nw', (4,) + FORMS)
def test_scenes_do_not_read_each_other(nw, flow, hd):
    """Scene 1's rows of qkv and dout hold 1e30: scene 0's out, lse and dqkv are bit-equal to a run with scene 1 removed.  100 rows: the
    scene ends inside the second 64-row key tile and inside the first tile of either wide form, whose last waves hold scene 0's last rows
    and none of scene 1's."""
    lens = (100, 65)
    qkv, go = [t.clone() for t in _inputs(lens, H * hd, flow != 'fp32')]
    qkv[100:] = 1e30; go[100:] = 1e30
    for p in (0.0, 0.1):
        out2, lse2, dx2 = _run(qkv, go, lens, flow, p, nw)
        out1, lse1, dx1 = _run(qkv[:100], go[:100], (100,), flow, p, nw)
        assert torch.isfinite(out1.float()).all() and torch.isfinite(dx1.float()).all()
        assert _same_bits(out2[:100], out1) and _same_bits(lse2[:, :100].contiguous(), lse1) and _same_bits(dx2[:100], dx1), p
