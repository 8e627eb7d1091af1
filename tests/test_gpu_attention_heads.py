"""head_dim 64 in the varlen flash attention kernels (csrc/attn_x3.hip at HD = 64), forward and backward, in the three data flows of the default
and the bf16 configurations: fp32 tensors with three bf16 planes per operand, fp32 tensors with bf16 operands, bf16 tensors.

Kernel tests against float64 softmax attention per scene and its autograd (the reference of tests/test_gpu_model.py
test_attention_varlen_fwd_bwd, at that test's bounds), with the head_dim 32 kernels run on the same tensors beside them; row isolation
between scenes and run-to-run determinism bit for bit; and the whole decoder at d_model / num_heads = 64 against fixtures generated from the
reference's own encoder.py (tools/gen_golden_encoder_heads.py)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from _detw import fill_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENS = [[48, 17], [1, 64, 65, 130], [0, 5, 0, 700], [513, 300]]          # | tile edges, a one-row scene | empty scenes | nine key tiles
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'encoder_heads_golden.npz'))
CLASSES = ['cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf', 'picture', 'counter', 'desk',
           'curtain', 'refrigerator', 'showercurtrain', 'toilet', 'sink', 'bathtub', 'otherfurniture']
CLASSES_B = ['table', 'chair', 'sofa', 'bookcase', 'board']


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12)) if a.numel() else 0.0


def _rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _inputs(lens, D, qk_scale=1.0, bf16_values=False):
    """(qkv [n, 3 D], dout [n, D]) on the CPU, the same for every head split of D; q and k scaled by ``qk_scale``"""
    n = sum(lens)
    g = torch.Generator().manual_seed(n + (1 if bf16_values else 0))
    qkv = torch.randn(n, 3 * D, generator=g) * (1.0 if bf16_values else 1.5)
    go = torch.randn(n, D, generator=g)
    qkv[:, :2 * D] *= qk_scale
    return (_rb(qkv), _rb(go)) if bf16_values else (qkv, go)


@functools.lru_cache(maxsize=None)
def _ref64(lens, H, hd, qk_scale=1.0, bf16_values=False):
    """float64 softmax attention per scene and its autograd: (out, dqkv)"""
    qkv, go = _inputs(lens, H * hd, qk_scale, bf16_values)
    ref_in = qkv.clone().double().requires_grad_()
    outs, o = [], 0
    for ln in lens:
        x = ref_in[o:o + ln]; o += ln
        q, k, v = x.chunk(3, -1)
        q = q.view(ln, H, hd).transpose(0, 1); k = k.view(ln, H, hd).transpose(0, 1); v = v.view(ln, H, hd).transpose(0, 1)
        a = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), -1)
        outs.append((a @ v).transpose(0, 1).reshape(ln, H * hd))
    ref = torch.cat(outs); ref.backward(go.double())
    return ref.detach(), ref_in.grad


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)


def _run(qkv, go, lens, H, dtype=torch.float32):
    """forward + backward of the product's attention: (out, dqkv)"""
    from unidet3d_amd.encoder import attention_varlen
    x = qkv.clone().to(dtype).to(DEV).requires_grad_()
    out = attention_varlen(x, _cu(lens), max(lens), H)
    out.backward(go.to(dtype).to(DEV))
    return out.detach(), x.grad


def _errors(lens, H, hd, qk_scale=1.0):
    qkv, go = _inputs(tuple(lens), H * hd, qk_scale)
    ref, dref = _ref64(tuple(lens), H, hd, qk_scale)
    out, dqkv = _run(qkv, go, lens, H)
    return _rel(out, ref), _rel(dqkv, dref)


@pytest.mark.parametrize('lens', LENS)
def test_head_dim_64_fp32_against_float64(lens):
    """The default fp32 path (three exact bf16 planes per operand) at H, hd = 4, 64 against float64, at the bounds the kernel family has at
    head_dim 32 -- and H, hd = 8, 32 on the same tensor beside it."""
    import _parity as PA
    from unidet3d_amd import precision as P
    assert not P.bf16() and P.get_fp32_math() == 'bf16x3'
    e64 = _errors(lens, 4, 64)
    e32 = _errors(lens, 8, 32)
    PA.log_errors(f'attention_hd64_{sum(lens)}', dict(out=e64[0], dqkv=e64[1]))
    PA.log_errors(f'attention_hd32_same_tensor_{sum(lens)}', dict(out=e32[0], dqkv=e32[1]))
    print('attention', lens, 'rel err out / dqkv vs float64: hd 64', e64, '| hd 32', e32)
    assert e32[0] < 5e-6 and e32[1] < 2e-5, e32
    assert e64[0] < 5e-6 and e64[1] < 2e-5, e64


@pytest.mark.parametrize('H', [2, 8])
def test_head_dim_64_at_other_widths(H):
    """d = 128 and d = 512: the head stride h * 64 and the row strides D, 3 D"""
    lens = [1, 64, 65, 130]
    e = _errors(lens, H, 64)
    print('attention hd 64, H =', H, 'rel err out / dqkv vs float64:', e)
    assert e[0] < 5e-6 and e[1] < 2e-5, e


def test_head_dim_64_on_peaked_softmax_is_as_accurate_as_head_dim_32():
    """q and k four times larger: logits reach tens, rows are near one-hot.  No project bound exists for this input, so the head_dim 32
    kernels on the same tensor are the yardstick: the reduction depth of S and dP doubled, the error may at most double."""
    import _parity as PA
    lens = [1, 64, 65, 130]
    e64 = _errors(lens, 4, 64, qk_scale=4.0)
    e32 = _errors(lens, 8, 32, qk_scale=4.0)
    PA.log_errors('attention_peaked_hd64', dict(out=e64[0], dqkv=e64[1]))
    PA.log_errors('attention_peaked_hd32', dict(out=e32[0], dqkv=e32[1]))
    print('attention, peaked softmax: rel err out / dqkv vs float64: hd 64', e64, '| hd 32', e32)
    assert e64[0] <= 2 * e32[0] and e64[1] <= 2 * e32[1], (e64, e32)


@pytest.mark.parametrize('lens', LENS)
def test_head_dim_64_bf16_operands_and_bf16_tensors(lens):
    """H, hd = 4, 64 with bf16 operands on fp32 tensors (precision.operands('bf16')) and on bf16 tensors, against float64 attention of the
    same bf16-valued inputs at the bounds of tests/test_gpu_bf16.py test_attention_on_bf16_tensors, and against each other."""
    from unidet3d_amd import precision as P
    H, hd = 4, 64
    qkv, go = _inputs(tuple(lens), H * hd, 1.0, True)
    ref, dref = _ref64(tuple(lens), H, hd, 1.0, True)
    with P.operands('bf16'):
        outf, dxf = _run(qkv, go, lens, H)                               # fp32 tensors, bf16 operands
    out, dx = _run(qkv, go, lens, H, torch.bfloat16)                     # bf16 tensors
    assert outf.dtype == torch.float32 and dxf.dtype == torch.float32
    assert out.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16
    ef = _rel(outf, ref), _rel(dxf, dref)
    eb = _rel(out.float(), ref), _rel(dx.float(), dref)
    print(f'attention hd 64 lens={lens}: bf16 operands out {ef[0]:.2e} grad {ef[1]:.2e} | bf16 tensors out {eb[0]:.2e} grad {eb[1]:.2e}')
    assert ef[0] < 2e-2 and ef[1] < 3e-2, ef
    assert eb[0] < 2e-2 and eb[1] < 3e-2, eb
    assert _rel(out.float(), outf) < 1.5e-2 and _rel(dx.float(), dxf) < 2e-2
    assert float((outf.double().cpu() - ref).abs().mean() / ref.abs().mean()) < 1e-2
    assert float((out.double().cpu() - ref).abs().mean() / ref.abs().mean()) < 1e-2


@pytest.mark.parametrize('H, hd', [(8, 32), (4, 64)])
@pytest.mark.parametrize('mode', ['fp32', 'bf16_operands', 'bf16_tensors'])
def test_scenes_do_not_read_each_other(mode, H, hd):
    """Scene 1's rows of qkv and dout hold 1e30: scene 0's out and dqkv must be bit-equal to a run with scene 1 removed -- no key tile and
    no transpose read crosses a scene boundary at either row width."""
    import contextlib
    from unidet3d_amd import precision as P
    lens = [64, 65]
    qkv, go = _inputs(tuple(lens), H * hd, 1.0, mode != 'fp32')
    qkv, go = qkv.clone(), go.clone()
    qkv[64:] = 1e30; go[64:] = 1e30
    dtype = torch.bfloat16 if mode == 'bf16_tensors' else torch.float32
    with (P.operands('bf16') if mode == 'bf16_operands' else contextlib.nullcontext()):
        out2, dx2 = _run(qkv, go, lens, H, dtype)
        out1, dx1 = _run(qkv[:64], go[:64], [64], H, dtype)
    assert torch.isfinite(out1).all() and torch.isfinite(dx1).all()
    assert torch.equal(out2[:64], out1) and torch.equal(dx2[:64], dx1)


@pytest.mark.parametrize('H, hd', [(8, 32), (4, 64)])
def test_attention_is_deterministic(H, hd):
    """two forward + backward passes, bit-equal: no floating-point atomics"""
    lens = [513, 300]
    qkv, go = _inputs(tuple(lens), H * hd)
    a, b = _run(qkv, go, lens, H), _run(qkv, go, lens, H)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------- the decoder against the reference's own encoder.py
CFG_H4 = dict(num_layers=2, datasets_classes=[CLASSES], in_channels=32, d_model=256, num_heads=4, hidden_dim=1024,
              dropout=0.0, activation_fn='gelu', datasets=['scannet'], angles=[False])
CFG_H2 = dict(num_layers=2, datasets_classes=[CLASSES, CLASSES_B], in_channels=32, d_model=128, num_heads=2, hidden_dim=256,
              dropout=0.0, activation_fn='gelu', datasets=['scannet', 's3dis'], angles=[False, True])


def _run_h4(m):
    m.zero_grad(set_to_none=True)
    x = [torch.from_numpy(G[f'H4.x{i}']).to(DEV).requires_grad_() for i in range(2)]
    c = [torch.from_numpy(G[f'H4.c{i}']).to(DEV) for i in range(2)]
    res = m(x, c, ['scannet', 'scannet'])
    loss = sum((t ** 2).sum() for t in res['cls_preds']) + sum(t.sum() for t in res['bboxes'])
    for a in res['aux_outputs']:
        loss = loss + sum((t * 0.5).sum() for t in a['cls_preds']) + sum((t ** 2).sum() for t in a['bboxes'])
    loss.backward()
    return res, x, loss


def test_decoder_with_four_heads_of_64_matches_reference_golden():
    from unidet3d_amd.encoder import UniDet3DEncoder
    m = fill_state_dict(UniDet3DEncoder(**CFG_H4), tag0=1100).to(DEV)
    res, x, loss = _run_h4(m)
    for i in range(2):
        assert _rel(res['cls_preds'][i], G[f'H4.cls{i}']) < 1e-3
        assert _rel(res['bboxes'][i], G[f'H4.box{i}']) < 1e-3
        assert _rel(x[i].grad, G[f'H4.gx{i}']) < 1e-3
        for l, a in enumerate(res['aux_outputs']):
            assert _rel(a['cls_preds'][i], G[f'H4.aux{l}.cls{i}']) < 1e-3
            assert _rel(a['bboxes'][i], G[f'H4.aux{l}.box{i}']) < 1e-3
    assert abs(loss.item() - float(G['H4.loss'])) < 1e-3 * abs(float(G['H4.loss']))
    gp = dict(m.named_parameters())
    rows = [k for k in G.files if k.startswith('H4.g.')]
    assert len(rows) == 7
    for k in rows:
        assert _rel(gp[k[5:]].grad[:8], G[k]) < 2e-3, k


def test_decoder_with_two_heads_of_64_mixed_batch_and_empty_scene_matches_reference_golden():
    from unidet3d_amd.encoder import UniDet3DEncoder
    m = fill_state_dict(UniDet3DEncoder(**CFG_H2), tag0=1700).to(DEV)
    x = [torch.from_numpy(G[f'H2.x{i}']).to(DEV) for i in range(3)]
    c = [torch.from_numpy(G[f'H2.c{i}']).to(DEV) for i in range(3)]
    assert [t.shape[0] for t in x] == [9, 70, 0]
    with torch.no_grad():
        res = m(x, c, ['s3dis', 'scannet', 's3dis'])
    for i in range(3):
        assert res['cls_preds'][i].shape == G[f'H2.cls{i}'].shape and res['bboxes'][i].shape == G[f'H2.box{i}'].shape
        assert _rel(res['cls_preds'][i], G[f'H2.cls{i}']) < 1e-3
        assert _rel(res['bboxes'][i], G[f'H2.box{i}']) < 1e-3


def test_decoder_with_four_heads_of_64_on_bf16_activations_matches_reference_golden_at_bf16_tolerance():
    """case H4 under precision.operands('bf16') with bf16 activations in HBM (u3d_attn_varlen_*_b16 at head_dim 64), at the bounds of the
    bf16 decoder golden test of tests/test_gpu_bf16.py"""
    from unidet3d_amd import precision as P
    from unidet3d_amd.encoder import UniDet3DEncoder
    m = fill_state_dict(UniDet3DEncoder(**CFG_H4), tag0=1100).to(DEV)
    with P.operands('bf16'), P.bf16_act_mode(True):
        res, x, loss = _run_h4(m)
    e = dict(cls=max(_rel(res['cls_preds'][i], G[f'H4.cls{i}']) for i in range(2)), box=max(_rel(res['bboxes'][i], G[f'H4.box{i}']) for i in range(2)),
             gx=max(_rel(x[i].grad, G[f'H4.gx{i}']) for i in range(2)), loss=abs(loss.item() - float(G['H4.loss'])) / abs(float(G['H4.loss'])))
    print('decoder H4, bf16 activations vs reference fixtures:', {k: f'{v:.1e}' for k, v in e.items()})
    for i in range(2):
        assert res['cls_preds'][i].dtype == torch.float32 and res['bboxes'][i].dtype == torch.float32
    assert e['cls'] < 5e-2 and e['box'] < 5e-2 and e['gx'] < 1e-1 and e['loss'] < 2e-2, e
