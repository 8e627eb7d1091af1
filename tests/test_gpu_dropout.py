"""Decoder dropout on the device: the mask function of csrc/dropout.h pinned to its numpy restatement (tests/_dropout.py); the
DROP instantiations of the varlen flash attention kernels, forward and backward, in the three data flows and at both head widths against
float64 attention with the dumped mask; p = 0 through the `_drop` entry points bit-equal to the entry points without dropout; heavy
dropout (all-dropped rows); isolation between scenes and determinism; the elementwise kernels; and the whole decoder in training mode
against a float64 restatement of the reference's layer order (unidet3d/encoder.py:19-22,38,55-61) that fetches every mask through
``dropout_key`` and the two mask ops."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import _dropout as DR
from _detw import fill_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P_DROP = 0.1
KEY = (0x5DEECE66D, 7)
BIG_KEY = ((1 << 63) + 12345, (1 << 40) + 3)              # a seed and an offset above 2^32
LENS = [[1, 64, 65, 130], [0, 5, 0, 700], [48, 17]]       # a one-row scene, tile edges on both sides | empty scenes, eleven key tiles | small
HEADS = [(4, 64), (8, 32)]
MODES = ['fp32', 'bf16_operands', 'bf16_tensors']
CLASSES = ['cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf', 'picture', 'counter', 'desk',
           'curtain', 'refrigerator', 'showercurtrain', 'toilet', 'sink', 'bathtub', 'otherfurniture']


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12)) if a.numel() else 0.0


def _rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)


def _mode_ctx(mode):
    from unidet3d_amd import precision as P
    return P.operands('bf16') if mode == 'bf16_operands' else contextlib.nullcontext()


# ------------------------------------------------------------------------------------------------------------------ the hash, pinned
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_attention_mask_equals_the_numpy_restatement(p):
    from unidet3d_amd import ops
    m = ops.dropout_mask_attn(p, KEY[0], KEY[1], 2, 260, DEV).cpu().numpy()
    assert np.array_equal(m, DR.mask_attn(p, KEY[0], KEY[1], 2, 260))


@pytest.mark.parametrize('key', [KEY, BIG_KEY])
def test_rows_mask_equals_the_numpy_restatement(key):
    from unidet3d_amd import ops
    m = ops.dropout_mask_rows(P_DROP, key[0], key[1], 257, 1024, DEV).cpu().numpy()
    assert np.array_equal(m, DR.mask_rows(P_DROP, key[0], key[1], 257, 1024))
    m = ops.dropout_mask_attn(P_DROP, key[0], key[1], 3, 70, DEV).cpu().numpy()
    assert np.array_equal(m, DR.mask_attn(P_DROP, key[0], key[1], 3, 70))


# -------------------------------------------------------------------------------------------------- attention against float64 + mask
@functools.lru_cache(maxsize=None)
def _inputs(lens, D, bf16_values=False):
    """(qkv [n, 3 D], dout [n, D]) on the CPU, the same for every head split of D (the inputs of tests/test_gpu_attention_heads.py)"""
    n = sum(lens)
    g = torch.Generator().manual_seed(n + (1 if bf16_values else 0))
    qkv = torch.randn(n, 3 * D, generator=g) * (1.0 if bf16_values else 1.5)
    go = torch.randn(n, D, generator=g)
    return (_rb(qkv), _rb(go)) if bf16_values else (qkv, go)


@functools.lru_cache(maxsize=None)
def _mask(p, key, H, n):
    """the dumped mask [H, n, n] as float64 on the CPU"""
    from unidet3d_amd import ops
    return ops.dropout_mask_attn(p, key[0], key[1], H, n, DEV).cpu().double()


@functools.lru_cache(maxsize=None)
def _ref64(lens, H, hd, p, key, bf16_values=False):
    """float64 softmax attention per scene with a = softmax(...) * mask / (1 - p), and its autograd: (out, dqkv)"""
    qkv, go = _inputs(lens, H * hd, bf16_values)
    mask = _mask(p, key, H, sum(lens))
    ref_in = qkv.clone().double().requires_grad_()
    outs, o = [], 0
    for ln in lens:
        x = ref_in[o:o + ln]
        q, k, v = x.chunk(3, -1)
        q = q.view(ln, H, hd).transpose(0, 1); k = k.view(ln, H, hd).transpose(0, 1); v = v.view(ln, H, hd).transpose(0, 1)
        a = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), -1) * mask[:, o:o + ln, o:o + ln] / (1.0 - p)
        outs.append((a @ v).transpose(0, 1).reshape(ln, H * hd))
        o += ln
    ref = torch.cat(outs); ref.backward(go.double())
    return ref.detach(), ref_in.grad


def _run(qkv, go, lens, H, dtype=torch.float32, p=P_DROP, key=KEY):
    """forward + backward of the product's attention with dropout: (out, dqkv)"""
    from unidet3d_amd.encoder import attention_varlen
    x = qkv.clone().to(dtype).to(DEV).requires_grad_()
    out = attention_varlen(x, _cu(lens), max(lens), H, 0, p, key)
    out.backward(go.to(dtype).to(DEV))
    return out.detach(), x.grad


@pytest.mark.parametrize('H, hd', HEADS)
@pytest.mark.parametrize('lens', LENS)
@pytest.mark.parametrize('mode', MODES)
def test_attention_with_dropout_against_float64(mode, lens, H, hd):
    """Bounds: those of tests/test_gpu_attention_heads.py for the flow, on the same max-norm relative measure (dropout adds one rounding
    of 1 / (1 - p)).  A transposed or scene-local index in any one kernel is an error of order 1 here.  Measured on MI355X: DESIGN 4.24."""
    bf = mode != 'fp32'
    qkv, go = _inputs(tuple(lens), H * hd, bf)
    ref, dref = _ref64(tuple(lens), H, hd, P_DROP, KEY, bf)
    with _mode_ctx(mode):
        out, dx = _run(qkv, go, lens, H, torch.bfloat16 if mode == 'bf16_tensors' else torch.float32)
    e = _rel(out.float(), ref), _rel(dx.float(), dref)
    print(f'attention + dropout {mode} lens={lens} H={H} hd={hd}: rel err out {e[0]:.2e} dqkv {e[1]:.2e}')
    if bf:
        assert e[0] < 2e-2 and e[1] < 3e-2, e
    else:
        assert e[0] < 5e-6 and e[1] < 2e-5, e


# ---------------------------------------------------------------------------------------------------------- p = 0 and heavy dropout
def _raw(sfx, drop, qkv, go, lens, H, dtype):
    """the entry points called directly: (out, lse, dqkv); ``drop`` = None (the entry points without dropout) or (p, seed, offset)"""
    from unidet3d_amd import _lib as L
    x, g = qkv.to(dtype).to(DEV).contiguous(), go.to(dtype).to(DEV).contiguous()
    n, d = g.shape
    hd, cu, extra = d // H, _cu(lens), (() if drop is None else tuple(drop))
    name = '_drop' if drop is not None else ''
    out, lse = torch.empty_like(g), torch.empty(H, n, dtype=torch.float32, device=DEV)
    dx, delta = torch.empty_like(x), torch.empty(H, n, dtype=torch.float32, device=DEV)
    L.call(f'u3d_attn_varlen_fwd{name}{sfx}', L.ptr(x), L.ptr(cu), len(lens), max(lens), n, H, hd, 1.0 / math.sqrt(hd), L.ptr(out), L.ptr(lse), 0.0,
           L.stream(), *extra)
    L.call(f'u3d_attn_varlen_bwd{name}{sfx}', L.ptr(x), L.ptr(out), L.ptr(g), L.ptr(lse), L.ptr(cu), len(lens), max(lens), n, H, hd, 1.0 / math.sqrt(hd),
           L.ptr(dx), L.ptr(delta), 0.0, L.stream(), *extra)
    torch.cuda.synchronize()
    return out, lse, dx


@pytest.mark.parametrize('H, hd', HEADS)
@pytest.mark.parametrize('sfx', ['', '_bf16', '_b16'])
def test_zero_probability_through_the_drop_entry_points_is_todays_call(sfx, H, hd):
    lens = [1, 64, 65, 130]
    qkv, go = _inputs(tuple(lens), H * hd, sfx != '')
    dtype = torch.bfloat16 if sfx == '_b16' else torch.float32
    a = _raw(sfx, None, qkv, go, lens, H, dtype)
    b = _raw(sfx, (0.0, KEY[0], KEY[1]), qkv, go, lens, H, dtype)
    for x, y, what in zip(a, b, ('out', 'lse', 'dqkv')):
        assert torch.equal(x, y), what


@pytest.mark.parametrize('H, hd', HEADS)
def test_heavy_dropout_gives_zero_rows_finite_gradients_and_the_undropped_lse(H, hd):
    """p = 0.9: queries whose keys are all dropped exist (scene 0 has one key, scene 1 three); their output rows are exactly zero, the
    gradients are finite and those of the float64 reference, and lse -- from the undropped probabilities -- is the p = 0 lse bit for bit."""
    lens, p = [1, 3, 64], 0.9
    qkv, go = _inputs(tuple(lens), H * hd)
    mask = _mask(p, KEY, H, sum(lens))
    out, lse, dx = _raw('', (p, KEY[0], KEY[1]), qkv, go, lens, H, torch.float32)
    _, lse0, _ = _raw('', None, qkv, go, lens, H, torch.float32)
    assert torch.equal(lse, lse0)
    dead, o = [], 0
    for ln in lens:
        blk = mask[:, o:o + ln, o:o + ln].sum(-1)            # [H, ln] kept keys per (head, query)
        dead += [(h, o + i) for h in range(H) for i in range(ln) if blk[h, i] == 0]
        o += ln
    assert dead, 'no all-dropped row at p = 0.9: the case tests nothing'
    for h, row in dead:
        assert (out[row, h * hd:(h + 1) * hd] == 0).all(), (h, row)
    ref, dref = _ref64(tuple(lens), H, hd, p, KEY)
    assert torch.isfinite(out).all() and torch.isfinite(dx).all()
    e = _rel(out, ref), _rel(dx, dref)
    print(f'attention, p = 0.9, H={H} hd={hd}: {len(dead)} all-dropped rows, rel err out {e[0]:.2e} dqkv {e[1]:.2e}')
    assert e[0] < 5e-6 and e[1] < 2e-5, e


# ----------------------------------------------------------------------------------------------------- isolation and determinism
@pytest.mark.parametrize('H, hd', HEADS)
def test_same_key_same_bits_and_the_next_offset_another_mask(H, hd):
    lens = [65, 130]
    qkv, go = _inputs(tuple(lens), H * hd)
    a, b = _run(qkv, go, lens, H), _run(qkv, go, lens, H)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = _run(qkv, go, lens, H, key=(KEY[0], KEY[1] + 1))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])


@pytest.mark.parametrize('H, hd', HEADS)
@pytest.mark.parametrize('mode', MODES)
def test_scenes_do_not_read_each_other_under_dropout(mode, H, hd):
    """Scene 1's rows of qkv and dout hold 1e30: scene 0's out and dqkv are bit-equal to a run with scene 1 removed (scene 0 keeps its
    packed rows 0 .. 63, so its mask is the same in both runs)."""
    lens = [64, 65]
    qkv, go = _inputs(tuple(lens), H * hd, mode != 'fp32')
    qkv, go = qkv.clone(), go.clone()
    qkv[64:] = 1e30; go[64:] = 1e30
    dtype = torch.bfloat16 if mode == 'bf16_tensors' else torch.float32
    with _mode_ctx(mode):
        out2, dx2 = _run(qkv, go, lens, H, dtype)
        out1, dx1 = _run(qkv[:64], go[:64], [64], H, dtype)
    assert torch.isfinite(out1).all() and torch.isfinite(dx1).all()
    assert torch.equal(out2[:64], out1) and torch.equal(dx2[:64], dx1)


# --------------------------------------------------------------------------------------------------------- the elementwise kernels
def _bf16_once(d):
    """float64 -> bfloat16 with ONE rounding to nearest even (torch converts through fp32: two roundings).  The two bf16 neighbours of d
    -- d's bits with the low 45 mantissa bits cleared, and one bf16 ulp further from zero -- are float64 values; the nearer wins, a tie
    goes to the even one.  Finite values in bf16's normal range."""
    b = d.contiguous().view(torch.int64)
    lo_b = b & ~((1 << 45) - 1)
    hi_b = lo_b + (1 << 45)
    lo, hi = lo_b.view(torch.float64), hi_b.view(torch.float64)
    r_lo, r_hi = (d - lo).abs(), (hi - d).abs()
    up = (r_hi < r_lo) | ((r_hi == r_lo) & ((lo_b >> 45) & 1).bool())
    return torch.where(up, hi, lo).to(torch.bfloat16)          # exact: both candidates are bf16 values


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('C', [256, 1024])
@pytest.mark.parametrize('n', [1, 63, 257])
def test_elementwise_dropout_equals_x_times_mask_over_keep_probability(n, C, dtype):
    """y and dx equal x * mask / (1 - p) formed in float64 from the dumped mask and rounded once: fp32 to 1 ulp, bf16 exactly"""
    from unidet3d_amd import dense, ops
    g = torch.Generator().manual_seed(n * C)
    x = (torch.randn(n, C, generator=g) * 3).to(dtype).to(DEV).requires_grad_()
    dy = torch.randn(n, C, generator=g).to(dtype).to(DEV)
    y = dense.dropout(x, P_DROP, BIG_KEY)
    y.backward(dy)
    mask = ops.dropout_mask_rows(P_DROP, BIG_KEY[0], BIG_KEY[1], n, C, DEV).double()
    assert y.dtype == dtype and x.grad.dtype == dtype
    for got, src, what in ((y.detach(), x.detach(), 'y'), (x.grad, dy, 'dx')):
        ref64 = src.double() * mask / (1.0 - P_DROP)
        ref = _bf16_once(ref64) if dtype == torch.bfloat16 else ref64.to(dtype)
        if dtype == torch.bfloat16:
            assert torch.equal(got, ref), what
        else:
            ulp = torch.nextafter(ref.abs(), torch.full_like(ref, math.inf)) - ref.abs()          # (a dropped negative value is -0.0 in ref, +0.0 in got)
            assert ((got - ref).abs() <= ulp).all(), (what, float(((got - ref).abs() / ulp).max()))
        assert ((got == 0) | (mask == 1)).all(), what


# ------------------------------------------------------------------------------------------------- the hidden dropout inside dense.mlp
@pytest.mark.parametrize('act', ['relu', 'gelu'])
@pytest.mark.parametrize('flow', ['fp32', 'bf16_act'])
def test_mlp_hidden_dropout_against_float64(flow, act):
    """z = act(x W1^T + b1) . M / (1 - p) . W2^T + b2 and its six gradients against float64 with the dumped mask, for both activations
    (ReLU: the fused derivative epilogue on the dropped activation, then the mask; GELU: the mask, then the derivative pass) and both
    data flows.  Bounds: the decoder's, 1e-3 for fp32 tensors, 5e-2 (result) / 1e-1 (gradients) for bf16 activations; a mask in the
    wrong place or a missing 1 / (1 - p) is an error of order 0.1 to 1.  The ReLU inputs keep every pre-activation at least 0.5 from
    zero (x >= 0, one sign per row of W1 and its bias), so that no rounding can flip a derivative the reference has."""
    from unidet3d_amd import dense, ops
    from unidet3d_amd import precision as P
    n, d, hid = 195, 256, 1024
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, d, generator=g)
    w1, b1 = torch.randn(hid, d, generator=g) * 0.06, torch.randn(hid, generator=g) * 0.1
    w2, b2 = torch.randn(d, hid, generator=g) * 0.03, torch.randn(d, generator=g) * 0.1
    dz = torch.randn(n, d, generator=g)
    if act == 'relu':
        sign = torch.where(torch.arange(hid) % 2 == 0, 1.0, -1.0)
        x, w1, b1 = x.abs(), w1.abs() * sign[:, None], 0.5 * sign
    t = [v.clone().to(DEV).requires_grad_() for v in (x, w1, b1, w2, b2)]
    with (P.operands('bf16') if flow == 'bf16_act' else contextlib.nullcontext()), (P.bf16_act_mode(True) if flow == 'bf16_act' else contextlib.nullcontext()):
        z = dense.mlp(*t, act, drop=(P_DROP, KEY))
        z.backward(dz.to(DEV))
    torch.cuda.synchronize()
    mask = ops.dropout_mask_rows(P_DROP, KEY[0], KEY[1], n, hid, DEV).cpu().double() / (1.0 - P_DROP)
    r = [v.clone().double().requires_grad_() for v in (x, w1, b1, w2, b2)]
    F = torch.nn.functional
    pre = F.linear(r[0], r[1], r[2])
    if act == 'relu':
        assert float(pre.detach().abs().min()) >= 0.5
    zr = F.linear((F.relu(pre) if act == 'relu' else F.gelu(pre)) * mask, r[3], r[4])
    zr.backward(dz.double())
    e = dict(z=_rel(z, zr), **{k: _rel(a.grad, b.grad) for k, a, b in zip(('dx', 'dw1', 'db1', 'dw2', 'db2'), t, r)})
    print(f'mlp + hidden dropout, {flow}, {act}:', {k: f'{v:.1e}' for k, v in e.items()})
    assert z.dtype == torch.float32
    if flow == 'fp32':
        assert max(e.values()) < 1e-3, e
    else:
        assert e['z'] < 5e-2 and max(v for k, v in e.items() if k != 'z') < 1e-1, e


# ------------------------------------------------------------------------------------------------------------------------ the decoder
CFG = dict(num_layers=2, datasets_classes=[CLASSES], in_channels=32, d_model=256, num_heads=8, hidden_dim=1024,
           activation_fn='gelu', datasets=['scannet'], angles=[False])
DEC_LENS = [65, 130]
DEC_SEED = 20240607


def _decoder(dropout):
    from unidet3d_amd.encoder import UniDet3DEncoder
    return fill_state_dict(UniDet3DEncoder(dropout=dropout, **CFG), tag0=1100).to(DEV)


@functools.lru_cache(maxsize=None)
def _decoder_inputs():
    g = torch.Generator().manual_seed(5)
    x = [torch.randn(n, 32, generator=g) for n in DEC_LENS]
    c = [torch.rand(n, 3, generator=g) * 4 for n in DEC_LENS]
    return x, c


def _loss(res):
    loss = sum((t ** 2).sum() for t in res['cls_preds']) + sum(t.sum() for t in res['bboxes'])
    for a in res['aux_outputs']:
        loss = loss + sum((t * 0.5).sum() for t in a['cls_preds']) + sum((t ** 2).sum() for t in a['bboxes'])
    return loss


def _run_decoder(m, x=None):
    m.zero_grad(set_to_none=True)
    xs, cs = _decoder_inputs()
    x = [t.to(DEV).requires_grad_() for t in xs]
    res = m(x, [t.to(DEV) for t in cs], ['scannet'] * len(DEC_LENS))
    loss = _loss(res)
    loss.backward()
    torch.cuda.synchronize()
    return res, x, loss


def _flat(res):
    out = list(res['cls_preds']) + list(res['bboxes'])
    for a in res['aux_outputs']:
        out += list(a['cls_preds']) + list(a['bboxes'])
    return out


def _ref_decoder(m, step):
    """The reference's decoder (unidet3d/encoder.py) in float64 torch ops with the masks training step ``step`` of ``m`` applies, fetched
    through ``dropout_key`` and the mask ops: (outputs in _flat order, input gradients, loss, parameter gradients by name)."""
    from unidet3d_amd import ops
    from unidet3d_amd.encoder import PredBBox, _bbox_pred_to_bbox
    F = torch.nn.functional
    p, H, d, NL = m.dropout_p, CFG['num_heads'], CFG['d_model'], CFG['num_layers']
    hd, n = d // H, sum(DEC_LENS)
    w = {k: v.detach().double().cpu().requires_grad_() for k, v in m.named_parameters()}
    xs, cs = _decoder_inputs()
    x = [t.double().requires_grad_() for t in xs]
    centers = torch.cat(cs).double()

    def rows_mask(layer, which, C):
        return ops.dropout_mask_rows(p, *m.dropout_key(step, layer, which), n, C, DEV).cpu().double() / (1.0 - p)

    f = F.linear(F.relu(F.linear(torch.cat(x), w['input_proj.0.weight'], w['input_proj.0.bias'])), w['input_proj.2.weight'], w['input_proj.2.bias'])
    feats = [f]
    for i in range(NL):
        a, fn = f'self_attn_layers.{i}.', f'ffn_layers.{i}.'
        qkv = F.linear(f, w[a + 'attn.in_proj_weight'], w[a + 'attn.in_proj_bias'])
        pm = ops.dropout_mask_attn(p, *m.dropout_key(step, i, 0), H, n, DEV).cpu().double() / (1.0 - p)
        outs, o = [], 0
        for ln in DEC_LENS:
            q, k, v = [t.view(ln, H, hd).transpose(0, 1) for t in qkv[o:o + ln].chunk(3, -1)]
            pr = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), -1) * pm[:, o:o + ln, o:o + ln]
            outs.append((pr @ v).transpose(0, 1).reshape(ln, d))
            o += ln
        att = F.linear(torch.cat(outs), w[a + 'attn.out_proj.weight'], w[a + 'attn.out_proj.bias']) * rows_mask(i, 1, d)
        f = F.layer_norm(att + f, (d,), w[a + 'norm.weight'], w[a + 'norm.bias'])
        hdn = F.gelu(F.linear(f, w[fn + 'net.0.weight'], w[fn + 'net.0.bias'])) * rows_mask(i, 2, CFG['hidden_dim'])
        z = F.linear(hdn, w[fn + 'net.3.weight'], w[fn + 'net.3.bias']) * rows_mask(i, 3, d)
        f = F.layer_norm(z + f, (d,), w[fn + 'norm.weight'], w[fn + 'norm.bias'])
        feats.append(f)
    cidx = torch.tensor(m.datasets_cls_idxs[0])
    per_layer = []
    for f in feats:
        nq = F.layer_norm(f, (d,), w['out_norm.weight'], w['out_norm.bias'])
        cls = F.linear(F.relu(F.linear(nq, w['outs_cls.0.weight'], w['outs_cls.0.bias'])), w['outs_cls.2.weight'], w['outs_cls.2.bias'])[:, cidx]
        box = _bbox_pred_to_bbox(centers, PredBBox.decode(F.linear(nq, w['out_bboxes.linear.weight'], w['out_bboxes.linear.bias']))[:, :6])
        per_layer.append((list(cls.split(DEC_LENS)), list(box.split(DEC_LENS))))
    res = dict(cls_preds=per_layer[-1][0], bboxes=per_layer[-1][1], aux_outputs=[dict(cls_preds=c, bboxes=b) for c, b in per_layer[:-1]])
    loss = _loss(res)
    loss.backward()
    return [t.detach() for t in _flat(res)], [t.grad for t in x], float(loss.detach()), {k: v.grad for k, v in w.items()}


def test_decoder_in_eval_mode_ignores_dropout_bit_for_bit():
    m1, m0 = _decoder(0.1).eval(), _decoder(0.0).eval()
    xs, cs = _decoder_inputs()
    with torch.no_grad():
        r1 = m1([t.to(DEV) for t in xs], [t.to(DEV) for t in cs], ['scannet'] * 2)
        r0 = m0([t.to(DEV) for t in xs], [t.to(DEV) for t in cs], ['scannet'] * 2)
    assert len(r1['aux_outputs']) == CFG['num_layers']
    for a, b in zip(_flat(r1), _flat(r0)):
        assert torch.equal(a, b)
    assert m1.dropout_step == 0


def test_decoder_in_training_mode_matches_the_float64_reference_with_the_same_masks():
    m = _decoder(0.1).train()
    m.set_dropout_state(DEC_SEED, 0)
    res, x, loss = _run_decoder(m)
    assert m.dropout_step == 1
    out = [t.detach().clone() for t in _flat(res)]
    grads = {k: v.grad.clone() for k, v in m.named_parameters()}
    ref_out, ref_gx, ref_loss, ref_g = _ref_decoder(m, 0)
    e = dict(out=max(_rel(a, b) for a, b in zip(out, ref_out)), gx=max(_rel(a.grad, b) for a, b in zip(x, ref_gx)),
             loss=abs(loss.item() - ref_loss) / abs(ref_loss), gw=max(_rel(grads[k], ref_g[k]) for k in ref_g))
    print('decoder with dropout 0.1, fp32 vs float64 with the same masks:', {k: f'{v:.1e}' for k, v in e.items()})
    assert set(grads) == set(ref_g)
    assert e['out'] < 1e-3 and e['gx'] < 1e-3 and e['loss'] < 1e-3 and e['gw'] < 1e-3, e
    # dropout is on: the same weights without it give other outputs
    m0 = _decoder(0.0).train()
    res0, _, _ = _run_decoder(m0)
    assert _rel(_flat(res0)[0], ref_out[0]) > 1e-2
    # the second step draws other masks and is the reference of step 1; the counter moves by one per forward
    res2, _, loss2 = _run_decoder(m)
    assert m.dropout_step == 2
    ref_out2, _, ref_loss2, _ = _ref_decoder(m, 1)
    assert max(_rel(a, b) for a, b in zip(_flat(res2), ref_out2)) < 1e-3 and abs(loss2.item() - ref_loss2) < 1e-3 * abs(ref_loss2)
    assert not torch.equal(_flat(res2)[0], out[0])
    # resume: the same state gives the same bits
    m.set_dropout_state(DEC_SEED, 0)
    res3, x3, loss3 = _run_decoder(m)
    assert m.dropout_step == 1
    for a, b in zip(_flat(res3), out):
        assert torch.equal(a, b)
    for k, v in m.named_parameters():
        assert torch.equal(v.grad, grads[k]), k
    for a, b in zip(x3, x):
        assert torch.equal(a.grad, b.grad)


def test_decoder_with_dropout_on_bf16_activations_matches_the_float64_reference_at_bf16_tolerance():
    """the same run under precision.operands('bf16') with bf16 activations in HBM, at the bounds the bf16-activation decoder test of
    tests/test_gpu_attention_heads.py uses"""
    from unidet3d_amd import precision as P
    m = _decoder(0.1).train()
    m.set_dropout_state(DEC_SEED, 0)
    with P.operands('bf16'), P.bf16_act_mode(True):
        res, x, loss = _run_decoder(m)
    ref_out, ref_gx, ref_loss, _ = _ref_decoder(m, 0)
    k = len(DEC_LENS)
    out = _flat(res)
    cls_i = [j for j in range(len(out)) if (j // k) % 2 == 0]
    e = dict(cls=max(_rel(out[j], ref_out[j]) for j in cls_i), box=max(_rel(out[j], ref_out[j]) for j in range(len(out)) if j not in cls_i),
             gx=max(_rel(a.grad, b) for a, b in zip(x, ref_gx)), loss=abs(loss.item() - ref_loss) / abs(ref_loss))
    print('decoder with dropout 0.1, bf16 activations vs float64 with the same masks:', {k_: f'{v:.1e}' for k_, v in e.items()})
    assert all(t.dtype == torch.float32 for t in out)
    assert e['cls'] < 5e-2 and e['box'] < 5e-2 and e['gx'] < 1e-1 and e['loss'] < 2e-2, e


def test_decoder_weight_gradients_on_the_side_stream_give_the_same_bits_under_dropout():
    from unidet3d_amd import sparse

    def run(mode):
        prev = sparse.set_wgrad_overlap(mode)
        try:
            m = _decoder(0.1).train()
            m.set_dropout_state(DEC_SEED, 0)
            _, _, loss = _run_decoder(m)
            return loss.detach().clone(), {k: v.grad.clone() for k, v in m.named_parameters()}
        finally:
            sparse.set_wgrad_overlap(prev)
    loss0, g0 = run(0)
    loss2, g2 = run(2)
    assert torch.equal(loss0, loss2)
    for k in g0:
        assert torch.equal(g0[k], g2[k]), k
