"""Head dims of the varlen attention entry points, decided before any HIP call (no device needed, as tests/test_cabi.py): 32 and 64 run,
every other value is U3D_EUNSUPPORTED with the head-dim message, and the native fp32 MFMA arm (U3D_FP32_MATH=mfma) stays at 32 and names
the mode that runs 64.  And the host side of a decoder whose head dim is 64: it constructs, with nn.MultiheadAttention's parameter layout."""
import ctypes

import pytest
import torch

ENTRY = [(d, s) for d in ('fwd', 'bwd') for s in ('', '_bf16', '_b16')]
CLASSES = ['cabinet', 'bed', 'chair', 'sofa', 'table']


def _caller(direction, suffix):
    """call(ptrs, hd, H): an attention entry point on tensors that are never dereferenced (the calls return before anything reads one)"""
    from unidet3d_amd import _lib
    l = _lib.lib()
    fn = getattr(l, f'u3d_attn_varlen_{direction}{suffix}')
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    n_ptr = 2 if direction == 'fwd' else 5              # leading tensors: qkv, cu | qkv, out, dout, lse, cu; then B, max_len, n_total, H, hd, scale
    tail = [p, p, 0.0, None]                            # out, lse | dqkv, delta_ws; flops_hint, stream

    def call(ptrs, hd, H=4, tail=tail):
        return fn(*ptrs, 1, 64, 64, H, hd, 0.125, *tail)
    return l, call, p, n_ptr, tail


@pytest.mark.parametrize('direction,suffix', ENTRY)
@pytest.mark.parametrize('hd', [16, 48, 128])
def test_other_head_dims_are_refused_before_any_hip_call(direction, suffix, hd):
    l, call, p, n_ptr, _ = _caller(direction, suffix)
    assert call([p] * n_ptr, hd) == -3                                   # U3D_EUNSUPPORTED
    assert f'head_dim {hd} unsupported'.encode() in l.u3d_last_error()


@pytest.mark.parametrize('direction,suffix', ENTRY)
def test_null_tensors_at_head_dim_64_are_invalid_arguments(direction, suffix):
    l, call, p, n_ptr, tail = _caller(direction, suffix)
    for i in range(n_ptr):
        assert call([None if j == i else p for j in range(n_ptr)], 64) == -1, f'NULL tensor {i}'        # U3D_EINVAL
    for i in (0, 1):
        t = list(tail)
        t[i] = None
        assert call([p] * n_ptr, 64, tail=t) == -1, f'NULL output {i}'


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
def test_native_fp32_mfma_arm_refuses_head_dim_64_and_names_the_mode_that_runs_it(direction):
    l, call, p, n_ptr, _ = _caller(direction, '')
    prev = l.u3d_fp32_math(-1)
    try:
        l.u3d_fp32_math(0)                                               # native fp32 MFMA kernels (U3D_FP32_MATH=mfma)
        assert call([p] * n_ptr, 64) == -3
        msg = l.u3d_last_error()
        assert b'head_dim 64 unsupported' in msg and b'mfma' in msg and b'bf16x3' in msg
        assert call([p] * n_ptr, 16) == -3 and b'head_dim 16 unsupported' in l.u3d_last_error()
    finally:
        l.u3d_fp32_math(prev)
    # the bf16-operand and bf16-tensor entry points do not depend on the fp32 math mode: they are covered by the tests above in either


@pytest.mark.parametrize('d_model,num_heads,hidden', [(256, 4, 1024), (128, 2, 256)])
def test_decoder_with_head_dim_64_constructs_with_the_multihead_attention_layout(d_model, num_heads, hidden):
    from unidet3d_amd.encoder import UniDet3DEncoder
    m = UniDet3DEncoder(num_layers=2, datasets_classes=[CLASSES], in_channels=32, d_model=d_model, num_heads=num_heads, hidden_dim=hidden,
                        dropout=0.0, activation_fn='gelu', datasets=['scannet'], angles=[False])
    assert d_model // num_heads == 64
    sd = m.state_dict()
    ref = torch.nn.MultiheadAttention(d_model, num_heads, batch_first=True).state_dict()
    assert {k: tuple(v.shape) for k, v in ref.items()} == dict(in_proj_weight=(3 * d_model, d_model), in_proj_bias=(3 * d_model,),
                                                               **{'out_proj.weight': (d_model, d_model), 'out_proj.bias': (d_model,)})
    for i in range(2):
        pre = f'self_attn_layers.{i}.attn.'
        assert {k[len(pre):]: tuple(v.shape) for k, v in sd.items() if k.startswith(pre)} == {k: tuple(v.shape) for k, v in ref.items()}
        assert m.self_attn_layers[i].attn.num_heads == num_heads
        assert tuple(sd[f'ffn_layers.{i}.net.0.weight'].shape) == (hidden, d_model) and tuple(sd[f'ffn_layers.{i}.norm.weight'].shape) == (d_model,)
    assert tuple(sd['input_proj.0.weight'].shape) == (d_model, 32) and tuple(sd['out_bboxes.linear.weight'].shape) == (8, d_model)
