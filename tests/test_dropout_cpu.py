"""Decoder dropout without a device: the model builds with dropout != 0 and keeps the reference's state_dict keys, the key scheme
(seed, step, layer, site) is injective and resumable, the `_drop` entry points exist and validate before any HIP call, and the mask
function (tests/_dropout.py, pinned to csrc/dropout.h by tests/test_gpu_dropout.py) passes the statistical conditions of a dropout
mask.  The hash is deterministic: the statistical outcomes are fixed, a failure means the hash is poor."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _dropout as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ['cabinet', 'bed', 'chair', 'sofa', 'table']
SEED, OFFSET = 0x5DEECE66D, 7


def _model(dropout, num_layers=2):
    from unidet3d_amd.encoder import UniDet3DEncoder
    return UniDet3DEncoder(num_layers=num_layers, datasets_classes=[CLASSES], in_channels=32, d_model=256, num_heads=4, hidden_dim=1024,
                           dropout=dropout, activation_fn='gelu', datasets=['scannet'], angles=[False])


def test_decoder_with_dropout_builds_with_the_reference_state_dict_keys():
    m, m0 = _model(0.1), _model(0.0)
    assert list(m.state_dict().keys()) == list(m0.state_dict().keys())
    assert m.dropout_p == 0.1 and m0.dropout_p == 0.0
    assert not any('dropout' in k for k in m.state_dict())


def test_dropout_key_is_injective_over_step_layer_and_site():
    m = _model(0.1, num_layers=6)
    m.set_dropout_state(1234, 0)
    keys = [m.dropout_key(s, l, w) for s in range(3) for l in range(6) for w in range(4)]
    assert all(k[0] == 1234 for k in keys)
    assert len({k[1] for k in keys}) == 3 * 6 * 4
    assert m.dropout_key(2, 5, 3) == (1234, 2 * 4 * 6 + 4 * 5 + 3)
    for bad in [(0, 6, 0), (0, 0, 4), (-1, 0, 0)]:
        with pytest.raises(ValueError):
            m.dropout_key(*bad)


def test_set_dropout_state_round_trips():
    m = _model(0.1)
    m.set_dropout_state((1 << 63) + 5, 41)
    assert (m.dropout_seed, m.dropout_step) == ((1 << 63) + 5, 41)
    assert m.dropout_key(41, 1, 2) == ((1 << 63) + 5, 41 * 8 + 4 + 2)
    m.set_dropout_state(3, 0)
    assert (m.dropout_seed, m.dropout_step) == (3, 0)
    with pytest.raises(ValueError):
        m.set_dropout_state(-1, 0)
    with pytest.raises(ValueError):
        m.set_dropout_state(1 << 64, 0)


# ---------------------------------------------------------------------------------------------------------------- the C interface
DROP_ATTN = [(d, s) for d in ('fwd', 'bwd') for s in ('', '_bf16', '_b16')]
DROP_OTHER = ['u3d_dropout_mask_attn', 'u3d_dropout_mask_rows', 'u3d_dropout_fwd', 'u3d_dropout_bwd', 'u3d_dropout_fwd_b16', 'u3d_dropout_bwd_b16']


def test_every_dropout_symbol_exists_with_the_headers_arity():
    from unidet3d_amd import _lib
    l = _lib.lib()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'u3d.h')).read(), flags=re.S)
    for name in [f'u3d_attn_varlen_{d}_drop{s}' for d, s in DROP_ATTN] + DROP_OTHER:
        assert hasattr(l, name), name
        m = re.search(r'\b' + name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert m, f'{name} is not declared in include/u3d.h'
        assert len([p for p in m.group(1).split(',') if p.strip()]) == len(_lib.PROTOTYPES[name][1]), name
    for d, s in DROP_ATTN:              # the existing argument list plus (double p, uint64 seed, uint64 offset)
        assert len(_lib.PROTOTYPES[f'u3d_attn_varlen_{d}_drop{s}'][1]) == len(_lib.PROTOTYPES[f'u3d_attn_varlen_{d}{s}'][1]) + 3


def _attn_caller(direction, suffix):
    from unidet3d_amd import _lib
    l = _lib.lib()
    fn = getattr(l, f'u3d_attn_varlen_{direction}_drop{suffix}')
    buf = ctypes.create_string_buffer(64)               # never dereferenced: the calls return before anything reads a tensor
    p = ctypes.addressof(buf)
    n_ptr = 2 if direction == 'fwd' else 5

    def call(prob, hd=32):
        return fn(*[p] * n_ptr, 1, 64, 64, 8, hd, 0.25, p, p, 0.0, None, prob, SEED, OFFSET)
    return l, call


@pytest.mark.parametrize('direction,suffix', DROP_ATTN)
def test_attention_drop_entry_points_refuse_a_bad_probability_before_any_hip_call(direction, suffix):
    l, call = _attn_caller(direction, suffix)
    for prob in (-0.1, 1.0, float('nan')):
        assert call(prob) == -1, prob                                    # U3D_EINVAL
        assert b'dropout' in l.u3d_last_error()
    assert call(0.1, hd=16) == -3 and b'head_dim 16 unsupported' in l.u3d_last_error()


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
def test_native_fp32_mfma_arm_refuses_dropout_and_names_the_mode_that_runs_it(direction):
    l, call = _attn_caller(direction, '')
    prev = l.u3d_fp32_math(-1)
    try:
        l.u3d_fp32_math(0)                                               # native fp32 MFMA kernels (U3D_FP32_MATH=mfma)
        assert call(0.1) == -3                                           # U3D_EUNSUPPORTED
        msg = l.u3d_last_error()
        assert b'dropout' in msg and b'mfma' in msg and b'bf16x3' in msg
        assert call(-0.1) == -1                                          # the probability is checked first
    finally:
        l.u3d_fp32_math(prev)


@pytest.mark.parametrize('name', DROP_OTHER)
def test_mask_and_elementwise_entry_points_refuse_a_bad_probability_before_any_hip_call(name):
    from unidet3d_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    fn = getattr(l, name)
    for prob in (-0.1, 1.0, float('nan')):
        if name == 'u3d_dropout_mask_attn':
            rc = fn(prob, SEED, OFFSET, 2, 16, p, None)
        elif name == 'u3d_dropout_mask_rows':
            rc = fn(prob, SEED, OFFSET, 4, 256, p, None)
        else:
            rc = fn(p, p, 4, 256, prob, SEED, OFFSET, None)
        assert rc == -1, (name, prob)


# ------------------------------------------------------------------------------------------------- statistics of the mask function
H, N_TOTAL = 2, 260
N = H * N_TOTAL * N_TOTAL          # 135 200 per mask


def _within(rate, q, n, what):
    """|rate - q| <= 5 sigma of a binomial with success probability q over n samples"""
    bound = 5.0 * math.sqrt(q * (1.0 - q) / n)
    print(f'{what}: rate {rate:.5f}, expected {q:.5f}, |diff| {abs(rate - q):.5f}, 5 sigma {bound:.5f} (n = {n})')
    assert abs(rate - q) <= bound, what


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_keep_fraction_overall_and_per_head(p):
    m = DR.mask_attn(p, SEED, OFFSET, H, N_TOTAL)
    assert m.shape == (H, N_TOTAL, N_TOTAL) and m.size == N
    _within(m.mean(), 1 - p, N, f'p={p} overall')
    for h in range(H):
        _within(m[h].mean(), 1 - p, N // H, f'p={p} head {h}')


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_masks_of_neighbouring_arguments_are_independent(p):
    """agreement rate of two independent masks: (1 - p)^2 + p^2"""
    m = DR.mask_attn(p, SEED, OFFSET, H, N_TOTAL)
    m1 = DR.mask_attn(p, SEED, OFFSET + 1, H, N_TOTAL)
    q = (1 - p) ** 2 + p ** 2
    _within((m[0] == m[1]).mean(), q, N_TOTAL * N_TOTAL, f'p={p} head 0 vs head 1')
    _within((m == m1).mean(), q, N, f'p={p} offset k vs k+1')
    off = ~np.eye(N_TOTAL, dtype=bool)
    t = (m == m.transpose(0, 2, 1))[:, off]
    _within(t.mean(), q, t.size // 2, f'p={p} mask vs transpose')          # (i, j) and (j, i) are one comparison: half the samples are distinct
    r = m[:, :-1] == m[:, 1:]
    _within(r.mean(), q, r.size, f'p={p} row i vs i+1')


def test_no_row_is_all_kept_or_all_dropped_at_one_half():
    m = DR.mask_attn(0.5, SEED, OFFSET, H, N_TOTAL)
    s = m.sum(-1)
    assert s.min() > 0 and s.max() < N_TOTAL, (s.min(), s.max())


def test_rows_mask_matches_the_attention_mask_of_head_zero_and_the_thresholds_are_exact():
    """one function behind both dumps; thr = floor(p 2^32); p = 0 keeps everything"""
    assert np.array_equal(DR.mask_rows(0.1, SEED, OFFSET, 7, 9), DR.mask_attn(0.1, SEED, OFFSET, 1, 9)[0, :7])
    assert DR.thr(0.5) == 1 << 31 and DR.thr(0.0) == 0 and DR.thr(0.1) == 429496729
    assert DR.mask_rows(0.0, SEED, OFFSET, 5, 64).all()
