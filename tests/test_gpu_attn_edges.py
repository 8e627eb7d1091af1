"""Varlen flash attention (csrc/attn.hip, csrc/attn_x3.hip, csrc/attn_common.h) on exact scenes, value kinds and decode edges: every data
flow and head width against float64 attention under the ELEMENTWISE bounds of tests/_attn_edges.py -- out, lse (an output here: the
entry points are called through _lib.call), dq, dk, dv -- for six random value kinds; the exact `group` kind under its acceptance (ties,
uniform rows, alpha = 0, exact zeros; forward at both tile-wave forms, with dropout at p = 0.5, backward); the work decode at head counts
1, 3, 5 and 16, many scenes and mostly empty batches; max_len over-estimates, which only add workgroups that exit.  The CPU side of the
cases and bounds: tests/test_attn_edges_cpu.py.  Measured ratios: profiles/attn_edges_ratios.txt (no assertion reads it)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _attn_edges as AE
from _gemm_edges import math_mode

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H = 2
KEY = (0x5DEECE66D, 11)
P_DROP = 0.5


def _run(c, flow, nw=0, p=0.0, max_len=None, backward=True):
    """the entry points of `flow` on a case: namespace(out, lse, dq, dk, dv) on the CPU (bf16 tensors as they are stored)"""
    from unidet3d_amd import _lib as L, precision as P
    dtype = torch.bfloat16 if flow == 'bf16_tensors' else torch.float32
    qkv, dout = c.qkv.to(dtype).to(DEV), c.dout.to(dtype).to(DEV)
    cu = torch.tensor([0] + list(np.cumsum(c.lens)), dtype=torch.int32, device=DEV)
    B, n, scale = len(c.lens), c.n, AE.scale_of(c.hd)
    max_len = max(c.lens) if max_len is None else max_len
    out = torch.full((n, c.D), float('nan'), dtype=dtype, device=DEV)
    lse = torch.full((c.H, n), float('nan'), dtype=torch.float32, device=DEV)
    dqkv = torch.full((n, 3 * c.D), float('nan'), dtype=dtype, device=DEV)
    delta = torch.empty(c.H, n, dtype=torch.float32, device=DEV)
    sfx = ('_drop' if p else '') + AE.FLOW_SUFFIX[flow]
    drop = (float(p), KEY[0], KEY[1]) if p else ()
    with math_mode(AE.FLOW_MATH[flow]), P.attn_tile_waves(nw):
        L.call('u3d_attn_varlen_fwd' + sfx, L.ptr(qkv), L.ptr(cu), B, max_len, n, c.H, c.hd, scale, L.ptr(out), L.ptr(lse), 0.0, L.stream(), *drop)
        if backward:
            L.call('u3d_attn_varlen_bwd' + sfx, L.ptr(qkv), L.ptr(out), L.ptr(dout), L.ptr(lse), L.ptr(cu), B, max_len, n, c.H, c.hd, scale,
                   L.ptr(dqkv), L.ptr(delta), 0.0, L.stream(), *drop)
    torch.cuda.synchronize()
    r = SimpleNamespace(out=out.cpu(), lse=lse.cpu(), dqkv=dqkv.cpu(), dq=None, dk=None, dv=None)
    if backward:
        r.dq, r.dk, r.dv = AE.split_dqkv(r.dqkv, c.D)
    return r


@functools.lru_cache(maxsize=None)
def _result(kind, lens, Hh, hd, flow, nw=0):
    return _run(AE.flow_case(kind, lens, Hh, hd, flow), flow, nw)


def _worst(worst, m):
    for k, v in m.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _print(flow, hd, what, worst):
    print(f'attn_edges {flow} hd={hd} {what}: error / bound ' + ' '.join(f'{k}={v:.4f}' for k, v in worst.items()))


def _check_random(kind, lens, Hh, hd, flow, worst):
    got = _result(kind, lens, Hh, hd, flow)
    m = AE.margins(AE.cached_reference(kind, lens, Hh, hd, flow), got)
    _worst(worst, m)
    return m


def _check_group(lens, Hh, hd, flow, worst, nw=0):
    c = AE.flow_case('group', lens, Hh, hd, flow)
    r = AE.cached_reference('group', lens, Hh, hd, flow)
    got = _result('group', lens, Hh, hd, flow, nw)
    m = {'out': AE.group_forward_margin(c, flow, got.out), 'lse': AE.margin(got.lse, r.lse, r.b_lse)}
    bad, mb = AE.group_backward_margins(c, r, got.dq, got.dk, got.dv)
    m.update(mb)
    _worst(worst, m)
    return bad, m


# ------------------------------------------------------------------------------------------------------------------ value kinds
@pytest.mark.parametrize('kind', AE.RANDOM_KINDS)
@pytest.mark.parametrize('flow, hd', AE.FLOW_HDS)
def test_value_kinds_against_float64(flow, hd, kind):
    worst, failed = {}, []
    for lens in AE.LAYOUTS:
        m = _check_random(kind, lens, H, hd, flow, worst)
        if not all(v <= 1.0 for v in m.values()):
            failed.append((lens, m))
    _print(flow, hd, kind, worst)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------ the exact kind
@pytest.mark.parametrize('flow, hd, nw', [('native', 32, 0)] + [(f, hd, nw) for f in AE.PLANE_FLOWS for hd in (32, 64) for nw in (4, 8)])
def test_group_forward(flow, hd, nw):
    worst, failed = {}, []
    for lens in AE.LAYOUTS:
        c = AE.flow_case('group', lens, H, hd, flow)
        r = AE.cached_reference('group', lens, H, hd, flow)
        got = _run(c, flow, nw, backward=False)
        m = {'out': AE.group_forward_margin(c, flow, got.out), 'lse': AE.margin(got.lse, r.lse, r.b_lse)}
        _worst(worst, m)
        if not all(v <= 1.0 for v in m.values()):
            failed.append((lens, m))
    _print(flow, hd, f'group forward NW={nw}', worst)
    assert not failed, failed


@pytest.mark.parametrize('flow, hd', [(f, hd) for f in AE.PLANE_FLOWS for hd in (32, 64)])
def test_group_forward_with_dropout(flow, hd):
    """p = 0.5: 1 / (1 - p) is exactly 2; the mask is the one the kernels regenerate (ops.dropout_mask_attn).  A row whose group keys are
    all dropped has closed form 0 and tolerance 0: exactly 0."""
    from unidet3d_amd import ops
    worst, failed, all_dropped = {}, [], 0
    for lens in AE.LAYOUTS:
        c = AE.flow_case('group', lens, H, hd, flow)
        r = AE.cached_reference('group', lens, H, hd, flow)
        mask = ops.dropout_mask_attn(P_DROP, KEY[0], KEY[1], H, c.n, DEV).cpu()
        got = _run(c, flow, 0, p=P_DROP, backward=False)
        ref = AE.group_closed(c, mask)[0]
        all_dropped += int((ref.view(c.n, H, hd).abs().sum(2) == 0).sum())
        m = {'out': AE.group_forward_margin(c, flow, got.out, mask), 'lse': AE.margin(got.lse, r.lse, r.b_lse)}
        _worst(worst, m)
        if not all(v <= 1.0 for v in m.values()):
            failed.append((lens, m))
    _print(flow, hd, 'group forward dropout', worst)
    assert all_dropped > 0          # the one-row scene and the single-key groups: half of them lose every key
    assert not failed, failed


@pytest.mark.parametrize('flow, hd', AE.FLOW_HDS)
def test_group_backward(flow, hd):
    worst, failed = {}, []
    for lens in AE.LAYOUTS:
        bad, m = _check_group(lens, H, hd, flow, worst)
        if bad or not all(v <= 1.0 for v in m.values()):
            failed.append((lens, bad, m))
    _print(flow, hd, 'group backward', worst)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------ decode edges
@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('flow', ['x3', 'bf16_tensors'])
def test_decode_edges(flow, hd):
    failed = []
    for Hh, lens, only in AE.DECODE_CASES:
        if only not in (None, hd):
            continue
        worst = {}
        m = _check_random('randn', lens, Hh, hd, flow, worst)
        bad, mg = _check_group(lens, Hh, hd, flow, worst)
        _print(flow, hd, f'decode H={Hh} B={len(lens)}', worst)
        if bad or not all(v <= 1.0 for v in list(m.values()) + list(mg.values())):
            failed.append((Hh, lens, bad, m, mg))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------ max_len
def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize('flow, hd', AE.FLOW_HDS)
def test_max_len_over_estimates_change_nothing(flow, hd):
    """the grid is sized from max_len: an over-estimate adds workgroups whose first row is past the scene's end, and they exit"""
    c = AE.flow_case('randn', AE.MAXLEN_LENS, H, hd, flow)
    base = _run(c, flow, max_len=max(AE.MAXLEN_LENS))
    assert torch.isfinite(base.out.float()).all() and torch.isfinite(base.lse).all() and torch.isfinite(base.dqkv.float()).all()
    for max_len in AE.MAXLEN_OVER:
        got = _run(c, flow, max_len=max_len)
        for nm in ('out', 'lse', 'dqkv'):
            assert _same_bits(getattr(got, nm), getattr(base, nm)), (nm, max_len)
