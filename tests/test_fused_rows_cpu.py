"""Host side of the bf16-row outputs of the convolution epilogue, no GPU: the store index of the epilogue against
``sparse.to_shadow``, the unchanged ABI with its added query and flag constants, the plan's rows-capable norms, the rows-only tensor,
and the refusals of ``u3d_spconv_gmm_ep`` for bf16-row outputs (decided before anything touches a device)."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _piece(row, col, ld, first):
    """u3d_common.h store_shadow as gmm_write_out calls it: the 8-byte piece (four bf16) that receives dst columns col .. col + 3 of
    ``row`` in a bf16-row buffer with leading dimension ``ld`` whose block starts at column ``first`` (both in bf16 elements)"""
    c4 = col >> 2
    g32, half, q = c4 >> 3, (c4 >> 2) & 1, c4 & 3
    return row * (ld >> 2) + (first >> 2) + g32 * 8 + q * 2 + half


def _epilogue_store(buf, x, first):
    """what the epilogue leaves in ``buf`` [n, ld] (bf16) for the fp32 block ``x`` [n, C] at first column ``first``"""
    n, C = x.shape
    ld = buf.shape[1]
    pieces = buf.view(-1, 4)
    for r in range(n):
        for col in range(0, C, 4):
            pieces[_piece(r, col, ld, first)] = x[r, col:col + 4].to(torch.bfloat16)      # round to nearest even


@pytest.mark.parametrize('C', [32, 64, 96, 192])
def test_store_index_of_the_epilogue_is_the_shadow_layout(C):
    from unidet3d_amd.sparse import to_shadow
    n = 5
    x = torch.randn(n, C, generator=torch.Generator().manual_seed(C))
    buf = torch.full((n, C), float('nan'), dtype=torch.bfloat16)
    _epilogue_store(buf, x, 0)
    assert torch.equal(buf.view(torch.int16), to_shadow(x).view(torch.int16))
    # a wider buffer: the block lands in its own columns and nowhere else
    wide = torch.full((n, C + 64), float('nan'), dtype=torch.bfloat16)
    _epilogue_store(wide, x, 32)
    assert torch.equal(wide[:, 32:32 + C].contiguous().view(torch.int16), to_shadow(x).view(torch.int16))
    assert bool(wide[:, :32].isnan().all()) and bool(wide[:, 32 + C:].isnan().all())


@pytest.mark.parametrize('c', [32, 96])
def test_two_column_blocks_make_the_shadow_of_the_concatenation(c):
    from unidet3d_amd.sparse import to_shadow
    n = 5
    g = torch.Generator().manual_seed(2 * c)
    a, b = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g)
    buf = torch.full((n, 2 * c), float('nan'), dtype=torch.bfloat16)
    _epilogue_store(buf, a, 0)
    _epilogue_store(buf, b, c)
    assert torch.equal(buf.view(torch.int16), to_shadow(torch.cat((a, b), dim=1)).view(torch.int16))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'u3d.h')).read(), flags=re.S)


def test_abi_is_unchanged_and_the_format_query_is_declared():
    from unidet3d_amd import _lib
    src = _header()
    assert int(re.search(r'#define\s+U3D_ABI_VERSION\s+(\d+)', src).group(1)) == _lib.ABI_VERSION == 117
    assert [n for n, _ in _lib.ConvEpilogue._fields_] == ['raw', 'raw_ld', 'raw_col', 'n_act', 'act', 'scale', 'shift', 'act_ld', 'act_col', 'relu']
    assert ctypes.sizeof(_lib.ConvEpilogue) == 8 + 16 + 8 + 3 * 16 + 2 * 16 + 8
    body = re.search(r'typedef\s+struct\s+u3d_conv_epilogue\s*\{(.*?)\}', src, flags=re.S).group(1)
    assert re.sub(r'\s+', ' ', body).strip() == ('float* raw; int64_t raw_ld, raw_col; int n_act; float* act[2]; const float* scale[2]; '
                                                 'const float* shift[2]; int64_t act_ld[2], act_col[2]; int relu[2];')
    assert re.search(r'\bint\s+u3d_spconv_gmm_ep_formats\s*\(\s*void\s*\)\s*;', src)
    assert _lib.PROTOTYPES['u3d_spconv_gmm_ep_formats'] == (ctypes.c_int, [])
    assert int(re.search(r'#define\s+U3D_EP_RELU\s+(\d+)', src).group(1)) == _lib.EP_RELU == 1
    assert int(re.search(r'#define\s+U3D_EP_BF16_ROWS\s+(\d+)', src).group(1)) == _lib.EP_BF16_ROWS == 2
    assert _lib.lib().u3d_spconv_gmm_ep_formats() == 3


def _net(planes, **kw):
    from unidet3d_amd.sparse import SparseBatchNorm, SparseSequential, SubMConv3d
    from unidet3d_amd.spconv_unet import SpConvUNet
    unet = SpConvUNet(planes, block_reps=2, **kw)
    front = SparseSequential(SubMConv3d(6, planes[0], 3, padding=1, indice_key='subm1'))
    back = SparseSequential(SparseBatchNorm(planes[0]), nn.ReLU())
    return front, unet, back


def test_plan_marks_every_norm_but_the_sink_rows_capable():
    from unidet3d_amd.sparse import _ConvBase
    from unidet3d_amd.spconv_unet import fusion_plan
    front, unet, back = _net([32, 64, 96])
    plan = fusion_plan(unet, front, back)
    assert fusion_plan(unet, front, back) is plan                        # still cached
    assert len(plan.norms) == 25
    capable = [n for n in plan.norms if plan.rows_capable(n)]
    assert set(plan.norms) - set(capable) == {back[0]}                   # the superpoint pooling reads the sink as fp32
    for n in capable:
        reader = plan.norms[n].reader
        assert isinstance(reader, _ConvBase) and reader.kernel_size != 1 and reader in plan.convs
        assert reader.in_channels == n.num_features                      # the reader gathers exactly this norm's rows
    assert len({plan.norms[n].reader for n in capable}) == len(capable)  # one reader each, nobody reads two norms
    # the concat norms: two producers, column blocks [0, c) and [c, 2c), both written into the level's activated buffer
    assert len(plan.cats) == 2
    for u, cat in plan.cats.items():
        c = u.num_planes[0]
        assert plan.rows_capable(cat.norm) and plan.norms[cat.norm].reader is u.blocks_tail[0].conv_branch[2]
        assert sorted((lo, hi) for _, lo, hi in plan.norms[cat.norm].producers) == [(0, c), (c, 2 * c)]
        for conv, lo, _ in plan.norms[cat.norm].producers:
            assert (cat.norm, True, (u, lo)) in plan.convs[conv].acts
    # without an announced producer the first norm is unfused: u3d_bn_apply writes its shadow, nothing to mark
    _, unet2, _ = _net([32, 64])
    plan2 = fusion_plan(unet2)
    first = unet2.blocks[0].conv_branch[0]
    assert not plan2.rows_capable(first) and sum(plan2.rows_capable(n) for n in plan2.norms) == len(plan2.norms) - 1


def test_post_activation_net_still_gets_an_empty_plan():
    from unidet3d_amd.spconv_unet import fusion_plan
    front, unet, back = _net([32, 64], normalize_before=False)
    plan = fusion_plan(unet, front, back)
    assert not plan.convs and not plan.norms and not plan.cats
    assert not plan.rows_capable(back[0])


def test_rows_only_tensor_has_no_values_and_refuses_every_other_reader():
    from unidet3d_amd import _lib, dense, sparse
    rows = torch.zeros(7, 64, dtype=torch.bfloat16)
    t = sparse.rows_only(rows)
    assert t.shape == (0, 64) and t.dtype == torch.float32 and sparse.rows_only_of(t) is rows
    before = dict(sparse.SHADOW_STATS)
    assert sparse.shadow_of(t) is rows
    assert sparse.SHADOW_STATS['hit'] == before['hit'] + 1 and sparse.SHADOW_STATS['miss'] == before['miss']
    assert sparse.rows_only_of(torch.zeros(0, 64)) is None
    bn = sparse.SparseBatchNorm(64).eval()
    with torch.no_grad():
        with pytest.raises(_lib.U3DError, match='bf16 rows only'):
            bn(t, relu=True)
        with pytest.raises(_lib.U3DError, match='bf16 rows only'):
            sparse.sparse_conv(t, torch.zeros(32, 27, 64), None)
        with pytest.raises(_lib.U3DError, match='bf16 rows only'):
            dense.linear(t, torch.zeros(32, 64))


def test_default_of_the_toggle_is_stated():
    """``None`` keeps meaning "on, except under bf16_rows" -- the fused bf16-row path is opt-in (set_fused_inference(True))"""
    from unidet3d_amd import precision as P
    from unidet3d_amd import sparse
    prev = sparse.set_fused_inference(None)
    try:
        with P.operands('bf16'), P.bf16_rows_mode(True):
            assert not sparse.fused_inference_on()
            with sparse.fused_inference(True):
                assert sparse.fused_inference_on()
        with P.operands('bf16'), P.bf16_rows_mode(False):
            assert sparse.fused_inference_on()
    finally:
        sparse.set_fused_inference(prev)


def test_bf16_row_refusals_are_decided_before_any_device_call():
    from unidet3d_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(64)                    # never dereferenced
    p = ctypes.addressof(buf)
    EINVAL, EUNSUPPORTED = -1, -3

    def call(flags, ld, col, Cs=32, Cd=32, fmt=1, raw=None):
        e = _lib.ConvEpilogue()
        e.raw, e.raw_ld, e.raw_col, e.n_act = raw, Cd, 0, 1
        e.act[0], e.scale[0], e.shift[0], e.act_ld[0], e.act_col[0], e.relu[0] = p, p, p, ld, col, flags
        return l.u3d_spconv_gmm_ep(fmt, p, 100, p, p, p, p, 27, 100, Cs, Cd, 100, 64, 1, None, None, None, ctypes.byref(e), 0.0, None)
    rows = _lib.EP_BF16_ROWS
    for flags in (rows, rows | _lib.EP_RELU):
        assert call(flags, 32 + 16, 0) == EINVAL and b'bf16 rows' in l.u3d_last_error()        # ld: a multiple of 4, not of 32
        assert call(flags, 64 + 32, 16) == EINVAL and b'bf16 rows' in l.u3d_last_error()       # col likewise
        assert call(flags, 64, 4) == EINVAL
        assert call(flags, 32, 32) == EINVAL                                                   # the block runs past the row
        assert call(flags, 0, 0) == EINVAL
        assert call(flags | 4, 32, 0) == EUNSUPPORTED and b'flag word' in l.u3d_last_error()   # an undefined bit
        assert call(flags | 4, 48, 0) == EUNSUPPORTED
    assert call(4, 32, 0) == EUNSUPPORTED and call(8 | _lib.EP_RELU, 32, 0) == EUNSUPPORTED
    # Cd that is no multiple of 32 with a bf16-row output (fmt 0, the 16 -> Cd launch): refused here, as a layout error
    assert call(rows, 64, 0, Cs=16, Cd=48, fmt=0) == EINVAL and b'bf16 rows' in l.u3d_last_error()
    assert call(rows, 48, 0, Cs=16, Cd=48, fmt=0) == EINVAL
    # no output at all stays refused as before
    e = _lib.ConvEpilogue()
    e.n_act = 0
    assert l.u3d_spconv_gmm_ep(1, p, 100, p, p, p, p, 27, 100, 32, 32, 100, 64, 1, None, None, None, ctypes.byref(e), 0.0, None) == EINVAL
    assert b'no output' in l.u3d_last_error()
