"""Sparse transposed convolution and convolution bias without a GPU: the checker of tests/_conv_transpose.py is checked (pair-list sums
against the dense float64 reference, sabotaged lists caught, the out-shape rule against torch's), the constructors, and the C contracts
that are decided before any HIP call (status code and error text of every refusal).
The tests of the first section are checks of the CHECKER: what they assert is about tests/_conv_transpose.py, the reference every GPU
test of the feature is held to.  Each ties itself to the library in one place -- the out shape of every configuration and scene through
``sparse.convt_out_shape`` (u3d_convt_out_shape), the bias-gradient constants through ``_lib`` -- so that none of them runs without the
feature it is the yardstick of."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_geometry as cg
import _conv_transpose as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3


# ---------------------------------------------------------------------------------------------------------------- the checker
def _lib_out_shape(cfg, shape):
    from unidet3d_amd import sparse as S
    k, s, p, q, d = T.geom(cfg)
    return S.convt_out_shape(S.conv_geometry(k, s, p, d), S.output_padding_of(q, S.conv_geometry(k, s, p, d)), shape)


@pytest.mark.parametrize('cfg', list(T.CONFIGS))
def test_pair_lists_reproduce_the_dense_reference_and_both_derivations_agree(cfg):
    for name in T.SCENES:
        oc, oshape, pairs = T.brute(cfg, name)
        n, n2 = T.n_rows(cfg, name)
        where = f'{cfg} on {name}'
        assert T.same_lists(pairs, T.forward_lists(cfg, name)), where
        for new_rows, in_rows in pairs:                       # both columns ascend strictly, at most min(n_in, n_out) pairs
            assert len(new_rows) <= min(n, n2) and (np.diff(new_rows) > 0).all() and (np.diff(in_rows) > 0).all(), where
        inp = T.make_inputs(cfg, name, 3, 5, seed=1)
        ref, got = T.reference(inp, cfg, name), T.pair_sum(inp, cfg, name)
        for q in ('y', 'dx', 'dw', 'dadd'):
            scale = max(1.0, float(ref[q].abs().max())) if ref[q].numel() else 1.0
            assert float((got[q] - ref[q]).abs().max() if ref[q].numel() else 0.0) <= 1e-12 * scale, (where, q)
        assert T.off_set_is_zero(inp['x'].double(), inp['w'].double(), cfg, name), where
        # the out-shape rule is torch's, and the library's
        _, B, shape, coords = T.scene(name)
        assert tuple(_lib_out_shape(cfg, shape)) == tuple(oshape), where
        assert tuple(T.dense_full(torch.zeros(len(coords), 1), torch.zeros(1, *T.geom(cfg)[0], 1), cfg, name).shape[2:]) == tuple(oshape), where


def test_k2s2p0_gives_eight_outputs_per_input_with_one_pair_each():
    for name in T.SCENES:
        oc, _, pairs = T.brute('k2s2p0', name)
        n = len(T.scene(name)[3])
        assert len(oc) == 8 * n and all(len(p[0]) == n for p in pairs), name
        assert tuple(_lib_out_shape('k2s2p0', T.scene(name)[2])) == tuple(2 * e for e in T.scene(name)[2]), name
        assert (np.bincount(np.concatenate([p[0] for p in pairs]), minlength=len(oc)) == 1).all(), name


def test_padding_at_and_beyond_the_reach_crops_and_leaves_input_rows_without_pairs():
    """p = d (k - 1) (k3s2p2) crops at both ends: the corner row keeps one tap of 27; one more unit of padding (``BEYOND``) and the rows on
    the grid's low faces have no pair at all -- they contribute nothing, and the lists still agree with the dense reference"""
    cnt = T.product_counts('k3s2p2', 'block_in_corner_0')
    assert float(cnt['dx'].min()) == 1 and float(cnt['dx'].max()) > 1
    shape = T.scene('block_in_corner_0')[2]
    assert tuple(_lib_out_shape(T.BEYOND, shape)) == T.out_shape(shape, T.BEYOND) == tuple(2 * e - 5 for e in shape)
    cnt = T.product_counts(T.BEYOND, 'block_in_corner_0')
    assert float(cnt['dx'].min()) == 0 and float(cnt['dx'].max()) > 0
    inp = T.make_inputs(T.BEYOND, 'block_in_corner_0', 3, 5, seed=4)
    ref, got = T.reference(inp, T.BEYOND, 'block_in_corner_0'), T.pair_sum(inp, T.BEYOND, 'block_in_corner_0')
    assert all(float((got[q] - ref[q]).abs().max()) <= 1e-12 * max(1.0, float(ref[q].abs().max())) for q in ref)
    assert T.same_lists(T.brute(T.BEYOND, 'block_in_corner_0')[2], T.forward_lists(T.BEYOND, 'block_in_corner_0'))


@pytest.mark.parametrize('sabotage', ['flip', 'drop_q'])
def test_sabotaged_lists_are_caught(sabotage):
    cfg, name = 'k3s2p1q1', 'block_in_far_corner'        # the far faces of the output grid exist only through q
    inp = T.make_inputs(cfg, name, 3, 5, seed=2)
    ref = T.reference(inp, cfg, name)
    oc, oshape, pairs = T.brute(cfg, name, flip=sabotage == 'flip', drop_q=sabotage == 'drop_q')
    shape = T.scene(name)[2]
    assert tuple(_lib_out_shape(cfg, shape)) == tuple(T.brute(cfg, name)[1])         # the library keeps q
    if sabotage == 'drop_q':
        assert tuple(oshape) != tuple(T.brute(cfg, name)[1]) and len(oc) != len(T.brute(cfg, name)[0])
        return
    got = T.pair_sum(inp, cfg, name, pairs=pairs)
    assert float((got['y'] - ref['y']).abs().max()) > 1e-3


def test_conv_bound_catches_a_wrong_result():
    c = T.case('k3s2p1q1', 'block5', 32, 32)
    assert tuple(_lib_out_shape('k3s2p1q1', T.scene('block5')[2])) == tuple(T.brute('k3s2p1q1', 'block5')[1])
    assert cg.excess(c['ref']['y'].float(), c['ref']['y'], c['bound']['fp32']['y']) <= 1.0
    bad = c['ref']['y'].float().clone()
    bad[3, 5] *= 1.0 + 2.0 ** -10
    assert cg.excess(bad, c['ref']['y'], c['bound']['fp32']['y']) > 1.0


def test_bias_gradient_bound_passes_fp64_sums_and_fails_a_plain_fp32_running_sum():
    from unidet3d_amd import _lib as L
    assert T.bias_rows(L.BIAS_GRAD_ROWS, L.BIAS_GRAD_STEP)[3] == 513         # one row above the first pass's range: the size used here
    for kind in T.BIAS_KINDS:
        dy = T.bias_values(kind, 513, 32)
        ref, bnd = T.bias_grad_reference(dy)
        assert bool(((ref.float().double() - ref).abs() <= bnd).all()), kind
        if kind == 'integer':
            assert torch.equal(T.running_sum_fp32(dy).double(), ref)           # exact in fp32 in any order
    dy = T.bias_values('cancelling', 513, 32)
    ref, bnd = T.bias_grad_reference(dy)
    assert bool(((T.running_sum_fp32(dy).double() - ref).abs() > bnd).any())
    big = T.bias_values('integer', 65537, 32)
    assert float(big.abs().sum(0).max()) < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------- constructors
def test_constructor_takes_ints_triples_and_numpy_integers():
    from unidet3d_amd import sparse as S
    import unidet3d_amd
    assert unidet3d_amd.sparse.SparseConvTranspose3d is S.SparseConvTranspose3d
    m = S.SparseConvTranspose3d(32, 64, np.int64(3), stride=np.array([2, 2, 1]), padding=np.int32(1), output_padding=(1, np.int64(1), 0), dilation=1)
    assert m.geom == (3, 3, 3, 2, 2, 1, 1, 1, 1, 1, 1, 1) and m.output_padding == (1, 1, 0) and all(type(a) is int for a in m.output_padding)
    assert tuple(m.weight.shape) == (64, 3, 3, 3, 32) and m.K == 27 and m.bias is None and m.general
    for cfg in T.CONFIGS:
        k, s, p, q, d = T.geom(cfg)
        m = S.SparseConvTranspose3d(32, 32, **T.layer_args(cfg))
        assert m.geom == (*k, *s, *p, *d) and m.output_padding == q
        for name in ('line_x_33', 'block5_odd_extent'):
            shape = T.scene(name)[2]
            assert tuple(S.convt_out_shape(m.geom, m.output_padding, shape)) == T.out_shape(shape, cfg)
    assert S.SparseConvTranspose3d(32, 32, 3, stride=1, dilation=2, output_padding=1).output_padding == (1, 1, 1)        # q < max(s, d)


@pytest.mark.parametrize('kw,text', [
    (dict(kernel_size=4), '1 <= extent <= 3'), (dict(kernel_size=3, stride=2, output_padding=2), 'smaller than max(stride, dilation)'),
    (dict(kernel_size=3, output_padding=1), 'smaller than max(stride, dilation)'), (dict(kernel_size=3, stride=2, output_padding=-1), 'output padding must be >= 0'),
    (dict(kernel_size=3, stride=2, output_padding=True), 'three ints'), (dict(kernel_size=3, stride=2, output_padding=1.0), 'three ints'),
    (dict(kernel_size=3, stride=2, output_padding=(1, 1)), 'three ints'), (dict(kernel_size=3, stride=2.0), 'three ints'),
    (dict(kernel_size=(3, 0, 3)), '1 <= extent <= 3')])
def test_constructor_refuses_with_the_constraint_in_the_text(kw, text):
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    with pytest.raises(L.U3DError, match=re.escape(text)):
        S.SparseConvTranspose3d(32, 64, **kw)


def test_bias_parameter_on_the_layer_kinds_that_take_one():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    torch.manual_seed(0)
    layers = [S.SparseInverseConv3d(32, 64, (3, 2, 1), indice_key='k', bias=True), S.SparseInverseConv3d(32, 64, 2, indice_key='k', bias=True),
              S.SparseConvTranspose3d(32, 64, 3, stride=2, padding=1, output_padding=1, bias=True), S.SparseConvTranspose3d(32, 64, 1, 2, bias=True)]
    for m in layers:
        lim = 1.0 / (m.K * 32) ** 0.5
        assert isinstance(m.bias, torch.nn.Parameter) and tuple(m.bias.shape) == (64,) and m.bias.dtype == torch.float32 and m.bias.requires_grad
        b = m.bias.detach()
        assert float(b.abs().max()) <= lim and float(b.abs().max()) > lim / 8 and float(b.min()) < 0 < float(b.max())
        assert sorted(m.state_dict()) == ['bias', 'weight']
    for m in (S.SubMConv3d(32, 64, 3), S.SparseConv3d(32, 64, 2, 2, bias=False), S.SparseInverseConv3d(32, 64, 2, indice_key='k'),
              S.SparseConvTranspose3d(32, 64, 2, 2)):
        assert m.bias is None and 'bias' in m._parameters and sorted(m.state_dict()) == ['weight']
        m.load_state_dict({'weight': torch.zeros_like(m.weight)})
    # the submanifold and the strided layer keep their refusal (tests/test_conv_general_cpu.py pins it)
    for make in (lambda: S.SubMConv3d(32, 64, 3, bias=True), lambda: S.SubMConv3d(32, 64, 1, bias=True), lambda: S.SparseConv3d(32, 64, 2, 2, bias=True)):
        with pytest.raises(L.U3DError, match='bias=True'):
            make()


def test_fusion_plan_steps_aside_for_a_bias_and_for_a_transposed_layer():
    from unidet3d_amd import sparse as S
    from unidet3d_amd.spconv_unet import SpConvUNet, fusion_plan
    front = S.SparseSequential(S.SubMConv3d(6, 32, 3, padding=1, indice_key='subm1'))
    back = S.SparseSequential(S.SparseBatchNorm(32), torch.nn.ReLU())
    assert fusion_plan(SpConvUNet([32, 64], block_reps=1), front, back).convs            # the reference shape is planned
    unet = SpConvUNet([32, 64], block_reps=1)
    unet.deconv._modules['2'] = S.SparseInverseConv3d(64, 32, 2, indice_key='spconv1', bias=True)
    assert not fusion_plan(unet, front, back).convs
    unet = SpConvUNet([32, 64], block_reps=1)
    unet.deconv._modules['2'] = S.SparseConvTranspose3d(64, 32, 2, 2, indice_key='up')
    assert not fusion_plan(unet, front, back).convs


# ---------------------------------------------------------------------------------------------------------------- C contracts
def _geom(k=3, s=2, p=1, d=1):
    t = lambda v: [v] * 3 if isinstance(v, int) else list(v)
    return (ctypes.c_int * 12)(*t(k), *t(s), *t(p), *t(d))


def _q(*v):
    return (ctypes.c_int * 3)(*(v if len(v) == 3 else v * 3))


def _refused(rc, code, lib):
    text = lib.u3d_last_error()
    assert rc == code and len(text) > 0, (rc, code, text)
    return text


def test_header_and_binding_agree_on_the_bias_constants():
    from unidet3d_amd import _lib as L
    src = open(os.path.join(ROOT, 'include', 'u3d.h')).read()
    assert int(re.search(r'#define\s+U3D_BIAS_GRAD_ROWS\s+(\d+)', src).group(1)) == L.BIAS_GRAD_ROWS
    assert int(re.search(r'#define\s+U3D_BIAS_GRAD_STEP\s+(\d+)', src).group(1)) == L.BIAS_GRAD_STEP
    l = L.lib()
    for n in (1, L.BIAS_GRAD_ROWS, L.BIAS_GRAD_ROWS + 1, 355867):
        assert l.u3d_bias_grad_ws_bytes(n, 32) == -(-n // L.BIAS_GRAD_ROWS) * 32 * 8
    assert l.u3d_bias_grad_ws_bytes(0, 32) == 0
    from unidet3d_amd.csrc import build as B
    assert 'sparse_bias.hip' in B.SOURCES and 'sparse_bias.hip' not in B.EXTRA
    assert '#pragma clang fp contract(off)' in open(os.path.join(B.HERE, 'sparse_bias.hip')).read()


def test_convt_out_shape_follows_torch_and_refuses_before_any_hip_call():
    from unidet3d_amd import _lib as L
    l = L.lib()
    out = (ctypes.c_int * 3)()
    for cfg in T.CONFIGS:
        k, s, p, q, d = T.geom(cfg)
        for shape in ((40, 3, 3), (5, 5, 5), (9, 6, 7), (1, 1, 1)):
            ref = T.out_shape(shape, cfg)
            rc = l.u3d_convt_out_shape(_geom(k, s, p, d), _q(*q), *shape, out)
            if min(ref) <= 0:
                assert b'empty' in _refused(rc, EINVAL, l)
                continue
            assert rc == 0 and tuple(out) == ref, (cfg, shape)
            assert tuple(F.conv_transpose3d(torch.zeros(1, 1, *shape), torch.zeros(1, 1, *k), stride=s, padding=p, output_padding=q, dilation=d).shape[2:]) == ref
    assert b'output padding' in _refused(l.u3d_convt_out_shape(_geom(), _q(2), 8, 8, 8, out), EINVAL, l)            # q >= max(s, d)
    assert b'output padding' in _refused(l.u3d_convt_out_shape(_geom(), _q(0, -1, 0), 8, 8, 8, out), EINVAL, l)
    assert l.u3d_convt_out_shape(_geom(3, 1, 1, 2), _q(1), 8, 8, 8, out) == 0 and tuple(out) == (11, 11, 11)          # q < d
    assert b'empty' in _refused(l.u3d_convt_out_shape(_geom(3, 2, 2), _q(0), 1, 8, 8, out), EINVAL, l)              # (1 - 1) 2 - 4 + 2 + 1 = -1
    assert b'32-bit' in _refused(l.u3d_convt_out_shape(_geom(3, 2, 1), _q(1), 1 << 30, 8, 8, out), EUNSUPPORTED, l)  # extent formed in int64
    assert b'outside 1..3' in _refused(l.u3d_convt_out_shape(_geom(4), _q(0), 8, 8, 8, out), EUNSUPPORTED, l)        # conv_geom's validation
    assert _refused(l.u3d_convt_out_shape(_geom(3, 0), _q(0), 8, 8, 8, out), EINVAL, l)
    assert _refused(l.u3d_convt_out_shape(_geom(), None, 8, 8, 8, out), EINVAL, l)
    assert _refused(l.u3d_convt_out_shape(_geom(), _q(0), 8, 8, 8, None), EINVAL, l)


def test_convt_mark_validates_before_any_hip_call():
    from unidet3d_amd import _lib as L
    l = L.lib()
    buf = ctypes.create_string_buffer(64)                  # never dereferenced: every call returns before anything reads it
    p = ctypes.addressof(buf)
    assert b'output padding' in _refused(l.u3d_convt_mark(p, 10, _geom(), _q(2), 1, 8, 8, 8, p, None, None), EINVAL, l)
    assert b'empty' in _refused(l.u3d_convt_mark(p, 10, _geom(3, 2, 2), _q(0), 1, 1, 8, 8, p, None, None), EINVAL, l)
    assert _refused(l.u3d_convt_mark(None, 10, _geom(), _q(1), 1, 8, 8, 8, p, None, None), EINVAL, l)
    assert _refused(l.u3d_convt_mark(p, 0, _geom(), _q(1), 1, 8, 8, 8, p, None, None), EINVAL, l)
    assert _refused(l.u3d_convt_mark(p, 10, _geom(), _q(1), 1, 8, 8, 8, p, p, None), EINVAL, l)                       # both forms
    assert _refused(l.u3d_convt_mark(p, 10, _geom(), _q(1), 1, 8, 8, 8, None, None, None), EINVAL, l)                 # neither
    assert b'32-bit' in _refused(l.u3d_convt_mark(p, 10, _geom(), _q(1), 1, 1 << 30, 8, 8, p, None, None), EUNSUPPORTED, l)
    assert b'direct-address' in _refused(l.u3d_convt_mark(p, 10, _geom(), _q(1), 8, 100_000, 100_000, 4096, p, None, None), EUNSUPPORTED, l)
    assert b'hashed' in _refused(l.u3d_convt_mark(p, 10, _geom(), _q(1), 1 << 20, 1 << 24, 1 << 24, 1 << 24, None, p, None), EUNSUPPORTED, l)
    assert b'offsets' in _refused(l.u3d_convt_mark(p, (1 << 31) // 27 + 1, _geom(), _q(1), 1, 8, 8, 8, p, None, None), EUNSUPPORTED, l)


@pytest.mark.parametrize('entry', ['add', 'grad'])
def test_bias_entry_points_validate_before_any_hip_call(entry):
    from unidet3d_amd import _lib as L
    l = L.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(a, b, n, C, ws=p):
        return l.u3d_bias_add(a, b, n, C, None) if entry == 'add' else l.u3d_bias_grad(a, n, C, b, ws, None)
    assert _refused(call(None, p, 4, 32), EINVAL, l) and _refused(call(p, None, 4, 32), EINVAL, l)
    assert _refused(call(p, p, 0, 32), EINVAL, l) and _refused(call(p, p, -1, 32), EINVAL, l)
    for C in (0, 16, 48, 31, 544, 1024):
        assert b'width' in _refused(call(p, p, 4, C), EUNSUPPORTED, l)
    assert b'rows' in _refused(call(p, p, 1 << 31, 32), EUNSUPPORTED, l)
    if entry == 'grad':
        assert b'workspace' in _refused(call(p, p, 4, 32, ws=None), EINVAL, l)


def test_bias_on_a_cpu_tensor_raises():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    with pytest.raises(L.U3DError):
        S.sparse_bias(torch.zeros(4, 32), torch.zeros(32))
    with pytest.raises(L.U3DError):
        S.bias_grad(torch.zeros(4, 32))
    # the bias itself: fp32 [C] on the rows' device, whatever the module was cast to
    for bad in (torch.zeros(32, dtype=torch.float16), torch.zeros(32, dtype=torch.float64), torch.zeros(64), torch.zeros(1, 32)):
        with pytest.raises(L.U3DError, match='the bias must be fp32'):
            S.bias_add_(torch.zeros(4, 32), bad)
