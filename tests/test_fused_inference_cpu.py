"""Host side of the fused inference path, no GPU: the successor plan ``spconv_unet.fusion_plan`` (which convolution
writes which norm, and which column block of the U-Net's concat buffers), the eval-mode (scale, shift) cache of ``SparseBatchNorm``,
the header / ctypes agreement on the added entry point and its struct, and the refusals of ``u3d_spconv_gmm_ep`` (decided before
anything touches a device)."""
import ctypes
import os
import re

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(planes, **kw):
    from unidet3d_amd.sparse import SparseBatchNorm, SparseSequential, SubMConv3d
    from unidet3d_amd.spconv_unet import SpConvUNet
    unet = SpConvUNet(planes, block_reps=2, **kw)
    front = SparseSequential(SubMConv3d(6, planes[0], 3, padding=1, indice_key='subm1'))
    back = SparseSequential(SparseBatchNorm(planes[0]), nn.ReLU())
    return front, unet, back


def _expected(planes, prefix='', feed='<first_producer>', sink='<last_consumer>'):
    """{norm: [(producer, lo, hi)]} and {convolution: (raw, [(norm, where)])} of a pre-activation U-Net with two blocks per stage, written
    out from the layer order: conv1 -> the block's second norm; conv2 -> the next block's first norm; the end of ``blocks`` -> the norm
    of ``conv`` and columns [0, c) of the concatenation; the down convolution -> the inner level; the inner level's last convolution ->
    ``deconv``'s norm; the inverse convolution -> columns [c, 2c)."""
    c = planes[0]
    me = prefix[:-1] if prefix else '<unet>'
    norms, convs = {}, {}

    def stage(name, prod, width, first_planned=False):
        for i in range(2):
            b = f'{prefix}{name}.block{i}.conv_branch.'
            if not (first_planned and i == 0):
                norms[b + '0'] = [(prod, 0, width)]
                convs[prod][1].append((b + '0', None))
            norms[b + '3'] = [(b + '2', 0, c)]
            convs[b + '2'] = (None, [(b + '3', None)])
            convs[b + '5'] = ('own', [])
            prod, width = b + '5', c
        return prod

    convs.setdefault(feed, ('own', []))
    last = stage('blocks', feed, c)
    if len(planes) > 1:
        tail0 = f'{prefix}blocks_tail.block0.conv_branch.0'
        convs[last] = ((me, 0), [(f'{prefix}conv.0', None), (tail0, (me, 0))])
        norms[f'{prefix}conv.0'] = [(last, 0, c)]
        convs[f'{prefix}conv.2'] = ('own', [])
        n2, c2 = _expected(planes[1:], f'{prefix}u.', f'{prefix}conv.2', f'{prefix}deconv.0')
        for k, v in c2.items():
            if k in convs:
                convs[k][1].extend(v[1])
            else:
                convs[k] = v
        norms.update(n2)
        convs[f'{prefix}deconv.2'] = ((me, c), [(tail0, (me, c))])
        norms[tail0] = [(last, 0, c), (f'{prefix}deconv.2', c, 2 * c)]
        last = stage('blocks_tail', None, 2 * c, first_planned=True)
    norms[sink] = [(last, 0, c)]
    convs[last][1].append((sink, None))
    return norms, convs


def test_plan_of_a_three_level_and_a_one_level_net():
    from unidet3d_amd.sparse import SparseBatchNorm
    from unidet3d_amd.spconv_unet import fusion_plan
    for planes in ([32, 64, 96], [32]):
        front, unet, back = _net(planes, return_blocks=True)
        plan = fusion_plan(unet, front, back)
        assert fusion_plan(unet, front, back) is plan                                     # cached on the module
        every = [m for m in unet.modules() if isinstance(m, SparseBatchNorm)] + [back[0]]
        assert len(plan.norms) == len(every) and set(plan.norms) == set(every)            # every norm exactly once (a dict: no repeats)
        norms, convs = plan.describe()
        want_n, want_c = _expected(planes)
        assert dict(norms) == want_n
        assert convs == want_c
        assert all(e.fused and e.relu for e in plan.norms.values())
        assert all(len(e.acts) <= 2 for e in plan.convs.values())
        assert set(plan.cats) == {m for m in unet.modules() if hasattr(m, 'blocks_tail')}
        for u, cat in plan.cats.items():
            assert cat.width == 2 * u.num_planes[0] and cat.norm is u.blocks_tail[0].conv_branch[0]
        # column blocks of a norm are disjoint and cover its width
        for n, e in plan.norms.items():
            assert sorted((lo, hi) for _, lo, hi in e.producers)[0][0] == 0
            assert sum(hi - lo for _, lo, hi in e.producers) == n.num_features


def test_plan_without_known_neighbours_leaves_the_first_norm_unfused():
    from unidet3d_amd.spconv_unet import fusion_plan
    _, unet, _ = _net([32, 64])
    plan = fusion_plan(unet)
    first = unet.blocks[0].conv_branch[0]
    assert plan.norms[first].producers == [] and not plan.norms[first].fused
    assert sum(not e.fused for e in plan.norms.values()) == 1
    last = unet.blocks_tail[1].conv_branch[5]
    assert plan.convs[last].raw == 'own' and plan.convs[last].acts == []


def test_post_activation_and_foreign_blocks_get_an_empty_plan():
    from unidet3d_amd.spconv_unet import ResidualBlock, fusion_plan

    class Other(ResidualBlock):
        pass
    for kw in (dict(normalize_before=False), dict(block=Other)):
        front, unet, back = _net([32, 64], **kw)
        plan = fusion_plan(unet, front, back)
        assert not plan.convs and not plan.norms and not plan.cats


def test_eval_affine_is_cached_by_parameter_and_buffer_version():
    from unidet3d_amd.sparse import SparseBatchNorm
    g = torch.Generator().manual_seed(3)
    bn = SparseBatchNorm(32, eps=1e-4)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(32, generator=g))
        bn.bias.copy_(torch.randn(32, generator=g))
        bn.running_mean.copy_(torch.randn(32, generator=g))
        bn.running_var.copy_(torch.rand(32, generator=g) * 1.5 + 0.5)

    def torch_expressions():          # the eval arm of sparse._BNReLUFn.forward
        invstd = torch.rsqrt(bn.running_var + bn.eps)
        scale = bn.weight.detach() * invstd
        return scale, bn.bias.detach() - bn.running_mean * scale

    bn.eval()
    with torch.no_grad():                                                                # inference
        pair = bn.eval_affine()
        assert all(torch.equal(a, b) for a, b in zip(pair, torch_expressions()))
        assert not pair[0].requires_grad and not pair[1].requires_grad
        for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
            same = bn.eval_affine()
            assert same[0] is pair[0] and same[1] is pair[1]
            t.mul_(1.25).add_(0.125)                                                     # bumps ``_version``
            new = bn.eval_affine()
            assert new[0] is not pair[0]
            assert all(torch.equal(a, b) for a, b in zip(new, torch_expressions()))
            assert not torch.equal(new[1], pair[1])
            pair = new
        bn.running_mean.data.add_(1.0)                                                   # through .data: the version does not move ...
        assert bn.eval_affine()[0] is pair[0]
        bn.invalidate_affine()                                                           # ... such writers say so
        assert all(torch.equal(a, b) for a, b in zip(bn.eval_affine(), torch_expressions()))


def test_eval_affine_does_not_outlive_what_moves_behind_the_version_counter():
    """the statistics kernels and a fused optimizer write running buffers / parameters without bumping ``_version``: a training-mode
    forward drops the cached rows, and rows computed with autograd on over trainable weight / bias are never reused"""
    from unidet3d_amd.sparse import SparseBatchNorm
    bn = SparseBatchNorm(32).eval()
    with torch.no_grad():
        first = bn.eval_affine()
        assert bn.eval_affine()[0] is first[0]
    with torch.enable_grad():                                                            # frozen-statistics fine-tuning: an optimizer may step
        a = bn.eval_affine()
        bn.weight.data.mul_(2.0)                                                         # what fused AdamW does: no version bump
        b = bn.eval_affine()
        assert b[0] is not a[0] and torch.equal(b[0], 2.0 * a[0])
        bn.weight.data.mul_(0.5)
    with torch.no_grad():
        c = bn.eval_affine()                                                             # the first inference call after that recomputes ...
        assert c[0] is not b[0] and torch.equal(c[0], first[0])
        assert bn.eval_affine()[0] is c[0]                                               # ... and is cached again
        bn.train()
        try:
            bn(torch.zeros(4, 32))                                                       # CPU tensor: refused (no fallback) ...
        except RuntimeError:                                                             # (U3DError, or torch's own without a device)
            pass
        assert bn._affine_cache is None                                                  # ... after the training-mode forward dropped the rows


def test_invalidate_weight_packs_drops_the_affine_caches():
    from unidet3d_amd.sparse import SparseBatchNorm
    from unidet3d_amd.unidet3d import UniDet3D
    bn = SparseBatchNorm(32)
    host = nn.Module()
    host.bn, host._packs = bn, None
    pair = bn.eval_affine()
    UniDet3D.invalidate_weight_packs(host)
    assert bn.eval_affine()[0] is not pair[0]
    assert 'eval_affine' in UniDet3D.invalidate_weight_packs.__doc__


def test_toggle_returns_the_previous_value_and_the_context_restores_it():
    from unidet3d_amd import sparse
    prev = sparse.set_fused_inference(False)
    try:
        assert sparse.set_fused_inference(True) is False and sparse._FUSED_INFERENCE is True
        with sparse.fused_inference(False):
            assert sparse._FUSED_INFERENCE is False
            assert not sparse.fusion_active()
        assert sparse._FUSED_INFERENCE is True
        with torch.no_grad():
            assert sparse.fusion_active(nn.ReLU().eval()) and not sparse.fusion_active(nn.ReLU().train())
        with torch.enable_grad():
            assert not sparse.fusion_active()
        # None, the default: on, except where inference gathers the bf16 shadows that only u3d_bn_apply writes
        from unidet3d_amd import precision as P
        assert sparse.set_fused_inference(None) is True
        with torch.no_grad():
            assert sparse.fusion_active()
            with P.operands('bf16'), P.bf16_rows_mode(True):
                assert not sparse.fusion_active()
                with sparse.fused_inference(True):
                    assert sparse.fusion_active()
            with P.operands('bf16'), P.bf16_rows_mode(False):
                assert sparse.fusion_active()
    finally:
        sparse.set_fused_inference(prev)


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'u3d.h')).read(), flags=re.S)


def test_header_and_ctypes_agree_on_the_added_entry_point():
    """the mechanism of tests/test_cabi.py (parameter count of the prototype against the ctypes table), and the struct field by field"""
    from unidet3d_amd import _lib
    src = _header()
    res, args = _lib.PROTOTYPES['u3d_spconv_gmm_ep']
    m = re.search(r'\bu3d_spconv_gmm_ep\s*\((.*?)\)\s*;', src, flags=re.S)
    assert m
    params = [p.strip() for p in m.group(1).split(',') if p.strip()]
    assert len(params) == len(args) and res is ctypes.c_int
    assert args[[p.split()[-1].lstrip('*') for p in params].index('ep')] == ctypes.POINTER(_lib.ConvEpilogue)
    body = re.search(r'typedef\s+struct\s+u3d_conv_epilogue\s*\{(.*?)\}\s*u3d_conv_epilogue\s*;', src, flags=re.S).group(1)
    fields = []
    for decl in [d.strip() for d in body.split(';') if d.strip()]:
        ctype = ctypes.c_void_p if '*' in decl else (ctypes.c_int64 if 'int64_t' in decl else ctypes.c_int)
        for name in re.sub(r'^(const\s+)?\w+\s*\*?', '', decl).split(','):
            n = re.match(r'\s*\*?\s*(\w+)\s*(?:\[(\d+)\])?', name)
            fields.append((n.group(1), ctype * int(n.group(2)) if n.group(2) else ctype))
    got = [(n, t) for n, t in _lib.ConvEpilogue._fields_]
    assert [n for n, _ in got] == [n for n, _ in fields]
    assert [ctypes.sizeof(t) for _, t in got] == [ctypes.sizeof(t) for _, t in fields]
    assert int(re.search(r'#define\s+U3D_ABI_VERSION\s+(\d+)', src).group(1)) == _lib.ABI_VERSION == 117      # added entry point: unchanged


def test_epilogue_refusals_are_decided_before_any_device_call():
    from unidet3d_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(64)                    # never dereferenced
    p = ctypes.addressof(buf)
    Cd = 32

    def call(ep, fmt=2, bn_partial=None):
        return l.u3d_spconv_gmm_ep(fmt, p, 100, p, p, p, p, 27, 100, 32, Cd, 100, 64, 1, None, None, bn_partial, ctypes.byref(ep), 0.0, None)

    def ep(raw=p, ld=Cd, col=0, n_act=0, act_ld=Cd, act_col=0):
        e = _lib.ConvEpilogue()
        e.raw, e.raw_ld, e.raw_col, e.n_act = raw, ld, col, n_act
        for j in range(min(n_act, 2)):
            e.act[j], e.scale[j], e.shift[j], e.act_ld[j], e.act_col[j] = p, p, p, act_ld, act_col
        return e
    EINVAL, EUNSUPPORTED = -1, -3
    assert call(ep(ld=Cd - 4)) == EINVAL and b'raw output' in l.u3d_last_error()           # leading dimension below Cd
    assert call(ep(ld=Cd + 2)) == EINVAL                                                   # not a multiple of 4 floats
    assert call(ep(ld=Cd + 8, col=6)) == EINVAL
    assert call(ep(ld=Cd + 4, col=8)) == EINVAL                                            # the block runs past the row
    assert call(ep(n_act=1, act_ld=Cd - 4)) == EINVAL and b'activated output 0' in l.u3d_last_error()
    assert call(ep(n_act=2, act_ld=Cd + 6)) == EINVAL
    assert call(ep(n_act=1, act_ld=Cd + 8, act_col=2)) == EINVAL
    assert call(ep(n_act=3)) == EUNSUPPORTED and b'at most two' in l.u3d_last_error()
    assert call(ep(raw=None)) == EINVAL and b'no output' in l.u3d_last_error()
    assert call(ep(n_act=1), bn_partial=p) == EUNSUPPORTED and b'exclude each other' in l.u3d_last_error()
    assert call(ep(), fmt=4) == EINVAL
    assert l.u3d_spconv_gmm_ep(2, p, 100, p, p, p, p, 27, 100, 32, Cd, 100, 64, 1, None, None, None, None, 0.0, None) == EINVAL
