"""The hand-over between the sparse LAYERS (sparse.SparseSequential, spconv_unet.ResidualBlock), checked on the launches themselves:
the batch-norm statistics a convolution's epilogue writes (sparse._EPILOGUE_STATS) reach the norm behind it on the feature tensor
(sparse.attach_stats / stats_of) -- the same buffer, exactly when that tensor is still the one the convolution returned -- and a norm
that finds none makes its own pass.  (tests/test_gpu_kernels.py checks the two kernels' arithmetic, calling them directly.)"""
import functools

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
C = 32
CONV, BN_FWD = 'u3d_spconv_gmm_x3', 'u3d_bn_forward'
PARTIAL, BN_PART, BN_TILES = 16, 3, 4            # positions in the argument lists (include/u3d.h): conv ``bn_partial``; norm ``partial``, ``n_tiles``


def _rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@functools.lru_cache(maxsize=None)
def _geometry(n_points, vs):
    """two synthetic scenes, voxelised as in test_batchnorm_statistics_from_the_convolution_epilogue; input rows and output gradient"""
    from unidet3d_amd import ops
    from unidet3d_amd.synthetic import make_scene
    vb = ops.voxelize([torch.from_numpy(make_scene(51 + i, n_points=n_points).points).to(DEV) for i in range(2)], vs, 128)
    g = torch.Generator().manual_seed(n_points)
    n = vb.coords.shape[0]
    return vb, torch.randn(n, C, generator=g).to(DEV), torch.randn(n, C, generator=g).to(DEV)


ONE_GROUP, GROUPS = (30_000, 0.02), (3_000, 0.05)


def _pin_groups(monkeypatch, n, groups):
    """the plan of a 32 -> 32 SubM convolution over n rows has one / several offset groups; where the row count alone does not give
    that, U3D_GMM_G pins it (as test_workgroup_tile_conv_equals_wave_tile_conv_bit_for_bit does).  Returns the tile height R."""
    from unidet3d_amd import sparse
    if (sparse._plan(C, C, 27, n)[1] == 1) != (groups == 1):
        monkeypatch.setenv('U3D_GMM_G', str(groups))
    R, G = sparse._plan(C, C, 27, n)
    assert (G == 1) == (groups == 1), (n, R, G)
    return R


def _fill(mods, seed):
    g = torch.Generator().manual_seed(seed)
    for m in mods.modules():
        if isinstance(m, nn.Module) and getattr(m, 'weight', None) is not None:
            if m.weight.dim() == 1:
                m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
                m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
            else:
                m.weight.data = torch.randn(m.weight.shape, generator=g) * 0.1
    return mods.to(DEV).train()


def _record(monkeypatch):
    """every ``_lib.call`` from here on as (entry point, arguments) in the returned list"""
    from unidet3d_amd import _lib as L
    log, real = [], L.call

    def call(name, *args):
        log.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(L, 'call', call)
    return log


def _run(monkeypatch, geometry, flag, between=None):
    """One training step of conv -> norm -> ReLU as a SparseSequential (``between``: the two layers run one after the other, with
    ``between`` applied to the tensor that passes from the convolution to the norm).  Returns the forward's launches and every result."""
    from unidet3d_amd import precision as P
    from unidet3d_amd import sparse
    vb, x0, go = _geometry(*geometry)
    net = _fill(sparse.SparseSequential(sparse.SubMConv3d(C, C, 3, indice_key='a'), sparse.SparseBatchNorm(C), nn.ReLU()), 5)
    x = x0.clone().requires_grad_()
    t = sparse.SparseConvTensor(x, vb.coords, vb.spatial_shape, 2, index=vb.index)
    monkeypatch.setattr(sparse, '_EPILOGUE_STATS', flag)
    log = _record(monkeypatch)
    with P.fp32_math('bf16x3'), sparse.conv_ts(False), sparse.conv_rs(False):
        out = net(t) if between is None else sparse.SparseSequential(net[1], net[2])(between(net[0](t)))
        fwd = list(log)
        out.features.backward(go)
    conv, bn = net[0], net[1]
    return dict(fwd=fwd, y=out.features.detach(), dx=x.grad, dw=conv.weight.grad, dg=bn.weight.grad, db=bn.bias.grad,
                rm=bn.running_mean.clone(), rv=bn.running_var.clone())


def _handed_over(fwd):
    """[(the convolution launch's partial pointer, the pointer and tile count the norm behind it got)] of a forward's launches"""
    convs = [a[PARTIAL] for name, a in fwd if name == CONV]
    norms = [(a[BN_PART], a[BN_TILES]) for name, a in fwd if name == BN_FWD]
    assert len(convs) >= len(norms) > 0, [name for name, _ in fwd]
    return convs, norms


def test_sequential_hands_the_epilogue_statistics_to_the_norm_when_one_launch_wrote_them(monkeypatch):
    """(a) one offset group, flag on: the convolution gets a buffer for its per-tile sums and the norm gets that same buffer with
    n_tiles = ceil(n / R); (f) outputs and every gradient agree with the flag-off run to the 2e-6 of the kernel-level test."""
    n = _geometry(*ONE_GROUP)[0].coords.shape[0]
    R = _pin_groups(monkeypatch, n, 1)
    on, off = _run(monkeypatch, ONE_GROUP, True), _run(monkeypatch, ONE_GROUP, False)
    convs, norms = _handed_over(on['fwd'])
    assert len(convs) == len(norms) == 1
    assert convs[0] is not None and norms[0] == (convs[0], (n + R - 1) // R), (convs, norms, n, R)
    assert _handed_over(off['fwd']) == ([None], [(None, 0)])                                # (b), flag off
    for k in ('y', 'dx', 'dw', 'dg', 'db', 'rm', 'rv'):
        print(f'{k}: epilogue statistics vs own pass {_rel(on[k], off[k]):.3e}')
    for k in ('y', 'dx', 'dw', 'dg', 'db', 'rm', 'rv'):
        assert _rel(on[k], off[k]) < 2e-6, (k, _rel(on[k], off[k]))


def test_no_statistics_change_hands_when_the_offsets_are_split_over_groups(monkeypatch):
    """(b) several offset groups: that launch writes no statistics, flag or not -- the convolution and the norm both get NULL"""
    n = _geometry(*GROUPS)[0].coords.shape[0]
    _pin_groups(monkeypatch, n, 9)
    for flag in (True, False):
        assert _handed_over(_run(monkeypatch, GROUPS, flag)['fwd']) == ([None], [(None, 0)]), flag


def test_statistics_do_not_follow_replaced_or_rewritten_features(monkeypatch):
    """(c) features replaced by a new tensor between the convolution and the norm, (d) features written in place (the stale-sum case
    of the version check): the convolution still wrote its sums, the norm gets NULL and makes its own pass -- in (d) with the result
    of the flag-off run on the same values, bit for bit."""
    n = _geometry(*ONE_GROUP)[0].coords.shape[0]
    _pin_groups(monkeypatch, n, 1)

    def replaced(x):
        return x.replace_feature(x.features * 1)

    def in_place(x):
        x.features.mul_(1)
        return x
    off = _run(monkeypatch, ONE_GROUP, False)
    for between in (replaced, in_place):
        got = _run(monkeypatch, ONE_GROUP, True, between)
        convs, norms = _handed_over(got['fwd'])
        assert convs[0] is not None and norms == [(None, 0)], (between.__name__, convs, norms)
        if between is in_place:
            assert all(torch.equal(got[k], off[k]) for k in ('y', 'rm', 'rv'))


def test_residual_block_hands_the_statistics_to_both_of_its_norms(monkeypatch):
    """(e) a ResidualBlock behind a convolution, training mode: its first norm gets the sums of that convolution, its second norm
    those of the block's first convolution -- each the same buffer, with n_tiles = ceil(n / R)."""
    from unidet3d_amd import precision as P
    from unidet3d_amd import sparse
    from unidet3d_amd.spconv_unet import ResidualBlock
    vb, x0, go = _geometry(*ONE_GROUP)
    n = vb.coords.shape[0]
    R = _pin_groups(monkeypatch, n, 1)
    net = _fill(sparse.SparseSequential(sparse.SubMConv3d(C, C, 3, indice_key='a'), ResidualBlock(C, C, indice_key='a')), 9)
    monkeypatch.setattr(sparse, '_EPILOGUE_STATS', True)
    log = _record(monkeypatch)
    with P.fp32_math('bf16x3'), sparse.conv_ts(False), sparse.conv_rs(False):
        out = net(sparse.SparseConvTensor(x0.clone().requires_grad_(), vb.coords, vb.spatial_shape, 2, index=vb.index))
    convs, norms = _handed_over(log)
    assert len(convs) == 3 and len(norms) == 2 and None not in convs and len(set(convs)) == 3, (convs, norms)
    assert norms == [(convs[0], (n + R - 1) // R), (convs[1], (n + R - 1) // R)], (convs, norms)
    assert torch.isfinite(out.features).all()
