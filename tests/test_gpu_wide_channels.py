"""Sparse layers at channel counts beyond the 32-channel five-level U-Net: any multiple of 32 up to 512 (csrc/spconv.hip's run-time
source-channel chunks, csrc/spconv_wgrad_blk.hip's channel-blocked weight gradient, csrc/bn.hip up to 512 columns).
The convolution checks are those of tests/test_gpu_conv_geometry.py, through its own helpers: NaN-poisoned allocations, elementwise
err / bound <= 1 against the float64 dense convolution under the derived bounds of tests/_conv_geometry.py, exact zeros for empty
offsets, the bare addend for rows without pairs -- no tolerance of this file's own.  The batch norm follows
test_gpu_kernels.test_batchnorm_relu_fwd_bwd (1e-5 / 1e-4 against nn.BatchNorm1d).
The channel pairs are the layers of the two U-Nets this width range is for (64 channels x five levels: 64 .. 320 planes, tail blocks up
to 512 -> 256; 32 channels x seven levels: 32 .. 224) plus the corners of the contract (32 <-> 512) and a pair that is a multiple of
32 only (352 -> 288: 32-channel chunks, 32-wide weight-gradient blocks)."""
import ctypes

import pytest
import torch

import _conv_geometry as cg
from test_gpu_conv_geometry import SELECTIONS, _check_case, _fresh, _level, _log, _operands, _plan_refused, _run, _selection

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SUBM_GEOMETRIES = ['single_voxel', 'two_voxels_apart', 'line_x_33', 'line_z_65', 'line_x_129', 'block5', 'block_in_far_corner',
                   'checkerboard8_mod3', 'empty_middle_scene']
DOWN_GEOMETRIES = ['child_5', 'full_cell', 'block5_odd_extent', 'block_odd_mixed_extent', 'line_x_65']
WIDE_SUBM = [(192, 192), (224, 224), (256, 256), (320, 320), (384, 192), (512, 256), (352, 288), (32, 512), (512, 32)]
WIDE_DOWN = [(64, 128), (128, 192), (160, 192), (192, 224), (192, 256), (256, 320)]
PLAN_SHAPES = [(320, 320), (512, 256)]
PLAN_GEOMETRIES = ['line_x_33', 'line_z_65', 'line_x_129', 'block5']


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('cin,cout', WIDE_SUBM)
def test_wide_subm_conv_on_the_degenerate_geometries(cin, cout, sel):
    ratios, bad = _fresh(), []
    with _selection(sel):
        for name in SUBM_GEOMETRIES:
            _check_case('subm', name, cin, cout, sel, ratios, bad)
    _log(sel, 'subm', cin, cout, ratios)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('cin,cout', WIDE_DOWN)
def test_wide_strided_and_inverse_conv_on_the_degenerate_geometries(cin, cout, sel):
    bad = []
    with _selection(sel):
        for op, a, b in (('down', cin, cout), ('inv', cout, cin)):
            ratios = _fresh()
            for name in DOWN_GEOMETRIES:
                _check_case(op, name, a, b, sel, ratios, bad)
            _log(sel, op, a, b, ratios)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('R', [32, 64])
@pytest.mark.parametrize('sel', ['mfma', 'bf16x3', 'bf16', 'bf16-rows'])
def test_wide_conv_under_every_plan(sel, R, monkeypatch):
    """U3D_GMM_R x U3D_GMM_G on the lines and the block, as test_gpu_conv_geometry.test_every_plan_at_every_tile_edge: every plan
    under the same bound, and 1, 3 and 9 offset groups within 2 * bound of each other (27-offset rulebooks: no plan is refused)."""
    monkeypatch.setenv('U3D_GMM_R', str(R))
    bad = []
    ratios = {G: _fresh() for G in (1, 3, 9)}
    with _selection(sel):
        for cin, cout in PLAN_SHAPES:
            for name in PLAN_GEOMETRIES:
                lvl, by_g = _level('subm', name), {}
                n = lvl['n']
                rows = sel == 'bf16-rows'
                for G in (1, 3, 9):
                    monkeypatch.setenv('U3D_GMM_G', str(G))
                    assert not _plan_refused(cin, cout, 27, n, rows, R, G) and not _plan_refused(cout, cin, 27, n, rows, R, G)
                    by_g[G] = _check_case('subm', name, cin, cout, sel, ratios[G], bad, tag=f'R={R} G={G} ')
                bnd = cg.case('subm', name, cin, cout)['bound'][_operands(sel)]
                for G in (3, 9):
                    for k in ('y', 'dx'):
                        d = (by_g[G][k].double().cpu() - by_g[1][k].double().cpu()).abs()
                        if not bool((d <= 2 * bnd[k]).all()):
                            bad.append(f'R={R} {sel} {cin}->{cout} on {name}: {k} of G={G} and G=1 differ by more than 2 * bound')
    for G in (1, 3, 9):
        _log(sel, 'wide_plans', 0, 0, ratios[G], dict(R=R, G=G))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('sel', ['bf16x3', 'mfma', 'bf16', 'bf16-rows'])
@pytest.mark.parametrize('cin,cout', PLAN_SHAPES)
def test_wide_weight_gradient_is_bit_reproducible(cin, cout, sel):
    """the channel-blocked walk adds its row ranges in a fixed order and issues no floating-point atomic: two runs, equal bits"""
    lvl, case = _level('subm', 'block5'), cg.case('subm', 'block5', cin, cout)
    with _selection(sel):
        a = _run('subm', lvl, case['inp'], sel)
        b = _run('subm', lvl, case['inp'], sel)
    assert bool(torch.isfinite(a['dw']).all()) and float(a['dw'].abs().max()) > 0
    for k in ('dw', 'y', 'dx'):
        assert torch.equal(a[k], b[k]), f'{k} of {cin}->{cout} {sel} differs between two runs'


@pytest.mark.parametrize('sel', SELECTIONS)
def test_rows_of_one_scene_do_not_see_the_other_scene_at_320_channels(sel):
    """test_gpu_conv_geometry.test_rows_of_one_scene_do_not_see_the_other_scene at 320 -> 320"""
    cin = cout = 320
    with _selection(sel):
        lvl, case = _level('subm', 'two_scenes_same_coords'), cg.case('subm', 'two_scenes_same_coords', cin, cout)
        b = lvl['coords'][:, 0]
        clean = _run('subm', lvl, case['inp'], sel)
        for dead in (1, 0):
            x, go = case['inp']['x'].clone(), case['inp']['go'].clone()
            x[b == dead] = float('nan')
            go[b == dead] = float('nan')
            got = _run('subm', lvl, case['inp'], sel, x=x, go=go)
            for k in ('y', 'dx'):
                live = (b != dead).to(DEV)
                where = f'subm {cin}->{cout} {sel}, scene {dead} NaN: {k}'
                assert bool(live.any()) and bool(torch.isfinite(got[k][live]).all()), where
                assert torch.equal(got[k][live], clean[k][live]), where
                assert bool(torch.isnan(got[k][~live]).any()), where          # the NaN did go through the launch


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.mark.parametrize('n', [3, 257, 5003])
@pytest.mark.parametrize('C', [288, 320, 384, 512])
@pytest.mark.parametrize('relu', [True, False])
def test_wide_batchnorm_relu_fwd_bwd(C, relu, n):
    """protocol and tolerances of test_gpu_kernels.test_batchnorm_relu_fwd_bwd"""
    from unidet3d_amd import sparse
    g = torch.Generator().manual_seed(C * 7 + n)
    x = torch.randn(n, C, generator=g) * 2 + 0.5
    go = torch.randn(n, C, generator=g)
    bn_o = torch.nn.BatchNorm1d(C, eps=1e-4, momentum=0.1)
    bn_o.weight.data = torch.rand(C, generator=g) + 0.5; bn_o.bias.data = torch.randn(C, generator=g) * 0.1
    bn_g = sparse.SparseBatchNorm(C).to(DEV)
    bn_g.load_state_dict(bn_o.state_dict())
    xo = x.clone().requires_grad_()
    yo = bn_o(xo); yo = torch.relu(yo) if relu else yo
    yo.backward(go)
    xg = x.clone().to(DEV).requires_grad_()
    yg = bn_g(xg, relu=relu); yg.backward(go.to(DEV))
    errs = dict(y=_rel(yg, yo), dx=_rel(xg.grad, xo.grad), dgamma=_rel(bn_g.weight.grad, bn_o.weight.grad), dbeta=_rel(bn_g.bias.grad, bn_o.bias.grad),
                mean=_rel(bn_g.running_mean, bn_o.running_mean), var=_rel(bn_g.running_var, bn_o.running_var))
    print('wide_bn', dict(C=C, n=n, relu=relu, **errs))
    assert errs['y'] < 1e-5 and errs['dx'] < 1e-4, errs
    assert errs['dgamma'] < 1e-4 and errs['dbeta'] < 1e-4, errs
    assert errs['mean'] < 1e-5 and errs['var'] < 1e-5, errs
    assert int(bn_g.num_batches_tracked) == int(bn_o.num_batches_tracked) == 1
    bn_o.eval(); bn_g.eval()
    with torch.no_grad():
        ye = bn_o(x); ye = torch.relu(ye) if relu else ye
        assert _rel(bn_g(x.to(DEV), relu=relu), ye) < 1e-5


def test_widths_outside_the_contract_are_still_refused():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse
    R, G = ctypes.c_int(0), ctypes.c_int(0)
    for cs, cd in ((48, 32), (32, 48), (544, 32), (32, 544)):
        for fn in (L.lib().u3d_spconv_plan, L.lib().u3d_spconv_plan_bf16a):
            assert fn(cs, cd, 27, 1000, ctypes.byref(R), ctypes.byref(G)) < 0, (cs, cd)
        with pytest.raises(L.U3DError, match='unsupported'):
            sparse._plan(cs, cd, 27, 1000)
    for cs, cd in ((16, 64), (224, 224), (512, 512), (32, 512), (512, 32)):
        assert L.lib().u3d_spconv_plan(cs, cd, 27, 1000, ctypes.byref(R), ctypes.byref(G)) == 0, (cs, cd)
