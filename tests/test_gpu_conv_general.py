"""General sparse-convolution layers (kernel extents 1..3 per axis, stride, padding, dilation) on the device.
Geometry: for every configuration x scene of tests/_conv_general.py the output rows, output shape, pair counts and all K pair lists
of csrc/rulebook.hip's general builder are bit-equal to the brute-force reference, under the bitmap and under the hashed index; the
builder reproduces the two hard-coded rulebooks where its geometry is theirs.
Numerics: y, dx, dW and the addend gradient of ``sparse_conv`` over those rulebooks (n_in != n_out at K = 27; K in {1, 4, 6, 8, 9}), forward
and inverse roles, ELEMENTWISE inside the derived bound of tests/_conv_geometry.py against the float64 dense reference, on NaN-poisoned
allocations.  Modules: a small stack runs forward and backward with the predicted shapes and indices, bit-identical across runs; the
U-Net's own two layer shapes still launch exactly the entry points they launched before the general builder existed.
The largest err / bound per kernel selection goes to the parity log (_parity.log_errors, test 'conv_general')."""
import json
import os

import numpy as np
import pytest
import torch

import _conv_general as G
import _conv_geometry as cg
import _parity
from test_gpu_conv_geometry import _groups, _operands, _poison, _selection

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SELECTIONS = ['bf16x3', 'bf16x3-wavetile', 'mfma', 'bf16', 'bf16-rows']        # ('-ts' is SubM k=3 only)
CHANNELS = [(16, 32), (32, 64), (64, 96), (160, 192)]


def _geom12(cfg):
    """the 12 integers the layer of this configuration hands to the builder, and the submanifold flag"""
    from unidet3d_amd import sparse
    subm = (G.CONFIGS[cfg] if isinstance(cfg, str) else cfg)[4]
    if subm:
        return sparse.SubMConv3d(32, 32, **G.layer_args(cfg))._subm_geom, True
    return sparse.SparseConv3d(32, 32, **G.layer_args(cfg)).geom, False


def _same_lists(got, ref, where):
    assert len(got) == len(ref), where
    for k, ((gi, go), (ri, ro)) in enumerate(zip(got, ref)):
        assert np.array_equal(gi, ri) and np.array_equal(go, ro), f'{where}: offset {k} differs'


def _build(cfg, name):
    """the device level of ``cfg`` on scene ``name``, every part bit for bit the brute-force reference's"""
    from unidet3d_amd import sparse
    _, B, shape, coords = G.scene(name)
    ix = sparse.OccupancyIndex.from_coords(coords.to(DEV), B, shape)
    n = ix.count()
    rows = ix.coords(n)
    assert n == len(coords) and torch.equal(rows.cpu(), coords), f'{name}: canonical rows'
    g12, subm = _geom12(cfg)
    oc, oshape, ix_out, rb = sparse.build_conv_rulebook(rows, ix, B, shape, g12, subm=subm)
    roc, roshape, rpairs = G.brute(cfg, name)
    where = f'{cfg} on {name}'
    assert list(oshape) == list(roshape), where
    assert oc.dtype == torch.int32 and torch.equal(oc.cpu(), roc), where
    assert (rb.K, rb.n_in, rb.n_out) == (len(rpairs), n, len(roc)) and rb.cap >= min(n, len(roc)), where
    assert rb.counts.cpu().tolist() == [len(i) for i, _ in rpairs], where
    _same_lists(rb.lists(), rpairs, where)
    assert rb.coords is None and rb.index is None, where           # never the tile-stationary kernels' tables
    assert ix_out.hashed == ix.hashed and ix_out.count() == len(roc), where
    return dict(rb=rb, n=n, n2=len(roc), oc=oc, index=ix_out)


_LEVELS = {}


def _level(cfg, name):
    if (cfg, name) not in _LEVELS:
        _LEVELS[(cfg, name)] = _build(cfg, name)
    return _LEVELS[(cfg, name)]


@pytest.mark.parametrize('cfg', list(G.CONFIGS))
def test_geometry_equals_the_brute_force_reference_bit_for_bit(cfg):
    for name in G.SCENES:
        assert not _level(cfg, name)['index'].hashed


@pytest.mark.parametrize('cfg', list(G.CONFIGS))
def test_geometry_under_the_hashed_index(cfg, monkeypatch):
    from unidet3d_amd import geometry
    monkeypatch.setattr(geometry, '_INDEX_MODE', 'hash')
    for name in G.SCENES:
        assert _build(cfg, name)['index'].hashed


@pytest.mark.parametrize('mode', ['bitmap', 'hash'])
def test_general_builder_reproduces_the_two_hard_coded_rulebooks(mode, monkeypatch):
    from unidet3d_amd import geometry, sparse
    monkeypatch.setattr(geometry, '_INDEX_MODE', mode)
    for name in G.SCENES:
        _, B, shape, coords = G.scene(name)
        rows = coords.to(DEV)
        ix = sparse.OccupancyIndex.from_coords(rows, B, shape)
        assert ix.hashed == (mode == 'hash')
        oc, oshape, ix2, rb = sparse.build_down_rulebook(rows, B, shape)
        goc, goshape, gix2, grb = sparse.build_conv_rulebook(rows, ix, B, shape, sparse.conv_geometry(2, 2, 0, 1))
        assert ix2.hashed == gix2.hashed == (mode == 'hash')
        assert torch.equal(oc, goc) and list(oshape) == list(goshape) and torch.equal(rb.counts, grb.counts), name
        _same_lists(grb.lists(), rb.lists(), f'k2s2 on {name}')
        rb = sparse.build_subm_rulebook(rows, ix)
        grb = sparse.build_conv_rulebook(rows, ix, B, shape, _geom12(G.SUBM_K3)[0], subm=True)[3]
        assert torch.equal(rb.counts, grb.counts) and grb.cap == rb.cap, name
        _same_lists(grb.lists(), rb.lists(), f'subm k3 on {name}')


# ---------------------------------------------------------------------------------------------------------------- numerics
def _run(mode, lvl, inp, sel):
    """forward (+ addend) and backward of ``sparse_conv`` over the level's rulebook -> dict(y, dx, dw, dadd) on the device"""
    from unidet3d_amd import sparse
    rb = lvl['rb']
    cout, cin = inp['w'].shape[0], inp['w'].shape[-1]
    rows = sel == 'bf16-rows'
    xg = inp['x'].to(DEV).clone().requires_grad_(cin != 16)         # 16 channels: the padded network input, whose gradient is not built
    wg, ag, gg = inp['w'].to(DEV).clone().requires_grad_(), inp['add'].to(DEV).clone().requires_grad_(), inp['go'].to(DEV).clone()
    if rows and cin % 32 == 0:
        sparse.attach_shadow(xg, sparse.to_shadow(xg))
    if rows and cout % 32 == 0:
        sparse.attach_shadow(gg, sparse.to_shadow(gg))
    ns, nd = xg.shape[0], gg.shape[0]
    assert (ns, nd) == ((rb.n_in, rb.n_out) if mode == 'fwd' else (rb.n_out, rb.n_in))
    _poison([nd * cout, _groups(cin, cout, rb.K, nd, rows and cin % 32 == 0) * nd * cout])
    y = sparse.sparse_conv(xg, wg, rb, mode, ag)
    _poison([ns * cin, wg.numel(), (_groups(cout, cin, rb.K, ns, rows) if cin != 16 else 1) * ns * cin, nd * cout])
    y.backward(gg)
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xg.grad, dw=wg.grad, dadd=ag.grad)


def _check_case(mode, cfg, name, cin, cout, sel, ratios, bad):
    lvl, case = _level(cfg, name), G.case(mode, cfg, name, cin, cout)
    got = _run(mode, lvl, case['inp'], sel)
    bnd = case['bound'][_operands(sel)]
    where = f'{mode} {cfg} {cin}->{cout} {sel} on {name}'
    for k in ('y', 'dx', 'dw', 'dadd'):
        if k == 'dx' and cin == 16:
            assert got['dx'] is None, where
            continue
        r = cg.excess(got[k], case['ref'][k], bnd[k])
        print(f'conv_general {where}: {k} err / bound = {r:.3g}')
        if r >= ratios[k][0]:
            ratios[k] = (r, f'{cfg} {name}')
        if not r <= 1.0:
            bad.append(f'{where}: {k} err / bound = {r:.3g}')
    # nothing left unwritten: an offset without pairs has an exactly zero dW slice, a row without pairs is exactly its addend
    dw = got['dw'].reshape(cout, lvl['rb'].K, cin)
    for k in np.nonzero(case['counts']['dw'].numpy() == 0)[0]:
        if not bool((dw[:, int(k), :] == 0).all()):
            bad.append(f'{where}: dW of the empty offset {int(k)} is not 0')
    lonely = (case['counts']['y'] == 0).nonzero().flatten().to(DEV)
    if len(lonely) and not torch.equal(got['y'][lonely], case['inp']['add'].to(DEV)[lonely]):
        bad.append(f'{where}: rows without pairs differ from the addend')


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('mode', ['fwd', 'inv'])
@pytest.mark.parametrize('cin,cout', CHANNELS)
def test_sparse_conv_over_general_rulebooks(cin, cout, mode, sel):
    """every configuration on every scene at every channel pair; weights [cout, k.., cin] in both modes: 'fwd' reads the input level,
    'inv' reads the output level and writes the input level (SparseInverseConv3d's roles)"""
    ratios, bad = {k: (0.0, None) for k in ('y', 'dx', 'dw', 'dadd')}, []
    with _selection(sel):
        for cfg in G.CONFIGS:
            for name in G.SCENES:
                _check_case(mode, cfg, name, cin, cout, sel, ratios, bad)
    rec = dict(selection=sel, mode=mode, cin=cin, cout=cout, **{f'{k}_ratio': v[0] for k, v in ratios.items()},
               **{f'{k}_worst': v[1] for k, v in ratios.items()})
    _parity.log_errors('conv_general', rec)
    print('conv_general', rec)
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------------------- modules
def _stack():
    from unidet3d_amd import sparse as S
    torch.manual_seed(5)
    return S.SparseSequential(S.SubMConv3d(32, 32, 3, indice_key='s1'), S.SparseConv3d(32, 64, 3, stride=2, padding=1, indice_key='d'),
                              S.SubMConv3d(64, 64, 3, dilation=2, indice_key='s2'), S.SparseInverseConv3d(64, 32, 3, indice_key='d')).to(DEV)


def _forward_backward(net, name, train):
    from unidet3d_amd import sparse as S
    _, B, shape, coords = G.scene(name)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(len(coords), 32, generator=g).to(DEV).requires_grad_()
    net.train(train)
    net.zero_grad(set_to_none=True)
    x = S.SparseConvTensor(feats, coords.to(DEV), shape, B)
    y = net(x)
    y.features.backward(torch.randn(y.features.shape, generator=g).to(DEV))
    torch.cuda.synchronize()
    return x, y, [y.features.detach().clone(), feats.grad.clone()] + [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize('name', ['empty_middle_scene', 'block5_odd_extent', 'line_x_65'])
def test_module_stack_runs_forward_and_backward(name):
    net = _stack()
    _, B, shape, coords = G.scene(name)
    x, y, first = _forward_backward(net, name, True)
    # the output is back on the input level; the strided level is the reference's
    assert y.spatial_shape == list(shape) and y.batch_size == B and torch.equal(y.indices.cpu(), coords) and tuple(y.features.shape) == (len(coords), 32)
    oc, oshape, ix2, rb = x.indice_dict[('__down__', 'd')]
    roc, roshape, rpairs = G.brute('k3s2p1', name)
    assert torch.equal(oc.cpu(), roc) and list(oshape) == list(roshape)
    _same_lists(rb.lists(), rpairs, name)
    assert rb.tag == ('__down__', 'd') and rb.coords is None and x.indice_dict['d'][0] is rb and (rb.K, rb.n_in, rb.n_out) == (27, len(coords), len(roc))
    assert x.indice_dict['s1'].coords is not None and x.indice_dict['s1'].K == 27           # the hard-coded SubM rulebook, as before
    s2 = x.indice_dict['s2']
    assert s2.coords is None and s2.tag == ('subm', 's2') and (s2.n_in, s2.n_out) == (len(roc), len(roc))
    # geometry() ahead of the feature pass gives the same entries (prepare_geometry's use)
    assert net[1].geometry(x)[3] is rb and net[2].geometry(y.__class__(None, oc, oshape, B, x.indice_dict, ix2)) is s2
    for t in first:
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    for train in (True, False, False):
        again = _forward_backward(net, name, train)[2]
        assert len(again) == len(first) and all(torch.equal(a, b) for a, b in zip(again, first)), f'{name}: train={train} differs between runs'


def test_unet_with_a_general_down_layer_runs_unfused_with_the_same_bits(monkeypatch):
    """SpConvUNet with its k=2 / s=2 pair swapped for SparseConv3d(3, s=2, p=1) + its inverse, eval mode under no_grad: the fusion
    plan is empty, no launch goes through the epilogue entry point with the toggle on, and the results are those of the toggle off"""
    from torch import nn
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    from unidet3d_amd.spconv_unet import SpConvUNet, begin_fusion, fusion_plan
    torch.manual_seed(9)
    front = S.SparseSequential(S.SubMConv3d(6, 32, 3, padding=1, indice_key='subm1'))
    unet = SpConvUNet([32, 64], block_reps=2)
    unet.conv._modules['2'] = S.SparseConv3d(32, 64, 3, stride=2, padding=1, indice_key='spconv1')
    unet.deconv._modules['2'] = S.SparseInverseConv3d(64, 32, 3, indice_key='spconv1')
    back = S.SparseSequential(S.SparseBatchNorm(32), nn.ReLU())
    net = nn.ModuleList([front, unet, back]).to(DEV).eval()
    assert not fusion_plan(unet, front, back).convs
    names, real = [], L.call

    def recorder(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, 'call', recorder)
    _, B, shape, coords = G.scene('empty_middle_scene')
    feats = torch.randn(len(coords), 6, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = {}
    with torch.no_grad():
        for on in (False, True):
            with S.fused_inference(on):
                del names[:]
                x = S.SparseConvTensor(feats, coords.to(DEV), shape, B)
                begin_fusion(x, unet, front, back)
                out[on] = back(unet(front(x))).features
                assert 'u3d_spconv_gmm_ep' not in names and names.count('u3d_conv_rulebook') == 1 and 'u3d_down_rulebook' not in names, names
    assert tuple(out[True].shape) == (len(coords), 32) and bool(torch.isfinite(out[True]).all()) and float(out[True].abs().max()) > 0
    assert torch.equal(out[True], out[False])
    assert len(net) == 3


def test_unet_layer_shapes_launch_the_entry_points_they_always_did(monkeypatch):
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    _, B, shape, coords = G.scene('block5_odd_extent')
    feats = torch.randn(len(coords), 32).to(DEV)
    torch.manual_seed(3)
    subm = S.SubMConv3d(32, 32, kernel_size=3, padding=1, bias=False, indice_key='subm1').to(DEV)
    down = S.SparseConv3d(32, 64, kernel_size=2, stride=2, bias=False, indice_key='spconv1').to(DEV)
    up = S.SparseInverseConv3d(64, 32, kernel_size=2, bias=False, indice_key='spconv1').to(DEV)
    names, real = [], L.call

    def recorder(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, 'call', recorder)

    def geometry_calls():
        out = [n for n in names if not n.startswith(('u3d_spconv_', 'u3d_weight_pack', 'u3d_tile_starts'))]
        conv = [n for n in names if n.startswith('u3d_spconv_')]
        names.clear()
        return out, conv
    with torch.no_grad():
        x = S.SparseConvTensor(feats, coords.to(DEV), shape, B)
        y = subm(x)
        geo, conv = geometry_calls()
        assert geo == ['u3d_index_mark', 'u3d_index_rank', 'u3d_subm_rulebook'] and len(conv) == 1 and conv[0].startswith('u3d_spconv_gmm'), (geo, conv)
        z = down(y)
        geo, conv = geometry_calls()
        assert geo == ['u3d_index_mark', 'u3d_index_rank', 'u3d_index_coords', 'u3d_down_rulebook'] and len(conv) == 1, (geo, conv)
        up(z)
        geo, conv = geometry_calls()
        assert geo == [] and len(conv) == 1, (geo, conv)
        # and a general layer does go through the new entry points
        S.SparseConv3d(32, 64, 3, stride=2, padding=1, indice_key='g').to(DEV)(y)
        geo, conv = geometry_calls()
        assert geo == ['u3d_conv_out_shape', 'u3d_conv_mark', 'u3d_index_rank', 'u3d_index_coords', 'u3d_conv_rulebook'] and len(conv) == 1, (geo, conv)


GOLDEN_STACK = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'general_stack_launch_names_before_geometry_module.json')


def _cache_key_kind(key):
    """an ``indice_dict`` key without what changes from run to run: the ``id()`` of a keyless layer, the address of the level's rows"""
    if not isinstance(key, tuple):
        return key
    if key[0] == '__index__':
        return ['__index__', list(key[1])]
    return [a[0] if isinstance(a, tuple) else a for a in key if not isinstance(a, int)]


def _general_stack_launches(monkeypatch):
    """The ``L.call`` names, in order, and the ``indice_dict`` keys of one inference pass of every layer kind over one cache: a dilated
    SubM layer, a general strided convolution, a max pool that shares its key, its inverse, a keyed and a keyless transposed layer, at
    32 channels on 'block5_odd_extent' with an empty tile history.  Weight packs and tile lists are left out, as in
    ``test_unet_layer_shapes_launch_the_entry_points_they_always_did``.  The recorded lists are this function run on the commit before
    the geometry moved into its own module."""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    torch.manual_seed(3)
    subm = S.SubMConv3d(32, 32, 3, dilation=2, indice_key='s')
    down = S.SparseConv3d(32, 32, 3, stride=2, padding=1, indice_key='d')
    pool = S.SparseMaxPool3d(3, stride=2, padding=1, indice_key='d')
    inv = S.SparseInverseConv3d(32, 32, 3, indice_key='d')
    up = S.SparseConvTranspose3d(32, 32, 3, stride=2, padding=1, output_padding=1, indice_key='u')
    anon = S.SparseConvTranspose3d(32, 32, 3, stride=2, padding=1, output_padding=1)
    torch.nn.ModuleList([subm, down, pool, inv, up, anon]).to(DEV).eval()
    _, B, shape, coords = G.scene('block5_odd_extent')
    feats = torch.randn(len(coords), 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    names, real = [], L.call

    def recorder(nm, *a):
        names.append(nm)
        return real(nm, *a)
    S._TILE_HISTORY.clear()
    monkeypatch.setattr(L, 'call', recorder)
    with torch.no_grad(), _selection('bf16x3'), S.conv_ts(False), S.conv_rs(False):
        x = S.SparseConvTensor(feats, coords.to(DEV), shape, B)
        y = subm(x)
        z = down(y)
        p = pool(y)
        w = inv(z)
        t = anon(up(w))
    torch.cuda.synchronize()
    monkeypatch.setattr(L, 'call', real)
    assert torch.equal(p.indices, z.indices) and torch.equal(w.indices, x.indices) and t.spatial_shape == [4 * s for s in shape]
    assert all(bool(torch.isfinite(v.features).all()) for v in (p, w, t)) and float(t.features.abs().max()) > 0
    keys = sorted((_cache_key_kind(k) for k in x.indice_dict), key=str)
    return dict(names=[nm for nm in names if not nm.startswith(('u3d_weight_pack', 'u3d_tile_starts'))], keys=keys)


@pytest.mark.parametrize('mode', ['bitmap', 'hash'])
def test_mixed_stack_launches_and_caches_exactly_what_it_did_before(mode, monkeypatch):
    from unidet3d_amd import geometry
    monkeypatch.setattr(geometry, '_INDEX_MODE', mode)
    before = json.load(open(GOLDEN_STACK))[mode]
    got = _general_stack_launches(monkeypatch)
    assert len(before['names']) > 20 and (mode == 'hash') == ('u3d_hash_index_build' in got['names']) == ('u3d_index_rank' not in got['names'])
    assert got['names'] == before['names'], [(i, a, b) for i, (a, b) in enumerate(zip(got['names'], before['names'])) if a != b][:5]
    assert got['keys'] == before['keys']
