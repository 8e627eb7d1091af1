"""Sparse transposed convolution and the bias of the sparse convolution layers on the device.
Geometry: for every configuration x scene of tests/_conv_transpose.py the output rows, output shape, pair counts and all K pair lists
of ``build_convt_rulebook`` are bit-equal to the brute-force reference, under the bitmap and under the hashed index.
Data: y, dx, dW and the addend gradient of ``sparse_conv(mode='inv')`` over those rulebooks ELEMENTWISE inside the bound of
tests/_conv_geometry.py against float64 ``F.conv_transpose3d``, on NaN-poisoned allocations.
Bias: u3d_bias_add returns the bits of y + b; u3d_bias_grad is inside the fp64-accumulation bound for every value kind, width and row
count at which the two passes change shape, touches nothing around its buffers, keeps a NaN in its column and repeats bit for bit.
Layers: the inverse and the transposed layer with a bias against float64, the order with an addend, partial requires_grad; a small
encoder / decoder stack with a norm behind the biased layer; and the reference-shaped U-Net launches, name for name, what it launched before the feature.
The largest err / bound per selection goes to the parity log (_parity.log_errors, test 'convt_bias')."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _conv_general as G
import _conv_geometry as cg
import _conv_transpose as T
import _parity
from test_gpu_conv_general import SELECTIONS, _same_lists
from test_gpu_conv_geometry import _groups, _operands, _poison, _selection

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
assert T.CHANNELS == [(16, 32), (32, 64), (64, 96), (160, 192)]


def _layer(cfg, cin=32, cout=32, **kw):
    from unidet3d_amd import sparse as S
    return S.SparseConvTranspose3d(cin, cout, **T.layer_args(cfg), **kw)


def _build(cfg, name):
    """the device level of ``cfg`` on scene ``name``, every part bit for bit the brute-force reference's"""
    from unidet3d_amd import sparse
    _, B, shape, coords = T.scene(name)
    ix = sparse.OccupancyIndex.from_coords(coords.to(DEV), B, shape)
    n = ix.count()
    rows = ix.coords(n)
    assert n == len(coords) and torch.equal(rows.cpu(), coords), f'{name}: canonical rows'
    m = _layer(cfg)
    oc, oshape, ix_out, rb = sparse.build_convt_rulebook(rows, B, shape, m.geom, m.output_padding)
    roc, roshape, rpairs = T.brute(cfg, name)
    where = f'{cfg} on {name}'
    assert list(oshape) == list(roshape), where
    assert oc.dtype == torch.int32 and torch.equal(oc.cpu(), roc), where
    assert (rb.K, rb.n_in, rb.n_out) == (len(rpairs), len(roc), n) and rb.cap == max(1, min(n, len(roc))), where
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


GEOMETRY_CONFIGS = list(T.CONFIGS) + [T.BEYOND]


@pytest.mark.parametrize('cfg', GEOMETRY_CONFIGS, ids=str)
def test_geometry_equals_the_brute_force_reference_bit_for_bit(cfg):
    for name in T.SCENES:
        lvl = _level(cfg, name)
        assert not lvl['index'].hashed
        if cfg == 'k2s2p0':                                          # 8 outputs per input row, one pair each
            assert lvl['n2'] == 8 * lvl['n'] and lvl['rb'].counts.cpu().tolist() == [lvl['n']] * 8, name


@pytest.mark.parametrize('cfg', GEOMETRY_CONFIGS, ids=str)
def test_geometry_under_the_hashed_index(cfg, monkeypatch):
    from unidet3d_amd import geometry
    monkeypatch.setattr(geometry, '_INDEX_MODE', 'hash')
    for name in T.SCENES:
        assert _build(cfg, name)['index'].hashed


# ---------------------------------------------------------------------------------------------------------------- data
def _run(lvl, inp, sel):
    """forward (+ addend) and backward of ``sparse_conv(mode='inv')`` over the level's rulebook -> dict(y, dx, dw, dadd) on the device"""
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
    assert (ns, nd) == (rb.n_out, rb.n_in)
    _poison([nd * cout, _groups(cin, cout, rb.K, nd, rows and cin % 32 == 0) * nd * cout])
    y = sparse.sparse_conv(xg, wg, rb, 'inv', ag)
    _poison([ns * cin, wg.numel(), (_groups(cout, cin, rb.K, ns, rows) if cin != 16 else 1) * ns * cin, nd * cout])
    y.backward(gg)
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xg.grad, dw=wg.grad, dadd=ag.grad)


def _check_case(cfg, name, cin, cout, sel, ratios, bad):
    lvl, case = _level(cfg, name), T.case(cfg, name, cin, cout)
    got = _run(lvl, case['inp'], sel)
    bnd = case['bound'][_operands(sel)]
    where = f'{cfg} {cin}->{cout} {sel} on {name}'
    for k in ('y', 'dx', 'dw', 'dadd'):
        if k == 'dx' and cin == 16:
            assert got['dx'] is None, where
            continue
        r = cg.excess(got[k], case['ref'][k], bnd[k])
        print(f'convt {where}: {k} err / bound = {r:.3g}')
        if r >= ratios[k][0]:
            ratios[k] = (r, f'{cfg} {name}')
        if not r <= 1.0:
            bad.append(f'{where}: {k} err / bound = {r:.3g}')
    dw = got['dw'].reshape(cout, lvl['rb'].K, cin)
    for k in np.nonzero(case['counts']['dw'].numpy() == 0)[0]:       # an offset without pairs has an exactly zero dW slice
        if not bool((dw[:, int(k), :] == 0).all()):
            bad.append(f'{where}: dW of the empty offset {int(k)} is not 0')


def _log(kind, sel, cin, cout, ratios):
    rec = dict(kind=kind, selection=sel, cin=cin, cout=cout, **{f'{k}_ratio': v[0] for k, v in ratios.items()},
               **{f'{k}_worst': v[1] for k, v in ratios.items()})
    _parity.log_errors('convt_bias', rec)
    print('convt_bias', rec)


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('cfg', list(T.CONFIGS))
def test_transposed_convolution_on_every_scene(cfg, sel):
    """every configuration on every scene at 32 -> 64 channels, under every kernel selection"""
    ratios, bad = {k: (0.0, None) for k in ('y', 'dx', 'dw', 'dadd')}, []
    with _selection(sel):
        for name in T.SCENES:
            _check_case(cfg, name, 32, 64, sel, ratios, bad)
    _log('all_scenes', sel, 32, 64, ratios)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('cin,cout', T.CHANNELS)
def test_transposed_convolution_at_every_channel_pair(cin, cout, sel):
    """the full selection x channel-pair grid on three scenes, every configuration"""
    ratios, bad = {k: (0.0, None) for k in ('y', 'dx', 'dw', 'dadd')}, []
    with _selection(sel):
        for cfg in T.CONFIGS:
            for name in T.FULL_GRID_SCENES:
                _check_case(cfg, name, cin, cout, sel, ratios, bad)
    _log('all_pairs', sel, cin, cout, ratios)
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------------------- bias kernels
GUARD = 64          # guard rows / elements around every buffer a kernel writes
SENTINEL = -12345.0


def _bias_rows():
    from unidet3d_amd import _lib as L
    return T.bias_rows(L.BIAS_GRAD_ROWS, L.BIAS_GRAD_STEP)


def _guarded(n, C):
    """an [n, C] fp32 view with GUARD sentinel rows on either side -> (view, whole buffer)"""
    buf = torch.full((n + 2 * GUARD, C), SENTINEL, dtype=torch.float32, device=DEV)
    return buf[GUARD:GUARD + n], buf


def _guards_untouched(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize('C', T.BIAS_WIDTHS)
def test_bias_add_returns_the_bits_of_y_plus_b(C):
    from unidet3d_amd import _lib as L
    for n in _bias_rows() + [65537]:
        g = torch.Generator().manual_seed(n + C)
        y = torch.randn(n, C, generator=g) * torch.exp(torch.randn(n, C, generator=g) * 2.0)
        b = torch.randn(C, generator=g)
        b[1], y[0, 2], y[n // 2, 3] = 0.0, float('inf'), -0.0
        view, buf = _guarded(n, C)
        view.copy_(y)
        L.call('u3d_bias_add', L.ptr(view), L.ptr(b.to(DEV)), n, C, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(view.cpu().view(torch.int32), (y + b).view(torch.int32)), (n, C)
        assert _guards_untouched(buf, n), (n, C)


def _bias_grad(dy_dev, n, C):
    """u3d_bias_grad on a device tensor with guarded db and workspace -> (db on the host, guards untouched)"""
    from unidet3d_amd import _lib as L
    need = L.lib().u3d_bias_grad_ws_bytes(n, C)
    assert need % 8 == 0 and need == -(-n // L.BIAS_GRAD_ROWS) * C * 8
    ws = torch.full((need // 8 + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    db = torch.full((C + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    L.call('u3d_bias_grad', L.ptr(dy_dev), n, C, L.ptr(db[GUARD:GUARD + C]), L.ptr(ws[GUARD:GUARD + need // 8]), L.stream())
    torch.cuda.synchronize()
    ok = all(bool((t[:GUARD] == SENTINEL).all()) and bool((t[GUARD + m:] == SENTINEL).all()) for t, m in ((ws, need // 8), (db, C)))
    return db[GUARD:GUARD + C].cpu(), ok


@pytest.mark.parametrize('C', T.BIAS_WIDTHS)
@pytest.mark.parametrize('kind', T.BIAS_KINDS)
def test_bias_grad_is_inside_the_fp64_accumulation_bound(kind, C):
    worst = 0.0
    for n in _bias_rows() + ([65537] if kind == 'integer' else []):
        dy = T.bias_values(kind, n, C)
        ref, bnd = T.bias_grad_reference(dy)
        view, buf = _guarded(n, C)
        view.copy_(dy)
        db, ok = _bias_grad(view, n, C)
        again, _ = _bias_grad(view, n, C)
        assert ok and _guards_untouched(buf, n), (kind, n, C)
        assert torch.equal(db.view(torch.int32), again.view(torch.int32)), (kind, n, C)          # one summation order
        r = cg.excess(db, ref, bnd)
        print(f'bias_grad {kind} n={n} C={C}: err / bound = {r:.3g}')
        worst = max(worst, r)
        assert r <= 1.0, (kind, n, C, r)
        if kind == 'integer':
            assert torch.equal(db.double(), ref), (n, C)
    _parity.log_errors('convt_bias', dict(kind='bias_grad', values=kind, C=C, db_ratio=worst))


def test_bias_grad_keeps_a_nan_in_its_column():
    from unidet3d_amd import _lib as L
    n, C = L.BIAS_GRAD_ROWS + 1, 96
    dy = T.bias_values('normal', n, C)
    ref, bnd = T.bias_grad_reference(dy)
    dy[n - 1, 37] = float('nan')
    db, ok = _bias_grad(dy.to(DEV), n, C)
    keep = torch.arange(C) != 37
    assert ok and bool(torch.isnan(db[37])) and bool(torch.isfinite(db[keep]).all())
    assert bool(((db.double() - ref).abs()[keep] <= bnd[keep]).all())


# ---------------------------------------------------------------------------------------------------------------- layers
def _tensor(name, feats):
    from unidet3d_amd import sparse as S
    _, B, shape, coords = T.scene(name)
    return S.SparseConvTensor(feats, coords.to(DEV), shape, B)


def _layer_inputs(n_src, n_dst, cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    k = G._t3(k)
    return dict(x=torch.randn(n_src, cin, generator=g), w=torch.randn(cout, *k, cin, generator=g) * 0.1, b=torch.randn(cout, generator=g),
                go=torch.randn(n_dst, cout, generator=g))


def _load(layer, inp):
    layer = layer.to(DEV)
    with torch.no_grad():
        layer.weight.copy_(inp['w'].to(DEV))
        layer.bias.copy_(inp['b'].to(DEV))
    return layer


def _check_layer(got, ref, bnd, where):
    for q in ('y', 'dx', 'dw', 'db'):
        r = cg.excess(got[q], ref[q], bnd[q])
        print(f'biased layer {where}: {q} err / bound = {r:.3g}')
        assert r <= 1.0, (where, q, r)


@pytest.mark.parametrize('kind', ['inverse', 'transposed'])
def test_layers_with_a_bias_against_float64(kind):
    from unidet3d_amd import sparse as S
    name, cin, cout = 'block_in_far_corner', 32, 64
    _, B, shape, coords = T.scene(name)
    n = len(coords)
    with _selection('bf16x3'):
        if kind == 'inverse':
            n2 = len(G.brute('k3s2p0', name)[0])
            inp = _layer_inputs(n2, n, cin, cout, 3, 3)
            layer = _load(S.SparseInverseConv3d(cin, cout, 3, indice_key='d', bias=True), inp)
            dense = lambda z, w: G.dense_inverse(z, w, 'k3s2p0', name)
        else:
            n2 = T.n_rows('k3s2p1q1', name)[1]
            inp = _layer_inputs(n, n2, cin, cout, 3, 4)
            layer = _load(_layer('k3s2p1q1', cin, cout, bias=True, indice_key='u'), inp)
            dense = lambda x, w: T.dense_convt(x, w, 'k3s2p1q1', name)
        x = inp['x'].to(DEV).requires_grad_()
        if kind == 'inverse':        # the inverse layer reads the level a strided k3s2p0 layer made
            down = S.SparseConv3d(cout, cin, 3, stride=2, padding=0, indice_key='d').to(DEV)
            with torch.no_grad():
                t = down(_tensor(name, torch.zeros(n, cout, device=DEV)))
            out = layer(t.replace_feature(x))
        else:
            out = layer(_tensor(name, x))
        out.features.backward(inp['go'].to(DEV))
        torch.cuda.synchronize()
    ref, bnd = T.layer_case(dense, inp, cin, cout)
    got = dict(y=out.features.detach(), dx=x.grad, dw=layer.weight.grad, db=layer.bias.grad)
    _check_layer(got, ref, bnd, f'{kind} on {name}')
    if kind == 'inverse':            # an input-level row beyond the last full window has no pair: exactly the bias
        lonely = (G.product_counts('inv', 'k3s2p0', name)['y'] == 0).nonzero().flatten()
        assert len(lonely) > 0
        assert torch.equal(got['y'][lonely.to(DEV)].cpu(), inp['b'].expand(len(lonely), cout))


def test_bias_follows_the_addend():
    """(conv + addend) + bias, in that order: the bits of the convolution's result with the addend, plus b in fp32"""
    from unidet3d_amd import sparse as S
    cfg, name = 'k3s2p1q1', 'block5'
    lvl, inp = _level(cfg, name), T.case(cfg, name, 32, 64)['inp']
    x, w, add, b = [inp[q].to(DEV) for q in ('x', 'w', 'add', 'b')]
    with torch.no_grad(), _selection('bf16x3'):
        base = S.sparse_conv(x, w, lvl['rb'], 'inv', add)
        got = S.sparse_bias(S.sparse_conv(x, w, lvl['rb'], 'inv', add), b)
    assert torch.equal(got, base + b) and not torch.equal(got, base)


def test_bias_gradient_follows_requires_grad(monkeypatch):
    """frozen weight + trainable bias: db arrives (and is right); trainable weight + frozen bias: no u3d_bias_grad launch"""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    name = 'block5'
    n = len(T.scene(name)[3])
    names, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    for make in (lambda: _layer('k2s2p0', 32, 32, bias=True), lambda: _layer('k3s2p1q1', 32, 32, bias=True)):
        for w_grad, b_grad in ((False, True), (True, False)):
            layer = make().to(DEV)
            layer.weight.requires_grad_(w_grad)
            layer.bias.requires_grad_(b_grad)
            del names[:]
            out = layer(_tensor(name, torch.randn(n, 32, generator=torch.Generator().manual_seed(3)).to(DEV)))
            go = torch.randn(out.features.shape, generator=torch.Generator().manual_seed(4))
            out.features.backward(go.to(DEV))
            torch.cuda.synchronize()
            assert names.count('u3d_bias_add') == 1 and names.count('u3d_bias_grad') == int(b_grad), names
            assert (layer.weight.grad is not None) == w_grad and (layer.bias.grad is not None) == b_grad
            if b_grad:
                ref, bnd = T.bias_grad_reference(go)
                assert cg.excess(layer.bias.grad, ref, bnd) <= 1.0


def test_empty_output_level_launches_nothing():
    """every input row on the low faces under padding beyond the reach: no output rows, zero counts, an exactly zero weight gradient"""
    from unidet3d_amd import sparse as S
    layer = _layer(T.BEYOND, 32, 32, bias=True).to(DEV)
    coords = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 1]], dtype=torch.int32, device=DEV)
    x = torch.randn(2, 32, device=DEV).requires_grad_()
    out = layer(S.SparseConvTensor(x, coords, (3, 3, 3), 1))
    rb = layer.geometry(S.SparseConvTensor(x, coords, (3, 3, 3), 1, out.indice_dict))[3]
    assert tuple(out.features.shape) == (0, 32) and tuple(out.indices.shape) == (0, 4) and out.spatial_shape == [1, 1, 1]
    assert rb.counts.cpu().tolist() == [0] * 27 and (rb.n_in, rb.n_out) == (0, 2)
    out.features.sum().backward()
    assert bool((layer.weight.grad == 0).all()) and bool((layer.bias.grad == 0).all()) and bool((x.grad == 0).all())
    empty = layer(S.SparseConvTensor(torch.zeros(0, 32, device=DEV), coords[:0], (3, 3, 3), 1))
    assert tuple(empty.features.shape) == (0, 32)


# ---------------------------------------------------------------------------------------------------------------- stack
def _stack():
    from unidet3d_amd import sparse as S
    torch.manual_seed(5)
    net = nn.ModuleList([S.SparseConv3d(32, 64, 3, stride=2, padding=1, indice_key='d'), S.SubMConv3d(64, 64, 3, indice_key='s'),
                         _layer('k3s2p1q1', 64, 32, bias=True, indice_key='u'), S.SparseBatchNorm(32)]).to(DEV)
    with torch.no_grad():
        net[2].bias.copy_(torch.randn(32, generator=torch.Generator().manual_seed(6)))        # a bias the statistics cannot miss
    return net


def _stack_step(net, name):
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(len(T.scene(name)[3]), 32, generator=g).to(DEV).requires_grad_()
    net.train()
    net.zero_grad(set_to_none=True)
    h = net[2](net[1](net[0](_tensor(name, feats))))
    out = net[3].on(h, feeds_conv=False)
    out.features.backward(torch.randn(out.features.shape, generator=g).to(DEV))
    torch.cuda.synchronize()
    return h, out, [out.features.detach().clone(), feats.grad.clone()] + [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize('name', ['empty_middle_scene', 'block5_odd_extent', 'line_x_65'])
def test_encoder_decoder_stack_with_a_norm_behind_the_biased_layer(name):
    net = _stack()
    h, out, first = _stack_step(net, name)
    _, B, shape, coords = T.scene(name)
    mid = G.out_shape(shape, 'k3s2p1')
    assert out.spatial_shape == [2 * m for m in mid] and out.batch_size == B and out.indices.shape[0] == out.features.shape[0] > 0
    for t in first:
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    # the norm sees the statistics of the value AFTER the bias: torch's batch norm on the float64 layer output
    bn = net[3]
    ref = F.batch_norm(h.features.detach().double().cpu(), None, None, bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(),
                       training=True, eps=bn.eps)
    rel = float((out.features.detach().double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-12))
    print(f'norm behind the biased layer on {name}: {rel:.3e}')
    assert rel < 2e-6                                               # the batch-norm tolerance of tests/test_gpu_sparse_layers.py
    again = _stack_step(net, name)[2]                               # (training mode moves only the running statistics)
    assert len(again) == len(first) and all(torch.equal(a, b) for a, b in zip(again, first)), name


def test_indice_key_rules_of_the_transposed_layer(monkeypatch):
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    name = 'block5'
    n = len(T.scene(name)[3])
    names, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    x = _tensor(name, torch.randn(n, 32, device=DEV))
    with torch.no_grad():
        a, b = _layer('k3s2p1q1', 32, 32, indice_key='u').to(DEV), _layer('k3s2p1q1', 32, 64, indice_key='u').to(DEV)
        ya, yb = a(x), b(x)
        assert names.count('u3d_convt_mark') == 1 and names.count('u3d_conv_rulebook') == 1 and torch.equal(ya.indices, yb.indices)
        rb = x.indice_dict[('__up__', 'u')][3]
        assert rb.tag == ('__up__', 'u') and rb.geom == ('convt', *a.geom, *a.output_padding) and a.geometry(x)[3] is rb
        with pytest.raises(L.U3DError, match='must share'):
            _layer('k3s2p1q0', 32, 32, indice_key='u').to(DEV)(x)
        with pytest.raises(L.U3DError, match='SparseConvTranspose3d'):
            S.SparseInverseConv3d(32, 32, 3, indice_key='u').to(DEV)(ya)
        with pytest.raises(L.U3DError, match='SparseConvTranspose3d'):
            S.SubMConv3d(32, 32, 3, indice_key='u').to(DEV)(x)
        with pytest.raises(L.U3DError, match='SparseConvTranspose3d'):
            S.SparseConv3d(32, 32, 3, stride=2, padding=1, indice_key='u').to(DEV)(x)
        S.SubMConv3d(32, 32, 3, indice_key='s').to(DEV)(x)
        S.SparseConv3d(32, 32, 3, stride=2, padding=1, indice_key='d').to(DEV)(x)
        for key, taker in (('s', 'SubMConv3d'), ('d', 'strided')):
            with pytest.raises(L.U3DError, match=taker):
                _layer('k3s2p1q1', 32, 32, indice_key=key).to(DEV)(x)
        # without a key the rulebook is the layer's own
        c = _layer('k3s2p1q1', 32, 32).to(DEV)
        c(x)
        assert ('__up__', ('__anon__', id(c))) in x.indice_dict and x.indice_dict[('__up__', ('__anon__', id(c)))][3].tag is None


# ---------------------------------------------------------------------------------------------------------------- nothing old moved
def _unet_pieces(bias):
    from unidet3d_amd import sparse as S
    from unidet3d_amd.spconv_unet import SpConvUNet
    torch.manual_seed(9)
    front = S.SparseSequential(S.SubMConv3d(6, 32, 3, padding=1, indice_key='subm1'))
    unet = SpConvUNet([32, 64], block_reps=2)
    if bias:
        up = unet.deconv._modules['2'] = S.SparseInverseConv3d(64, 32, 2, indice_key='spconv1', bias=True)
        with torch.no_grad():
            up.bias.copy_(torch.randn(32, generator=torch.Generator().manual_seed(1)))
    back = S.SparseSequential(S.SparseBatchNorm(32), nn.ReLU())
    return front, unet, back, nn.ModuleList([front, unet, back]).to(DEV)


GOLDEN_LAUNCHES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'unet_launch_names_before_convt_bias.json')


def _unet_launches():
    """The ``L.call`` names, in order, of one training step (forward + backward) of the reference-shaped U-Net between a first
    convolution and a last norm, on the pair-list kernels of the default precision.  Weight packs and tile lists are left out, as
    ``test_unet_layer_shapes_launch_the_entry_points_they_always_did`` leaves them out: when they are built follows what earlier steps of
    the process asked of rulebooks with the same keys.  Uses nothing the feature added: the recorded list is this function run on the
    commit before it."""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    front, unet, back, net = _unet_pieces(False)
    names, real = [], L.call

    def recorder(nm, *a):
        names.append(nm)
        return real(nm, *a)
    name = 'empty_middle_scene'
    n = len(T.scene(name)[3])
    net.train()
    S._TILE_HISTORY.clear()
    L.call = recorder
    try:
        with _selection('bf16x3'), S.conv_ts(False), S.conv_rs(False):
            out = back(unet(front(_tensor(name, torch.randn(n, 6, generator=torch.Generator().manual_seed(2)).to(DEV)))))
            out.features.sum().backward()
            S.join_wgrad_stream()
        torch.cuda.synchronize()
    finally:
        L.call = real
    assert all(p.grad is not None for p in net.parameters())
    return [nm for nm in names if not nm.startswith(('u3d_weight_pack', 'u3d_tile_starts'))]


def test_reference_shaped_unet_launches_exactly_what_it_launched_before():
    from unidet3d_amd.spconv_unet import fusion_plan
    front, unet, back, _ = _unet_pieces(False)
    assert fusion_plan(unet, front, back).convs
    before = json.load(open(GOLDEN_LAUNCHES))
    names = _unet_launches()
    assert len(before) > 50 and not any(nm.startswith(('u3d_bias_', 'u3d_convt_')) for nm in names), sorted(set(names))
    assert names == before, [(i, a, b) for i, (a, b) in enumerate(zip(names, before)) if a != b][:5] + [len(names), len(before)]


def test_unet_with_a_biased_layer_runs_unfused_with_the_same_bits(monkeypatch):
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    from unidet3d_amd.spconv_unet import begin_fusion, fusion_plan
    front, unet, back, net = _unet_pieces(True)
    net.eval()
    assert not fusion_plan(unet, front, back).convs
    names, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    name = 'empty_middle_scene'
    feats = torch.randn(len(T.scene(name)[3]), 6, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = {}
    with torch.no_grad():
        for on in (False, True):
            with S.fused_inference(on):
                del names[:]
                x = _tensor(name, feats)
                begin_fusion(x, unet, front, back)
                out[on] = back(unet(front(x))).features
                assert 'u3d_spconv_gmm_ep' not in names and names.count('u3d_bias_add') == 1, names
    assert bool(torch.isfinite(out[True]).all()) and float(out[True].abs().max()) > 0 and torch.equal(out[True], out[False])
