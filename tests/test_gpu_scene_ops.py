"""Per-scene operations on the device (csrc/sparse_scene.hip; ``geometry.scene_offsets``, ``sparse.topk_mask`` / ``prune_topk`` /
``SparseTopKPrune``, ``global_pool`` / ``SparseGlobalMaxPool`` / ``SparseGlobalAvgPool``) against the references of tests/_scene_ops.py,
on NaN-poisoned allocations.  Bit for bit: scene ranges, masks, kept lists and positions, the maximum with its winning rows, both
backwards.  The average's forward alone has a bound (``_scene_ops.avg_bound``); its largest err / bound goes to
profiles/scene_ops_ratios.txt.  Scene sizes come from the two plan queries: the edges of a block, of a scene's blocks, of a chunk."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch import nn

import _scene_ops as SO

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = os.path.join(ROOT, 'profiles', 'scene_ops_ratios.txt')
WIDTHS = [4, 32, 36, 100, 256, 260, 512]
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257]
_RATIOS = {}


def _poison(sizes):
    """allocate and free NaN-filled blocks of these 4-byte element counts: the caching allocator hands them to the next torch.empty"""
    blocks = [torch.full((int(s),), float('nan'), dtype=torch.float32, device=DEV) for s in sizes if s > 0]
    del blocks


def _record(monkeypatch):
    from unidet3d_amd import _lib as L
    names, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    return names


def _host_reads(monkeypatch):
    """every way this library reads a device value on the host"""
    reads = []
    for name in ('item', 'tolist', 'cpu'):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda real, name: lambda t, *a, **k: (reads.append(name) if t.is_cuda else None, real(t, *a, **k))[1])(real, name))
    return reads


def _tensor(sizes, feats=None, C=4, seed=None, library_rows=False):
    """a SparseConvTensor of these scene sizes; ``library_rows``: the coordinate rows carry the mark of rows the library wrote"""
    from unidet3d_amd import sparse as S, geometry
    coords = SO.coords_of(sizes, seed=seed)
    f = feats if feats is not None else torch.zeros(len(coords), C, device=DEV)
    c = coords.to(DEV)
    return S.SparseConvTensor(f, geometry.mark_canonical(c) if library_rows else c, SO.grid_for(sizes), len(sizes)), coords


def _topk_plan(n, B):
    from unidet3d_amd import _lib
    R, P = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.lib().u3d_scene_topk_plan(n, B, ctypes.byref(R), ctypes.byref(P)) == 0
    return R.value, P.value


def _pool_plan(n, B, C):
    from unidet3d_amd import _lib
    R, Q = ctypes.c_int(0), ctypes.c_int64(0)
    assert _lib.lib().u3d_scene_pool_plan(n, B, C, ctypes.byref(R), ctypes.byref(Q)) == 0
    return R.value, Q.value


# ---------------------------------------------------------------------------------------------------------------- scene ranges
OFFSET_CASES = [[1], [257], [0, 64, 255], [63, 0, 65], [256, 1, 0], [0, 0, 0], [0, 0, 64, 0, 0, 0, 257, 0], [65, 1, 63, 64, 255, 256, 257, 1],
                [0, 0, 0, 0, 0, 0, 0, 256]]


def test_scene_offsets_with_empty_scenes_everywhere(monkeypatch):
    from unidet3d_amd import geometry
    reads = _host_reads(monkeypatch)
    for sizes in OFFSET_CASES:
        coords = SO.coords_of(sizes)
        _poison([len(sizes) + 2])
        del reads[:]
        if not len(coords):
            continue
        off, flag = geometry.scene_offsets(coords.to(DEV), len(sizes))
        assert not reads, 'no host read'
        assert off.dtype == torch.int32 and off.tolist() == SO.ref_offsets(coords, len(sizes)) and flag.tolist() == [0], sizes
    x, _ = _tensor([3, 0, 5])
    assert x.scene_offsets.tolist() == [0, 3, 3, 8] and x.replace_feature(x.features).scene_offsets is x.scene_offsets


def test_a_wrong_order_raises(monkeypatch):
    from unidet3d_amd import sparse as S, geometry
    from unidet3d_amd._lib import U3DError
    coords = SO.coords_of([70, 0, 300])
    for edit, B, msg in ((lambda c: c[5:6, 0].fill_(2) and c[290:291, 0].fill_(0), 3, 'the batch indices descend'),
                         (lambda c: c[369:, 0].fill_(3), 3, r'a batch index lies outside \[0, 3\)'),
                         (lambda c: c[:1, 0].fill_(-1), 3, r'a batch index lies outside \[0, 3\)'),
                         (lambda c: None, 2, r'a batch index lies outside \[0, 2\)')):
        c = coords.clone()
        edit(c)
        f = torch.randn(len(c), 8, device=DEV)
        assert geometry.scene_offsets(c.to(DEV), B)[1].item() != 0
        for call in (lambda x: S.topk_mask(x, f[:, 0].contiguous(), 5), lambda x: S.prune_topk(x, f[:, :1].contiguous(), [5] * B),
                     lambda x: S.global_pool(x, 'max'), lambda x: S.SparseGlobalAvgPool()(x)):
            with pytest.raises(U3DError, match=msg):
                call(S.SparseConvTensor(f, c.to(DEV), [8, 8, 8], B))
    torch.cuda.synchronize()                                               # wrong ranges gave wrong values, never an access outside a tensor


# ---------------------------------------------------------------------------------------------------------------- top-k
def _check_topk(sizes, kinds, ks, monkeypatch_reads=None, block=256):
    from unidet3d_amd import sparse as S
    B, n = len(sizes), sum(sizes)
    x, coords = _tensor(sizes)
    off = SO.ref_offsets(coords, B)
    for kind in kinds:
        s = SO.scores(kind, n, off, seed=n + 7, block=block)
        dev = s.to(DEV)
        for k in ks:
            for largest in (True, False):
                ref = SO.ref_topk_mask(s, off, k, largest)
                _poison([n, n, n, n // 4 + 1])
                if monkeypatch_reads is not None:
                    del monkeypatch_reads[:]
                mask, kept, pos, n_keep = S._scene_topk(x, dev if kind != 'two' else dev.view(n, 1), k, largest, 'topk_mask')
                where = f'{kind} sizes={sizes} k={k} largest={largest}'
                if monkeypatch_reads is not None:
                    assert len(monkeypatch_reads) == 1, f'{where}: one host read, got {monkeypatch_reads}'
                assert mask.dtype == torch.bool and torch.equal(mask.cpu(), ref), f'{where}: {int((mask.cpu() != ref).sum())} rows differ'
                kept_ref, pos_ref = SO.compact_reference(ref)
                assert n_keep == len(kept_ref) and torch.equal(kept.cpu(), kept_ref) and torch.equal(pos.cpu(), pos_ref), where


SMALL_SCENES = [[1], [255, 256, 257], [513, 0, 64], [0, 65, 0, 63, 1], [300, 300]]


@pytest.mark.parametrize('sizes', SMALL_SCENES, ids=lambda s: '-'.join(map(str, s)))
def test_topk_mask_every_kind_and_k(sizes, monkeypatch):
    R, P = _topk_plan(sum(sizes), len(sizes))
    assert R == 256 and P * R >= max(sizes)                               # these scenes take one trip; 255 / 256 / 257 / 513 are the block edges
    kinds = [k for k in SO.SCORE_KINDS if not (k == 'scene_tie' and len(sizes) == 1) and not (k == 'block_tie' and sum(sizes) < 270)]
    _check_topk(sizes, kinds, SO.k_values(sizes), _host_reads(monkeypatch))
    x, _ = _tensor(sizes)
    from unidet3d_amd import sparse as S
    s = SO.scores('two', sum(sizes), None, seed=1).to(DEV)
    assert torch.equal(S.topk_mask(x, s, 3), S.topk_mask(x, s, 3)) and torch.equal(S.topk_mask(x, s, 3), S.topk_mask(x, s.view(-1, 1), [3] * len(sizes)))


def test_topk_at_the_edges_of_a_scene_s_blocks():
    """B = 8: 64 workgroups per scene, so a scene of more than 64 * 256 rows takes a second trip through every histogram pass"""
    R, P = _topk_plan(100_000, 8)
    e = R * P
    sizes = [e - 1, e, e + 1, 0, 2 * e + 1, 255, 256, 257]
    assert _topk_plan(sum(sizes), 8) == (R, P) and e == 16384
    half = [s // 2 for s in sizes]
    _check_topk(sizes, ['random', 'scene_tie'], [half, 1000])
    _check_topk(sizes, ['equal'], [[s - 1 if s else 0 for s in sizes]])


def test_topk_two_scenes_of_200k_rows():
    R, P = _topk_plan(196_610, 2)
    sizes = [R * P + 1, 2 * R * P + 1]
    assert sum(sizes) == 196_610 and P == 256
    _check_topk(sizes, ['random', 'two'], [[1000, sizes[1] // 2]], block=R * P)


def test_prune_topk_is_prune_of_the_mask(monkeypatch):
    from unidet3d_amd import sparse as S
    reads = _host_reads(monkeypatch)
    sizes = [257, 0, 300, 64]
    B, n, C = len(sizes), sum(sizes), 36
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(n, C, generator=g)
    for kind, k in (('random', 100), ('equal', [10, 3, 299, 70]), ('special', 64), ('scene_tie', [250, 0, 8, 8])):
        off = SO.ref_offsets(SO.coords_of(sizes), B)
        s = SO.scores(kind, n, off, seed=4).to(DEV)
        outs = []
        for way in ('topk', 'mask', 'module', 'topk'):
            f = feats.to(DEV).requires_grad_()
            x, coords = _tensor(sizes, f)
            x.indice_dict['mark'] = 1
            _poison([n * C, n * C, n, n, n])
            del reads[:]
            if way == 'mask':
                y = S.prune(x, S.topk_mask(x, s, k))
            else:
                y = S.prune_topk(x, s, k) if way == 'topk' else S.SparseTopKPrune(k)(x, s)
                assert len(reads) == 1, f'{way}: one host read, got {reads}'
            ref = SO.ref_topk_mask(s.cpu(), off, k)
            assert SO.same(y.features, feats[ref]) and torch.equal(y.indices.cpu(), coords[ref]), (kind, way)
            assert y.indice_dict == {} and y.batch_size == B and y.spatial_shape == x.spatial_shape      # a new voxel set: a fresh cache
            dy = torch.randn(y.features.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
            y.features.backward(dy)
            dx = torch.zeros(n, C)
            dx[ref] = dy.cpu()
            assert SO.same(f.grad, dx), (kind, way)
            outs.append((y.features.detach(), y.indices, f.grad))
        for o in outs[1:]:
            assert all(SO.same(a, b) for a, b in zip(o, outs[0])), kind
    # every row kept: the level of x; nothing kept: an empty tensor
    x, coords = _tensor(sizes, feats.to(DEV))
    x.indice_dict['mark'] = 1
    s = SO.scores('random', n, None).to(DEV)
    for full in (S.prune_topk(x, s, max(sizes)), S.prune(x, S.topk_mask(x, s, max(sizes)))):
        assert full.indices is x.indices and full.indice_dict is x.indice_dict and SO.same(full.features, feats) and full.features is not x.features
    for none in (S.prune_topk(x, s, 0), S.prune(x, S.topk_mask(x, s, 0))):
        assert tuple(none.features.shape) == (0, C) and tuple(none.indices.shape) == (0, 4) and none.indice_dict == {}
    empty = S.prune_topk(none, torch.zeros(0, device=DEV), 5)
    assert tuple(empty.features.shape) == (0, C) and tuple(S.topk_mask(none, torch.zeros(0, 1, device=DEV), [1] * B).shape) == (0,)


# ---------------------------------------------------------------------------------------------------------------- pooling
def _pool_cases(C):
    R, _ = _pool_plan(1000, 3, C)
    assert R == 64
    cases = [[R - 1, R, R + 1], [2 * R + 1, 0, 1], [0, 0, 5 * R + 3, 0], [1]]
    if C == 32:
        R2, _ = _pool_plan(70_001, 2, C)
        assert R2 == 128
        cases.append([70_001 - 2 * R2 - 1, 2 * R2 + 1])                   # a plan with longer chunks, 545 of them in one scene
    return cases


@pytest.mark.parametrize('C', WIDTHS)
def test_global_pool_forward_and_backward(C, monkeypatch):
    from unidet3d_amd import sparse as S
    reads = _host_reads(monkeypatch)
    worst = 0.0
    for sizes in _pool_cases(C):
        B, n = len(sizes), sum(sizes)
        off = SO.ref_offsets(SO.coords_of(sizes), B)
        for kind in (SO.VALUE_KINDS if n < 10_000 else ['randn', 'integer']):
            xv = SO.values(kind, n, C, off, seed=C + n)
            dy = torch.from_numpy(np.random.default_rng(C).standard_normal((B, C)).astype(np.float32))
            where = f'{kind} C={C} sizes={sizes}'
            for mode in ('max', 'avg'):
                f = xv.to(DEV).requires_grad_()
                x, _ = _tensor(sizes, f, library_rows=True)
                _poison([B * C, B * C, n * C, n * C * 2])
                del reads[:]
                y = (S.SparseGlobalMaxPool() if mode == 'max' else S.SparseGlobalAvgPool())(x) if kind == 'randn' else S.global_pool(x, mode)
                y.backward(dy.to(DEV))
                assert not reads, f'{where} {mode}: no host read, got {reads}'
                assert y.dtype == torch.float32 and tuple(y.shape) == (B, C) and not hasattr(y, '_u3d_shadow')
                if mode == 'max':
                    y_ref, arg_ref = SO.ref_global_max(xv, off)
                    _, arg = S.global_pool_forward(f.detach(), x, 'max')
                    assert SO.same(y, y_ref), f'{where}: max differs in {int((SO.bits(y) != SO.bits(y_ref)).sum())} elements'
                    assert arg.dtype == torch.int32 and torch.equal(arg.cpu(), arg_ref), where
                    assert SO.same(f.grad, SO.ref_global_max_bwd(dy, arg_ref, n)), where
                else:
                    ok, ratio = SO.avg_check(y, xv, off)
                    worst = max(worst, ratio)
                    assert ok, f'{where}: avg err / bound = {ratio}'
                    if kind == 'integer':                                  # exact sums: one division, one rounding
                        assert SO.same(y, torch.from_numpy(SO.ref_global_avg(xv, off, np.float64).astype(np.float32))), where
                    assert SO.same(f.grad, SO.ref_global_avg_bwd(dy, off, n)), where
                    assert SO.same(S.global_pool(x, 'avg'), y), f'{where}: two runs differ'
                if kind == 'nan_inf':                                      # one row, one column: nothing leaks to other columns or scenes
                    assert int((~torch.isfinite(y)).sum()) == 2, where
    _RATIOS[C] = worst
    if len(_RATIOS) == len(WIDTHS):
        os.makedirs(os.path.dirname(RATIOS), exist_ok=True)
        with open(RATIOS, 'w') as fh:
            fh.write('global average pooling, forward: largest |y - y_ref| / bound per width, bound = 2^-24 |y_ref| + n_b 2^-52 mean|x| + 2^-149\n'
                     '(y_ref: numpy longdouble; every scene size and value kind of tests/test_gpu_scene_ops.py)\n')
            for c in WIDTHS:
                fh.write(f'C = {c:3d}  {_RATIOS[c]:.4f}\n')


def test_partial_requires_grad_and_the_order_flag_rule(monkeypatch):
    from unidet3d_amd import sparse as S
    sizes = [100, 0, 77]
    n = sum(sizes)
    names = _record(monkeypatch)
    for mode in ('max', 'avg'):
        x, _ = _tensor(sizes, torch.randn(n, 32, device=DEV), library_rows=True)
        conv = S.SubMConv3d(32, 32, 3).to(DEV)
        del names[:]
        assert not S.global_pool(x, mode).requires_grad                    # nothing asks: no graph at all
        assert 'u3d_scene_pool_bwd' not in names and names.count('u3d_scene_pool_fwd') == 1 and names.count('u3d_scene_offsets') == 1
        del names[:]
        y = S.global_pool(conv(x), mode)
        y.sum().backward()
        S.join_wgrad_stream()
        assert names.count('u3d_scene_pool_bwd') == 1 and names.count('u3d_scene_offsets') == 0 and conv.weight.grad is not None      # ranges cached
        f = torch.randn(n, 32, device=DEV).requires_grad_()
        w = torch.randn(n, 32, device=DEV).requires_grad_()
        del names[:]
        (S.global_pool(x.replace_feature(f), mode) * S.global_pool(x.replace_feature(w.detach()), mode)).sum().backward()
        assert names.count('u3d_scene_pool_bwd') == 1 and f.grad is not None and w.grad is None
    # rows a caller handed in: the flag is read once per voxel set; rows the library wrote: never
    reads = _host_reads(monkeypatch)
    x, _ = _tensor(sizes, torch.randn(n, 32, device=DEV))
    S.global_pool(x, 'max')
    assert reads == ['item']
    del reads[:]
    S.global_pool(x, 'avg'), S.global_pool(x.replace_feature(x.features * 2), 'max')
    assert not reads, 'the verdict travels with the voxel set'
    down = S.SparseConv3d(32, 32, 2, stride=2).to(DEV)(x)
    grid = torch.zeros(2, 4, 4, 4, 8, device=DEV)
    grid[1, 2, 3, 1] = 1.0
    made = S.SparseConvTensor.from_dense(grid)
    del reads[:]                                                           # (the level counts of the strided layer and of from_dense)
    S.global_pool(down, 'avg'), S.global_pool(made, 'max')
    assert not reads, 'rows the library wrote are canonical by construction'


def test_sequential_ends_in_a_global_pool():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    sizes = [90, 40]
    n = sum(sizes)
    torch.manual_seed(2)
    f = torch.randn(n, 32, device=DEV)
    for m, mode in ((S.SparseGlobalMaxPool(), 'max'), (S.SparseGlobalAvgPool(), 'avg')):
        body = [S.SubMConv3d(32, 32, 3, indice_key='s'), S.SparseBatchNorm(32), nn.ReLU()]
        seq = S.SparseSequential(*body, m).to(DEV)
        x, _ = _tensor(sizes, f, seed=1)
        y = seq(x)
        h = S.SparseSequential(*body).to(DEV)(_tensor(sizes, f, seed=1)[0])
        assert isinstance(y, torch.Tensor) and tuple(y.shape) == (2, 32) and SO.same(y, S.global_pool(h, mode))
        with pytest.raises(U3DError, match=f'SparseSequential: {type(m).__name__} must come last'):
            S.SparseSequential(body[0], m, body[1]).to(DEV)(x)
    assert not S.global_pool(_tensor([0, 0], torch.zeros(0, 8, device=DEV))[0], 'max').any()       # no rows: zeros [B, C], no launch


# ---------------------------------------------------------------------------------------------------------------- a stack
def _stack():
    from unidet3d_amd import sparse as S
    torch.manual_seed(11)
    return nn.ModuleDict(dict(s=S.SubMConv3d(32, 32, 3, indice_key='s'), bn=S.SparseBatchNorm(32), score=S.SubMConv3d(32, 4, 1, indice_key='c'),
                              up=S.SparseConvTranspose3d(32, 32, 2, stride=2, indice_key='u'), pool=S.SparseGlobalMaxPool())).to(DEV)


def _stack_step(net, ours: bool, sizes, k):
    from unidet3d_amd import sparse as S
    coords = SO.coords_of(sizes, [16, 16, 16], seed=9)
    feats = torch.randn(len(coords), 32, generator=torch.Generator().manual_seed(12)).to(DEV).requires_grad_()
    net.train()
    net.zero_grad(set_to_none=True)
    h = net['bn'].on(net['s'](S.SparseConvTensor(feats, coords.to(DEV), [16, 16, 16], len(sizes))), relu=True, feeds_conv=True)
    scores = net['score'](h).features.detach().amax(1)
    if ours:
        q = S.prune_topk(h, scores, k)
    else:                                                                  # what users write today: one topk, one scatter, one host wait per scene
        keep = torch.zeros(len(coords), dtype=torch.bool, device=DEV)
        for b in range(len(sizes)):
            rows = torch.nonzero(h.indices[:, 0] == b)[:, 0]
            if len(rows):
                keep[rows[torch.topk(scores[rows], min(k, len(rows))).indices]] = True
        q = S.prune(h, keep)
    y = net['pool'](net['up'](q))
    y.backward(torch.randn(y.shape, generator=torch.Generator().manual_seed(13)).to(DEV))
    S.join_wgrad_stream()
    torch.cuda.synchronize()
    return [y.detach().clone(), q.features.detach().clone(), q.indices.clone(), feats.grad.clone()] + \
           [p.grad.clone() for p in net.parameters() if p.grad is not None], scores.cpu()


def test_generative_neck_stack_against_the_python_loop_mask():
    sizes, k = [300, 0, 500], 100
    net = _stack()
    first, scores = _stack_step(net, True, sizes, k)
    off = [0, 300, 300, 800]
    assert all(len(set(scores[off[b]:off[b + 1]].tolist())) == off[b + 1] - off[b] for b in range(3)), 'distinct scores: torch.topk has one answer'
    assert first[1].shape[0] == 200 and len(first) >= 8 and all(bool(torch.isfinite(t.float()).all()) for t in first)
    assert float(first[3].abs().max()) > 0 and tuple(first[0].shape) == (3, 32) and not first[0][1].any()      # the empty scene pools to +0.0
    ref, _ = _stack_step(net, False, sizes, k)
    assert len(ref) == len(first)
    for i, (a, b) in enumerate(zip(first, ref)):
        assert SO.same(a, b), f'tensor {i}: {int((a != b).sum())} elements differ'
    again, _ = _stack_step(net, True, sizes, k)
    assert all(SO.same(a, b) for a, b in zip(again, first))
