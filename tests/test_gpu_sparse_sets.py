"""Sparse tensors on different voxel sets on the device (csrc/sparse_sets.hip, ``geometry.build_union_level`` / ``compact_mask``,
``sparse.sparse_add`` / ``prune``) against the references of tests/_sparse_sets.py.  Every comparison is bit for bit: the operations are
copies and single fp32 additions.
Geometry: union rows, both destination-major maps and both source-major maps for every relation x scene, under the bitmap and the hashed
index; ``rows_of`` outside the grid and the batch.  Compaction: every mask kind at the wave, block and block-scan edges.  Row kernels:
widths 4 .. 512 (every lane-slot fill, the column loop past 256), every value kind, NaN-poisoned allocations, guard rows, absent and
out-of-range map entries.  Autograd: forward and backward per relation and mask kind, partial ``requires_grad`` by launch names, x + x,
the left fold, run-to-run identity.  Levels: a new set starts from an empty ``indice_dict``; the shortcuts keep level and cache.  A
generative decoder stack against the same stack on explicit torch indexing.  The reference-shaped U-Net launches what it launched."""
import json

import pytest
import torch
from torch import nn

import _sparse_sets as SS
from test_gpu_conv_transpose import GOLDEN_LAUNCHES, _unet_launches

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDTHS = [4, 8, 16, 32, 36, 96, 160, 256, 260, 512]
ALL_WIDTH_SCENES = ['block5', 'line_x_65']
LARGE_WIDTHS = [4, 36, 260]
ROW_RELATIONS = ['overlap', 'parity', 'disjoint']
GEOMETRY_KERNELS = ('u3d_index_mark', 'u3d_index_rank', 'u3d_index_coords', 'u3d_index_rows', 'u3d_cells_of_coords', 'u3d_hash_index_build',
                    'u3d_hash_index_coords', 'u3d_mask_compact')
NEW_ENTRY_POINTS = ('u3d_index_rows', 'u3d_mask_compact', 'u3d_rows_take', 'u3d_rows_take2')
GUARD = 3
SENTINEL = 12345.0


def _poison(sizes):
    """allocate and free NaN-filled blocks of these 4-byte element counts: the caching allocator hands them to the next torch.empty"""
    blocks = [torch.full((int(s),), float('nan'), dtype=torch.float32, device=DEV) for s in sizes if s > 0]
    del blocks


def _record(monkeypatch):
    from unidet3d_amd import _lib as L
    names, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    return names


def _index(coords_dev, B, shape):
    """the occupancy index of an operand; an empty one through ``from_marks`` with a mark that marks nothing"""
    from unidet3d_amd import geometry
    if len(coords_dev):
        return geometry.OccupancyIndex.from_coords(coords_dev, B, shape)
    return geometry.OccupancyIndex.from_marks(B, shape, DEV, lambda bitmap: torch.empty(0, dtype=torch.int64, device=DEV) if bitmap is None else None)


def _sparse(coords, feats, B, shape):
    from unidet3d_amd import sparse as S
    return S.SparseConvTensor(feats, coords.to(DEV), shape, B)


# ---------------------------------------------------------------------------------------------------------------- geometry
def _check_union(name, rel, hashed):
    from unidet3d_amd import geometry
    p = SS.pair(name, rel)
    a, b = p['a'].to(DEV), p['b'].to(DEV)
    ia, ib = _index(a, p['B'], p['shape']), _index(b, p['B'], p['shape'])
    assert ia.hashed == ib.hashed == hashed
    lvl = geometry.build_union_level(a, ia, b, ib, p['B'], p['shape'])
    where = f'{rel} on {name}'
    assert lvl.n == len(p['u']) and lvl.coords.dtype == torch.int32 and torch.equal(lvl.coords.cpu(), p['u']), where
    assert lvl.index.hashed == hashed and lvl.index.count() == lvl.n, where
    for w in 'ab':
        rows, into = getattr(lvl, f'rows_{w}'), lvl.into(w)
        assert rows.dtype == into.dtype == torch.int32 and lvl.into(w) is into
        assert torch.equal(rows.cpu(), p[f'rows_{w}']), f'{where}: rows_{w}'
        assert torch.equal(into.cpu(), p[f'into_{w}']), f'{where}: into_{w}'
    na, nb = len(a), len(b)
    assert lvl.same == ('a' if lvl.n == na else 'b' if lvl.n == nb else None), where
    if lvl.same is not None:                             # the union IS that operand's level: its own objects, nothing new
        assert lvl.coords is (a if lvl.same == 'a' else b) and lvl.index is (ia if lvl.same == 'a' else ib), where


@pytest.mark.parametrize('name', SS.SCENES)
def test_union_level_equals_the_reference(name):
    for rel in SS.relations(name):
        _check_union(name, rel, False)


@pytest.mark.parametrize('name', SS.SCENES)
def test_union_level_under_the_hashed_index(name, monkeypatch):
    from unidet3d_amd import geometry
    monkeypatch.setattr(geometry, '_INDEX_MODE', 'hash')
    for rel in SS.relations(name):
        _check_union(name, rel, True)


@pytest.mark.parametrize('mode', ['auto', 'hash'])
def test_rows_of_outside_the_grid_and_the_batch(mode, monkeypatch):
    from unidet3d_amd import geometry
    monkeypatch.setattr(geometry, '_INDEX_MODE', mode)
    for name in ('block_in_far_corner', 'empty_middle_scene', 'block_in_corner_0', 'line_z_65'):
        _, B, shape, coords = SS.scene(name)
        ix = _index(coords.to(DEV), B, shape)
        X, Y, Z = shape
        b, x, y, z = coords[-1].tolist()
        f = coords[0].tolist()
        probes = [[b, -1, y, z], [b, x, -1, z], [b, x, y, -1], [b, X, y, z], [b, x, Y, z], [b, x, y, Z], [b, x + X, y, z], [b, x, y, z + 64],
                  [B, x, y, z], [-1, x, y, z], [B + 5, f[1], f[2], f[3]], [-(2 ** 31), x, y, z], [2 ** 31 - 1, x, y, z],
                  [b, 2 ** 31 - 1, y, z], [b, x, y, -(2 ** 31)]]
        absent = [c for c in ([b, x, y, (z + 1) % Z], [f[0], f[1], (f[2] + 2) % Y, f[3]]) if c not in coords.tolist()]
        q = torch.tensor(probes + absent + coords.tolist(), dtype=torch.int32)
        _poison([len(q)])
        rows = ix.rows_of(q.to(DEV)).cpu()
        assert rows.tolist() == [-1] * (len(probes) + len(absent)) + list(range(len(coords))), (mode, name)
    assert tuple(ix.rows_of(torch.zeros(0, 4, dtype=torch.int32, device=DEV)).shape) == (0,)


# ---------------------------------------------------------------------------------------------------------------- compaction
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537])
def test_mask_compaction_equals_nonzero(n, monkeypatch):
    from unidet3d_amd import geometry
    reads, item = [], torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, 'item', lambda t: (reads.append(1), item(t))[1])
    for kind in SS.MASK_KINDS:
        keep = SS.mask(kind, n, seed=n)
        kept_ref, pos_ref = SS.compact_reference(keep)
        dev = keep.to(DEV)
        _poison([n, n])
        del reads[:]
        kept, pos, count = geometry.compact_mask(dev)
        assert len(reads) == 1, f'{kind}: the count is read once'
        where = f'{kind} n={n}'
        assert count == len(kept_ref) == kept.shape[0] and kept.dtype == pos.dtype == torch.int32, where
        assert torch.equal(kept.cpu(), torch.nonzero(keep)[:, 0].int()) and torch.equal(kept.cpu(), kept_ref), where
        assert torch.equal(pos.cpu(), pos_ref), where
        again = geometry.compact_mask(dev)
        assert torch.equal(again[0], kept) and torch.equal(again[1], pos) and again[2] == count, where
    del reads[:]
    kept, pos, count = geometry.compact_mask(torch.zeros(0, dtype=torch.bool, device=DEV))
    assert (tuple(kept.shape), tuple(pos.shape), count, reads) == ((0,), (0,), 0, [])


# ---------------------------------------------------------------------------------------------------------------- row kernels
def _widths(name):
    return WIDTHS if name in ALL_WIDTH_SCENES else LARGE_WIDTHS


def _operands(p, kind, C):
    return SS.values(kind, len(p['a']), C, 0), SS.values(kind, len(p['b']), C, 1)


@pytest.mark.parametrize('name', ALL_WIDTH_SCENES + [SS.LARGE])
def test_row_kernels_are_bit_equal_at_every_width_and_value_kind(name):
    from unidet3d_amd import sparse as S
    bad = []
    for rel in ROW_RELATIONS:
        p = SS.pair(name, rel)
        maps = {k: p[k].to(DEV) for k in ('rows_a', 'rows_b', 'into_a', 'into_b')}
        nu = len(p['u'])
        for C in _widths(name):
            for kind in SS.VALUE_KINDS:
                a, b = _operands(p, kind, C)
                where = f'{rel} {kind} C={C} on {name}'
                ad, bd = a.to(DEV), b.to(DEV)
                _poison([nu * C])
                y = S.rows_take2(ad, maps['rows_a'], bd, maps['rows_b'])
                ref = SS.join_reference(a, p['rows_a'], b, p['rows_b'])
                if not SS.same(y, ref):
                    bad.append(f'{where}: join differs in {int((SS.bits(y) != SS.bits(ref)).sum())} elements')
                if not torch.equal(torch.isnan(y).cpu(), torch.isnan(ref)):
                    bad.append(f'{where}: a NaN left its row or column')
                # the gradients' gather (source-major maps) and the pruning pair (kept list forward, position list backward)
                dy = SS.values(kind, nu, C, 2)
                _poison([len(a) * C])
                if not SS.same(S.rows_take(dy.to(DEV), maps['into_a']), SS.take_reference(dy, p['into_a'])):
                    bad.append(f'{where}: gather by into_a differs')
                keep = SS.mask('random', len(a), seed=C)
                kept, pos = SS.compact_reference(keep)
                yk, dxk = SS.prune_reference(a, keep, SS.values(kind, len(kept), C, 3))
                _poison([len(kept) * C])
                if not SS.same(S.rows_take(ad, kept.to(DEV)), yk):
                    bad.append(f'{where}: gather by the kept list differs')
                _poison([len(a) * C])
                if not SS.same(S.rows_take(SS.values(kind, len(kept), C, 3).to(DEV), pos.to(DEV)), dxk):
                    bad.append(f'{where}: gather by the position list differs')
    assert not bad, '\n'.join(bad[:40])


def _raw(entry, n_out, C, *args_before):
    """the entry point itself on a destination of GUARD + n_out + GUARD rows filled with a sentinel -> the whole buffer"""
    from unidet3d_amd import _lib as L
    buf = torch.full((2 * GUARD + n_out, C), SENTINEL, dtype=torch.float32, device=DEV)
    L.call(entry, *args_before, C, buf[GUARD:].data_ptr(), L.stream())
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize('C', WIDTHS)
def test_guard_rows_and_absent_map_entries(C):
    """rows before and after y untouched at row counts around the rows-in-flight and workgroup edges; -1, n_src and every other value
    outside [0, n_src) give rows of +0.0 and read nothing"""
    from unidet3d_amd import _lib as L
    for n_src, n_out in ((5, 1), (5, 7), (64, 65), (130, 257), (3, 1030)):
        g = torch.Generator().manual_seed(n_out)
        x, b = torch.randn(n_src, C, generator=g), torch.randn(n_src + 2, C, generator=g)
        special = torch.tensor([-1, n_src, 0, n_src - 1, 2 ** 31 - 1, -(2 ** 31), n_src + 1, -2], dtype=torch.int32)
        rows = torch.cat([special, torch.randint(-1, n_src + 1, (n_out,), generator=g).int()])[:n_out]
        rows_b = torch.cat([special.flip(0), torch.randint(-1, n_src + 3, (n_out,), generator=g).int()])[:n_out]
        xd, bd, rd, rbd = x.to(DEV), b.to(DEV), rows.to(DEV), rows_b.to(DEV)
        where = f'C={C} n_src={n_src} n_out={n_out}'
        buf = _raw('u3d_rows_take', n_out, C, L.ptr(xd), L.ptr(rd), n_out, n_src)
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n_out:] == SENTINEL).all()), where
        ref = SS.take_reference(x, rows)
        assert SS.same(buf[GUARD:GUARD + n_out], ref), where
        out = (rows < 0) | (rows >= n_src)
        assert not bool((SS.bits(buf[GUARD:GUARD + n_out])[out] != 0).any()), where
        buf = _raw('u3d_rows_take2', n_out, C, L.ptr(xd), L.ptr(rd), n_src, L.ptr(bd), L.ptr(rbd), n_src + 2, n_out)
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n_out:] == SENTINEL).all()), where
        pa, pb = ((rows >= 0) & (rows < n_src))[:, None], ((rows_b >= 0) & (rows_b < n_src + 2))[:, None]
        ga, gb = SS.take_reference(x, rows), SS.take_reference(b, rows_b)
        assert SS.same(buf[GUARD:GUARD + n_out], torch.where(pa & pb, ga + gb, torch.where(pa, ga, gb))), where


def test_coordinate_rows_travel_as_four_channel_rows():
    from unidet3d_amd import sparse as S
    _, B, shape, coords = SS.scene(SS.LARGE)
    coords = coords.clone()
    coords[5] = torch.tensor([-1, -(2 ** 31), 2 ** 31 - 1, 0x7fc00001])          # bit patterns that are NaNs as floats: not touched
    keep = SS.mask('random', len(coords))
    kept = SS.compact_reference(keep)[0]
    got = S.rows_take(coords.to(DEV).view(torch.float32), kept.to(DEV)).view(torch.int32)
    assert torch.equal(got.cpu(), coords[keep])


# ---------------------------------------------------------------------------------------------------------------- autograd
AUTOGRAD_SCENES = ['block5', 'empty_middle_scene', 'line_x_65', 'single_voxel']


def _add_case(name, rel, kind='normal', C=32, grads=(True, True)):
    p = SS.pair(name, rel)
    a, b = _operands(p, kind, C)
    fa, fb = a.to(DEV).requires_grad_(grads[0]), b.to(DEV).requires_grad_(grads[1])
    return p, a, b, _sparse(p['a'], fa, p['B'], p['shape']), _sparse(p['b'], fb, p['B'], p['shape'])


@pytest.mark.parametrize('name', AUTOGRAD_SCENES)
def test_sparse_add_forward_and_backward(name):
    from unidet3d_amd import sparse as S
    for rel in SS.relations(name):
        for kind in ('normal', 'neg_zero'):
            p, a, b, A, B_ = _add_case(name, rel, kind)
            where = f'{rel} {kind} on {name}'
            _poison([len(p['u']) * 32])
            y = S.sparse_add(A, B_)
            assert y.indices.dtype == torch.int32 and torch.equal(y.indices.cpu(), p['u']), where
            assert y.spatial_shape == list(p['shape']) and y.batch_size == p['B'], where
            assert SS.same(y.features, SS.join_reference(a, p['rows_a'], b, p['rows_b'])), where
            for attr in ('_u3d_shadow', '_u3d_stats', '_u3d_from_conv'):
                assert not hasattr(y.features, attr), where
            dy = SS.values(kind, len(p['u']), 32, 2)
            _poison([len(a) * 32, len(b) * 32])
            y.features.backward(dy.to(DEV))
            for t, into in ((A, p['into_a']), (B_, p['into_b'])):
                if t.features.shape[0] == 0 and t.features.grad is None:       # an empty operand may stay outside the graph
                    continue
                assert SS.same(t.features.grad, SS.take_reference(dy, into)), where
            if rel != 'both_empty':
                again = S.sparse_add(*_add_case(name, rel, kind)[3:])
                assert SS.same(again.features, y.features) and torch.equal(again.indices, y.indices), where


def test_sparse_add_builds_only_the_gradients_asked_for(monkeypatch):
    from unidet3d_amd import sparse as S
    names = _record(monkeypatch)
    for grads in ((True, True), (True, False), (False, True), (False, False)):
        p, a, b, A, B_ = _add_case('block5', 'overlap', grads=grads)
        y = S.sparse_add(A, B_)
        assert names.count('u3d_rows_take2') == 1 and 'u3d_rows_take' not in names, names       # the forward builds no backward map
        assert names.count('u3d_index_rows') == 2, names
        assert y.features.requires_grad == any(grads)
        del names[:]
        if not any(grads):
            continue
        dy = torch.randn(len(p['u']), 32, generator=torch.Generator().manual_seed(4))
        y.features.backward(dy.to(DEV))
        torch.cuda.synchronize()
        assert names.count('u3d_rows_take') == sum(grads) == names.count('u3d_index_rows') and len(names) == 2 * sum(grads), (grads, names)
        for t, into, want in ((A, p['into_a'], grads[0]), (B_, p['into_b'], grads[1])):
            assert (t.features.grad is not None) == want
            if want:
                assert SS.same(t.features.grad, SS.take_reference(dy, into))
        del names[:]


def test_sparse_add_of_a_tensor_and_itself():
    from unidet3d_amd import sparse as S
    for kind in ('normal', 'neg_zero', 'nan_row'):
        p, a, _, A, _ = _add_case('block5', 'equal', kind)
        y = S.sparse_add(A, A)
        assert y.indices is A.indices and SS.same(y.features, a + a)
        dy = SS.values('normal', len(a), 32, 2)
        y.features.backward(dy.to(DEV))
        assert SS.same(A.features.grad, dy + dy)


@pytest.mark.parametrize('name', ['block5', 'empty_middle_scene'])
def test_three_operands_fold_from_the_left(name):
    from unidet3d_amd import sparse as S
    _, B, shape, coords = SS.scene(name)
    n = len(coords)
    i = torch.arange(n)
    masks = [i % 2 == 0, i % 3 != 1, i >= n // 2]
    vals = [SS.values('normal', int(m.sum()), 32, s) * 10.0 ** (3 * s) for s, m in enumerate(masks)]      # scales apart: the order shows
    ts = lambda: [_sparse(coords[m].contiguous(), v.to(DEV).requires_grad_(), B, shape) for m, v in zip(masks, vals)]
    t1, t2 = ts(), ts()
    folded, nested = S.sparse_add(*t1), S.sparse_add(S.sparse_add(t2[0], t2[1]), t2[2])
    assert torch.equal(folded.indices, nested.indices) and SS.same(folded.features, nested.features)
    u, ra, rb = SS.union_reference(coords[masks[0]], coords[masks[1]])[:3]
    ab = SS.join_reference(vals[0], ra, vals[1], rb)
    u2, r1, r2 = SS.union_reference(u, coords[masks[2]])[:3]
    assert torch.equal(folded.indices.cpu(), u2) and SS.same(folded.features, SS.join_reference(ab, r1, vals[2], r2))
    dy = torch.randn(len(u2), 32, generator=torch.Generator().manual_seed(8)).to(DEV)
    folded.features.backward(dy)
    nested.features.backward(dy)
    for x, y in zip(t1, t2):
        assert SS.same(x.features.grad, y.features.grad)
    for t, m in zip(t1, masks):
        into = SS.union_reference(coords[m], u2)[3]
        assert SS.same(t.features.grad, SS.take_reference(dy.cpu(), into))


@pytest.mark.parametrize('name', AUTOGRAD_SCENES + [SS.LARGE])
def test_prune_forward_and_backward(name):
    from unidet3d_amd import sparse as S
    _, B, shape, coords = SS.scene(name)
    n = len(coords)
    for kind in SS.MASK_KINDS:
        for values in ('normal', 'neg_zero'):
            keep = SS.mask(kind, n, coords)
            x = SS.values(values, n, 32, 0)
            f = x.to(DEV).requires_grad_()
            m = keep.to(DEV)
            where = f'{kind} {values} on {name}'
            _poison([int(keep.sum()) * 32, int(keep.sum()) * 4])
            y = (S.SparsePrune() if kind == 'random' else S.prune)(_sparse(coords, f, B, shape), m)
            dy = SS.values(values, int(keep.sum()), 32, 2)
            ry, rdx = SS.prune_reference(x, keep, dy)
            assert y.indices.dtype == torch.int32 and torch.equal(y.indices.cpu(), coords[keep]) and SS.same(y.features, ry), where
            assert y.spatial_shape == list(shape) and y.batch_size == B and not m.requires_grad, where
            _poison([n * 32])
            y.features.backward(dy.to(DEV))
            assert SS.same(f.grad, rdx), where
            again = S.prune(_sparse(coords, x.to(DEV), B, shape), m)
            assert SS.same(again.features, y.features) and torch.equal(again.indices, y.indices), where


# ---------------------------------------------------------------------------------------------------------------- levels
def test_a_result_on_a_new_set_starts_from_an_empty_cache(monkeypatch):
    from unidet3d_amd import sparse as S
    conv = S.SubMConv3d(32, 32, 3, indice_key='subm1').to(DEV)
    names = _record(monkeypatch)
    with torch.no_grad():
        p, a, b, A, B_ = _add_case('block5', 'overlap')
        conv(A), conv(B_)
        A.indice_dict[S.FUSE_KEY] = object()
        assert A.indice_dict['subm1'].n_in == len(a) and any(k[0] == '__index__' for k in A.indice_dict if isinstance(k, tuple))
        y = S.sparse_add(A, B_)
        assert y.indice_dict == {} and y.indice_dict is not A.indice_dict and y.indice_dict is not B_.indice_dict
        assert len(p['u']) not in (len(a), len(b)) and y._index is not None and y._index.count() == len(p['u'])
        del names[:]
        out = conv(y)
        rb = y.indice_dict['subm1']
        assert names.count('u3d_subm_rulebook') == 1 and (rb.n_in, rb.n_out) == (len(p['u']),) * 2 and out.features.shape[0] == len(p['u'])
        assert A.indice_dict['subm1'].n_in == len(a) and B_.indice_dict['subm1'].n_in == len(b)
        # the same for a pruned level
        keep = SS.mask('alternating', len(p['u'])).to(DEV)
        z = S.prune(out, keep)
        assert z.indice_dict == {} and z._index is None
        del names[:]
        out2 = conv(z)
        assert names.count('u3d_subm_rulebook') == 1 and z.indice_dict['subm1'].n_in == int(keep.sum()) == out2.features.shape[0]
        assert y.indice_dict['subm1'] is rb and rb.n_in == len(p['u'])


def test_shortcuts_keep_the_level_and_the_cache(monkeypatch):
    """The three shortcuts.  Learning that a shortcut applies takes the one count (the union's index, the compaction); past it no level
    is built: no coordinate rows are written, and a layer behind the result finds the cached rulebook."""
    from unidet3d_amd import sparse as S
    conv = S.SubMConv3d(32, 32, 3, indice_key='subm1').to(DEV)
    names = _record(monkeypatch)
    with torch.no_grad():
        for rel, keeper in (('a_in_b', 'b'), ('b_in_a', 'a'), ('equal', 'a')):
            for mode in ('auto', 'hash'):
                from unidet3d_amd import geometry
                monkeypatch.setattr(geometry, '_INDEX_MODE', mode)
                p, a, b, A, B_ = _add_case('block5', rel)
                K = A if keeper == 'a' else B_
                conv(K)
                rb, ix = K.indice_dict['subm1'], K._index
                del names[:]
                y = S.sparse_add(A, B_)
                assert y.indices is K.indices and y.indice_dict is K.indice_dict and y._index is ix and ix is not None, (rel, mode)
                assert not any(nm in ('u3d_index_coords', 'u3d_hash_index_coords') for nm in names), names
                assert SS.same(y.features, SS.join_reference(a, p['rows_a'], b, p['rows_b'])), (rel, mode)
                del names[:]
                conv(y)
                assert y.indice_dict['subm1'] is rb and not any(nm in GEOMETRY_KERNELS or 'rulebook' in nm for nm in names), names
        monkeypatch.setattr(geometry, '_INDEX_MODE', 'auto')
        # every mask bit set: the level of x; the compaction is the one launch
        p, a, b, A, B_ = _add_case('block5', 'equal')
        conv(A)
        del names[:]
        y = S.prune(A, torch.ones(len(a), dtype=torch.bool, device=DEV))
        assert names == ['u3d_mask_compact'] and y.indices is A.indices and y.indice_dict is A.indice_dict and y._index is A._index
        assert SS.same(y.features, a) and y.features is not A.features
        # one indices object: no geometry at all
        A2 = A.replace_feature(b.to(DEV))
        del names[:]
        y = S.sparse_add(A, A2)
        assert names == [] and y.indices is A.indices and y.indice_dict is A.indice_dict and SS.same(y.features, a + b)


def test_empty_cases_launch_nothing(monkeypatch):
    from unidet3d_amd import sparse as S
    names = _record(monkeypatch)
    p, a, b, A, B_ = _add_case('block5', 'a_empty')
    y = S.sparse_add(A, B_)
    assert names == [] and y.indices is B_.indices and y.indice_dict is B_.indice_dict and SS.same(y.features, b)
    y.features.backward(torch.ones(len(b), 32, device=DEV))
    assert names == [] and A.features.grad is None and bool((B_.features.grad == 1).all())
    p, a, b, A, B_ = _add_case('block5', 'b_empty')
    y = S.sparse_add(A, B_)
    assert names == [] and y.indices is A.indices and y.indice_dict is A.indice_dict and SS.same(y.features, a)
    p, a, b, A, B_ = _add_case('block5', 'both_empty')
    y = S.sparse_add(A, B_)
    assert names == [] and tuple(y.features.shape) == (0, 32) and tuple(y.indices.shape) == (0, 4)
    # no mask bit set: an empty tensor on a new (empty) level; the compaction is the one launch, the backward launches nothing
    p, a, b, A, B_ = _add_case('block5', 'equal')
    z = S.prune(A, torch.zeros(len(a), dtype=torch.bool, device=DEV))
    assert names == ['u3d_mask_compact'] and tuple(z.features.shape) == (0, 32) and tuple(z.indices.shape) == (0, 4) and z.indice_dict == {}
    assert z.indices.dtype == torch.int32 and z.spatial_shape == A.spatial_shape
    del names[:]
    z.features.sum().backward()
    assert names == [] and tuple(A.features.grad.shape) == (len(a), 32) and not bool((SS.bits(A.features.grad) != 0).any())
    z2 = S.prune(z, torch.zeros(0, dtype=torch.bool, device=DEV))
    assert names == [] and tuple(z2.features.shape) == (0, 32)


def test_rows_only_tensors_are_refused():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    p, a, b, A, B_ = _add_case('block5', 'overlap')
    ghost = A.replace_feature(S.rows_only(torch.zeros(len(a), 32, dtype=torch.bfloat16, device=DEV)))
    with pytest.raises(U3DError, match='bf16 rows only'):
        S.sparse_add(ghost, B_)
    with pytest.raises(U3DError, match='bf16 rows only'):
        S.sparse_add(B_, ghost)
    with pytest.raises(U3DError, match='bf16 rows only'):
        S.prune(ghost, torch.zeros(0, dtype=torch.bool, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- module stack
class _RefJoin(torch.autograd.Function):
    """the union add as explicit torch indexing on the reference maps"""

    @staticmethod
    def forward(ctx, a, b, rows_a, rows_b, into_a, into_b):
        ctx.into = (into_a, into_b)
        pa, pb = (rows_a >= 0)[:, None], (rows_b >= 0)[:, None]
        ga, gb = a[rows_a.clamp(min=0).long()], b[rows_b.clamp(min=0).long()]
        return torch.where(pa & pb, ga + gb, torch.where(pa, ga, torch.where(pb, gb, torch.zeros((), device=a.device))))

    @staticmethod
    def backward(ctx, dy):
        return dy[ctx.into[0].long()], dy[ctx.into[1].long()], None, None, None, None


class _RefPrune(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep):
        ctx.keep = keep
        return x[keep]

    @staticmethod
    def backward(ctx, dy):
        dx = torch.zeros(ctx.keep.shape[0], dy.shape[1], device=dy.device)
        dx[ctx.keep] = dy
        return dx, None


def _decoder():
    from unidet3d_amd import sparse as S
    torch.manual_seed(21)
    return nn.ModuleDict(dict(
        d1=S.SparseConv3d(32, 32, 3, stride=2, padding=1, indice_key='d1'), d2=S.SparseConv3d(32, 64, 3, stride=2, padding=1, indice_key='d2'),
        u1=S.SparseConvTranspose3d(64, 32, 2, stride=2, indice_key='u1'), s=S.SubMConv3d(32, 32, 3, indice_key='s'), bn=S.SparseBatchNorm(32),
        u2=S.SparseConvTranspose3d(32, 32, 2, stride=2, indice_key='u2'))).to(DEV)


def _decoder_step(net, name, ours: bool):
    """forward + backward -> (stage tensors, [features, input gradient, every parameter gradient], the mask)"""
    from unidet3d_amd import sparse as S
    _, B, shape, coords = SS.scene(name)
    g = torch.Generator().manual_seed(31)
    feats = torch.randn(len(coords), 32, generator=g).to(DEV).requires_grad_()
    net.train()
    net.zero_grad(set_to_none=True)
    e1 = net['d1'](_sparse(coords, feats, B, shape))
    e2 = net['d2'](e1)
    up = net['u1'](e2)
    if ours:
        j = S.sparse_add(up, e1)
    else:
        u, ra, rb, ia, ib = (t.to(DEV) for t in SS.union_reference(up.indices.cpu(), e1.indices.cpu()))
        j = S.SparseConvTensor(_RefJoin.apply(up.features, e1.features, ra, rb, ia, ib), u, up.spatial_shape, B)
    h = net['bn'].on(net['s'](j), relu=True, feeds_conv=False)
    keep = h.features.detach()[:, 0] > 0
    if ours:
        q = S.prune(h, keep)
    else:
        q = S.SparseConvTensor(_RefPrune.apply(h.features, keep), h.indices[keep], h.spatial_shape, B)
    out = net['u2'](q)
    out.features.backward(torch.randn(out.features.shape, generator=g).to(DEV))
    S.join_wgrad_stream()
    torch.cuda.synchronize()
    stages = dict(e1=e1, e2=e2, up=up, j=j, q=q, out=out)
    return stages, [out.features.detach().clone(), feats.grad.clone()] + [p.grad.clone() for p in net.parameters()], keep.cpu()


@pytest.mark.parametrize('name', ['block5', 'empty_middle_scene'])
def test_generative_decoder_stack(name):
    net = _decoder()
    stages, first, keep = _decoder_step(net, name, True)
    _, B, shape, coords = SS.scene(name)
    # the coordinates of every stage from the brute-force geometry
    c1, s1, _ = SS.brute_on('conv', 'k3s2p1', B, shape, coords)
    c2, s2, _ = SS.brute_on('conv', 'k3s2p1', B, s1, c1)
    cu, su, _ = SS.brute_on('convt', (2, 2, 0, 0, 1), B, s2, c2)
    cj = SS.union_reference(cu, c1)[0]
    cq = cj[keep]
    co, so, _ = SS.brute_on('convt', (2, 2, 0, 0, 1), B, su, cq)
    for key, c, s in (('e1', c1, s1), ('e2', c2, s2), ('up', cu, su), ('j', cj, su), ('q', cq, su), ('out', co, so)):
        t = stages[key]
        assert torch.equal(t.indices.cpu(), c) and t.spatial_shape == list(s) and t.features.shape[0] == len(c), f'{key} on {name}'
    assert tuple(su) == tuple(s1) and 0 < len(cq) < len(cj) and len(co) == 8 * len(cq)
    for t in first:
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    # features and every gradient: the same stack with the two operations as explicit torch indexing on the reference maps
    ref_stages, ref, ref_keep = _decoder_step(net, name, False)
    assert torch.equal(keep, ref_keep) and len(ref) == len(first)
    for i, (a, b) in enumerate(zip(first, ref)):
        assert SS.same(a, b), f'tensor {i} on {name}: {int((SS.bits(a) != SS.bits(b)).sum())} elements differ'
    again = _decoder_step(net, name, True)[1]
    assert all(SS.same(a, b) for a, b in zip(again, first)), name


# ---------------------------------------------------------------------------------------------------------------- nothing old moved
def test_reference_shaped_unet_launches_exactly_what_it_launched_before():
    before = json.load(open(GOLDEN_LAUNCHES))
    names = _unet_launches()
    assert len(before) > 50 and not any(nm in NEW_ENTRY_POINTS for nm in names), sorted(set(names))
    assert names == before, [(i, a, b) for i, (a, b) in enumerate(zip(names, before)) if a != b][:5] + [len(names), len(before)]
