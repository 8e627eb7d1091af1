"""Dense interchange of sparse tensors on the device (csrc/sparse_dense.hip, ``SparseConvTensor.dense`` / ``from_dense``, ``ToDense``)
against the references of tests/_dense.py.  Every comparison is bit for bit: every operation here is a copy.
Kernels through the C ABI: scatter and gather in both layouts into NaN-poisoned destinations between guard regions -- every element
written, the guards intact --, the scatter under both index forms, the gather with coordinates outside grid and batch.  Cases: the full
product of widths, occupancy kinds and value kinds on the two smallest grids; on the other grids every occupancy kind at four widths
with normal values and every value kind on the random occupancy.  ``from_dense``: indices, features, position list, count, one host
read, both round-trip facts.  Autograd: both backward passes, launches by name, nothing launched that nobody asked for.  One layer stack
that ends in ``ToDense`` against the same stack with the torch composition behind it."""
import pytest
import torch

import _dense as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                      # fp32 elements before and after a destination (256 bytes: the destination stays 16-byte aligned)
POISON = 0x7fc0dead             # a NaN no reference holds
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1


def _buffer(numel):
    return torch.full((2 * GUARD + numel,), POISON, dtype=torch.int32, device=DEV).view(torch.float32)


def _check(buf, ref):
    """None, or what is wrong with a poisoned buffer whose interior should hold ``ref``"""
    got = buf.view(torch.int32).cpu()
    if not bool((got[:GUARD] == POISON).all() and (got[GUARD + ref.numel():] == POISON).all()):
        return 'a guard region was written'
    inner, want = got[GUARD:GUARD + ref.numel()], D.bits(ref).reshape(-1)
    if not torch.equal(inner, want):
        return f'{int((inner != want).sum())} elements differ, {int((inner == POISON).sum())} were never written'
    return None


def _record(monkeypatch):
    from unidet3d_amd import _lib as L
    names, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    return names


def _cases(name):
    small = name in D.SMALL_GRIDS
    for C in (D.WIDTHS if small else D.OTHER_WIDTHS):
        for occ in D.OCCUPANCIES:
            for kind in (D.VALUE_KINDS if small or occ == 'random10' else ['normal']):
                yield C, occ, kind


def _sparse(coords, feats, B, shape):
    from unidet3d_amd import sparse as S
    return S.SparseConvTensor(feats, coords.to(DEV), shape, B)


# ---------------------------------------------------------------------------------------------------------------- kernels, C ABI
@pytest.mark.parametrize('name', list(D.GRIDS))
def test_scatter_writes_every_element_once(name, monkeypatch):
    """both layouts, both index forms; an empty tensor is not the entry point's case (n > 0) but ``dense()``'s own, below"""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import geometry
    B, shape = D.grid(name)
    indexes, bad = {}, []
    for C, occ, kind in _cases(name):
        coords = D.case(name, occ)[2]
        n = len(coords)
        if not n:
            continue
        if occ not in indexes:
            cd, forms = coords.to(DEV), []
            for mode in ('bitmap', 'hash'):
                monkeypatch.setattr(geometry, '_INDEX_MODE', mode)
                forms.append(geometry.OccupancyIndex.from_coords(cd, B, shape))
            assert [ix.hashed for ix in forms] == [False, True]
            indexes[occ] = (cd, forms)
        f = D.values(kind, n, C)
        fd = f.to(DEV)
        for cf in (False, True):
            ref = D.dense_reference(f, coords, B, shape, cf)
            for ix in indexes[occ][1]:
                buf = _buffer(ref.numel())
                L.call('u3d_dense_scatter', L.ptr(fd), n, C, *ix.table(), B, *shape, int(cf), buf[GUARD:].data_ptr(), L.stream())
                msg = _check(buf, ref)
                if msg:
                    bad.append(f'{occ} {kind} C={C} channels_first={cf} hashed={ix.hashed} on {name}: {msg}')
    assert not bad, '\n'.join(bad[:40])


def _outside(B, shape):
    X, Y, Z = shape
    return torch.tensor([[B, 0, 0, 0], [-1, 0, 0, 0], [0, X, 0, 0], [0, -1, 0, 0], [0, 0, Y, 0], [0, 0, -1, 0], [0, 0, 0, Z], [0, 0, 0, -1],
                         [INT_MIN, 0, 0, 0], [INT_MAX, 0, 0, 0], [0, INT_MIN, 0, 0], [0, INT_MAX, 0, 0], [0, 0, INT_MIN, 0], [0, 0, INT_MAX, 0],
                         [0, 0, 0, INT_MIN], [0, 0, 0, INT_MAX], [INT_MAX, INT_MAX, INT_MAX, INT_MAX], [INT_MIN, INT_MIN, INT_MIN, INT_MIN],
                         [B - 1, X - 1, Y - 1, Z + 63], [B + 65535, 0, 0, 0]], dtype=torch.int32)


@pytest.mark.parametrize('name', list(D.GRIDS))
def test_gather_writes_every_row_and_reads_nothing_outside(name):
    from unidet3d_amd import _lib as L
    B, shape = D.grid(name)
    outside = _outside(B, shape)
    grids, bad = {}, []
    for C, occ, kind in _cases(name):
        if (C, kind) not in grids:
            last = D.values(kind, D.n_cells(name), C, 5).view(B, *shape, C)
            first = last.permute(0, 4, 1, 2, 3).contiguous()
            grids[(C, kind)] = ((last, last.to(DEV)), (first, first.to(DEV)))
        inside = D.case(name, occ)[2]
        # outside rows first, last and in the middle: a whole 64-row tile of them where the occupancy has that many rows
        coords = torch.cat([outside[:7], inside[:len(inside) // 2], outside, outside, outside, outside[:5], inside[len(inside) // 2:], outside[7:]])
        cd = coords.to(DEV)
        for cf in (False, True):
            host, dev = grids[(C, kind)][cf]
            ref = D.gather_reference(host, coords, B, shape, cf)
            buf = _buffer(ref.numel())
            L.call('u3d_dense_gather', L.ptr(dev), B, *shape, C, int(cf), L.ptr(cd), len(coords), buf[GUARD:].data_ptr(), L.stream())
            msg = _check(buf, ref)
            if msg:
                bad.append(f'{occ} {kind} C={C} channels_first={cf} on {name}: {msg}')
    assert not bad, '\n'.join(bad[:40])


# ---------------------------------------------------------------------------------------------------------------- from_dense
@pytest.mark.parametrize('name', list(D.GRIDS))
def test_from_dense_equals_argwhere(name, monkeypatch):
    from unidet3d_amd import geometry
    from unidet3d_amd import sparse as S
    reads, item = [], torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, 'item', lambda t: (reads.append(1), item(t))[1])
    B, shape = D.grid(name)
    bad = []
    for C, occ, kind in _cases(name):
        if name in D.SMALL_GRIDS and C not in D.OTHER_WIDTHS and kind != D.VALUE_KINDS[D.WIDTHS.index(C) % len(D.VALUE_KINDS)]:
            continue                                   # the other widths of the small grids: one value kind each, in turn
        x = D.dense_input(name, occ, kind, C)
        rc, rf, kept_ref, pos_ref = D.from_dense_reference(x)
        xd = x.to(DEV)
        where = f'{occ} {kind} C={C} on {name}'
        del reads[:]
        t = S.SparseConvTensor.from_dense(xd)
        if len(reads) != 1:
            bad.append(f'{where}: {len(reads)} host reads')
        if not (t.indices.dtype == torch.int32 and t.indices.is_cuda and torch.equal(t.indices.cpu(), rc)):
            bad.append(f'{where}: indices differ')
        if not D.same(t.features, rf):
            bad.append(f'{where}: features differ')
        if not (t.spatial_shape == list(shape) and t.batch_size == B and t.indice_dict == {} and t._index is None):
            bad.append(f'{where}: geometry fields')
        kept, pos, count = geometry.active_cells(xd)
        if not (count == len(kept_ref) and torch.equal(kept.cpu(), kept_ref) and torch.equal(pos.cpu(), pos_ref)):
            bad.append(f'{where}: kept / pos / count differ')
        # from_dense(x).dense(channels_first=False) is x, but for a -0.0 in an inactive cell (the cells that hold nothing but -0.0)
        back = t.dense(channels_first=False)
        if not D.same(back, D.dense_reference(rf, rc, B, shape, False)):
            bad.append(f'{where}: the way back differs')
        differ = D.bits(back) != D.bits(x)
        idle_neg = int((D.bits(x.view(-1, C)) == D.NEG_ZERO).all(1).sum())
        if not (idle_neg >= (len(rc) < D.n_cells(name)) and int(differ.sum()) == C * idle_neg and bool((D.bits(x)[differ] == D.NEG_ZERO).all())):
            bad.append(f'{where}: the way back differs from x in more than the -0.0 of inactive cells')
    assert not bad, '\n'.join(bad[:40])


@pytest.mark.parametrize('name', ['two_items_105', 'z_line_130_empty_middle', 'large'])
def test_from_dense_of_dense_keeps_the_rows_that_are_not_all_zero(name):
    from unidet3d_amd import sparse as S
    B, shape = D.grid(name)
    for occ in D.OCCUPANCIES:
        coords = D.case(name, occ)[2]
        for kind in D.VALUE_KINDS:
            f = D.values(kind, len(coords), 36)
            t = S.SparseConvTensor.from_dense(_sparse(coords, f.to(DEV), B, shape).dense(channels_first=False))
            keep = D.nonzero_rows(f)
            assert torch.equal(t.indices.cpu(), coords[keep]) and D.same(t.features, f[keep]), (occ, kind, name)
            # ... and through the channels-first layout with torch's permute in between
            t2 = S.SparseConvTensor.from_dense(_sparse(coords, f.to(DEV), B, shape).dense().permute(0, 2, 3, 4, 1).contiguous())
            assert torch.equal(t2.indices, t.indices) and D.same(t2.features, t.features), (occ, kind, name)


# ---------------------------------------------------------------------------------------------------------------- the methods, autograd
@pytest.mark.parametrize('name', list(D.GRIDS))
def test_dense_forward_and_backward(name):
    from unidet3d_amd import sparse as S
    B, shape = D.grid(name)
    C = 36
    for occ in D.OCCUPANCIES:
        coords = D.case(name, occ)[2]
        for kind in ('normal', 'neg_zero'):
            f = D.values(kind, len(coords), C)
            for cf in (True, False):
                fd = f.to(DEV).requires_grad_()
                t = _sparse(coords, fd, B, shape)
                y = (S.ToDense()(t) if cf else t.dense(channels_first=False))
                where = f'{occ} {kind} channels_first={cf} on {name}'
                assert y.is_contiguous() and y.dtype == torch.float32 and D.same(y, D.dense_reference(f, coords, B, shape, cf)), where
                for attr in ('_u3d_shadow', '_u3d_stats', '_u3d_from_conv'):
                    assert not hasattr(y, attr), where
                if not len(coords):
                    continue                                         # an empty tensor stays outside the graph: one fill, no Function
                dy = D.values(kind, D.n_cells(name), C, 7).view(y.shape)
                y.backward(dy.to(DEV))
                assert D.same(fd.grad, D.gather_reference(dy, coords, B, shape, cf)), where


def test_dense_launches(monkeypatch):
    """one launch forward (plus the index, once per tensor), one backward -- and only when the features ask; an empty tensor is one fill,
    a zero-size result nothing"""
    from unidet3d_amd import sparse as S
    B, shape, coords = D.case('two_items_105', 'checkerboard')
    f = D.values('normal', len(coords), 32)
    names = _record(monkeypatch)
    reads, item = [], torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, 'item', lambda t: (reads.append(1), item(t))[1])
    for grad in (False, True):
        for cf in (True, False):
            t = _sparse(coords, f.to(DEV).requires_grad_(grad), B, shape)
            del names[:], reads[:]
            y = t.dense(channels_first=cf)
            assert names.count('u3d_dense_scatter') == 1 and names[-1] == 'u3d_dense_scatter' and 'u3d_dense_gather' not in names, names
            assert all(nm.startswith('u3d_index_') for nm in names[:-1]) and reads == [], (names, reads)
            assert y.requires_grad == grad
            del names[:]
            y2 = t.dense(channels_first=cf)                          # the index is the tensor's: built once
            assert names == ['u3d_dense_scatter'] and D.same(y2, y)
            del names[:]
            if grad:
                y.backward(torch.ones_like(y))
                torch.cuda.synchronize()
                assert names == ['u3d_dense_gather'] and reads == [], names
    # a larger graph in which the features take no gradient: the backward reaches the Function and launches nothing
    t = _sparse(coords, f.to(DEV), B, shape)
    w = torch.ones((), device=DEV, requires_grad=True)
    y = t.dense() * w
    del names[:]
    y.sum().backward()
    assert names == [] and w.grad is not None
    # no rows: zeros by one fill; a zero-size result: nothing at all
    e = _sparse(coords[:0], torch.zeros(0, 32, device=DEV), B, shape)
    y = e.dense()
    assert names == [] and tuple(y.shape) == (B, 32, *shape) and not bool((D.bits(y) != 0).any())
    z = _sparse(coords[:0], torch.zeros(0, 32, device=DEV), B, (0, 5, 7)).dense(channels_first=False)
    assert names == [] and tuple(z.shape) == (B, 0, 5, 7, 32)


def test_from_dense_backward_and_launches(monkeypatch):
    from unidet3d_amd import sparse as S
    names = _record(monkeypatch)
    for name in ('two_items_105', 'z_line_130_empty_middle'):
        B, shape = D.grid(name)
        for occ in D.OCCUPANCIES:
            for kind in ('normal', 'neg_zero'):
                x = D.dense_input(name, occ, kind, 32)
                rc, rf, kept, pos = D.from_dense_reference(x)
                where = f'{occ} {kind} on {name}'
                xd = x.to(DEV).requires_grad_()
                del names[:]
                t = S.SparseConvTensor.from_dense(xd)
                assert names == ['u3d_dense_active', 'u3d_mask_compact'] + (['u3d_rows_take', 'u3d_cells_coords'] if len(rc) else []), (where, names)
                assert D.same(t.features, rf) and t.features.requires_grad, where
                df = D.values(kind, len(rc), 32, 9)
                del names[:]
                t.features.backward(df.to(DEV))
                torch.cuda.synchronize()
                assert names == (['u3d_rows_take'] if len(rc) else []), (where, names)
                assert tuple(xd.grad.shape) == tuple(x.shape) and D.same(xd.grad, D.dense_reference(df, rc, B, shape, False)), where
                # nothing asks for a gradient: no graph, no launch
                t = S.SparseConvTensor.from_dense(x.to(DEV))
                assert not t.features.requires_grad and t.features.grad_fn is None, where
    # no active cell: an empty tensor, nothing launched past the count
    x = torch.zeros(2, 3, 5, 7, 32)
    x[1, 2] = -0.0
    del names[:]
    t = S.SparseConvTensor.from_dense(x.to(DEV).requires_grad_())
    assert names == ['u3d_dense_active', 'u3d_mask_compact'] and tuple(t.features.shape) == (0, 32) and tuple(t.indices.shape) == (0, 4)
    assert t.indices.dtype == torch.int32 and t.spatial_shape == [3, 5, 7] and t.batch_size == 2 and t.indice_dict == {}
    assert not bool((D.bits(t.dense(channels_first=False)) != 0).any()) and names[2:] == []
    # a layer reads the new tensor: the occupancy index is built then, from the new coordinates
    x = D.dense_input('two_items_105', 'checkerboard', 'normal', 32)
    t = S.SparseConvTensor.from_dense(x.to(DEV))
    conv = S.SubMConv3d(32, 32, 3).to(DEV)
    del names[:]
    with torch.no_grad():
        out = conv(t)
    assert t._index is not None and 'u3d_index_mark' in names and out.features.shape[0] == t.features.shape[0]


def test_rows_only_tensors_are_refused():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    B, shape, coords = D.case('two_items_105', 'checkerboard')
    ghost = _sparse(coords, S.rows_only(torch.zeros(len(coords), 32, dtype=torch.bfloat16, device=DEV)), B, shape)
    for call in (ghost.dense, lambda: ghost.dense(channels_first=False), lambda: S.ToDense()(ghost)):
        with pytest.raises(U3DError, match='bf16 rows only'):
            call()


# ---------------------------------------------------------------------------------------------------------------- a layer stack
def test_a_stack_that_ends_in_to_dense():
    """forward: the reference scatter of the same stack's features without ``ToDense``; backward under a fixed d_dense: the weight
    gradients of the same stack with torch's zeros + index assignment + permute behind it, bit for bit -- the backward adds only copies
    and the library is bit-reproducible.  (The input rows take no gradient: the 16-channel input layer has no input-gradient kernel.)"""
    from unidet3d_amd import sparse as S
    torch.manual_seed(5)
    B, shape, coords = D.case('two_items_105', 'checkerboard')
    seq = S.SparseSequential(S.SubMConv3d(16, 32, 3), S.SparseConv3d(32, 32, 2, 2), S.ToDense()).to(DEV)
    bare = S.SparseSequential(seq[0], seq[1])
    f = D.values('normal', len(coords), 16)

    def step(ours, d_dense=None):
        seq.zero_grad(set_to_none=True)
        x = _sparse(coords, f.to(DEV), B, shape)
        if ours:
            y, out = seq(x), None
        else:
            out = bare(x)
            c = out.indices.long()
            d = torch.zeros(B, *out.spatial_shape, 32, device=DEV)
            d[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = out.features
            y = d.permute(0, 4, 1, 2, 3).contiguous()
        if d_dense is None:
            d_dense = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).to(DEV)
        y.backward(d_dense)
        S.join_wgrad_stream()
        torch.cuda.synchronize()
        return y.detach(), out, [p.grad.clone() for p in seq.parameters()], d_dense

    y, _, grads, d_dense = step(True)
    ry, out, ref, _ = step(False, d_dense)
    assert isinstance(y, torch.Tensor) and tuple(y.shape) == (B, 32, 1, 2, 3) and out.spatial_shape == [1, 2, 3] and out.features.shape[0] > 1
    assert D.same(y, D.dense_reference(out.features.detach().cpu(), out.indices.cpu(), B, out.spatial_shape, True)) and D.same(y, ry)
    assert len(grads) == len(ref) == 2
    for i, (a, b) in enumerate(zip(grads, ref)):
        assert float(a.abs().max()) > 0 and D.same(a, b), f'gradient {i}: {int((D.bits(a) != D.bits(b)).sum())} elements differ'
    again = step(True, d_dense)
    assert D.same(again[0], y) and all(D.same(a, b) for a, b in zip(again[2], grads))
