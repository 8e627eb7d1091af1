"""Sparse tensors on different voxel sets, host side (no GPU): the references of tests/_sparse_sets.py against a dense float64 grid and
against sabotaged results, the argument errors of ``sparse_add`` / ``prune`` that need no device, the validation of the four C entry
points before any HIP call with their ``u3d_last_error`` texts, the size query, and the presence of the new symbols."""
import ctypes
import os
import re

import pytest
import torch

import _sparse_sets as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 8
NEW_SYMBOLS = ['u3d_index_rows', 'u3d_mask_compact', 'u3d_mask_compact_ws_bytes', 'u3d_rows_take', 'u3d_rows_take2']


def _operands(p, kind, C=C):
    return SS.values(kind, len(p['a']), C, 0), SS.values(kind, len(p['b']), C, 1)


# ---------------------------------------------------------------------------------------------------------------- the checker
@pytest.mark.parametrize('name', SS.SCENES)
def test_reference_equals_the_dense_float64_sum(name):
    """integer values: every sum is exact in fp32 and in float64, so the two roads must agree exactly"""
    for rel in SS.relations(name):
        p = SS.pair(name, rel)
        a, b = _operands(p, 'integer')
        y = SS.join_reference(a, p['rows_a'], b, p['rows_b'])
        assert y.dtype == torch.float32 and tuple(y.shape) == (len(p['u']), C)
        assert torch.equal(y.double(), SS.dense_sum(a, p['a'], b, p['b'], p['u'], p['B'], p['shape'])), (name, rel)


@pytest.mark.parametrize('name', SS.SCENES)
def test_reference_geometry_is_canonical_and_consistent(name):
    _, B, shape, coords = SS.scene(name)
    for rel in SS.relations(name):
        p = SS.pair(name, rel)
        u = p['u'].long()
        key = ((u[:, 0] * shape[0] + u[:, 1]) * shape[1] + u[:, 2]) * shape[2] + u[:, 3]
        assert bool((key[1:] > key[:-1]).all()), (name, rel)
        for w in 'ab':
            rows, into, c = p[f'rows_{w}'], p[f'into_{w}'], p[w]
            assert int((rows >= 0).sum()) == len(c) and torch.equal(rows[into.long()], torch.arange(len(c), dtype=torch.int32))
            assert torch.equal(p['u'][into.long()], c), (name, rel)
        assert bool(((p['rows_a'] >= 0) | (p['rows_b'] >= 0)).all())
    n = len(coords)
    sizes = {rel: (len(SS.pair(name, rel)['a']), len(SS.pair(name, rel)['b']), len(SS.pair(name, rel)['u'])) for rel in SS.RELATIONS}
    assert sizes['equal'] == (n, n, n) and sizes['both_empty'] == (0, 0, 0) and sizes['a_empty'] == (0, n, n) and sizes['b_empty'] == (n, 0, n)
    assert sizes['disjoint'][2] == sizes['disjoint'][0] + sizes['disjoint'][1] == n
    assert sizes['a_in_b'][2] == sizes['a_in_b'][1] and sizes['b_in_a'][2] == sizes['b_in_a'][0]
    if n >= 3:
        assert sizes['overlap'][2] < sizes['overlap'][0] + sizes['overlap'][1] and max(sizes['overlap'][:2]) < n


def test_scenes_0_and_2_relation():
    p = SS.pair(*reversed(SS.SCENES_0_2))
    assert len(p['a']) == 27 and len(p['b']) == 12 and len(p['u']) == 39
    assert set(p['a'][:, 0].tolist()) == {0} and set(p['b'][:, 0].tolist()) == {2}


def test_sabotaged_results_are_caught():
    # rows in arrival order (a's rows, then b's new ones) instead of canonical order; interleaved sets, where the two orders differ
    p = SS.pair('block5', 'parity')
    a, b = _operands(p, 'normal')
    ref = SS.join_reference(a, p['rows_a'], b, p['rows_b'])
    only_b = p['rows_a'] < 0
    arrival = torch.cat([torch.nonzero(~only_b)[:, 0], torch.nonzero(only_b)[:, 0]])
    assert not torch.equal(arrival, torch.arange(len(arrival))) and not SS.same(ref[arrival], ref)
    assert not SS.same(p['u'][arrival], p['u'])
    # a dropped row
    p = SS.pair('block5', 'overlap')
    a, b = _operands(p, 'normal')
    ref = SS.join_reference(a, p['rows_a'], b, p['rows_b'])
    assert not SS.same(ref[:-1], ref) and not SS.same(torch.cat([ref[:3], ref[4:]]), ref)
    # an add into zeros on the -0.0 kind: the values are equal as numbers, the bits are not
    a, b = _operands(p, 'neg_zero')
    ref = SS.join_reference(a, p['rows_a'], b, p['rows_b'])
    zeros = torch.zeros(len(p['u']), C)
    zeros.index_add_(0, p['into_a'].long(), a)
    zeros.index_add_(0, p['into_b'].long(), b)
    assert torch.equal(zeros, ref) and not SS.same(zeros, ref)
    assert int((SS.bits(ref) == SS.bits(torch.tensor(-0.0))).sum()) > 0
    # the same for the pruning backward: a dropped row's gradient is +0.0, a kept -0.0 stays
    keep = SS.mask('alternating', len(p['u']))
    dy = SS.values('neg_zero', int(keep.sum()), C, 3)
    _, dx = SS.prune_reference(ref, keep, dy)
    assert not bool((SS.bits(dx[~keep]) != 0).any()) and int((SS.bits(dx[keep]) == SS.bits(torch.tensor(-0.0))).sum()) > 0


def test_value_kinds():
    p = SS.pair('block5', 'overlap')
    a, b = _operands(p, 'flt_max')
    ref = SS.join_reference(a, p['rows_a'], b, p['rows_b'])
    both = (p['rows_a'] >= 0) & (p['rows_b'] >= 0)
    assert bool(torch.isfinite(ref).all()) and float(ref[both].abs().max()) <= 1.2e38 < 2.0e38 <= float(a.abs().min())
    assert not bool(torch.isfinite(SS.join_reference(a, p['rows_a'], -b, p['rows_b'])[both]).any())      # signs alike: overflow
    a, b = _operands(p, 'nan_row')
    ref = SS.join_reference(a, p['rows_a'], b, p['rows_b'])
    bad = torch.isnan(ref)
    rows = {int(p['into_a'][len(p['a']) // 2]), int(p['into_b'][len(p['b']) // 2])}
    assert set(torch.nonzero(bad.any(1))[:, 0].tolist()) == rows and set(torch.nonzero(bad.any(0))[:, 0].tolist()) == set(SS.NAN_CHANNELS(C))


def test_masks_and_compaction_reference():
    for n in (1, 63, 64, 65, 257):
        for kind in SS.MASK_KINDS:
            m = SS.mask(kind, n)
            assert m.dtype == torch.bool and tuple(m.shape) == (n,)
            kept, pos = SS.compact_reference(m)
            assert bool((kept[1:] > kept[:-1]).all()) and int((pos >= 0).sum()) == len(kept) == int(m.sum())
            assert torch.equal(pos[kept.long()], torch.arange(len(kept), dtype=torch.int32))
    assert SS.mask('runs64', 257).tolist() == ([True] * 64 + [False] * 64) * 2 + [True]
    assert int(SS.mask('first', 65).sum()) == 1 == int(SS.mask('last', 65).sum()) and bool(SS.mask('last', 65)[64])
    _, B, shape, coords = SS.scene('empty_middle_scene')
    m = SS.mask('scene_dropped', len(coords), coords)
    assert 0 < int(m.sum()) < len(coords) and len(set(coords[~m][:, 0].tolist())) == 1


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def _tensor(n, C=8, shape=(8, 8, 8), B=1, dtype=torch.float32):
    from unidet3d_amd import sparse as S
    return S.SparseConvTensor(torch.zeros(n, C, dtype=dtype), torch.zeros(n, 4, dtype=torch.int32), shape, B)


def test_sparse_add_argument_errors():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    with pytest.raises(U3DError, match=r'batch_size: 1 and 2'):
        S.sparse_add(_tensor(3), _tensor(3, B=2))
    with pytest.raises(U3DError, match=r'spatial_shape: \[8, 8, 8\] and \[8, 8, 9\]'):
        S.sparse_add(_tensor(3), _tensor(3, shape=(8, 8, 9)))
    with pytest.raises(U3DError, match=r'channel count: \(3, 8\) and \(2, 16\)'):
        S.sparse_add(_tensor(3), _tensor(2, C=16))
    with pytest.raises(U3DError, match='batch_size'):                      # every operand of a fold is checked
        S.sparse_add(_tensor(3, B=2), _tensor(3, B=2), _tensor(3))
    with pytest.raises(U3DError, match='multiple of 4'):
        S.sparse_add(_tensor(3, C=6), _tensor(3, C=6))
    with pytest.raises(U3DError, match='fp32'):
        S.sparse_add(_tensor(3, dtype=torch.float64), _tensor(3, dtype=torch.float64))
    with pytest.raises(U3DError, match='no CPU fallback'):
        S.sparse_add(_tensor(3), _tensor(2))
    assert 'fold from the LEFT' in S.sparse_add.__doc__


def test_prune_argument_errors():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    x = _tensor(5)
    for bad in (torch.ones(5), torch.ones(5, dtype=torch.uint8), torch.ones(5, dtype=torch.int64), [True] * 5):
        with pytest.raises(U3DError, match='torch.bool'):
            S.prune(x, bad)
    for bad in (torch.ones(4, dtype=torch.bool), torch.ones(6, dtype=torch.bool), torch.ones(5, 1, dtype=torch.bool)):
        with pytest.raises(U3DError, match='one entry per row'):
            S.prune(x, bad)
    with pytest.raises(U3DError, match='no CPU fallback'):
        S.prune(x, torch.ones(5, dtype=torch.bool))
    with pytest.raises(U3DError, match='no CPU fallback'):
        S.SparsePrune()(x, torch.ones(5, dtype=torch.bool))
    m = S.SparsePrune()
    assert isinstance(m, S.SparseModule) and not list(m.parameters())
    with pytest.raises(U3DError, match='no CPU fallback'):
        S.rows_take(torch.zeros(3, 8), torch.zeros(3, dtype=torch.int32))


def test_geometry_module_has_the_entry_points_and_imports_only_the_abi():
    from unidet3d_amd import geometry, sparse
    assert callable(geometry.build_union_level) and callable(geometry.compact_mask) and callable(geometry.OccupancyIndex.rows_of)
    assert sparse.build_union_level is geometry.build_union_level and sparse.compact_mask is geometry.compact_mask
    src = open(geometry.__file__).read()
    assert re.findall(r'^from \. import (.*)$', src, flags=re.M) == ['_lib as L'] and not re.search(r'^from \.\w', src, flags=re.M)


# ---------------------------------------------------------------------------------------------------------------- entry points
def _entry_points():
    from unidet3d_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(64)               # never dereferenced: the calls return before anything reads a tensor
    return l, ctypes.addressof(buf)


def test_new_symbols_are_in_the_header_the_library_and_the_table():
    from unidet3d_amd import _lib
    l = _lib.lib()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'u3d.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert hasattr(l, name) and name in _lib.PROTOTYPES, name
    assert 'sparse_sets.hip' in __import__('unidet3d_amd.csrc.build', fromlist=['SOURCES']).SOURCES
    assert 'contract(off)' in open(os.path.join(ROOT, 'unidet3d_amd', 'csrc', 'sparse_sets.hip')).read()


def test_mask_compact_size_query():
    l, _ = _entry_points()
    q = l.u3d_mask_compact_ws_bytes
    assert [q(n) for n in (0, 1, 256, 257)] == [0, (2 + 64) * 4, (2 + 64) * 4, (4 + 64) * 4] and q(-5) == 0
    assert q(65537) == (2 * 257 + 64) * 4


def test_index_rows_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, 16, p, p, 0, 1, 8, 8, 8, p, None]       # coords, n, bitmap, rank, hash_slots, B, X, Y, Z, rows_out, stream
    for i in (0, 2, 3, 9):
        a = args()
        a[i] = None
        assert l.u3d_index_rows(*a) == -1 and b'index_rows: NULL pointer' in l.u3d_last_error(), i      # U3D_EINVAL
    for i, v in ((1, 0), (1, -2), (5, 0), (6, 0), (7, -1), (8, 0), (4, -1)):
        a = args()
        a[i] = v
        assert l.u3d_index_rows(*a) == -1 and b'index_rows' in l.u3d_last_error(), (i, v)
    a = args()
    a[1] = 1 << 31
    assert l.u3d_index_rows(*a) == -3 and b'32-bit' in l.u3d_last_error()                                  # U3D_EUNSUPPORTED


def test_mask_compact_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, 16, p, p, p, p, None]                   # mask, n, kept, pos, n_kept, ws, stream
    for i in (0, 2, 3, 4, 5):
        a = args()
        a[i] = None
        assert l.u3d_mask_compact(*a) == -1 and b'mask_compact: NULL pointer or no rows' in l.u3d_last_error(), i
    for n in (0, -1):
        a = args()
        a[1] = n
        assert l.u3d_mask_compact(*a) == -1 and b'no rows' in l.u3d_last_error()
    a = args()
    a[1] = 1 << 31
    assert l.u3d_mask_compact(*a) == -3 and b'32-bit' in l.u3d_last_error()


def test_rows_take_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, p, 16, 16, 32, p, None]                 # x, rows, n_out, n_src, C, y, stream
    for i in (0, 1, 5):
        a = args()
        a[i] = None
        assert l.u3d_rows_take(*a) == -1 and b'rows_take: NULL pointer' in l.u3d_last_error(), i
    for i, v in ((2, 0), (2, -1), (3, -1)):
        a = args()
        a[i] = v
        assert l.u3d_rows_take(*a) == -1 and b'rows_take' in l.u3d_last_error(), (i, v)
    for width in (0, 2, 6, 30, 516, 1024):
        a = args()
        a[4] = width
        assert l.u3d_rows_take(*a) == -3 and b'width' in l.u3d_last_error(), width
    for i in (2, 3):
        a = args()
        a[i] = 1 << 31
        assert l.u3d_rows_take(*a) == -3 and b'32-bit' in l.u3d_last_error(), i


def test_rows_take2_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, p, 16, p, p, 16, 16, 32, p, None]       # a, rows_a, n_a, b, rows_b, n_b, n_out, C, y, stream
    for i in (0, 1, 3, 4, 8):
        a = args()
        a[i] = None
        assert l.u3d_rows_take2(*a) == -1 and b'rows_take2: NULL pointer' in l.u3d_last_error(), i
    for i, v in ((6, 0), (6, -1), (2, -1), (5, -1)):
        a = args()
        a[i] = v
        assert l.u3d_rows_take2(*a) == -1 and b'rows_take2' in l.u3d_last_error(), (i, v)
    for width in (0, 2, 6, 30, 516, 1024):
        a = args()
        a[7] = width
        assert l.u3d_rows_take2(*a) == -3 and b'width' in l.u3d_last_error(), width
    for i in (2, 5, 6):
        a = args()
        a[i] = 1 << 31
        assert l.u3d_rows_take2(*a) == -3 and b'32-bit' in l.u3d_last_error(), i
