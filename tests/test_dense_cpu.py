"""Dense interchange of sparse tensors, host side (no GPU): the references of tests/_dense.py against a plain Python loop and against
sabotaged results, the validation of the four C entry points before any HIP call with their ``u3d_last_error`` texts, the argument errors
of ``dense`` / ``from_dense`` / ``ToDense`` that need no device, and the presence of the new symbols."""
import ctypes
import os
import re

import pytest
import torch

import _dense as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['u3d_dense_scatter', 'u3d_dense_gather', 'u3d_dense_active', 'u3d_cells_coords']
SMALL = 'two_items_105'
C = 8


# ---------------------------------------------------------------------------------------------------------------- the checker
@pytest.mark.parametrize('occ', D.OCCUPANCIES)
def test_references_equal_a_plain_loop(occ):
    B, (X, Y, Z), coords = D.case(SMALL, occ)
    for kind in D.VALUE_KINDS:
        f = D.values(kind, len(coords), C)
        last, first = torch.zeros(B, X, Y, Z, C), torch.zeros(B, C, X, Y, Z)
        for i, (b, x, y, z) in enumerate(coords.tolist()):
            for c in range(C):
                last[b, x, y, z, c] = first[b, c, x, y, z] = f[i, c]
        assert D.same(D.dense_reference(f, coords, B, (X, Y, Z), False), last), (occ, kind)
        assert D.same(D.dense_reference(f, coords, B, (X, Y, Z), True), first), (occ, kind)
        # the gather is the inverse on the rows, in either layout, and gives +0.0 rows outside
        probes = torch.cat([coords, torch.tensor([[B, 0, 0, 0], [-1, 0, 0, 0], [0, X, 0, 0], [0, 0, -1, 0], [0, 0, 0, Z], [2 ** 31 - 1, 0, 0, 0],
                                                  [0, -(2 ** 31), 0, 0]], dtype=torch.int32)])
        for cf, d in ((False, last), (True, first)):
            rows = D.gather_reference(d, probes, B, (X, Y, Z), cf)
            assert D.same(rows[:len(coords)], f) and not bool((D.bits(rows[len(coords):]) != 0).any()), (occ, kind, cf)
        # from_dense by a loop over the cells in ascending cell number
        x = D.dense_input(SMALL, occ, kind, C)
        rc, rf, kept, pos = D.from_dense_reference(x)
        flat, cells = x.view(-1, C), []
        for cell in range(flat.shape[0]):
            if any(v != 0 for v in flat[cell].tolist()):       # (nan != 0 is True)
                cells.append(cell)
        assert kept.tolist() == cells and D.same(rf, flat[cells]) and D.cell_numbers(rc, (X, Y, Z)).tolist() == cells, (occ, kind)
        assert [int(p) for p in pos.tolist()] == [cells.index(c) if c in cells else -1 for c in range(flat.shape[0])], (occ, kind)


def test_grids_and_occupancies_have_their_edges():
    assert D.n_cells('one_cell') == 1 and D.n_cells(SMALL) == 210 and D.grid(SMALL) == (2, (3, 5, 7))
    assert D.grid('z_line_64')[1][2] == 64 and D.grid('z_line_65')[1][2] == 65 and D.grid('z_line_130_empty_middle')[1][2] == 130
    for name in D.GRIDS:
        B, shape, _ = D.case(name, 'full')
        S = shape[0] * shape[1] * shape[2]
        sizes = {occ: len(D.case(name, occ)[2]) for occ in D.OCCUPANCIES}
        middle = name == 'z_line_130_empty_middle'
        assert sizes['empty'] == 0 and sizes['first'] == 1 == sizes['last'] and sizes['full'] == (B - middle) * S, name
        assert D.case(name, 'first')[2].tolist() == [[0, 0, 0, 0]] and D.case(name, 'last')[2].tolist() == [[B - 1, *[s - 1 for s in shape]]]
        if middle:
            assert all(1 not in D.case(name, occ)[2][:, 0].tolist() for occ in D.OCCUPANCIES)
        if S > 64:
            c = D.cell_numbers(D.case(name, 'tile_pair')[2], shape) % S
            assert set((c // 64 % 2).tolist()) == {0} and int((c < 64).sum()) == 64 * (B - middle)
    assert len(D.case('large', 'random10')[2]) == len(D.SP.scene(D.SP.LARGE)[3]) > 2000
    assert len(D.case('full_8', 'full')[2]) == 1024


def test_sabotaged_results_are_caught():
    B, shape, coords = D.case(SMALL, 'checkerboard')
    f = D.values('neg_zero', len(coords), C)
    ref = D.dense_reference(f, coords, B, shape, False)
    # an add into zeros: equal as numbers, not as bits
    c = coords.long()
    added = torch.zeros(B, *shape, C).index_put_((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), f, accumulate=True)
    assert torch.equal(added, ref) and not D.same(added, ref)
    assert int((D.bits(ref) == D.NEG_ZERO).sum()) > 0 and int((D.bits(added) == D.NEG_ZERO).sum()) == 0
    # x and z swapped in the cell number: the same shape, other cells
    f = D.values('normal', len(coords), C)
    ref = D.dense_reference(f, coords, B, shape, False)
    X, Y, Z = shape
    swapped = torch.zeros(B * X * Y * Z, C)
    swapped[((c[:, 0] * Z + c[:, 3]) * Y + c[:, 2]) * X + c[:, 1]] = f
    swapped = swapped.view(B, X, Y, Z, C)
    assert swapped.shape == ref.shape and not D.same(swapped, ref)
    assert not D.same(D.dense_reference(f, coords, B, shape, True), ref.permute(0, 4, 3, 2, 1).contiguous())
    # a tile that runs on into the next batch item: item 1 shifted by the 23 cells that fill item 0's second tile
    flat = ref.view(B, X * Y * Z, C)
    crossed = torch.cat([flat[0], torch.roll(flat[1], 128 - X * Y * Z, 0)]).view(ref.shape)
    assert not D.same(crossed, ref)
    # from_dense: a NaN alone makes a cell active, a cell of -0.0 alone does not
    x = D.dense_input(SMALL, 'random10', 'normal', C)
    coords2, feats, kept, pos = D.from_dense_reference(x)
    only_nan = torch.isnan(feats).any(1)
    assert int(only_nan.sum()) == 1 and int((feats[only_nan] != 0).sum()) == 1
    neg = (D.bits(x.view(-1, C)) == D.NEG_ZERO).all(1)
    assert int(neg.sum()) == 1 and int(pos[neg]) == -1
    assert len(kept) == len(D.case(SMALL, 'random10')[2]) + 1


def test_round_trip_facts_hold_for_the_references():
    for kind in D.VALUE_KINDS:
        B, shape, coords = D.case(SMALL, 'checkerboard')
        f = D.values(kind, len(coords), C)
        rc, rf, _, _ = D.from_dense_reference(D.dense_reference(f, coords, B, shape, False))
        keep = D.nonzero_rows(f)
        assert torch.equal(rc, coords[keep]) and D.same(rf, f[keep]), kind
        assert bool(keep.all()) == (kind != 'neg_zero')
        x = D.dense_input(SMALL, 'checkerboard', kind, C)
        rc, rf, _, _ = D.from_dense_reference(x)
        back = D.dense_reference(rf, rc, B, shape, False)
        differ = D.bits(back) != D.bits(x)
        assert bool(differ.any()) and bool((D.bits(x)[differ] == D.NEG_ZERO).all()) and not bool((D.bits(back)[differ] != 0).any()), kind


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def _tensor(n=3, C=8, shape=(8, 8, 8), B=1, dtype=torch.float32):
    from unidet3d_amd import sparse as S
    return S.SparseConvTensor(torch.zeros(n, C, dtype=dtype), torch.zeros(n, 4, dtype=torch.int32), shape, B)


def test_dense_argument_errors():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    with pytest.raises(U3DError, match='no CPU fallback'):
        _tensor().dense()
    with pytest.raises(U3DError, match='no CPU fallback'):
        S.ToDense()(_tensor())
    with pytest.raises(U3DError, match='fp32'):
        _tensor(dtype=torch.float64).dense()
    with pytest.raises(U3DError, match='fp32'):
        _tensor().replace_feature(torch.zeros(3, 2, 4)).dense()
    for width in (2, 6, 516):
        with pytest.raises(U3DError, match='multiple of 4'):
            _tensor(C=width).dense(channels_first=False)
    m = S.ToDense()
    assert isinstance(m, S.SparseModule) and not list(m.parameters())
    doc = ' '.join(S.SparseConvTensor.dense.__doc__.split())
    for text in ('every other cell +0.0', 'writes every element of the result once', 'No host read', 'not all-zero'):
        assert text in doc, text


def test_from_dense_argument_errors():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    fd = S.SparseConvTensor.from_dense
    with pytest.raises(U3DError, match='no CPU fallback'):
        fd(torch.zeros(1, 2, 2, 2, 8))
    for bad in (torch.zeros(1, 2, 2, 2, 8, dtype=torch.float64), torch.zeros(1, 2, 2, 2, 8, dtype=torch.bfloat16), torch.zeros(2, 2, 2, 8),
                torch.zeros(1, 1, 2, 2, 2, 8), [[0.0]]):
        with pytest.raises(U3DError, match=r'fp32 tensor \[B, X, Y, Z, C\]'):
            fd(bad)
    for width in (2, 6, 516):
        with pytest.raises(U3DError, match='multiple of 4'):
            fd(torch.zeros(1, 2, 2, 2, width))
    with pytest.raises(U3DError, match='contiguous'):
        fd(torch.zeros(1, 8, 2, 2, 2).permute(0, 2, 3, 4, 1))
    with pytest.raises(U3DError, match='contiguous'):
        fd(torch.zeros(1, 2, 2, 2, 16)[..., ::2])
    assert 'a NaN makes a cell active' in fd.__doc__


def test_a_grid_of_two_to_the_31_cells_is_refused():
    from unidet3d_amd import geometry, sparse as S
    from unidet3d_amd._lib import U3DError
    assert geometry.dense_cells(2, (1024, 1024, 1023), 'dense') == 2 ** 31 - 2 ** 21
    with pytest.raises(U3DError, match=r'dense: the grid 2 x 1024 x 1024 x 1024 has 2147483648 cells'):
        geometry.dense_cells(2, (1024, 1024, 1024), 'dense')
    t = _tensor(shape=(1024, 1024, 1024), B=2)
    for call in (t.dense, lambda: t.dense(channels_first=False), lambda: S.ToDense()(t)):
        with pytest.raises(U3DError, match=r'dense: the grid 2 x 1024 x 1024 x 1024 has 2147483648 cells'):
            call()
    with pytest.raises(U3DError, match=r'from_dense: the grid 32768 x 1 x 65536 x 1 has 2147483648 cells'):
        S.SparseConvTensor.from_dense(torch.zeros(1, 1, 1, 1, 4).expand(32768, 1, 65536, 1, 4))


def test_a_module_behind_to_dense_is_refused():
    from torch import nn
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    for seq in (S.SparseSequential(S.ToDense(), nn.ReLU()), S.SparseSequential(S.SubMConv3d(8, 8, 3), S.ToDense(), nn.Identity()),
                S.SparseSequential(S.ToDense(), S.ToDense())):
        with pytest.raises(U3DError, match='ToDense must come last'):
            seq(_tensor())
    with pytest.raises(U3DError, match='no CPU fallback'):          # as the last module it is accepted: the refusal is dense()'s
        S.SparseSequential(S.ToDense())(_tensor())
    with pytest.raises(U3DError, match='no CPU fallback'):
        S.SparseSequential(nn.Identity(), S.ToDense())(_tensor())


def test_geometry_module_has_the_helpers_and_imports_only_the_abi():
    from unidet3d_amd import geometry, sparse
    assert sparse.active_cells is geometry.active_cells and sparse.cells_coords is geometry.cells_coords and sparse.dense_cells is geometry.dense_cells
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
    raw = open(os.path.join(ROOT, 'include', 'u3d.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert hasattr(l, name) and name in _lib.PROTOTYPES, name
    assert re.search(r'\* S2 +Dense interchange', raw)
    assert 'sparse_dense.hip' in __import__('unidet3d_amd.csrc.build', fromlist=['SOURCES']).SOURCES
    src = open(os.path.join(ROOT, 'unidet3d_amd', 'csrc', 'sparse_dense.hip')).read()
    assert 'atomic' not in re.sub(r'//.*', '', src) and 'asm' not in re.sub(r'//.*', '', src) and 'hipMemset' not in src


GRIDS_TOO_LARGE = [(2, 1024, 1024, 1024), (1, 2 ** 31 - 1, 2, 1), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (1, 1, 1 << 16, 1 << 15)]
EMPTY_GRIDS = [(0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 0)]


def test_dense_scatter_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, 16, 32, p, p, 0, 1, 8, 8, 8, 1, p, None]     # feats, n, C, bitmap, rank, hash_slots, B, X, Y, Z, channels_first, dense, stream
    for layout in (0, 1):
        for i in (0, 3, 4, 11):
            a = args()
            a[i], a[10] = None, layout
            assert l.u3d_dense_scatter(*a) == -1 and b'dense_scatter: NULL pointer' in l.u3d_last_error(), i      # U3D_EINVAL
        for i, v in ((1, 0), (1, -3), (5, -1)):
            a = args()
            a[i], a[10] = v, layout
            assert l.u3d_dense_scatter(*a) == -1 and b'dense_scatter' in l.u3d_last_error(), (i, v)
        for g in EMPTY_GRIDS:
            a = args()
            a[6:10], a[10] = g, layout
            assert l.u3d_dense_scatter(*a) == -1 and b'dense_scatter: an empty grid' in l.u3d_last_error(), g
        for width in (0, 2, 6, 516):
            a = args()
            a[2], a[10] = width, layout
            assert l.u3d_dense_scatter(*a) == -3 and b'width' in l.u3d_last_error(), width                       # U3D_EUNSUPPORTED
        for g in GRIDS_TOO_LARGE:
            a = args()
            a[6:10], a[10] = g, layout
            assert l.u3d_dense_scatter(*a) == -3 and b'2^31 cells' in l.u3d_last_error(), g
        a = args()
        a[1], a[10] = 1 << 31, layout
        assert l.u3d_dense_scatter(*a) == -3 and b'32-bit' in l.u3d_last_error()
        a = args()                                                   # a grid below 2^31 cells that one launch cannot hold
        a[6:10], a[2], a[10] = (1, 1024, 1024, 1024), 512, layout
        assert l.u3d_dense_scatter(*a) == -3 and b'workgroups' in l.u3d_last_error()


def test_dense_gather_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, 1, 8, 8, 8, 32, 1, p, 16, p, None]           # dense, B, X, Y, Z, C, channels_first, coords, n, rows, stream
    for layout in (0, 1):
        for i in (0, 7, 9):
            a = args()
            a[i], a[6] = None, layout
            assert l.u3d_dense_gather(*a) == -1 and b'dense_gather: NULL pointer' in l.u3d_last_error(), i
        for n in (0, -1):
            a = args()
            a[8], a[6] = n, layout
            assert l.u3d_dense_gather(*a) == -1 and b'no rows' in l.u3d_last_error(), n
        for g in EMPTY_GRIDS:
            a = args()
            a[1:5], a[6] = g, layout
            assert l.u3d_dense_gather(*a) == -1 and b'dense_gather: an empty grid' in l.u3d_last_error(), g
        for width in (0, 2, 6, 516):
            a = args()
            a[5], a[6] = width, layout
            assert l.u3d_dense_gather(*a) == -3 and b'width' in l.u3d_last_error(), width
        for g in GRIDS_TOO_LARGE:
            a = args()
            a[1:5], a[6] = g, layout
            assert l.u3d_dense_gather(*a) == -3 and b'2^31 cells' in l.u3d_last_error(), g
        a = args()
        a[8], a[6] = 1 << 31, layout
        assert l.u3d_dense_gather(*a) == -3 and b'32-bit' in l.u3d_last_error()


def test_dense_active_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, 16, 32, p, None]                              # x, n_cells, C, mask, stream
    for i in (0, 3):
        a = args()
        a[i] = None
        assert l.u3d_dense_active(*a) == -1 and b'dense_active: NULL pointer' in l.u3d_last_error(), i
    for n in (0, -1):
        a = args()
        a[1] = n
        assert l.u3d_dense_active(*a) == -1 and b'no rows' in l.u3d_last_error(), n
    for width in (0, 2, 6, 516):
        a = args()
        a[2] = width
        assert l.u3d_dense_active(*a) == -3 and b'width' in l.u3d_last_error(), width
    for n in (1 << 31, 1 << 40):                                     # B X Y Z >= 2^31 cells
        a = args()
        a[1] = n
        assert l.u3d_dense_active(*a) == -3 and b'32-bit' in l.u3d_last_error(), n


def test_cells_coords_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, 16, 8, 8, 8, p, None]                         # cells, n, X, Y, Z, coords, stream
    for i in (0, 5):
        a = args()
        a[i] = None
        assert l.u3d_cells_coords(*a) == -1 and b'cells_coords: NULL pointer' in l.u3d_last_error(), i
    for n in (0, -1):
        a = args()
        a[1] = n
        assert l.u3d_cells_coords(*a) == -1 and b'no rows' in l.u3d_last_error(), n
    for g in EMPTY_GRIDS[1:]:
        a = args()
        a[2:5] = g[1:]
        assert l.u3d_cells_coords(*a) == -1 and b'cells_coords: an empty grid' in l.u3d_last_error(), g
    for g in GRIDS_TOO_LARGE:
        if g[1] * g[2] * g[3] >= 2 ** 31:
            a = args()
            a[2:5] = g[1:]
            assert l.u3d_cells_coords(*a) == -3 and b'2^31 cells' in l.u3d_last_error(), g
    a = args()
    a[1] = 1 << 31
    assert l.u3d_cells_coords(*a) == -3 and b'32-bit' in l.u3d_last_error()
