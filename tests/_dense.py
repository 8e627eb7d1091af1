"""Dense interchange of sparse tensors (``SparseConvTensor.dense`` / ``from_dense`` / ``ToDense``; csrc/sparse_dense.hip): grids, occupancy
kinds, value kinds and the references, written straight from the definition.  Case builders and checkers only: plain CPU tensors, no test
functions, no device use.  tests/test_dense_cpu.py checks the checker, tests/test_gpu_dense.py runs the kernels.

References: ``torch.zeros`` + index ASSIGNMENT of the rows (a bit copy -- not an addition into zeros: 0 + (-0.0) is +0.0 and would hide a
copy that is not a copy) + ``permute().contiguous()`` for channels first; ``np.argwhere((x != 0).any(-1))`` for ``from_dense`` (row-major
= ascending cell number = canonical order).  Every comparison is bit for bit (``same``): every operation here is a copy."""
import numpy as np
import torch

import _sparse_pool as SP
import _sparse_sets as SS

same, bits, VALUE_KINDS = SS.same, SS.bits, SS.VALUE_KINDS

# the smallest grid at which each edge exists: name -> (B, (X, Y, Z))
GRIDS = {
    'one_cell': (1, (1, 1, 1)),
    'two_items_105': (2, (3, 5, 7)),          # 105 cells per item: a full and a partial 64-cell tile, none may cross items; non-cubic
    'z_line_64': (1, (2, 2, 64)),             # z line of exactly one bitmap word
    'z_line_65': (1, (1, 3, 65)),             # one cell past a bitmap word
    'z_line_130_empty_middle': (3, (4, 4, 130)),      # three-word z lines; the middle batch item never holds a voxel
    'full_8': (2, (8, 8, 8)),
    'large': (2, (24, 24, 24)),               # 216 tiles per item; 'random10' is ``_sparse_pool.LARGE``
}
SMALL_GRIDS = ['one_cell', 'two_items_105']                   # the full product with WIDTHS runs here
OCCUPANCIES = ['empty', 'first', 'last', 'full', 'random10', 'checkerboard', 'tile_pair']
WIDTHS = [4, 8, 12, 16, 32, 36, 64, 68, 128, 256, 260, 512]  # every fill of a lane group, both sides of a 64-channel chunk, the column loop
OTHER_WIDTHS = [4, 36, 68, 260]                               # on the other grids
NEG_ZERO = torch.tensor(-0.0).view(torch.int32).item()


def grid(name):
    return GRIDS[name]


def n_cells(name):
    B, (X, Y, Z) = GRIDS[name]
    return B * X * Y * Z


def occupancy(kind, name):
    """bool numpy [B, X, Y, Z]"""
    B, shape = GRIDS[name]
    S = shape[0] * shape[1] * shape[2]
    cell = np.arange(B * S).reshape(B, *shape)
    if kind == 'empty':
        m = np.zeros_like(cell, dtype=bool)
    elif kind == 'first':
        m = cell == 0
    elif kind == 'last':                                   # the last cell of the last item
        m = cell == B * S - 1
    elif kind == 'full':
        m = np.ones_like(cell, dtype=bool)
    elif kind == 'random10':
        if name == 'large':
            c = SP.scene(SP.LARGE)[3].numpy()
            m = np.zeros_like(cell, dtype=bool)
            m[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = True
        else:
            m = np.random.RandomState(len(name)).rand(B, *shape) < 0.10
    elif kind == 'checkerboard':
        b, x, y, z = np.indices((B, *shape))
        m = (x + y + z + b) % 2 == 0
    elif kind == 'tile_pair':                              # a full 64-cell tile beside an empty one, item by item
        m = ((cell % S) // 64) % 2 == 0
    else:
        raise KeyError(kind)
    if name == 'z_line_130_empty_middle':
        m = m.copy()
        m[1] = False
    return m


def coords_of(mask):
    """int32 [n, 4] canonical (argwhere is row-major)"""
    return torch.tensor(np.ascontiguousarray(np.argwhere(mask)), dtype=torch.int32).reshape(-1, 4)


def cell_numbers(coords, shape):
    c = coords.long()
    return ((c[:, 0] * shape[0] + c[:, 1]) * shape[1] + c[:, 2]) * shape[2] + c[:, 3]


_CASES = {}


def case(name, occ):
    """(B, shape, coords) of an occupancy kind on a grid; built once"""
    if (name, occ) not in _CASES:
        B, shape = GRIDS[name]
        _CASES[(name, occ)] = (B, shape, coords_of(occupancy(occ, name)))
    return _CASES[(name, occ)]


def values(kind, n, C, seed=0):
    return SS.values(kind, n, C, seed)


# ---------------------------------------------------------------------------------------------------------------- references
def dense_reference(feats, coords, B, shape, channels_first=True):
    """zeros, then index assignment of the rows, then permute().contiguous() for channels first"""
    d = torch.zeros(B, *shape, feats.shape[1], dtype=torch.float32)
    c = coords.long()
    d[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = feats
    return d.permute(0, 4, 1, 2, 3).contiguous() if channels_first else d


def gather_reference(dense, coords, B, shape, channels_first=True):
    """rows[i] = dense[cell of coords[i]], a row of +0.0 for a coordinate outside the grid or the batch"""
    d = dense.permute(0, 2, 3, 4, 1) if channels_first else dense
    c = coords.long()
    lim = torch.tensor([B, *shape])
    ok = ((c >= 0) & (c < lim)).all(1)
    rows = torch.zeros(len(c), d.shape[-1], dtype=torch.float32)
    k = c[ok]
    rows[ok] = d[k[:, 0], k[:, 1], k[:, 2], k[:, 3]]
    return rows


def from_dense_reference(x):
    """(coords int32 [n, 4], features [n, C], kept int32 [n] = active cell numbers ascending, pos int32 [n_cells]) of a channels-last grid"""
    coords = coords_of((x != 0).any(-1).numpy())
    c = coords.long()
    kept = cell_numbers(coords, x.shape[1:4]).int()
    pos = torch.full((x.numel() // x.shape[-1],), -1, dtype=torch.int32)
    pos[kept.long()] = torch.arange(len(kept), dtype=torch.int32)
    return coords, x[c[:, 0], c[:, 1], c[:, 2], c[:, 3]], kept, pos


def dense_input(name, occ, kind, C, seed=0):
    """A channels-last grid for ``from_dense``: the rows ``values(kind)`` at the cells of the occupancy kind, +0.0 elsewhere; then, where
    the grid still has inactive cells, one cell that holds only -0.0 (stays inactive) and one cell whose only non-zero value is a NaN
    (becomes active).  A value kind's all-zero rows (``neg_zero``) leave their cells inactive: the reference goes by the values alone."""
    B, shape, coords = case(name, occ)
    x = dense_reference(values(kind, len(coords), C, seed), coords, B, shape, False)
    flat = x.view(-1, C)
    idle = torch.nonzero(~(flat != 0).any(1))[:, 0]
    if len(idle) >= 1:
        flat[idle[(len(idle) - 1) // 2]] = -0.0
    if len(idle) >= 2:
        flat[idle[-1], C - 1] = float('nan')
    return x


def nonzero_rows(feats):
    """the rows that ``from_dense(t.dense(channels_first=False))`` keeps: those that are not all-zero"""
    return (feats != 0).any(1)
