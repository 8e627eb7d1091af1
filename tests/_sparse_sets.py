"""Sparse tensors on different voxel sets (``sparse_add``, ``prune``; csrc/sparse_sets.hip): operand pairs, masks, value kinds and the
references, written straight from the definition.  Case builders and checkers only: plain CPU tensors, no test functions, no device use.
tests/test_sparse_sets_cpu.py checks the checker, tests/test_gpu_sparse_sets.py runs the kernels.

Voxel sets come from ``_conv_general.SCENES`` (``_conv_geometry.geometries()`` underneath); an operand pair is two masks over one scene's
rows, so both operands live on one grid and are canonical (a subset of a canonical order is canonical).

Geometry: the union is ``np.unique`` over the stacked rows (lexicographic on (b, x, y, z) == canonical order); the maps come from a
dictionary of the rows.  Values: ``torch.where`` on presence -- NOT an addition into zeros: 0 + (-0.0) is +0.0 and would hide a copy that
is not a copy.  Every comparison is bit for bit (``same``): the operations are copies and single fp32 additions."""
import numpy as np
import torch

import _conv_general as G
import _conv_geometry as cg
import _conv_transpose as T
import _sparse_pool as SP

SCENES = list(G.SCENES)
LARGE = SP.LARGE
RELATIONS = ['equal', 'disjoint', 'a_in_b', 'b_in_a', 'overlap', 'parity', 'a_empty', 'b_empty', 'both_empty']
SCENES_0_2 = ('scenes_0_2', 'empty_middle_scene')          # A only in scene 0, B only in scene 2: this scene alone has them
MASK_KINDS = ['all_true', 'all_false', 'first', 'last', 'alternating', 'runs63', 'runs64', 'runs65', 'random', 'scene_dropped']
VALUE_KINDS = ['normal', 'integer', 'neg_zero', 'nan_row', 'flt_max']
NAN_CHANNELS = lambda C: [c for c in range(C) if c % 3 == 1]


def scene(name):
    return SP.scene(name)


def relations(name):
    return RELATIONS + ([SCENES_0_2[0]] if name == SCENES_0_2[1] else [])


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(got, ref) -> bool:
    """bit for bit, shape and dtype included"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    return torch.equal(bits(got), bits(ref)) if got.dtype == torch.float32 else torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------------------------- operand pairs
def _operand_masks(rel, coords):
    n = len(coords)
    i = torch.arange(n)
    all_, none = torch.ones(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    if rel == 'equal':
        return all_, all_
    if rel == 'disjoint':
        return i < n // 2, i >= n // 2
    if rel == 'a_in_b':
        return i % 3 == 0, all_
    if rel == 'b_in_a':
        return all_, i % 3 == 0
    if rel == 'overlap':
        return i < (2 * n + 2) // 3, i >= n // 3
    if rel == 'parity':
        even = coords[:, 1:].sum(1) % 2 == 0
        return even, ~even
    if rel == 'scenes_0_2':
        return coords[:, 0] == 0, coords[:, 0] == 2
    if rel == 'a_empty':
        return none, all_
    if rel == 'b_empty':
        return all_, none
    if rel == 'both_empty':
        return none, none
    raise KeyError(rel)


def union_reference(a_coords, b_coords):
    """(union coords int32 [n_u, 4] canonical, rows_a, rows_b int32 [n_u]: operand row or -1, into_a [n_a], into_b [n_b]) from the definition"""
    stacked = np.concatenate([a_coords.numpy().reshape(-1, 4), b_coords.numpy().reshape(-1, 4)]).astype(np.int64)
    u = np.unique(stacked, axis=0) if len(stacked) else stacked
    row_of = {tuple(r): j for j, r in enumerate(u.tolist())}
    out = [torch.tensor(u.astype(np.int32)).reshape(-1, 4)]
    for c in (a_coords, b_coords):
        mine = {tuple(r): i for i, r in enumerate(c.tolist())}
        out.append(torch.tensor([mine.get(tuple(r), -1) for r in u.tolist()], dtype=torch.int32))
    for c in (a_coords, b_coords):
        out.append(torch.tensor([row_of[tuple(r)] for r in c.tolist()], dtype=torch.int32))
    return tuple(out)


_PAIRS = {}


def pair(name, rel):
    """dict(B, shape, a, b: operand coords; u, rows_a, rows_b, into_a, into_b: ``union_reference``) of relation ``rel`` on scene ``name``"""
    if (name, rel) not in _PAIRS:
        _, B, shape, coords = scene(name)
        ma, mb = _operand_masks(rel, coords)
        a, b = coords[ma].contiguous(), coords[mb].contiguous()
        u, ra, rb, ia, ib = union_reference(a, b)
        _PAIRS[(name, rel)] = dict(B=B, shape=tuple(shape), a=a, b=b, u=u, rows_a=ra, rows_b=rb, into_a=ia, into_b=ib)
    return _PAIRS[(name, rel)]


# ---------------------------------------------------------------------------------------------------------------- masks
def mask(kind, n, coords=None, seed=0):
    """torch.bool [n].  'scene_dropped': every row of the scene (batch entry) of the middle row goes -- with ``coords``; without, the
    middle third of the rows."""
    i = torch.arange(n)
    if kind == 'all_true':
        return torch.ones(n, dtype=torch.bool)
    if kind == 'all_false':
        return torch.zeros(n, dtype=torch.bool)
    if kind == 'first':
        return i == 0
    if kind == 'last':
        return i == n - 1
    if kind == 'alternating':
        return i % 2 == 0
    if kind.startswith('runs'):
        return (i // int(kind[4:])) % 2 == 0
    if kind == 'random':
        return torch.rand(n, generator=torch.Generator().manual_seed(100 + seed)) < 0.5
    if kind == 'scene_dropped':
        if coords is None or n == 0:
            return (i < n // 3) | (i >= (2 * n) // 3)
        return coords[:, 0] != coords[n // 2, 0]
    raise KeyError(kind)


def compact_reference(keep):
    """(kept int32 ascending, pos int32 [n]: position or -1) from the definition"""
    kept = torch.nonzero(keep)[:, 0].int()
    pos = torch.full((len(keep),), -1, dtype=torch.int32)
    pos[kept.long()] = torch.arange(len(kept), dtype=torch.int32)
    return kept, pos


# ---------------------------------------------------------------------------------------------------------------- values
def values(kind, n, C, seed):
    """fp32 [n, C] of one operand.  'flt_max': |v| in [2e38, 3.2e38], sign by ``seed`` parity -- operands of seeds of different parity
    have opposite signs in every row, so overlapping rows cancel to a finite value and would overflow with the signs alike."""
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == 'integer':
        return torch.randint(-64, 65, (n, C), generator=g).float()
    if kind == 'flt_max':
        return (2.0e38 + 1.2e38 * torch.rand(n, C, generator=g)).float() * (1.0 if seed % 2 == 0 else -1.0)
    x = torch.randn(n, C, generator=g)
    if kind == 'neg_zero':
        x[torch.arange(n) % 2 == seed % 2] = -0.0            # whole rows; with seeds of different parity half the common rows add -0.0 to a value
        x[torch.arange(n) % 5 == 0] = -0.0                   # ... and every fifth row is -0.0 in BOTH operands where both have it
    elif kind == 'nan_row' and n:
        x[n // 2, NAN_CHANNELS(C)] = float('nan')
    elif kind not in ('normal', 'neg_zero', 'nan_row'):
        raise KeyError(kind)
    return x


def take_reference(x, rows):
    """y[j] = x[rows[j]] bit for bit, a row of +0.0 where rows[j] is outside [0, len(x))"""
    rows = rows.long()
    ok = (rows >= 0) & (rows < len(x))
    if not len(x):
        return torch.zeros(len(rows), x.shape[1], dtype=x.dtype)
    return torch.where(ok[:, None], x[rows.clamp(0, len(x) - 1)], torch.zeros((), dtype=x.dtype))


def join_reference(a, rows_a, b, rows_b):
    """the union-add forward: fp32 a + b where both rows are present, the bits of the present one where one is (``torch.where``)"""
    pa, pb = (rows_a >= 0)[:, None], (rows_b >= 0)[:, None]
    ga, gb = take_reference(a, rows_a), take_reference(b, rows_b)
    return torch.where(pa & pb, ga + gb, torch.where(pa, ga, gb))


def prune_reference(x, keep, dy=None):
    """(y, dx): the kept rows in their old order; dx[i] = dy[position of i], +0.0 for a dropped row"""
    kept, pos = compact_reference(keep)
    y = x[kept.long()]
    return y, (None if dy is None else take_reference(dy, pos))


# ---------------------------------------------------------------------------------------------------------------- brute-force levels of a stack
def brute_on(kind, cfg, B, shape, coords):
    """``_conv_general.brute`` (kind 'conv') / ``_conv_transpose.brute`` (kind 'convt') of configuration ``cfg`` on ANY rows: both read
    their scene through a module global, which is pointed at these rows for the call.  -> (out_coords, out_shape, pairs)"""
    name = f'__rows_{hash((B, tuple(shape), tuple(coords.reshape(-1).tolist())))}'
    mod = G if kind == 'conv' else T
    orig = mod.scene
    mod.scene = lambda nm: (nm, B, tuple(shape), coords) if nm == name else orig(nm)
    try:
        return mod.brute(cfg, name)
    finally:
        mod.scene = orig


def dense_sum(a, a_coords, b, b_coords, u, B, shape):
    """the same sum by another road: both operands scattered into a dense float64 grid, added, sampled at the union's rows"""
    grid = cg._scatter(a.double(), a_coords, B, shape) + cg._scatter(b.double(), b_coords, B, shape)
    return cg._sample(grid, u)
