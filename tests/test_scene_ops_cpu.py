"""Per-scene operations without a device: the references of tests/_scene_ops.py against second opinions and against sabotaged results,
the argument errors of ``topk_mask`` / ``prune_topk`` / ``SparseTopKPrune`` / ``global_pool`` that need no device, the validation of the
C entry points of include/u3d.h section S3 before any HIP call, the two plan queries, and the header / library / ctypes table agreement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _scene_ops as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('u3d_scene_offsets', 'u3d_scene_topk_plan', 'u3d_scene_topk_ws_bytes', 'u3d_scene_topk', 'u3d_scene_pool_plan',
               'u3d_scene_pool_ws_bytes', 'u3d_scene_pool_fwd', 'u3d_scene_pool_bwd')
SIZES = [5, 0, 17, 64, 0, 0, 33, 1]


def _offsets(sizes):
    return [0] + np.cumsum(sizes).tolist()


# ---------------------------------------------------------------------------------------------------------------- the checker
def test_offsets_reference_and_builders():
    for sizes in ([3], [0, 4], [4, 0], SIZES, [0, 0, 0]):
        c = SO.coords_of(sizes)
        assert c.dtype == torch.int32 and tuple(c.shape) == (sum(sizes), 4)
        assert SO.ref_offsets(c, len(sizes)) == _offsets(sizes)
        X, Y, Z = SO.grid_for(sizes)
        cell = ((c[:, 0].long() * X + c[:, 1]) * Y + c[:, 2]) * Z + c[:, 3]
        assert bool((cell[1:] > cell[:-1]).all())                         # canonical order
    c = SO.coords_of(SIZES, [8, 8, 8], seed=3)
    assert SO.ref_offsets(c, len(SIZES)) == _offsets(SIZES) and len(np.unique(c.numpy(), axis=0)) == len(c)


def test_rank_keys_follow_the_definition():
    f = lambda *b: SO._from_bits(list(b))
    k = SO.rank_keys(f(0x7fc00000, 0xffc00001, 0x7f800000, 0x7f7fffff, 0x00800000, 0x007fffff, 0x00000001, 0x00000000, 0x80000000, 0x80000001,
                       0xff800000)).tolist()
    assert k[0] == k[1] == 0xffffffff                                     # all NaNs equal, whatever sign and payload
    assert k[1] > k[2] > k[3] > k[4] > k[5] > k[6] > k[7] == k[8] > k[9] > k[10]      # NaN > +inf > ... > denormals > +0 == -0 > -denormal > -inf
    s = SO.rank_keys(f(0x7fc00000, 0x7f800000, 0x3f800000, 0x00000001, 0x80000000, 0x00000000, 0xff800000), largest=False).tolist()
    assert s[0] == 0xffffffff and s[1] < s[2] < s[3] < s[4] == s[5] < s[6] < s[0]      # numbers reversed, NaN still on top


@pytest.mark.parametrize('kind', SO.SCORE_KINDS)
def test_topk_reference_agrees_with_torch_stable_sort(kind):
    off = _offsets(SIZES)
    n = off[-1]
    s = SO.scores(kind, n, off, seed=5, block=60)
    for k in SO.k_values(SIZES):
        ref = SO.ref_topk_mask(s, off, k)
        assert torch.equal(ref, SO.torch_sort_mask(s, off, k)), (kind, k)
        assert [int(ref[off[b]:off[b + 1]].sum()) for b in range(len(SIZES))] == [min(kb, nb) for kb, nb in zip(SO.per_scene_k(k, len(SIZES)), SIZES)]
        if kind not in ('special',):                                      # without NaNs ``largest=False`` is the stable ascending sort
            small = SO.ref_topk_mask(s, off, k, largest=False)
            assert torch.equal(small, SO.torch_sort_mask(-s, off, k)), (kind, k)
    kept, pos = SO.compact_reference(ref)
    assert torch.equal(pos[kept.long()], torch.arange(len(kept), dtype=torch.int32)) and int((pos >= 0).sum()) == len(kept)


def test_smallest_keeps_nans_first_and_ties_on_the_lower_row():
    s = torch.tensor([1.0, float('nan'), -2.0, -2.0, 0.0, -0.0, float('nan'), 5.0])
    assert torch.nonzero(SO.ref_topk_mask(s, [0, 8], 3, largest=False))[:, 0].tolist() == [1, 2, 6]
    assert torch.nonzero(SO.ref_topk_mask(s, [0, 8], 4, largest=False))[:, 0].tolist() == [1, 2, 3, 6]
    assert torch.nonzero(SO.ref_topk_mask(s, [0, 8], 4, largest=True))[:, 0].tolist() == [0, 1, 6, 7]
    assert torch.nonzero(SO.ref_topk_mask(s, [0, 8], 5, largest=True))[:, 0].tolist() == [0, 1, 4, 6, 7]      # +0.0 == -0.0: the lower row


def _sabotaged_mask(s, off, k, how):
    """what a wrong kernel would give"""
    key = SO.rank_keys(s).tolist()
    if how == 'nan_dropped':                                              # NaNs rank last instead of first
        key = [0 if v == 0xffffffff else v for v in key]
    mask = torch.zeros(len(key), dtype=torch.bool)
    for b, kb in enumerate(SO.per_scene_k(k, len(off) - 1)):
        tie = (lambda i: -i) if how == 'tie_order' else (lambda i: i)     # ties to the HIGHER row
        order = sorted(range(off[b], off[b + 1]), key=lambda i: (-key[i], tie(i)))
        mask[order[:kb + (1 if how == 'off_by_one' else 0)]] = True
    return mask


def test_the_mask_check_catches_sabotage():
    off = _offsets(SIZES)
    half = [s // 2 for s in SIZES]
    for how, kind in (('tie_order', 'equal'), ('tie_order', 'two'), ('nan_dropped', 'special'), ('off_by_one', 'random'), ('off_by_one', 'equal')):
        s = SO.scores(kind, off[-1], off, seed=2)
        assert not torch.equal(_sabotaged_mask(s, off, half, how), SO.ref_topk_mask(s, off, half)), (how, kind)
    s = SO.scores('random', off[-1], off, seed=2)
    assert torch.equal(_sabotaged_mask(s, off, half, 'none'), SO.ref_topk_mask(s, off, half))


def test_pool_references_and_their_sabotage():
    off = _offsets(SIZES)
    n, C = off[-1], 8
    for kind in SO.VALUE_KINDS:
        x = SO.values(kind, n, C, off, seed=1)
        y, arg = SO.ref_global_max(x, off)
        for b in range(len(SIZES)):
            for c in range(C):
                h, a = SO.take_max_walk(x[off[b]:off[b + 1], c].tolist())
                if a < 0:                                                 # an empty scene: +0.0 and -1
                    assert int(arg[b, c]) == -1 and SO.bits(y[b, c]).item() == 0
                else:
                    assert int(arg[b, c]) == off[b] + a and SO.same(y[b, c], x[off[b] + a, c]), (kind, b, c)
        dy = torch.from_numpy(np.random.default_rng(0).standard_normal((len(SIZES), C)).astype(np.float32))
        dx = SO.ref_global_max_bwd(dy, arg, n)
        assert int((dx != 0).sum()) <= C * sum(1 for s in SIZES if s) and SO.same(dx[arg[0].long(), torch.arange(C)], dy[0])
        ok, ratio = SO.avg_check(torch.from_numpy(SO.ref_global_avg(x, off, np.float64).astype(np.float32)), x, off)
        assert ok and ratio <= 1.0, (kind, ratio)
        da = SO.ref_global_avg_bwd(dy, off, n)
        assert SO.same(da[off[2]], dy[2] * (torch.tensor(1.0) / torch.tensor(float(SIZES[2]))))
    x = SO.values('negative', n, C, off)
    y, arg = SO.ref_global_max(x, off)
    assert bool((y[[0, 2, 3, 6, 7]] < 0).all()) and bool((y[[1, 4, 5]] == 0).all())       # a maximum that starts from 0 would be 0 everywhere
    x = SO.values('nan_inf', n, C, off)
    y, _ = SO.ref_global_max(x, off)
    assert int(torch.isnan(y).sum()) == 1 and int(torch.isinf(y).sum()) == 1                # one row and column each: nothing leaks
    x = SO.values('integer', n, C, off)
    exact = SO.ref_global_avg(x, off)
    assert np.array_equal(exact.astype(np.float32), SO.ref_global_avg(x, off, np.float64).astype(np.float32))
    # sabotage: a wrong empty-scene row, an fp32 accumulation gone wrong by one ulp of the bound, a tie taken from the later row
    good = torch.from_numpy(exact.astype(np.float32))
    bad = good.clone()
    bad[1] = 1e-30
    assert SO.avg_check(good, x, off)[0] and not SO.avg_check(bad, x, off)[0]
    xr = SO.values('randn', n, C, off)
    good = torch.from_numpy(SO.ref_global_avg(xr, off).astype(np.float32))
    bad = good.clone()
    bad[3, 2] = np.nextafter(np.nextafter(bad[3, 2].numpy(), np.float32(9)), np.float32(9)).item()
    assert SO.avg_check(good, xr, off)[0] and not SO.avg_check(bad, xr, off)[0]
    xt = SO.values('ties', n, C, off)
    _, arg = SO.ref_global_max(xt, off)
    assert arg[:, 0].tolist() == [o if s else -1 for o, s in zip(off, SIZES)]


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def _tensor(n, C=8, B=2, dtype=torch.float32):
    from unidet3d_amd import sparse as S
    return S.SparseConvTensor(torch.zeros(n, C, dtype=dtype), torch.zeros(n, 4, dtype=torch.int32), (8, 8, 8), B)


def test_topk_argument_errors():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    x, s = _tensor(5), torch.zeros(5)
    for fn, name in ((S.topk_mask, 'topk_mask'), (S.prune_topk, 'prune_topk')):
        for bad in (torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.bfloat16), torch.zeros(5, dtype=torch.int32), [0.0] * 5):
            with pytest.raises(U3DError, match=name + r': the scores must be a torch.float32 tensor'):
                fn(x, bad, 1)
        for bad in (torch.zeros(4), torch.zeros(6), torch.zeros(5, 2), torch.zeros(1, 5), torch.zeros(())):
            with pytest.raises(U3DError, match=name + r': the scores must have one entry per row'):
                fn(x, bad, 1)
        for bad in (-1, [1, -3]):
            with pytest.raises(U3DError, match=name + r': k must be >= 0, got -'):
                fn(x, s, bad)
        for bad in ([1], [1, 2, 3], ()):
            with pytest.raises(U3DError, match=name + r': k must have one entry per scene: \d for batch_size 2'):
                fn(x, s, bad)
        for bad in (1.5, True, 'ab', [1, 2.0], torch.tensor([1, 2]), None):
            with pytest.raises(U3DError, match=name + r': k must be an int or a sequence of ints'):
                fn(x, s, bad)
        with pytest.raises(U3DError, match=name + r': the scores live on meta, the tensor on cpu'):
            fn(x, torch.zeros(5, device='meta'), 1)
        with pytest.raises(U3DError, match='multiple of 4'):
            fn(_tensor(5, C=6), s, 1)
        with pytest.raises(U3DError, match='no CPU fallback'):             # every refusal above came before this one: nothing was launched
            fn(x, s, [1, 2])
        with pytest.raises(U3DError, match='no CPU fallback'):
            fn(x, s.view(5, 1), 0)
        ghost = S.SparseConvTensor(S.rows_only(torch.zeros(4, 32, dtype=torch.bfloat16)), torch.zeros(4, 4, dtype=torch.int32), (8, 8, 8), 2)
        with pytest.raises(U3DError, match=name + ': this tensor exists as bf16 rows only'):
            fn(ghost, torch.zeros(0), 1)
    m = S.SparseTopKPrune(3, largest=False)
    assert isinstance(m, S.SparseModule) and not list(m.parameters()) and (m.k, m.largest) == (3, False)
    assert S.SparseTopKPrune([1, 2]).k == [1, 2] and S.SparseTopKPrune((4,)).largest is True
    with pytest.raises(U3DError, match='prune_topk: .*no CPU fallback'):
        m(x, s)
    for bad in (-1, [2, -1]):
        with pytest.raises(U3DError, match='SparseTopKPrune: k must be >= 0'):
            S.SparseTopKPrune(bad)
    for bad in (1.0, None, 'k', [1.0], True):
        with pytest.raises(U3DError, match='SparseTopKPrune: k must be an int or a sequence of ints'):
            S.SparseTopKPrune(bad)
    assert 'row ascending' in S.topk_mask.__doc__ and 'torch.topk' in S.topk_mask.__doc__


def test_global_pool_argument_errors_and_the_sequential_rule():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    x = _tensor(5)
    with pytest.raises(U3DError, match=r"global_pool: mode must be 'max' or 'avg', got 'sum'"):
        S.global_pool(x, 'sum')
    with pytest.raises(U3DError, match='global_pool: 6 channels'):
        S.global_pool(_tensor(5, C=6), 'max')
    with pytest.raises(U3DError, match='global_pool: 516 channels'):
        S.global_pool(_tensor(5, C=516), 'avg')
    with pytest.raises(U3DError, match='global_pool: features must be fp32'):
        S.global_pool(_tensor(5, dtype=torch.float64), 'avg')
    ghost = S.SparseConvTensor(S.rows_only(torch.zeros(4, 32, dtype=torch.bfloat16)), torch.zeros(4, 4, dtype=torch.int32), (8, 8, 8), 2)
    with pytest.raises(U3DError, match='global_pool: this tensor exists as bf16 rows only'):
        S.global_pool(ghost, 'max')
    for m, mode in ((S.SparseGlobalMaxPool(), 'max'), (S.SparseGlobalAvgPool(), 'avg')):
        assert isinstance(m, S.SparseModule) and not list(m.parameters()) and m.returns_dense
        with pytest.raises(U3DError, match='global_pool: .*no CPU fallback'):
            m(x)
        seq = S.SparseSequential(m, torch.nn.Identity())
        with pytest.raises(U3DError, match=f'SparseSequential: {type(m).__name__} must come last: what it returns is a dense tensor'):
            seq(x)
        with pytest.raises(U3DError, match='no CPU fallback'):             # as the last module it is allowed: the refusal is the kernel's
            S.SparseSequential(torch.nn.Identity(), m)(x)
    with pytest.raises(U3DError, match='SparseSequential: ToDense must come last: what it returns is a dense tensor, no layer of this library reads one'):
        S.SparseSequential(S.ToDense(), S.SparseGlobalMaxPool())(x)


def test_scene_offsets_argument_errors_and_the_order_messages():
    from unidet3d_amd import geometry, sparse as S
    from unidet3d_amd._lib import U3DError
    assert S.scene_offsets is geometry.scene_offsets and S.check_scene_order is geometry.check_scene_order
    for bad in (0, -1, 1.0, True):
        with pytest.raises(U3DError, match='scene_offsets: batch_size must be an int >= 1'):
            geometry.scene_offsets(torch.zeros(3, 4, dtype=torch.int32), bad)
    for bad in (torch.zeros(3, 3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int64), torch.zeros(12, dtype=torch.int32)):
        with pytest.raises(U3DError, match=r'scene_offsets: coordinates must be int32 \[n, 4\]'):
            geometry.scene_offsets(bad, 2)
    with pytest.raises(U3DError, match='no CPU fallback'):
        geometry.scene_offsets(torch.zeros(3, 4, dtype=torch.int32), 2)
    off, flag = geometry.scene_offsets(torch.zeros(0, 4, dtype=torch.int32), 3)           # no rows: zeros, no launch
    assert off.tolist() == [0, 0, 0, 0] and flag.tolist() == [0]
    geometry.check_scene_order(0, 'x', 2)
    with pytest.raises(U3DError, match=r'topk_mask: the batch indices descend: the tensor is not in canonical order'):
        geometry.check_scene_order(1, 'topk_mask', 2)
    for flag in (2, 3):                                                                    # outside the batch is said first
        with pytest.raises(U3DError, match=r'global_pool: a batch index lies outside \[0, 4\)'):
            geometry.check_scene_order(flag, 'global_pool', 4)
    c = torch.zeros(3, 4, dtype=torch.int32)
    assert not geometry.is_canonical(c) and geometry.is_canonical(geometry.mark_canonical(c))
    x = _tensor(0)
    assert x.scene_offsets.tolist() == [0, 0, 0] and x.replace_feature(x.features)._scene is x._scene


# ---------------------------------------------------------------------------------------------------------------- entry points
def _entry_points():
    from unidet3d_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(64)               # never dereferenced: the calls return before anything reads a tensor
    return l, ctypes.addressof(buf)


def test_new_symbols_are_in_the_header_the_library_and_the_table():
    from unidet3d_amd import _lib
    l = _lib.lib()
    text = open(os.path.join(ROOT, 'include', 'u3d.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r'\b' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S)
        assert m and hasattr(l, name) and name in _lib.PROTOTYPES, name
        assert len([p for p in m.group(1).split(',') if p.strip()]) == len(_lib.PROTOTYPES[name][1]), name
    assert 'sparse_scene.hip' in __import__('unidet3d_amd.csrc.build', fromlist=['SOURCES']).SOURCES
    src = open(os.path.join(ROOT, 'unidet3d_amd', 'csrc', 'sparse_scene.hip')).read()
    assert 'contract(off)' in src and not re.search(r'atomic\w*\s*\(\s*\(?\s*(float|double)', src)
    assert int(re.search(r'#define\s+U3D_ABI_VERSION\s+(\d+)', text).group(1)) == 117 == _lib.ABI_VERSION == l.u3d_version()
    assert re.search(r'\* S3  Per-scene operations', text)


def test_plan_queries():
    l, _ = _entry_points()
    R, P = ctypes.c_int(0), ctypes.c_int(0)
    for n, B, want in ((1, 1, 1), (256, 1, 1), (257, 1, 2), (100_000, 1, 391), (356_000, 8, 64), (500_000, 1, 512), (5000, 16, 20), (10, 1000, 1)):
        assert l.u3d_scene_topk_plan(n, B, ctypes.byref(R), ctypes.byref(P)) == 0 and (R.value, P.value) == (256, want), (n, B)
        assert l.u3d_scene_topk_ws_bytes(n, B) >= (4 * B * 256 + 10 * B + 4 * ((n + 255) // 256)) * 4
    assert l.u3d_scene_topk_plan(1000, 2, None, None) == 0
    assert l.u3d_scene_topk_plan(0, 1, None, None) == -1 and l.u3d_scene_topk_plan(5, 0, None, None) == -1
    assert l.u3d_scene_topk_plan(1 << 31, 1, None, None) == -3 and b'32-bit' in l.u3d_last_error()
    assert l.u3d_scene_topk_plan(5, 65536, None, None) == -3 and b'65535' in l.u3d_last_error()
    assert l.u3d_scene_topk_ws_bytes(0, 1) == 0 == l.u3d_scene_topk_ws_bytes(5, 0)
    Q = ctypes.c_int64(0)
    for n, B, rows in ((1, 1, 64), (65536, 4, 64), (65537, 4, 128), (356_000, 8, 384), (500_000, 1, 512)):
        assert l.u3d_scene_pool_plan(n, B, 32, ctypes.byref(R), ctypes.byref(Q)) == 0
        assert (R.value, Q.value) == (rows, (n + rows - 1) // rows + B), (n, B)
        assert R.value % 64 == 0 and 512 <= (n + R.value - 1) // R.value <= 1024 or R.value == 64         # the chip is filled, the second pass short
        assert l.u3d_scene_pool_ws_bytes(n, B, 32) == Q.value * 32 * 8
    assert l.u3d_scene_pool_plan(100, 1, 6, None, None) == -3 and b'width 6' in l.u3d_last_error()
    assert l.u3d_scene_pool_plan(0, 1, 32, None, None) == -1 and l.u3d_scene_pool_ws_bytes(0, 1, 32) == 0


def test_scene_offsets_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, 16, 2, p, p, None]                       # coords, n, B, offsets, flag, stream
    for i in (0, 3, 4):
        a = args()
        a[i] = None
        assert l.u3d_scene_offsets(*a) == -1 and b'scene_offsets: NULL pointer' in l.u3d_last_error(), i
    for i, v in ((1, 0), (1, -3), (2, 0), (2, -1)):
        a = args()
        a[i] = v
        assert l.u3d_scene_offsets(*a) == -1 and b'scene_offsets' in l.u3d_last_error(), (i, v)
    a = args()
    a[1] = 1 << 31
    assert l.u3d_scene_offsets(*a) == -3 and b'32-bit' in l.u3d_last_error()
    a = args()
    a[2] = 70000
    assert l.u3d_scene_offsets(*a) == -3 and b'65535' in l.u3d_last_error()


def test_scene_topk_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, p, p, p, p, 16, 2, 1, p, p, p, p, p, None]      # scores, coords, offsets, flag, k, n, B, largest, mask, kept, pos, result, ws
    for i in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12):
        a = args()
        a[i] = None
        assert l.u3d_scene_topk(*a) == -1 and b'scene_topk: NULL pointer' in l.u3d_last_error(), i
    for i, v in ((5, 0), (5, -1), (6, 0)):
        a = args()
        a[i] = v
        assert l.u3d_scene_topk(*a) == -1 and b'scene_topk' in l.u3d_last_error(), (i, v)
    a = args()
    a[5] = 1 << 31
    assert l.u3d_scene_topk(*a) == -3 and b'32-bit' in l.u3d_last_error()


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
def test_scene_pool_validates_before_any_hip_call(direction):
    l, p = _entry_points()
    if direction == 'fwd':
        fn, args = l.u3d_scene_pool_fwd, (lambda: [p, p, 16, 2, 32, 0, p, p, p, None])         # x, offsets, n, B, C, mode, y, arg, ws
        ptrs, (i_n, i_b, i_c, i_mode, i_arg) = (0, 1, 6, 8), (2, 3, 4, 5, 7)
    else:
        fn, args = l.u3d_scene_pool_bwd, (lambda: [p, p, p, p, 16, 2, 32, 0, p, None])         # dy, coords, offsets, arg, n, B, C, mode, dx
        ptrs, (i_n, i_b, i_c, i_mode, i_arg) = (0, 1, 2, 8), (4, 5, 6, 7, 3)
    what = f'scene_pool_{direction}'.encode()
    for i in ptrs + (i_arg,):
        a = args()
        a[i] = None
        assert fn(*a) == -1 and what + b': NULL pointer' in l.u3d_last_error(), i
    for i, v in ((i_n, 0), (i_n, -1), (i_b, 0), (i_mode, 2), (i_mode, -1)):
        a = args()
        a[i] = v
        assert fn(*a) == -1 and what in l.u3d_last_error(), (i, v)
    for width in (0, 2, 6, 30, 516, 1024):
        a = args()
        a[i_c] = width
        assert fn(*a) == -3 and b'width' in l.u3d_last_error(), width
    a = args()
    a[i_n] = 1 << 31
    assert fn(*a) == -3 and b'32-bit' in l.u3d_last_error()
