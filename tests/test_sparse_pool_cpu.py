"""Sparse pooling, host side (no GPU): the pair-list references of tests/_sparse_pool.py against torch's dense pooling on the float64 grid,
the layer constructors, the validation of the three C entry points before any HIP call, and the refusal of CPU tensors."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _conv_general as G
import _conv_geometry as cg
import _sparse_pool as SP

C = 4


def _pad(d, p, value):
    return F.pad(d, (p[2], p[2], p[1], p[1], p[0], p[0]), value=value)          # (F.pad lists the last axis first)


def _dense(cfg, name, x):
    """x float64 [n, C] on the input rows -> (grid [B, C, X, Y, Z] with 0 at inactive cells, occupancy mask [B, 1, X, Y, Z])"""
    _, B, shape, coords = SP.scene(name)
    return cg._scatter(x, coords, B, shape), cg._scatter(torch.ones(len(coords), 1, dtype=x.dtype), coords, B, shape)


@pytest.mark.parametrize('cfg', SP.CONFIGS)
def test_max_reference_equals_dense_max_pool(cfg):
    """forward and autograd backward of F.max_pool3d on the grid with -inf at inactive and padded cells (padded explicitly: torch refuses
    padding > kernel / 2), every scene and finite value kind; torch's dense rule is 'first maximal element of the scan', ours too"""
    k, s, p, d, _ = G.geom(cfg)
    for name in SP.SCENES:
        oc, oshape, _ = SP.brute(cfg, name)
        for kind in SP.FINITE_KINDS:
            c = SP.case(cfg, name, kind, C)
            if not c['n_out']:
                assert c['max']['y'].shape == (0, C) and not bool(c['max']['dx'].any())
                continue
            x = c['x'].double().requires_grad_()
            grid, mask = _dense(cfg, name, x)
            grid = _pad(torch.where(mask > 0, grid, torch.full((), float('-inf'), dtype=torch.float64)), p, float('-inf'))
            y = F.max_pool3d(grid, k, s, 0, d)
            assert tuple(y.shape[2:]) == tuple(oshape), (cfg, name)
            y = cg._sample(y, oc)
            where = f'{cfg} {kind} on {name}'
            assert torch.equal(y.detach(), c['max']['y'].double()), where
            y.backward(c['dy'].double())
            assert torch.equal(x.grad, c['max']['dx']) or SP.overlapping(cfg), where       # one term per element: exactly
            assert SP.excess(x.grad, c['max']['dx'], c['max']['dx_bound'] + 1e-300) <= 1.0, where


@pytest.mark.parametrize('cfg', SP.CONFIGS)
def test_avg_reference_equals_dense_sum_over_count(cfg):
    """conv3d(x, ones) / conv3d(mask, ones) at the output rows, forward and autograd backward"""
    k, s, p, d, _ = G.geom(cfg)
    ones = torch.ones(1, 1, *k, dtype=torch.float64)
    for name in SP.SCENES:
        oc, oshape, _ = SP.brute(cfg, name)
        for kind in SP.FINITE_KINDS:
            c = SP.case(cfg, name, kind, C)
            if not c['n_out']:
                continue
            x = c['x'].double().requires_grad_()
            grid, mask = _dense(cfg, name, x)
            B, X = grid.shape[0], grid.shape[2:]
            num = F.conv3d(grid.reshape(B * C, 1, *X), ones, stride=s, padding=p, dilation=d).reshape(B, C, *oshape)
            den = F.conv3d(mask, ones, stride=s, padding=p, dilation=d)
            assert torch.equal(cg._sample(den, oc)[:, 0].round().int(), c['avg']['count']), (cfg, name)
            y = cg._sample(num, oc) / cg._sample(den, oc)
            where = f'{cfg} {kind} on {name}'
            tol = lambda ref: 1e-13 * (1 + ref.abs().max())
            assert float((y.detach() - c['avg']['y']).abs().max()) <= tol(c['avg']['y']), where
            y.backward(c['dy'].double())
            assert float((x.grad - c['avg']['dx']).abs().max()) <= tol(c['avg']['dx']), where


def test_references_on_the_value_kinds_by_hand():
    """one window of three rows at offsets 1, 4, 6 of K = 8: the selection rule spelled out"""
    pairs = [(([], []) if k not in (1, 4, 6) else ([{1: 0, 4: 1, 6: 2}[k]], [0])) for k in range(8)]
    nan, inf = float('nan'), float('inf')
    x = torch.tensor([[-3.0, 1.0, 0.0, -0.0, nan, 2.0, -inf, 5.0],
                      [-2.0, 1.0, -0.0, 0.0, 7.0, nan, -inf, inf],
                      [-2.0, 0.0, 0.0, -0.0, 8.0, 9.0, -inf, inf]])
    y, arg = SP.max_forward(x, pairs, 1)
    assert arg[0].tolist() == [4, 1, 1, 1, 1, 4, 1, 4]                     # all-negative, tie -> first, signed zeros stay, NaN wins and stays
    assert torch.equal(SP.bits(y), SP.bits(torch.tensor([[-2.0, 1.0, 0.0, -0.0, nan, nan, -inf, inf]])))
    dy = torch.arange(1.0, 9.0)[None]
    dx, bound = SP.max_backward(dy, arg, pairs, 3)
    assert dx.tolist() == [[0, 2, 3, 4, 5, 0, 7, 0], [1, 0, 0, 0, 0, 6, 0, 8], [0] * 8] and not bool(bound.any())
    ya, cnt, _ = SP.avg_forward(torch.tensor([[3.0], [-3.0], [6.0]]), pairs, 1)
    assert cnt.tolist() == [3] and float(ya) == 2.0
    t = SP.table(pairs, 1, 'out')
    assert t.tolist() == [[-1, 0, -1, -1, 1, -1, 2, -1]]
    assert SP.table(pairs, 3, 'in').tolist() == [[-1, 0] + [-1] * 6, [-1] * 4 + [0, -1, -1, -1], [-1] * 6 + [0, -1]]


def test_value_kinds_tell_wrong_kernels_apart():
    """what the bit-equal GPU checks rest on: a zero-initialised maximum fails the all-negative kind, a sign-blind maximum (+0 for a
    window of both zeros) the signed zeros, and a gradient sent to every equal element the ties"""
    cfg, name = 'k3s2p1', 'block5'
    pairs, n_out = SP.brute(cfg, name)[2], len(SP.brute(cfg, name)[0])

    def amax(x, init):
        y = torch.full((n_out, C), init)
        for pi, po in pairs:
            y[SP._lt(po)] = torch.maximum(y[SP._lt(po)], x[SP._lt(pi)])
        return y

    c = SP.case(cfg, name, 'negative', C)
    assert bool((c['max']['y'] < 0).all()) and not torch.equal(amax(c['x'], 0.0), c['max']['y'])
    c = SP.case(cfg, name, 'zeros', C)
    blind = torch.where(amax((SP.bits(c['x']) >= 0).float(), 0.0) > 0, torch.tensor(0.0), torch.tensor(-0.0))      # +0 if any +0 in the window
    assert not torch.equal(SP.bits(blind), SP.bits(c['max']['y']))
    c = SP.case(cfg, name, 'ties', C)
    dx = torch.zeros(c['n_in'], C, dtype=torch.float64)
    for pi, po in pairs:
        dx[SP._lt(pi)] += torch.where(c['x'][SP._lt(pi)] == c['max']['y'][SP._lt(po)], c['dy'][SP._lt(po)].double(), torch.zeros((), dtype=torch.float64))
    assert not torch.equal(dx, c['max']['dx'])


def test_large_scene_and_overlap_predicate():
    _, B, shape, coords = SP.scene(SP.LARGE)
    assert B == 2 and tuple(shape) == (24, 24, 24) and 2400 <= len(coords) <= 3000
    key = ((coords[:, 0].long() * 24 + coords[:, 1]) * 24 + coords[:, 2]) * 24 + coords[:, 3]
    assert bool((key[1:] > key[:-1]).all())                                # canonical order
    assert [c for c in SP.CONFIGS if not SP.overlapping(c)] == ['k2s2p0', 'k122s2p0', 'k1s2p0', 'k3s3p1']
    assert any(SP.case(c, n, 'normal', C)['n_out'] == 0 for c in SP.CONFIGS for n in SP.SCENES)     # an empty output level exists


# ---------------------------------------------------------------------------------------------------------------- layers
def test_layer_constructors():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    for cls, mode in ((S.SparseMaxPool3d, 'max'), (S.SparseAvgPool3d, 'avg')):
        m = cls(2)
        assert m.mode == mode and m.geom == (2, 2, 2, 2, 2, 2, 0, 0, 0, 1, 1, 1) and m.K == 8 and m.kernel_size == 2      # stride=None: the kernel
        assert isinstance(m, S.SparseModule) and not list(m.parameters()) and m.indice_key is None
        m = cls(3, 2, 1, indice_key='p')
        assert m.geom == S.SparseConv3d(8, 8, 3, 2, 1).geom and m.indice_key == 'p' and m.stride == (2, 2, 2) and m.padding == (1, 1, 1)
        m = cls((3, 2, 1), None, (1, 0, 0), (2, 1, 1))
        assert m.geom == (3, 2, 1, 3, 2, 1, 1, 0, 0, 2, 1, 1) and m.K == 6 and m.kernel_size == (3, 2, 1)
        for bad in (dict(kernel_size=4), dict(kernel_size=0), dict(kernel_size=(3, 3)), dict(kernel_size=2, stride=0),
                    dict(kernel_size=2, padding=-1), dict(kernel_size=2, dilation=0), dict(kernel_size=2.0), dict(kernel_size=3, subm=True)):
            with pytest.raises(U3DError):
                cls(**bad)
        for width in (6, 2, 516):
            x = S.SparseConvTensor(torch.zeros(3, width), torch.zeros(3, 4, dtype=torch.int32), (8, 8, 8), 1)
            with pytest.raises(U3DError, match='channels'):
                cls(2)(x)


def test_a_cpu_tensor_is_refused():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    with pytest.raises(U3DError, match='no CPU fallback'):
        S.sparse_pool(torch.zeros(3, 8), None, 'max')
    with pytest.raises(U3DError, match='no CPU fallback'):
        S.sparse_pool(torch.zeros(3, 8), None, 'avg')
    with pytest.raises(U3DError, match='mode'):
        S.sparse_pool(torch.zeros(3, 8), None, 'sum')
    x = S.SparseConvTensor(torch.zeros(3, 8), torch.zeros(3, 4, dtype=torch.int32), (8, 8, 8), 1)
    with pytest.raises(U3DError):
        S.SparseMaxPool3d(2)(x)


def test_pool_and_conv_share_the_geometry_lookup():
    """same cache keys, same agreement check: a pool finds a convolution's rulebook under a shared key, a differing geometry is refused"""
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    x = S.SparseConvTensor(torch.zeros(3, 8), torch.zeros(3, 4, dtype=torch.int32), (8, 8, 8), 1)
    rb = S.Rulebook(torch.zeros(27, 1, dtype=torch.int32), torch.zeros(27, 1, dtype=torch.int32), torch.zeros(27, dtype=torch.int32), 27, 3, 1)
    conv = S.SparseConv3d(8, 8, 3, 2, 1, indice_key='q')
    rb.geom = conv._rb_geom
    x.indice_dict[('__down__', 'q')] = (None, [4, 4, 4], None, rb)
    assert S.SparseMaxPool3d(3, 2, 1, indice_key='q').geometry(x)[3] is rb and conv.geometry(x)[3] is rb
    assert S.SparseAvgPool3d(3, 2, 1, indice_key='q').geometry(x)[3] is rb
    with pytest.raises(U3DError, match='share an indice_key'):
        S.SparseMaxPool3d(3, 2, 0, indice_key='q').geometry(x)
    with pytest.raises(U3DError, match='share an indice_key'):
        S.SparseMaxPool3d(3, indice_key='q').geometry(x)                  # stride=None: stride 3
    with pytest.raises(U3DError, match="role must be 'out' or 'in'"):
        rb.neighbours('dst')


# ---------------------------------------------------------------------------------------------------------------- entry points
def _entry_points():
    from unidet3d_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(64)               # never dereferenced: the calls return before anything reads a tensor
    return l, ctypes.addressof(buf)


def test_pair_table_validates_before_any_hip_call():
    l, p = _entry_points()
    args = lambda: [p, p, p, 8, 16, 16, p, None]        # pair_key, pair_val, counts, K, cap, n, table, stream
    for i in (0, 1, 2, 6):
        a = args()
        a[i] = None
        assert l.u3d_pair_table(*a) == -1, f'NULL pointer {i}'                               # U3D_EINVAL
    for i, v in ((5, 0), (5, -3), (4, 0)):
        a = args()
        a[i] = v
        assert l.u3d_pair_table(*a) == -1, (i, v)
    assert b'pair_table' in l.u3d_last_error()
    for K in (0, 28):
        a = args()
        a[3] = K
        assert l.u3d_pair_table(*a) == -3 and b'offsets unsupported' in l.u3d_last_error()     # U3D_EUNSUPPORTED
    a = args()
    a[5] = (1 << 31) // 8
    assert l.u3d_pair_table(*a) == -3 and b'32-bit' in l.u3d_last_error()


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
def test_pool_entry_points_validate_before_any_hip_call(direction):
    l, p = _entry_points()
    fn = getattr(l, f'u3d_sparse_pool_{direction}')
    # fwd: x, table, n, K, C, mode, y, arg, count, stream | bwd: dy, table, n, K, C, mode, arg, count, dx, stream
    args = lambda mode=0: [p, p, 16, 8, 32, mode, p, p, p, None]
    out, arg, count = (6, 7, 8) if direction == 'fwd' else (8, 6, 7)
    for mode in (0, 1):
        for i in (0, 1, out, (arg, count)[mode]):           # (the last: the one of arg / count this mode needs)
            a = args(mode)
            a[i] = None
            assert fn(*a) == -1, f'NULL pointer {i}'
        for n in (0, -1):
            a = args(mode)
            a[2] = n
            assert fn(*a) == -1 and b'no rows' in l.u3d_last_error()
        for width in (0, 2, 6, 30, 516, 1024):
            a = args(mode)
            a[4] = width
            assert fn(*a) == -3 and b'width' in l.u3d_last_error(), width
        for K in (0, 28):
            a = args(mode)
            a[3] = K
            assert fn(*a) == -3 and b'offsets unsupported' in l.u3d_last_error()
        a = args(mode)
        a[2], a[4] = (1 << 31) // 512, 512
        assert fn(*a) == -3 and b'32-bit' in l.u3d_last_error()
    assert fn(*args(2)) == -1 and b'mode 2' in l.u3d_last_error()
