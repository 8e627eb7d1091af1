"""Sparse max / average pooling on the device (csrc/sparse_pool.hip) against the references of tests/_sparse_pool.py.
Table: ``Rulebook.neighbours`` bit-equal to the table of the brute-force pair lists.  Max: y and arg bit-equal on every configuration x
scene x value kind, the backward inside gamma_(m-1) sum|terms| (zero where windows do not overlap).  Average: forward and backward inside
gamma_(m+2) sum|terms|, count = the pair count.  Widths 4 .. 512 cover every lane-slot fill and the column loop past 256 (all of them
on two small scenes, a subset on the large one, one per other scene in rotation).  NaN row: row and column isolation, guard rows
untouched.  Empty levels launch nothing.  Modules: stacks with a pool run forward and backward twice, bit-identical, and share rulebooks
with convolutions through ``indice_key``.  The largest err / bound per operation goes to the parity log (test 'sparse_pool')."""
import pytest
import torch

import _conv_general as G
import _parity
import _sparse_pool as SP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDTHS = [4, 8, 16, 32, 36, 96, 160, 256, 260, 512]
ALL_WIDTH_SCENES = ['block5', 'line_x_65']
LARGE_WIDTHS = [4, 36, 260]


def _widths(name):
    if name in ALL_WIDTH_SCENES:
        return WIDTHS
    return LARGE_WIDTHS if name == SP.LARGE else [WIDTHS[SP.SCENES.index(name) % len(WIDTHS)]]


def _poison(sizes):
    """allocate and free NaN-filled blocks of these 4-byte element counts: the caching allocator hands them to the next torch.empty"""
    blocks = [torch.full((int(s),), float('nan'), dtype=torch.float32, device=DEV) for s in sizes if s > 0]
    del blocks


_LEVELS = {}


def _level(cfg, name):
    """the device rulebook of ``cfg`` on scene ``name`` (its lists are checked against ``brute`` by tests/test_gpu_conv_general.py)"""
    if (cfg, name) not in _LEVELS:
        from unidet3d_amd import sparse
        _, B, shape, coords = SP.scene(name)
        rows = coords.to(DEV)
        ix = sparse.OccupancyIndex.from_coords(rows, B, shape)
        geom = sparse.SparseMaxPool3d(**{k: v for k, v in G.layer_args(cfg).items()}).geom
        rb = sparse.build_conv_rulebook(rows, ix, B, shape, geom)[3]
        oc, _, pairs = SP.brute(cfg, name)
        assert (rb.n_in, rb.n_out, rb.K) == (len(coords), len(oc), len(pairs)), (cfg, name)
        _LEVELS[(cfg, name)] = rb
    return _LEVELS[(cfg, name)]


def _worse(ratios, op, r, where):
    if r >= ratios.setdefault(op, (0.0, None))[0]:
        ratios[op] = (r, where)


def _log(tag, ratios):
    rec = dict(case=tag, **{f'{k}_ratio': v[0] for k, v in ratios.items()}, **{f'{k}_worst': v[1] for k, v in ratios.items()})
    _parity.log_errors('sparse_pool', rec)
    print('sparse_pool', rec)


# ---------------------------------------------------------------------------------------------------------------- table
@pytest.mark.parametrize('cfg', SP.CONFIGS)
def test_neighbour_tables_equal_the_brute_force_tables(cfg):
    for name in SP.SCENES:
        rb = _level(cfg, name)
        _, _, pairs = SP.brute(cfg, name)
        for role, n in (('out', rb.n_out), ('in', rb.n_in)):
            _poison([n * rb.K])
            t = rb.neighbours(role)
            assert t.dtype == torch.int32 and tuple(t.shape) == (n, rb.K) and rb.neighbours(role) is t
            assert torch.equal(t.cpu(), SP.table(pairs, n, role)), f'{cfg} on {name}: {role}'


# ---------------------------------------------------------------------------------------------------------------- max
def _run(rb, c, mode):
    from unidet3d_amd import sparse
    C = c['x'].shape[1]
    _poison([rb.n_out * C, rb.n_out * C // 4, rb.n_out])
    y, aux = sparse.sparse_pool_forward(c['x'].to(DEV), rb, mode)
    _poison([rb.n_in * C])
    dx = sparse.sparse_pool_backward(c['dy'].to(DEV), rb, mode, aux)
    return y, aux, dx


@pytest.mark.parametrize('cfg', SP.CONFIGS)
def test_max_pool_is_bit_equal_and_its_backward_inside_the_bound(cfg):
    """every scene x value kind.  The all-negative kind fails a zero-initialised maximum, the signed zeros and the ties a kernel that takes
    the hardware maximum or sends the gradient to every equal element (tests/test_sparse_pool_cpu.py shows that they do)."""
    ratios, bad = {}, []
    for name in SP.SCENES:
        rb = _level(cfg, name)
        for C in _widths(name):
            for kind in SP.KINDS:
                c = SP.case(cfg, name, kind, C)
                if not c['n_out']:
                    continue
                y, arg, dx = _run(rb, c, 'max')
                where = f'{cfg} {kind} C={C} on {name}'
                if not torch.equal(SP.bits(y), SP.bits(c['max']['y'])):
                    bad.append(f'{where}: y differs in {int((SP.bits(y) != SP.bits(c["max"]["y"])).sum())} elements')
                if not (arg.dtype == torch.uint8 and torch.equal(arg.cpu(), c['max']['arg'])):
                    bad.append(f'{where}: arg differs')
                r = SP.excess(dx, c['max']['dx'], c['max']['dx_bound'])
                print(f'sparse_pool max {where}: dx err / bound = {r:.3g}')
                _worse(ratios, 'max_dx', r, where)
                if not r <= 1.0:
                    bad.append(f'{where}: dx err / bound = {r:.3g}')
                if not SP.overlapping(cfg) and not torch.equal(SP.bits(dx), SP.bits(c['max']['dx'].float())):
                    bad.append(f'{where}: dx of non-overlapping windows is not bit-equal')
    _log(f'max {cfg}', ratios)
    assert not bad, '\n'.join(bad[:40])


# ---------------------------------------------------------------------------------------------------------------- average
@pytest.mark.parametrize('cfg', SP.CONFIGS)
def test_avg_pool_forward_and_backward_inside_the_bound(cfg):
    ratios, bad = {}, []
    for name in SP.SCENES:
        rb = _level(cfg, name)
        for C in _widths(name):
            for kind in SP.FINITE_KINDS:
                c = SP.case(cfg, name, kind, C)
                if not c['n_out']:
                    continue
                y, count, dx = _run(rb, c, 'avg')
                where = f'{cfg} {kind} C={C} on {name}'
                if not (count.dtype == torch.int32 and torch.equal(count.cpu(), c['avg']['count'])):
                    bad.append(f'{where}: count differs')
                for op, got in (('y', y), ('dx', dx)):
                    r = SP.excess(got, c['avg'][op], c['avg'][f'{op}_bound'])
                    print(f'sparse_pool avg {where}: {op} err / bound = {r:.3g}')
                    _worse(ratios, f'avg_{op}', r, where)
                    if not r <= 1.0:
                        bad.append(f'{where}: {op} err / bound = {r:.3g}')
    _log(f'avg {cfg}', ratios)
    assert not bad, '\n'.join(bad[:40])


# ---------------------------------------------------------------------------------------------------------------- NaN row, guard rows
GUARD = 3
SENTINEL = 12345.0


def _raw(direction, src, tab, n, K, C, mode, aux=None):
    """the entry point itself on destination buffers of n + GUARD rows filled with a sentinel -> (dst, arg, count) as written"""
    from unidet3d_amd import _lib as L
    dst = torch.full((n + GUARD, C), SENTINEL, dtype=torch.float32, device=DEV)
    if direction == 'fwd':
        arg = torch.full((n + GUARD, C), 77, dtype=torch.uint8, device=DEV)
        count = torch.full((n + GUARD,), 77, dtype=torch.int32, device=DEV)
        L.call('u3d_sparse_pool_fwd', L.ptr(src), L.ptr(tab), n, K, C, mode, L.ptr(dst), L.ptr(arg), L.ptr(count), L.stream())
        return dst, arg, count
    arg, count = (aux, None) if mode == L.POOL_MAX else (None, aux)
    L.call('u3d_sparse_pool_bwd', L.ptr(src), L.ptr(tab), n, K, C, mode, L.ptr(arg), L.ptr(count), L.ptr(dst), L.stream())
    return dst, None, None


@pytest.mark.parametrize('mode', ['max', 'avg'])
@pytest.mark.parametrize('cfg,name,C', [('k3s2p1', SP.LARGE, 36), ('k2s2p0', SP.LARGE, 260), ('k3s1p1', 'block5', 512), ('k331s221p110', 'line_x_65', 8)])
def test_nan_row_stays_in_its_windows_and_channels_and_guard_rows_are_untouched(cfg, name, C, mode):
    from unidet3d_amd import _lib as L
    rb = _level(cfg, name)
    c = SP.case(cfg, name, 'normal', C)
    m = {'max': L.POOL_MAX, 'avg': L.POOL_AVG}[mode]
    n_in, n_out, K = rb.n_in, rb.n_out, rb.K
    t_out, t_in = rb.neighbours('out'), rb.neighbours('in')
    ch = torch.tensor(SP.NAN_CHANNELS(C))

    def poisoned(t, n):
        r = SP.nan_row(n)
        t = t.clone()
        t[r, ch] = float('nan')
        return t, r

    def check(got, clean, tab, r, n, all_nan):
        """rows of ``tab`` that hold r, channels ch: the only elements that may differ from the clean run (NaN all of them if ``all_nan``)"""
        got, clean = got.cpu(), clean.cpu()
        assert torch.equal(got[n:], torch.full((GUARD, C), SENTINEL)), 'guard rows written'
        hit = torch.zeros(n, C, dtype=torch.bool)
        rows = (tab.cpu() == r).any(1).nonzero().flatten()
        assert len(rows) >= 1
        hit[rows[:, None], ch[None, :]] = True
        diff = SP.bits(got[:n]) != SP.bits(clean[:n])
        assert not bool((diff & ~hit).any()), 'an element outside the NaN row\'s windows / channels changed'
        assert bool(torch.isnan(got[:n][hit]).any())
        if all_nan:
            assert bool(torch.isnan(got[:n][hit]).all())
        assert not bool(torch.isnan(got[:n][~hit]).any())

    x = c['x'].to(DEV)
    y0, arg0, cnt0 = _raw('fwd', x, t_out, n_out, K, C, m)
    xn, r = poisoned(c['x'], n_in)
    y1, arg1, cnt1 = _raw('fwd', xn.to(DEV), t_out, n_out, K, C, m)
    check(y1, y0, t_out, r, n_out, all_nan=True)
    # the aux buffer of the mode is written for the n rows only, the other one not at all
    if mode == 'max':
        assert bool((arg1[n_out:] == 77).all()) and bool((cnt1 == 77).all()) and torch.equal(arg0[:n_out].cpu(), c['max']['arg'])
    else:
        assert bool((cnt1[n_out:] == 77).all()) and bool((arg1 == 77).all()) and torch.equal(cnt1[:n_out].cpu(), c['avg']['count'])
    aux = (arg0 if mode == 'max' else cnt0)[:n_out].contiguous()
    dy = c['dy'].to(DEV)
    dx0, _, _ = _raw('bwd', dy, t_in, n_in, K, C, m, aux)
    dyn, r = poisoned(c['dy'], n_out)
    dx1, _, _ = _raw('bwd', dyn.to(DEV), t_in, n_in, K, C, m, aux)
    check(dx1, dx0, t_in, r, n_in, all_nan=mode == 'avg')


# ---------------------------------------------------------------------------------------------------------------- empty levels
def _spy_calls(monkeypatch):
    from unidet3d_amd import _lib as L
    seen, real = [], L.call

    def spy(name, *a):
        seen.append(name)
        return real(name, *a)
    monkeypatch.setattr(L, 'call', spy)
    return seen


@pytest.mark.parametrize('mode', ['max', 'avg'])
def test_empty_levels_launch_nothing(mode, monkeypatch):
    from unidet3d_amd import sparse as S
    cls = S.SparseMaxPool3d if mode == 'max' else S.SparseAvgPool3d
    seen = _spy_calls(monkeypatch)
    # no input rows (the functional form over the builder's rulebook of an empty level: it needs no input index)
    feats = torch.empty(0, 32, device=DEV, requires_grad=True)
    oc, oshape, _, rb = S.build_conv_rulebook(torch.empty(0, 4, dtype=torch.int32, device=DEV), None, 2, (8, 8, 8), cls(3, 2, 1).geom)
    assert (rb.n_in, rb.n_out) == (0, 0) and tuple(oc.shape) == (0, 4) and list(oshape) == [4, 4, 4]
    y = S.sparse_pool(feats, rb, mode)
    assert tuple(y.shape) == (0, 32) and y.requires_grad
    y.sum().backward()
    assert tuple(feats.grad.shape) == (0, 32)
    assert tuple(rb.neighbours('out').shape) == (0, 27) and tuple(rb.neighbours('in').shape) == (0, 27)
    # input rows, no output rows: a padding-free stride drops a voxel at the edge
    cfg, name = next((c, n) for c in SP.CONFIGS for n in SP.SCENES if len(SP.brute(c, n)[0]) == 0 and len(SP.scene(n)[3]) > 0)
    _, B, shape, coords = SP.scene(name)
    c = SP.case(cfg, name, 'normal', 32)
    feats = c['x'].to(DEV).requires_grad_()
    y = cls(**G.layer_args(cfg))(S.SparseConvTensor(feats, coords.to(DEV), shape, B))
    assert tuple(y.features.shape) == (0, 32) and y.features.requires_grad
    y.features.sum().backward()
    assert tuple(feats.grad.shape) == (c['n_in'], 32) and not bool(feats.grad.any())
    assert not [s for s in seen if 'pool' in s or s == 'u3d_pair_table'], seen


# ---------------------------------------------------------------------------------------------------------------- modules
def _stack(pool, k):
    from unidet3d_amd import sparse as S
    torch.manual_seed(7)
    return S.SparseSequential(S.SubMConv3d(32, 32, 3, indice_key='s1'), S.SparseBatchNorm(32), torch.nn.ReLU(), pool,
                              S.SubMConv3d(32, 32, 3, indice_key='s2'), S.SparseInverseConv3d(32, 32, k, indice_key='p')).to(DEV)


def _forward_backward(net, name):
    from unidet3d_amd import sparse as S
    _, B, shape, coords = SP.scene(name)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(len(coords), 32, generator=g).to(DEV).requires_grad_()
    net.train()
    net.zero_grad(set_to_none=True)
    x = S.SparseConvTensor(feats, coords.to(DEV), shape, B)
    y = net(x)
    y.features.backward(torch.randn(y.features.shape, generator=g).to(DEV))
    torch.cuda.synchronize()
    return x, y, [y.features.detach().clone(), feats.grad.clone()] + [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize('kind', ['max_k2s2', 'avg_k3s2p1'])
@pytest.mark.parametrize('name', ['block5_odd_extent', SP.LARGE])
def test_module_stack_with_a_pool_runs_twice_bit_identical(name, kind):
    from unidet3d_amd import sparse as S
    pool, k, cfg = (S.SparseMaxPool3d(2, 2, indice_key='p'), 2, 'k2s2p0') if kind == 'max_k2s2' else (S.SparseAvgPool3d(3, 2, 1, indice_key='p'), 3, 'k3s2p1')
    net = _stack(pool, k)
    _, B, shape, coords = SP.scene(name)
    x, y, first = _forward_backward(net, name)
    assert y.spatial_shape == list(shape) and y.batch_size == B and torch.equal(y.indices.cpu(), coords) and tuple(y.features.shape) == (len(coords), 32)
    oc, oshape, _, rb = x.indice_dict[('__down__', 'p')]
    roc, roshape, _ = SP.brute(cfg, name)
    assert torch.equal(oc.cpu(), roc) and list(oshape) == list(roshape) and rb.K == k ** 3
    assert all(torch.isfinite(t).all() for t in first) and float(first[1].abs().max()) > 0
    _, _, second = _forward_backward(net, name)
    assert all(torch.equal(SP.bits(a), SP.bits(b)) for a, b in zip(first, second))


def test_pool_and_conv_share_a_rulebook_through_the_indice_key():
    from unidet3d_amd import sparse as S
    from unidet3d_amd._lib import U3DError
    _, B, shape, coords = SP.scene('block5')
    feats = torch.randn(len(coords), 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    x = S.SparseConvTensor(feats, coords.to(DEV), shape, B)
    conv, pool = S.SparseConv3d(32, 64, 3, 2, 1, indice_key='q').to(DEV), S.SparseMaxPool3d(3, 2, 1, indice_key='q')
    yc, yp = conv(x), pool(x)
    rb = x.indice_dict[('__down__', 'q')][3]
    assert conv.geometry(x)[3] is rb and pool.geometry(x)[3] is rb and torch.equal(yc.indices, yp.indices)
    assert yp.features.grad_fn is None and not yp.features.requires_grad          # the input did not require a gradient
    c = SP.case('k3s2p1', 'block5', 'normal', 32)
    assert torch.equal(SP.bits(pool(x.replace_feature(c['x'].to(DEV))).features), SP.bits(c['max']['y']))
    with pytest.raises(U3DError, match='share an indice_key'):
        S.SparseAvgPool3d(3, 2, 0, indice_key='q')(x)
    with pytest.raises(U3DError, match='share an indice_key'):
        S.SparseConv3d(32, 64, 2, 2, indice_key='q').to(DEV)(x)
    # autograd through the functional form: dx of the reference
    xg = c['x'].to(DEV).requires_grad_()
    y = S.sparse_pool(xg, rb, 'max')
    assert y.grad_fn is not None
    y.backward(c['dy'].to(DEV))
    assert SP.excess(xg.grad, c['max']['dx'], c['max']['dx_bound']) <= 1.0


def test_neighbour_tables_are_rebuilt_ahead_by_precompute_tiles(monkeypatch):
    from unidet3d_amd import sparse as S
    _, B, shape, coords = SP.scene('block5')
    feats = torch.zeros(len(coords), 8, device=DEV, requires_grad=True)
    pool = S.SparseAvgPool3d(2, indice_key='h')
    S._TILE_HISTORY.pop(('__down__', 'h'), None)
    pool(S.SparseConvTensor(feats, coords.to(DEV), shape, B)).features.sum().backward()
    assert S._TILE_HISTORY[('__down__', 'h')] == {('nbr', 'out'), ('nbr', 'in')}
    x = S.SparseConvTensor(feats, coords.to(DEV), shape, B)
    rb = pool.geometry(x)[3]
    assert not rb._nbr
    rb.precompute_tiles()
    assert set(rb._nbr) == {'out', 'in'} and ('__down__', 'h') not in S._TILE_HISTORY
    seen = _spy_calls(monkeypatch)
    pool(x)
    assert 'u3d_pair_table' not in seen and 'u3d_sparse_pool_fwd' in seen
