"""LayerNorm kernels (csrc/norm.hip) through the C ABI at every lane-slot fill state, template, grid and reduce-loop edge and value
kind against float64: u3d_layer_norm_fwd / _fwd_b16, u3d_layer_norm_bwd / _bwd_b16 / _bwd_sum, u3d_layer_norm_ws_bytes, the LayerNorm
half of u3d_ln_linear, and the wrappers dense.layer_norm / dense.ln_linear.

Cases, float64 references and acceptance bounds come from tests/_ln_edges.py (derived there, checked on the host by
tests/test_ln_edges_cpu.py); comparisons are elementwise error / bound <= 1, the `ints` kind bit for bit.  y is referred to the
device's own (mean, rstd), the backward to the stats it is given, so only the `rstd` check depends on the accuracy of rsqrtf.  Every
output buffer carries guard rows that must come back untouched, the workspace is allocated at exactly u3d_layer_norm_ws_bytes plus a
guarded tail, and every input is followed by NaN rows, so a row read past M poisons a result."""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _ln_edges as LE
from _parity import log_errors

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = -12288.0          # exact in bf16 too
N_GUARD = 8
WS_BYTE, WS_TAIL = 0xA5, 256


def _L():
    from unidet3d_amd import _lib as L
    return L


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(a):
    """[M, C] (or [C]) input followed by N_GUARD rows (elements) of NaN"""
    if a is None:
        return None
    a = torch.from_numpy(np.ascontiguousarray(a))
    return torch.cat([a, torch.full((N_GUARD,) + tuple(a.shape[1:]), float('nan'), dtype=a.dtype)]).to(DEV)


def _out(*shape, dtype=torch.float32):
    """output buffer of `shape` followed by N_GUARD guard rows (elements)"""
    return torch.full((shape[0] + N_GUARD,) + tuple(shape[1:]), GUARD, dtype=dtype, device=DEV)


def _intact(t, n):
    return bool((t[n:] == GUARD).all())


def _untouched(t):
    return bool((t == GUARD).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _np(t, n):
    return t[:n].cpu().numpy()


def _ws(M, C):
    """exactly u3d_layer_norm_ws_bytes(M, C) bytes and a guarded tail"""
    n = int(_L().lib().u3d_layer_norm_ws_bytes(M, C))
    if not os.environ.get('U3D_LN_BLOCKS'):
        assert n == LE.ws_bytes(M, C), (M, C, n)
    return torch.full((n + WS_TAIL,), WS_BYTE, dtype=torch.uint8, device=DEV), n


def _worst(acc, ms):
    for k, v in ms.items():
        acc[k] = max(acc.get(k, 0.0), v)


def _report(name, worst, **rec):
    for key, acc in sorted(worst.items()):
        print(name, rec, key, 'worst error / bound', {k: round(v, 4) for k, v in acc.items()})
    log_errors(name, dict(worst_error_over_bound={' '.join(k): v for k, v in worst.items()}, **rec))


# ============================================================================================================ calls
def _forward(c, with_res=True, b16=False, x=None):
    """one forward call into fresh guarded buffers -> namespace of device tensors (x: another first operand than c.x)"""
    L = _L()
    M, C = c.M, c.C
    f = SimpleNamespace(M=M, C=C, x=_rows(c.x if x is None else x), res=_rows(c.res) if with_res else None, gamma=_rows(c.gamma), beta=_rows(c.beta),
                        y=_out(M, C), s=_out(M, C), stats=_out(M, 2), y16=_out(M, C, dtype=torch.bfloat16) if b16 else None)
    args = (L.ptr(f.x), L.ptr(f.res), L.ptr(f.gamma), L.ptr(f.beta), M, C, LE.EPS, L.ptr(f.s), L.ptr(f.y))
    if b16:
        L.call('u3d_layer_norm_fwd_b16', *args, L.ptr(f.y16), L.ptr(f.stats), L.stream())
    else:
        L.call('u3d_layer_norm_fwd', *args, L.ptr(f.stats), L.stream())
    what = ('forward guards', c.kind, M, C, with_res, b16)
    assert _intact(f.y, M) and _intact(f.stats, M) and (_intact(f.s, M) if with_res else _untouched(f.s)), what
    assert f.y16 is None or _intact(f.y16, M), what
    return f


def _backward(entry, s, stats, gamma, dys, b16=False):
    """one backward call: entry 'bwd' (u3d_layer_norm_bwd, or _bwd_b16 with `b16`) on dys[0], or 'sum' (u3d_layer_norm_bwd_sum) on
    (dy, dy2, dy3), entries None = NULL.  s, stats, gamma, dys: numpy"""
    L = _L()
    M, C = s.shape
    ws, n_ws = _ws(M, C)
    b = SimpleNamespace(M=M, C=C, s=_rows(s), stats=_rows(np.asarray(stats, np.float32).reshape(M, 2)), gamma=_rows(gamma), dys=[_rows(d) for d in dys],
                        dx=_out(M, C), dx16=_out(M, C, dtype=torch.bfloat16) if b16 else None, dgamma=_out(C), dbeta=_out(C))
    tail = (M, C, L.ptr(b.dx))
    outs = (L.ptr(b.dgamma), L.ptr(b.dbeta), L.ptr(ws), L.stream())
    if entry == 'sum':
        dy, dy2, dy3 = b.dys
        L.call('u3d_layer_norm_bwd_sum', L.ptr(b.s), L.ptr(dy), L.ptr(dy2), L.ptr(dy3), L.ptr(b.gamma), L.ptr(b.stats), *tail, L.ptr(b.dx16), *outs)
    elif b16:
        L.call('u3d_layer_norm_bwd_b16', L.ptr(b.s), L.ptr(b.dys[0]), L.ptr(b.gamma), L.ptr(b.stats), *tail, L.ptr(b.dx16), *outs)
    else:
        L.call('u3d_layer_norm_bwd', L.ptr(b.s), L.ptr(b.dys[0]), L.ptr(b.gamma), L.ptr(b.stats), *tail, *outs)
    what = ('backward guards', entry, M, C, b16)
    assert _intact(b.dx, M) and _intact(b.dgamma, C) and _intact(b.dbeta, C) and bool((ws[n_ws:] == WS_BYTE).all()), what
    assert b.dx16 is None or _intact(b.dx16, M), what
    return b


def _fwd_host(f):
    return SimpleNamespace(stats=_np(f.stats, f.M), y=_np(f.y, f.M), s=_np(f.s, f.M))


def _bwd_host(b):
    return SimpleNamespace(dx=_np(b.dx, b.M), dgamma=_np(b.dgamma, b.C), dbeta=_np(b.dbeta, b.C))


# ============================================================================================================ checked runs
def _check_forward(c, worst, with_res=True):
    """u3d_layer_norm_fwd and _fwd_b16 of one case against the references -> (the fp32 rows s, the device stats), numpy"""
    M, C = c.M, c.C
    what = (c.kind, M, C, with_res)
    f = _forward(c, with_res)
    h = _fwd_host(f)
    s = LE.row_sum_in(c, with_res)
    if with_res:
        assert LE.same_bits(h.s, s), what                                         # one IEEE addition
    assert np.isfinite(h.y).all() and np.isfinite(h.stats).all(), what             # no row past M was read
    ms = LE.forward_margins(s, h, c.gamma, c.beta)
    _worst(worst.setdefault(('u3d_layer_norm_fwd', c.kind), {}), ms)
    assert max(ms.values()) <= 1.0, (what, ms)
    assert bool((h.y[:, 1] == 0).all()), what                                      # gamma = beta = 0
    if c.kind == 'ints':
        assert LE.same_bits(h.stats[:, 0], LE.exact_mean(s)), what                 # a true division, every row its own
    g = _forward(c, with_res, b16=True)
    assert _same(g.y, f.y) and _same(g.stats, f.stats) and _same(g.s, f.s), what
    assert _same(g.y16[:M], g.y[:M].to(torch.bfloat16)), what                      # one rounding, to nearest even
    f2 = _forward(c, with_res)
    assert _same(f2.y, f.y) and _same(f2.stats, f.stats) and _same(f2.s, f.s), what
    return s, h.stats


def _check_backward(c, s, stats, worst, full=True):
    """u3d_layer_norm_bwd_sum on (dy, dy2, dy3), run twice, against the references; `full`: also the plain and _b16 entry points"""
    M, C = s.shape
    what = (c.kind, M, C)
    b = _backward('sum', s, stats, c.gamma, (c.dy, c.dy2, c.dy3), b16=True)
    hb = _bwd_host(b)
    assert np.isfinite(hb.dx).all() and np.isfinite(hb.dgamma).all() and np.isfinite(hb.dbeta).all(), what
    ref = LE.bwd_ref(s, stats, c.gamma, LE.grad_sum(c.dy, c.dy2, c.dy3))
    ms = LE.backward_margins(ref, hb)
    _worst(worst.setdefault(('u3d_layer_norm_bwd_sum', c.kind), {}), ms)
    assert max(ms.values()) <= 1.0, (what, ms)
    if c.kind == 'ints':                                                           # bit for bit: no row lost, doubled or misattributed
        assert np.array_equal(hb.dgamma.astype(np.float64), ref.dgamma) and np.array_equal(hb.dbeta.astype(np.float64), ref.dbeta), what
    assert _same(b.dx16[:M], b.dx[:M].to(torch.bfloat16)), what
    b2 = _backward('sum', s, stats, c.gamma, (c.dy, c.dy2, c.dy3), b16=True)               # fixed-order reductions: the same bits again
    assert _same(b2.dx, b.dx) and _same(b2.dx16, b.dx16) and _same(b2.dgamma, b.dgamma) and _same(b2.dbeta, b.dbeta), what
    if not full:
        return
    p = _backward('bwd', s, stats, c.gamma, (c.dy,))
    hp = _bwd_host(p)
    ref1 = LE.bwd_ref(s, stats, c.gamma, c.dy)
    ms = LE.backward_margins(ref1, hp)
    _worst(worst.setdefault(('u3d_layer_norm_bwd', c.kind), {}), ms)
    assert max(ms.values()) <= 1.0, (what, ms)
    p16 = _backward('bwd', s, stats, c.gamma, (c.dy,), b16=True)
    q = _backward('sum', s, stats, c.gamma, (c.dy, None, None))
    for o in (p16, q):
        assert _same(o.dx, p.dx) and _same(o.dgamma, p.dgamma) and _same(o.dbeta, p.dbeta), what
    assert _same(p16.dx16[:M], p.dx[:M].to(torch.bfloat16)), what


def _check_case(c, worst, with_res=True, full=True):
    s, stats = _check_forward(c, worst, with_res)
    _check_backward(c, s, LE.unit_stats(c.M) if c.kind == 'ints' else stats, worst, full)


# ============================================================================================================ 1. widths and kinds
@pytest.mark.parametrize('C', LE.WIDTHS)
def test_every_kind_at_every_lane_slot_fill_state(C):
    worst = {}
    for M in LE.KIND_ROWS:
        for kind in LE.KINDS:
            _check_case(LE.make_case(kind, M, C), worst, with_res=True, full=M == LE.KIND_ROWS[0])
    _check_case(LE.make_case('randn', LE.KIND_ROWS[0], C), worst, with_res=False)          # res = NULL: sum_out is not written
    _report('ln_edges_widths', worst, C=C, template=LE.template(C), rows=LE.KIND_ROWS)


@pytest.mark.parametrize('C', LE.WIDTHS)
def test_constant_and_tiny_rows_give_rstd_of_eps_alone(C):
    """var = 0 (constant rows: up to the rounding of the mean; tiny rows: the squares underflow): rstd = fl(1 / sqrt(eps)) within the
    rstd bound -- which for the tiny kind is 4u and a little --, and y = beta wherever s is the row's mean"""
    for kind in ('const', 'tiny'):
        c = LE.make_case(kind, 9, C)
        f = _fwd_host(_forward(c))
        r = LE.fwd_ref(LE.row_sum_in(c))
        rows = np.arange(0, 9, 2) if kind == 'const' else np.arange(9)
        assert bool((r.var[rows] < 1e-30).all())
        assert LE.margin(f.stats[rows, 1], np.full(len(rows), 1 / np.sqrt(LE.EPS)), r.b_rstd[rows]) <= 1.0, (kind, C)
        if kind == 'tiny':
            assert bool((r.b_rstd[rows] < 4.001 * LE.U * r.rstd[rows]).all())
        else:                                                  # sharper: from the mean the device itself wrote
            ref, bound = LE.const_row_rstd(LE.row_sum_in(c)[rows, 0], f.stats[rows, 0], C)
            assert LE.margin(f.stats[rows, 1], ref, bound) <= 1.0, (kind, C)
    c = LE.make_case('const', 9, C)
    f = _fwd_host(_forward(c))
    assert LE.same_bits(f.y[0], c.beta) and LE.same_bits(f.stats[0], np.array([0.0, f.stats[0, 1]], np.float32))     # the all-zero row


# ============================================================================================================ 2. row counts
@pytest.mark.parametrize('C', LE.EVERY_M_WIDTHS)
def test_every_row_count_up_to_9(C):
    worst = {}
    for M in range(1, 10):
        _check_case(LE.make_case('ints', M, C), worst, full=False)
        _check_case(LE.make_case('randn', M, C), worst, full=False)
    _report('ln_edges_every_row_count', worst, C=C)


@pytest.mark.parametrize('C', LE.NB_WIDTHS)
def test_backward_workgroup_counts_at_the_reduce_loop_edges(C):
    """M = 4 nb and 4 nb - 3 for nb at every edge of layer_norm_reduce_k's three loops; integers: bit for bit"""
    worst = {}
    for M in LE.nb_rows():
        _check_case(LE.make_case('ints', M, C), worst, full=False)
    for nb in (17, 49, 113, 129):
        _check_case(LE.make_case('randn', 4 * nb - 3, C), worst, full=False)
    _report('ln_edges_reduce_edges', worst, C=C, nb=LE.NB_EDGES)


@pytest.mark.parametrize('M,C', [(M, 64) for M in LE.CAPPED_ROWS] + list(LE.CAPPED_WIDE))
def test_capped_backward_grid_and_row_stride_loop(M, C):
    """more rows than 4 x cap workgroup rows: the row-stride loop with a ragged last trip, the 1024-workgroup regime from M = 65536"""
    worst = {}
    _check_case(LE.make_case('ints', M, C), worst, full=False)
    if M in (2049, 65537):
        _check_case(LE.make_case('randn', M, C), worst, full=False)
    _report('ln_edges_capped', worst, M=M, C=C, nb=LE.ln_blocks(M))


def test_no_rows():
    """M = 0: the forward returns U3D_OK and writes nothing; the backward is not returned early -- dgamma and dbeta come back as
    +0.0 in every column, dx stays untouched"""
    L = _L()
    for C in (36, 772):
        c = LE.make_case('randn', 0, C)
        f = _forward(c)
        assert _untouched(f.y) and _untouched(f.s) and _untouched(f.stats)
        g = _forward(c, b16=True)
        assert _untouched(g.y) and _untouched(g.y16)
        for entry, dys, b16 in (('sum', (c.dy, c.dy2, c.dy3), True), ('bwd', (c.dy,), False)):
            b = _backward(entry, LE.row_sum_in(c), np.zeros((0, 2), np.float32), c.gamma, dys, b16=b16)
            assert _untouched(b.dx) and (b.dx16 is None or _untouched(b.dx16))
            zero = torch.zeros(C, device=DEV)
            assert _same(b.dgamma[:C], zero) and _same(b.dbeta[:C], zero)          # +0.0, not -0.0
    assert int(L.lib().u3d_layer_norm_ws_bytes(0, 64)) >= 2 * 64 * 4


# ============================================================================================================ 3. refused arguments
def _refused(C, M=5):
    """every entry point at width C into guarded buffers: -> ([(name, rc)], outputs)"""
    L = _L()
    lib, p, st = L.lib(), L.ptr, L.stream()
    Cb = max(abs(C), 8)
    x, r = torch.ones(M + N_GUARD, Cb, device=DEV), torch.ones(M + N_GUARD, Cb, device=DEV)
    gamma, beta = torch.ones(Cb, device=DEV), torch.zeros(Cb, device=DEV)
    stats = torch.ones(M + N_GUARD, 2, device=DEV)
    o = dict(y=_out(M, Cb), s=_out(M, Cb), stats=_out(M, 2), y16=_out(M, Cb, dtype=torch.bfloat16), dx=_out(M, Cb), dx16=_out(M, Cb, dtype=torch.bfloat16),
             dgamma=_out(Cb), dbeta=_out(Cb), ws=_out(2 * 2 * Cb + 64), Y=_out(M, 8), PRE=_out(M, 8))
    W, bias = torch.ones(8, Cb, device=DEV), torch.zeros(8, device=DEV)
    rcs = [('u3d_layer_norm_fwd', lib.u3d_layer_norm_fwd(p(x), p(r), p(gamma), p(beta), M, C, LE.EPS, p(o['s']), p(o['y']), p(o['stats']), st)),
           ('u3d_layer_norm_fwd_b16', lib.u3d_layer_norm_fwd_b16(p(x), p(r), p(gamma), p(beta), M, C, LE.EPS, p(o['s']), p(o['y']), p(o['y16']), p(o['stats']), st)),
           ('u3d_layer_norm_bwd', lib.u3d_layer_norm_bwd(p(x), p(r), p(gamma), p(stats), M, C, p(o['dx']), p(o['dgamma']), p(o['dbeta']), p(o['ws']), st)),
           ('u3d_layer_norm_bwd_b16', lib.u3d_layer_norm_bwd_b16(p(x), p(r), p(gamma), p(stats), M, C, p(o['dx']), p(o['dx16']), p(o['dgamma']), p(o['dbeta']),
                                                                 p(o['ws']), st)),
           ('u3d_layer_norm_bwd_sum', lib.u3d_layer_norm_bwd_sum(p(x), p(r), p(r), p(r), p(gamma), p(stats), M, C, p(o['dx']), p(o['dx16']), p(o['dgamma']),
                                                                 p(o['dbeta']), p(o['ws']), st)),
           ('u3d_ln_linear', lib.u3d_ln_linear(p(x), p(r), p(gamma), p(beta), LE.EPS, p(o['s']), p(o['y']), p(o['stats']), p(W), p(bias), 2, p(o['PRE']), p(o['Y']),
                                               M, C, 8, None, 0.0, st))]
    torch.cuda.synchronize()
    return rcs, o


@pytest.mark.parametrize('C', sorted(LE.REFUSED_WIDTHS))
def test_refused_widths_return_the_documented_status_and_launch_nothing(C):
    rcs, outs = _refused(C)
    assert all(rc == LE.REFUSED_WIDTHS[C] for _, rc in rcs), (C, rcs)
    for k, t in outs.items():
        assert _untouched(t), (C, k)


def test_missing_pointers_are_invalid_arguments():
    L = _L()
    lib, p, st = L.lib(), L.ptr, L.stream()
    c = LE.make_case('randn', 5, 64)
    f = _forward(c)
    y, stats, dx, dg, db = _out(5, 64), _out(5, 2), _out(5, 64), _out(64), _out(64)
    assert lib.u3d_layer_norm_fwd(p(f.x), p(f.res), p(f.gamma), p(f.beta), 5, 64, LE.EPS, None, p(y), p(stats), st) == LE.EINVAL       # res without sum_out
    assert lib.u3d_layer_norm_fwd_b16(p(f.x), p(f.res), p(f.gamma), p(f.beta), 5, 64, LE.EPS, None, p(y), None, p(stats), st) == LE.EINVAL
    assert lib.u3d_ln_linear(p(f.x), p(f.res), p(f.gamma), p(f.beta), LE.EPS, None, p(y), p(stats), p(f.x), None, 0, None, p(dx), 5, 64, 8, None, 0.0, st) == LE.EINVAL
    for name, args in (('u3d_layer_norm_bwd', ()), ('u3d_layer_norm_bwd_b16', (None,))):
        assert getattr(lib, name)(p(f.s), p(f.x), p(f.gamma), p(f.stats), 5, 64, p(dx), *args, p(dg), p(db), None, st) == LE.EINVAL   # no workspace
    assert lib.u3d_layer_norm_bwd_sum(p(f.s), p(f.x), None, None, p(f.gamma), p(f.stats), 5, 64, p(dx), None, p(dg), p(db), None, st) == LE.EINVAL
    assert lib.u3d_layer_norm_fwd(p(f.x), None, p(f.gamma), p(f.beta), -1, 64, LE.EPS, None, p(y), p(stats), st) == LE.EINVAL
    torch.cuda.synchronize()
    for t in (y, stats, dx, dg, db):
        assert _untouched(t)
    assert lib.u3d_layer_norm_fwd(p(f.x), None, p(f.gamma), p(f.beta), 5, 64, LE.EPS, None, p(y), p(stats), st) == LE.OK                 # no res: sum_out may be NULL
    assert _intact(y, 5) and not _untouched(y)                  # the call ran


# ============================================================================================================ 4. summed gradients
@pytest.mark.parametrize('C', LE.SUM_WIDTHS)
def test_bwd_sum_equals_the_plain_backward_fed_the_sum_in_the_kernels_order(C):
    for M in (5, 2053):
        c = LE.make_case('randn', M, C)
        s = LE.row_sum_in(c)
        stats = LE.model_forward(c).stats                       # any consistent statistics do: both calls are given the same
        assert not LE.same_bits(LE.grad_sum(c.dy, c.dy2, c.dy3), LE.grad_sum(c.dy, c.dy3, c.dy2))
        for dys in ((c.dy, c.dy2, None), (c.dy, c.dy2, c.dy3), (c.dy, None, c.dy3)):
            a = _backward('sum', s, stats, c.gamma, dys, b16=True)
            b = _backward('bwd', s, stats, c.gamma, (LE.grad_sum(*dys),), b16=True)
            what = (C, M, [d is not None for d in dys])
            assert _same(a.dx, b.dx) and _same(a.dx16, b.dx16) and _same(a.dgamma, b.dgamma) and _same(a.dbeta, b.dbeta), what


# ============================================================================================================ 5. isolation
@pytest.mark.parametrize('C', [64, 772])
def test_a_poisoned_row_stays_in_its_row_forward(C):
    M, k = 9, 4
    c = LE.make_case('randn', M, C)
    clean = _forward(c, b16=True)
    keep = [i for i in range(M) if i != k]
    for name, row in (('nan', np.full(C, np.nan, np.float32)), ('inf', np.full(C, np.inf, np.float32)), ('3e38', None)):
        x = c.x.copy()
        if row is None:
            x[k, C // 2] = 3e38                                # the squares overflow in this row
        else:
            x[k] = row
        f = _forward(c, b16=True, x=x)
        for a, b in ((f.y, clean.y), (f.stats, clean.stats), (f.s, clean.s), (f.y16, clean.y16)):
            assert _same(a[keep], b[keep]), (C, name)
        assert not bool(torch.isfinite(f.stats[k]).all()) or name == '3e38'
        assert not _same(f.y[k], clean.y[k]), (C, name)


@pytest.mark.parametrize('M,C', [(131, 36), (2100, 260)])
def test_a_poisoned_gradient_stays_in_its_row_and_column_backward(M, C):
    c = LE.make_case('randn', M, C)
    s = LE.row_sum_in(c)
    stats = LE.model_forward(c).stats
    clean = _backward('sum', s, stats, c.gamma, (c.dy, c.dy2, c.dy3))
    k, col = M // 2 + 1, C - 3
    keep = [i for i in range(M) if i != k]
    cols = [j for j in range(C) if j != col]
    dy = c.dy.copy()
    dy[k, col] = np.nan
    b = _backward('sum', s, stats, c.gamma, (dy, c.dy2, c.dy3))
    assert _same(b.dx[keep], clean.dx[keep])
    assert _same(b.dgamma[cols], clean.dgamma[cols]) and _same(b.dbeta[cols], clean.dbeta[cols])
    assert bool(torch.isnan(b.dgamma[col])) and bool(torch.isnan(b.dbeta[col])) and bool(torch.isnan(b.dx[k]).all())
    ref = _backward('sum', s, stats, c.gamma, (c.dy, c.dy2, None))
    dy2 = c.dy2.copy()
    dy2[k] = np.nan
    b = _backward('sum', s, stats, c.gamma, (c.dy, dy2, None))
    assert _same(b.dx[keep], ref.dx[keep])
    assert bool(torch.isnan(b.dgamma[:C]).all()) and bool(torch.isnan(b.dbeta[:C]).all())


# ============================================================================================================ 6. u3d_ln_linear
@pytest.mark.parametrize('C', [64, 384])
@pytest.mark.parametrize('M', [1, 333])
def test_ln_linear_is_layer_norm_fwd_then_linear_act_bit_for_bit(M, C):
    L = _L()
    N = 8
    c = LE.make_case('randn', M, C)
    rng = np.random.default_rng([M, C, 7])
    W, bias = _d((rng.standard_normal((N, C)) / np.sqrt(C)).astype(np.float32)), _d(rng.standard_normal(N).astype(np.float32))
    for with_res in (True, False):
        f = _forward(c, with_res)
        for act in (0, 1, 2):
            what = (M, C, with_res, act)
            Y0, P0 = _out(M, N), _out(M, N) if act == 2 else None
            L.call('u3d_linear_act', L.ptr(f.y), L.ptr(W), L.ptr(bias), act, L.ptr(P0), L.ptr(Y0), M, N, C, None, 0.0, L.stream())
            g = SimpleNamespace(x=_rows(c.x), res=_rows(c.res) if with_res else None, nq=_out(M, C), s=_out(M, C), stats=_out(M, 2), Y=_out(M, N),
                                P=_out(M, N) if act == 2 else None)
            L.call('u3d_ln_linear', L.ptr(g.x), L.ptr(g.res), L.ptr(f.gamma), L.ptr(f.beta), LE.EPS, L.ptr(g.s), L.ptr(g.nq), L.ptr(g.stats), L.ptr(W), L.ptr(bias),
                   act, L.ptr(g.P), L.ptr(g.Y), M, C, N, None, 0.0, L.stream())
            assert _same(g.nq, f.y) and _same(g.stats, f.stats) and _same(g.s, f.s), what          # guards included
            assert _same(g.Y, Y0) and _intact(g.Y, M) and not _untouched(g.Y), what
            assert act != 2 or (_same(g.P, P0) and _intact(g.P, M)), what


# ============================================================================================================ 7. wrappers
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('C', [384, 772])
def test_dense_layer_norm_returns_the_bits_of_the_c_abi(C, bf16):
    from unidet3d_amd import dense, dense16, precision as P
    M = 37
    c = LE.make_case('randn', M, C)
    x, res, w, b = (_d(a).requires_grad_() for a in (c.x, c.res, c.gamma, c.beta))
    with (P.operands('bf16') if bf16 else contextlib.nullcontext()):
        act16 = dense._flow(x, C).act16                          # bf16 activations: the _b16 entry points, copies attached to y and dx
        assert act16 == (bf16 and P.bf16_act() and C % 32 == 0)
        y = dense.layer_norm(x, w, b, LE.EPS, res)
        y16 = dense16.b16_of(y) if act16 else None
        y.backward(_d(c.dy))
    f = _forward(c, b16=act16)
    assert _same(y.detach(), f.y[:M])
    s = _np(f.s, M)
    g = _backward('sum', s, _np(f.stats, M), c.gamma, (c.dy, None, None), b16=act16)
    assert _same(x.grad, g.dx[:M]) and _same(res.grad, x.grad) and _same(w.grad, g.dgamma[:C]) and _same(b.grad, g.dbeta[:C])
    if act16:
        assert y16 is not None and _same(y16, f.y16[:M])


@pytest.mark.parametrize('C', [64, 384])
def test_dense_ln_linear_normalises_as_the_c_abi(C):
    from unidet3d_amd import dense
    M, N = 37, 8
    c = LE.make_case('randn', M, C)
    rng = np.random.default_rng([C, 11])
    x, w, b = (_d(a).requires_grad_() for a in (c.x, c.gamma, c.beta))
    W, bias = _d((rng.standard_normal((N, C)) / np.sqrt(C)).astype(np.float32)).requires_grad_(), _d(rng.standard_normal(N).astype(np.float32)).requires_grad_()
    nq, y = dense.ln_linear(x, w, b, LE.EPS, W, bias)
    f = _forward(c, with_res=False)
    assert _same(nq.detach(), f.y[:M])
    nq.backward(_d(c.dy))                                        # the head unused: the LayerNorm backward alone, on dy
    g = _backward('bwd', c.x, _np(f.stats, M), c.gamma, (c.dy,))
    assert _same(x.grad, g.dx[:M]) and _same(w.grad, g.dgamma[:C]) and _same(b.grad, g.dbeta[:C])
    assert y.shape == (M, N)
