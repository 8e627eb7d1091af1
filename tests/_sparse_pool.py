"""Sparse max / average pooling over a convolution rulebook: scenes, value kinds, the float64 references written from the brute-force pair
lists of tests/_conv_general.py by the definition in include/u3d.h (section P1), and the rounding bounds.  Helpers only: plain CPU
tensors, no test functions, no device use.  tests/test_sparse_pool_cpu.py checks the checker against torch's dense pooling,
tests/test_gpu_sparse_pool.py runs the kernels.

Definition.  Window of output row j = its pairs (i_k, j) over the offsets k, ascending.  Max: walk the window, take the first value,
replace the held one only by a value > it or by a NaN while it is none; y has the bits of the selected element, arg its offset.  Max
backward: dx[i, c] = sum over k ascending of dy[j_k, c] where arg[j_k, c] == k.  Average: y = (sum of the window) / count_j; backward
dx[i, c] = sum over k of dy[j_k, c] / count_{j_k}.

Bounds, with u = 2^-24, m the number of terms of an element, gamma_n = n u / (1 - n u): max forward and arg bit-equal; max backward
gamma_(m-1) sum|terms| (m - 1 additions; zero, i.e. bit-equal, where windows do not overlap); average forward and backward gamma_(m+2)
sum|terms| with the terms taken after their division in float64 (m - 1 additions, and per term a reciprocal and a product, or one
division of the sum).  Non-finite value kinds are for the maximum (a selection); the average is checked on the finite ones."""
import numpy as np
import torch

import _conv_general as G

U = 2.0 ** -24
CONFIGS = [c for c, v in G.CONFIGS.items() if not v[4]]                   # the strided layers: a pool moves to a new level
LARGE = 'two_grids_24_fill10'                                             # more rows than one workgroup serves at any width
SCENES = list(G.SCENES) + [LARGE]
FINITE_KINDS = ['normal', 'negative', 'ties', 'zeros']
KINDS = FINITE_KINDS + ['inf', 'nan_row']
NAN_CHANNELS = lambda C: [c for c in range(C) if c % 3 == 1]              # the channels of the NaN row that hold a NaN

_LARGE = None


def scene(name):
    """(name, B, shape, coords int32 [n, 4] canonical)"""
    global _LARGE
    if name != LARGE:
        return G.scene(name)
    if _LARGE is None:
        rng = np.random.RandomState(24)
        cells = np.argwhere(rng.rand(2, 24, 24, 24) < 0.10)                # argwhere is row-major: canonical order
        _LARGE = (LARGE, 2, (24, 24, 24), torch.tensor(np.ascontiguousarray(cells), dtype=torch.int32).contiguous())
    return _LARGE


def brute(cfg, name):
    """``_conv_general.brute`` (out_coords, out_shape, K x (in_rows, out_rows)), on this module's scenes"""
    if name != LARGE:
        return G.brute(cfg, name)
    orig, G.scene = G.scene, scene                  # brute reads its scene through the module global
    try:
        return G.brute(cfg, name)
    finally:
        G.scene = orig


def overlapping(cfg):
    """windows overlap on some axis: stride < dilation (kernel - 1) + 1"""
    k, s, p, d, _ = G.geom(cfg)
    return any(s[a] < d[a] * (k[a] - 1) + 1 for a in range(3))


def values(kind, n, C, seed):
    """float32 [n, C] of one value kind"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g)
    if kind == 'negative':
        x = -(x.abs() + 0.5)
    elif kind == 'ties':
        x = torch.randint(-1, 2, (n, C), generator=g).float()
    elif kind == 'zeros':
        x = torch.where(torch.rand(n, C, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    elif kind == 'inf':
        r = torch.rand(n, C, generator=g)
        x = torch.where(r < 0.08, torch.tensor(float('inf')), torch.where(r < 0.16, torch.tensor(float('-inf')), x))
    elif kind == 'nan_row' and n:
        x[nan_row(n), NAN_CHANNELS(C)] = float('nan')
    else:
        assert kind in ('normal', 'nan_row'), kind
    return x


def nan_row(n):
    return n // 2


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64).clamp(min=0)
    return n * U / (1 - n * U)


def _lt(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long)


def table(pairs, n, role):
    """the destination-major table int32 [n, K] of the pair lists: role 'out' -> each output row's inputs, 'in' -> each input row's outputs"""
    t = torch.full((n, len(pairs)), -1, dtype=torch.int32)
    for k, (pi, po) in enumerate(pairs):
        key, val = (po, pi) if role == 'out' else (pi, po)
        t[_lt(key), k] = torch.as_tensor(np.asarray(val), dtype=torch.int32)
    return t


def pair_count(pairs, n_out):
    c = torch.zeros(n_out, dtype=torch.int32)
    for _, po in pairs:
        c[_lt(po)] += 1                             # (no row repeats inside an offset)
    return c


def max_forward(x, pairs, n_out):
    """y float32 [n_out, C] (the selected elements, bit for bit) and arg uint8 [n_out, C]"""
    C = x.shape[1]
    y, arg = torch.zeros(n_out, C, dtype=torch.float32), torch.zeros(n_out, C, dtype=torch.uint8)
    have = torch.zeros(n_out, dtype=torch.bool)
    for k, (pi, po) in enumerate(pairs):
        if not len(pi):
            continue
        pi, po = _lt(pi), _lt(po)
        v, h = x[pi], y[po]
        rep = ~have[po][:, None] | (v > h) | (torch.isnan(v) & ~torch.isnan(h))
        y[po] = torch.where(rep, v, h)
        arg[po] = torch.where(rep, torch.tensor(k, dtype=torch.uint8), arg[po])
        have[po] = True
    assert bool(have.all()), 'an output row without a pair'
    return y, arg


def max_backward(dy, arg, pairs, n_in):
    """(dx float64 [n_in, C], bound): the first term as it is, the others added in ascending offset order"""
    C = dy.shape[1]
    dx, S, m = [torch.zeros(n_in, C, dtype=torch.float64) for _ in range(3)]
    for k, (pi, po) in enumerate(pairs):
        if not len(pi):
            continue
        pi, po = _lt(pi), _lt(po)
        sel = arg[po] == k
        t = torch.where(sel, dy[po].double(), torch.zeros((), dtype=torch.float64))
        dx[pi] += t
        S[pi] += t.abs()
        m[pi] += sel
    return dx, gamma(m - 1) * S


def avg_forward(x, pairs, n_out):
    """(y float64 [n_out, C], count int32 [n_out], bound)"""
    cnt = pair_count(pairs, n_out)
    assert n_out == 0 or int(cnt.min()) >= 1, 'an output row without a pair'
    y, S = [torch.zeros(n_out, x.shape[1], dtype=torch.float64) for _ in range(2)]
    for pi, po in pairs:
        if len(pi):
            pi, po = _lt(pi), _lt(po)
            t = x[pi].double() / cnt[po].double()[:, None]
            y[po] += t
            S[po] += t.abs()
    return y, cnt, gamma(cnt.double()[:, None] + 2) * S


def avg_backward(dy, pairs, n_in, n_out):
    """(dx float64 [n_in, C], bound)"""
    cnt = pair_count(pairs, n_out)
    dx, S = [torch.zeros(n_in, dy.shape[1], dtype=torch.float64) for _ in range(2)]
    m = torch.zeros(n_in, dtype=torch.float64)
    for pi, po in pairs:
        if len(pi):
            pi, po = _lt(pi), _lt(po)
            t = dy[po].double() / cnt[po].double()[:, None]
            dx[pi] += t
            S[pi] += t.abs()
            m[pi] += 1
    return dx, gamma(m[:, None] + 2) * S


_CASES = {}


def case(cfg, name, kind, C):
    """inputs, references and bounds of one configuration x scene x value kind x width: computed once per process, shared, never written to.
    -> dict(x, dy, n_in, n_out, K, pairs, max=dict(y, arg, dx, dx_bound), avg=dict(y, count, y_bound, dx, dx_bound) for finite kinds)"""
    key = (cfg, name, kind, C)
    if key not in _CASES:
        coords = scene(name)[3]
        oc, _, pairs = brute(cfg, name)
        n_in, n_out = len(coords), len(oc)
        seed = ((CONFIGS.index(cfg) * 100 + SCENES.index(name)) * 10 + KINDS.index(kind)) * 1000 + C
        x, dy = values(kind, n_in, C, seed), values('normal', n_out, C, seed + 500)
        y, arg = max_forward(x, pairs, n_out)
        dx, dxb = max_backward(dy, arg, pairs, n_in)
        c = dict(x=x, dy=dy, n_in=n_in, n_out=n_out, K=len(pairs), pairs=pairs, max=dict(y=y, arg=arg, dx=dx, dx_bound=dxb))
        if kind in FINITE_KINDS:
            ya, cnt, yb = avg_forward(x, pairs, n_out)
            da, db = avg_backward(dy, pairs, n_in, n_out)
            c['avg'] = dict(y=ya, count=cnt, y_bound=yb, dx=da, dx_bound=db)
        _CASES[key] = c
    return _CASES[key]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def excess(got, ref, bnd):
    """largest err / bound over the elements (0 / 0 = 0; anything over a zero bound, or a non-finite value, = inf)"""
    got = torch.as_tensor(got).detach().double().cpu()
    assert got.shape == ref.shape == bnd.shape, (got.shape, ref.shape, bnd.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float('inf')))
    return float(torch.nan_to_num(ratio, nan=float('inf'), posinf=float('inf')).max())
