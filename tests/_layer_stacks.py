"""Sparse layer STACKS checked layer by layer on the product's own tensors: stack specifications, the brute-force levels they pass
through, a CPU evaluation of a stack in float64 / float32 (``emulate``) and the checker (``check``).  Helpers only: plain CPU tensors, no
test functions, no device use.  tests/test_layer_stacks_cpu.py checks the checker, tests/test_gpu_layer_stacks.py runs the kernels.

A stack is a list of operations over numbered tensors: tensor 0 is the stack's input, operation i produces tensor i + 1 and names the
tensor(s) it reads in ``src``.  A RUN of a stack (the product's, recorded by hooks, or ``emulate``'s) is
    dict(records=[...], grads={tensor number: gradient that reached it}, x0=input features)
with one record per executed operation: dict(kind, src, x=[input features], y, level=(B, shape, coords) of y, params={name: value},
pgrads={name: gradient}, and for a norm rm0 / rv0 / rm1 / rv1 (running statistics before and after), relu, training, scale / shift
(eval mode: the module's own ``eval_affine()`` rows); for a prune its ``keep`` mask).  ``grads[i + 1]`` is dy of record i and, at the
same time, the dx of the operation(s) that read tensor i + 1: a tensor read by two operations holds the sum of their dx.

``check`` takes each record's OWN input as the run produced it, evaluates that one operation in float64 and holds y, dx and the parameter
gradients to the bound the project derived for that operation kind (nothing new is derived here):
  convolutions   pair-list sum over the brute-force pairs (``_sparse_sets.brute_on``), L from the same expression on ones, S from it on
                 absolute values, ``_conv_geometry.bound`` / ``excess``; gradients by autograd on the same expression.  A bias is one more
                 fp32 rounding of a value bounded by S + |b|; its gradient ``_conv_transpose.bias_grad_reference``.  A row without pairs
                 is exactly the bias (or zero), an offset without pairs has an exactly zero dW slice (its bound is zero).
  pools          ``_sparse_pool.max_forward`` (bit for bit) / ``max_backward`` / ``avg_forward`` / ``avg_backward``.
  batch norm     training: ``_bn_edges.stats_ref`` / ``y_ref`` / ``bwd_ref`` with the ReLU decisions of the run's own y > 0, running
                 statistics included; eval: y within u (|x s| + |y|) of x s + shift on the module's own fp32 rows (one multiply and one
                 add; a fused multiply-add lies inside), dx by ``_bn_edges.eval_bwd_ref``, dgamma / dbeta by ``bwd_ref``'s sums on the
                 running statistics.
  bare ReLU      y == relu(x), dx == where(x > 0, dy, 0), exactly.
  sparse_add, prune   ``_sparse_sets.join_reference`` / ``take_reference`` / ``prune_reference``, bit for bit.
and the chain: the features an operation received are bit-equal to what its producer returned; its output level equals the level the
brute-force geometry tracks (indices int32 in canonical order, spatial_shape, batch_size); every tensor and every parameter received a
gradient.  Because every link is checked the stack is checked, no error compounds and no ReLU or max-pool decision can differ between
the two sides."""
from types import SimpleNamespace

import numpy as np
import torch

import _bn_edges as BE
import _conv_geometry as cg
import _conv_transpose as T
import _sparse_pool as SP
import _sparse_sets as SS

U = 2.0 ** -24
EPS, MOM = 1e-4, 0.1
CONV_KINDS = ('subm', 'conv', 'inv', 'convt')
OPERANDS = {'bf16x3': 'fp32', 'mfma': 'fp32', 'bf16': 'bf16', 'bf16-rows': 'bf16'}


# ---------------------------------------------------------------------------------------------------------------- stacks
def _linear(*ops):
    """operations that each read the tensor before them"""
    return [dict(o, src=[i]) for i, o in enumerate(ops)]


def _conv(kind, cin, cout, k=3, s=1, p=0, d=1, q=0, key=None, bias=False, of=None):
    return dict(kind=kind, cin=cin, cout=cout, k=k, s=s, p=p, d=d, q=q, key=key, bias=bias, of=of)


def _bn(C, relu):
    return dict(kind='bn', C=C, relu=relu)


STACKS = {
    # encoder and decoder
    'E': _linear(_conv('subm', 32, 32, key='s0'), _bn(32, True), _conv('conv', 32, 64, 3, 2, 1, key='d'), _bn(64, True),
                 _conv('subm', 64, 64, d=2, key='s1'), dict(kind='relu'), _conv('inv', 64, 32, key='d', bias=True, of=2), _bn(32, False)),
    # growth and pools
    'P': _linear(_conv('conv', 32, 32, 3, 1, 1), dict(kind='relu'), dict(kind='maxpool', k=2, s=2, p=0, d=1, key='p'),
                 _conv('subm', 32, 32, k=(1, 3, 3)), dict(kind='avgpool', k=3, s=2, p=1, d=1, key=None), _bn(32, True)),
    # up-sampling and sets: tensor 0 is read by operations 0 and 5; both branches are pruned, by masks that each keep cells the other
    # drops, so the union (operation 7) is a NEW voxel set; the second 's0' layer (operation 8) runs on it
    'T': [dict(_conv('conv', 32, 64, 2, 2, 0, key='d'), src=[0]), dict(_bn(64, True), src=[1]),
          dict(_conv('convt', 64, 32, 3, 2, 1, 1, 1, key='u', bias=True), src=[2]), dict(kind='relu', src=[3]), dict(kind='prune', r=1, src=[4]),
          dict(_conv('subm', 32, 32, key='s0'), src=[0]), dict(kind='prune', r=0, src=[6]), dict(kind='add', src=[5, 7]),
          dict(_conv('subm', 32, 32, key='s0'), src=[8]), dict(_bn(32, True), src=[9])],
    # the same without the prune of the up-sampled branch: that branch then covers every voxel of the other, the union IS its level, and
    # ``sparse_add`` keeps its ``indice_dict`` -- the one tensor 0 filled.  The second 's0' layer meets the rulebook of ANOTHER level there:
    # the product must refuse it (tests/test_gpu_layer_stacks.py)
    'T0': [dict(_conv('conv', 32, 64, 2, 2, 0, key='d'), src=[0]), dict(_bn(64, True), src=[1]),
           dict(_conv('convt', 64, 32, 3, 2, 1, 1, 1, key='u', bias=True), src=[2]), dict(kind='relu', src=[3]),
           dict(_conv('subm', 32, 32, key='s0'), src=[0]), dict(kind='prune', r=0, src=[5]), dict(kind='add', src=[4, 6]),
           dict(_conv('subm', 32, 32, key='s0'), src=[7]), dict(_bn(32, True), src=[8])],
    # an empty middle level
    'Z': _linear(_conv('subm', 32, 32), _conv('conv', 32, 64, 3, 2, 0, key='d'), _bn(64, False), dict(kind='relu'),
                 _conv('inv', 64, 32, key='d', bias=True, of=1), _bn(32, False)),
}
TWO_VOXELS = ('two_voxels_no_tap', 2, (8, 8, 8), torch.tensor([[0, 7, 7, 7], [1, 7, 0, 0]], dtype=torch.int32))
SCENES = {'E': ['block5_odd_extent', 'empty_middle_scene', 'line_x_65'], 'P': ['empty_middle_scene', 'block_odd_mixed_extent', 'single_voxel'],
          'T': ['two_scenes_same_coords', 'empty_middle_scene'], 'T0': ['two_scenes_same_coords', 'empty_middle_scene'], 'Z': [TWO_VOXELS[0]]}
# rows of the levels a stack passes through, in order: what the scenes were chosen for (checked in test_layer_stacks_cpu.py)
ROWS = {('E', 'block5_odd_extent'): (250, 54), ('E', 'empty_middle_scene'): (39, 35), ('E', 'line_x_65'): (65, 132),
        ('P', 'empty_middle_scene'): (39, 205, 45, 16), ('P', 'block_odd_mixed_extent'): (64, 150, 12, 4), ('P', 'single_voxel'): (1, 27, 8, 4),
        ('Z', TWO_VOXELS[0]): (2, 0)}


def scene(name):
    return TWO_VOXELS if name == TWO_VOXELS[0] else SS.scene(name)


def prune_mask(coords, r=0):
    """a mask of stack T, from the coordinates alone: the voxels with (x + y + z) % 3 != r"""
    return coords[:, 1:].long().sum(1) % 3 != r


def consumers(ops):
    """tensor number -> the operations that read it"""
    out = {}
    for i, o in enumerate(ops):
        for t in o['src']:
            out.setdefault(t, []).append(i)
    return out


# ---------------------------------------------------------------------------------------------------------------- levels
_GEO = {}


def _lists(pairs, src_first):
    """per offset (source rows, destination rows) as long tensors"""
    out = []
    for a, b in pairs:
        s, d = (a, b) if src_first else (b, a)
        out.append((torch.as_tensor(np.asarray(s), dtype=torch.long), torch.as_tensor(np.asarray(d), dtype=torch.long)))
    return out


def geometry(stack, name):
    """[(B, shape, coords)] of every tensor and, per operation, a namespace of what its reference needs: n_src, n_dst, ``pairs`` (source
    rows, destination rows per offset) for the convolutions; ``sp`` (the (in_rows, out_rows) lists of ``_sparse_pool``) for the pools;
    keep for the prune; rows_a / rows_b / into_a / into_b for the add.  Brute force, computed once per (stack, scene)."""
    if (stack, name) in _GEO:
        return _GEO[stack, name]
    ops = STACKS[stack]
    _, B, shape, coords = scene(name)
    lv, geo = [(B, tuple(shape), coords)], []
    for o in ops:
        b, sh, c = lv[o['src'][0]]
        g = SimpleNamespace()
        kind = o['kind']
        if kind in ('subm', 'conv', 'maxpool', 'avgpool'):
            oc, osh, pairs = SS.brute_on('conv', (o['k'], o['s'], o['p'], o['d'], kind == 'subm'), b, sh, c)
            g.n_src, g.n_dst, g.pairs, g.sp = len(c), len(oc), _lists(pairs, True), pairs
            lv.append((b, tuple(osh), oc))
        elif kind == 'convt':
            oc, osh, pairs = SS.brute_on('convt', (o['k'], o['s'], o['p'], o['q'], o['d']), b, sh, c)
            g.n_src, g.n_dst, g.pairs = len(c), len(oc), _lists(pairs, False)           # kept as (new-level rows, input rows)
            lv.append((b, tuple(osh), oc))
        elif kind == 'inv':
            f, fo = geo[o['of']], ops[o['of']]
            back = lv[fo['src'][0]]
            assert torch.equal(lv[o['of'] + 1][2], c), 'the inverse layer must read the level its strided layer produced'
            g.n_src, g.n_dst, g.pairs = f.n_dst, f.n_src, [(d, s) for s, d in f.pairs]
            lv.append(back)
        elif kind == 'prune':
            g.keep = prune_mask(c, o['r'])
            lv.append((b, sh, c[g.keep].contiguous()))
        elif kind == 'add':
            cb = lv[o['src'][1]][2]
            u, g.rows_a, g.rows_b, g.into_a, g.into_b = SS.union_reference(c, cb)
            lv.append((b, sh, u))
        else:
            lv.append((b, sh, c))
        geo.append(g)
    _GEO[stack, name] = (lv, geo)
    return _GEO[stack, name]


# ---------------------------------------------------------------------------------------------------------------- parameters and inputs
def _kernel(o):
    return (o['k'],) * 3 if isinstance(o['k'], int) else tuple(o['k'])


def params(stack):
    """fp32 parameters of every operation from one fixed generator: weights 0.1 randn, gamma rand + 0.5, beta 0.1 randn, and running
    statistics that are not the module's defaults (mean 0.1 randn, variance rand + 0.5)"""
    g = torch.Generator().manual_seed(7000 + sorted(STACKS).index(stack))
    out = []
    for o in STACKS[stack]:
        p = {}
        if o['kind'] in CONV_KINDS:
            p['w'] = 0.1 * torch.randn(o['cout'], *_kernel(o), o['cin'], generator=g)
            if o['bias']:
                p['b'] = 0.1 * torch.randn(o['cout'], generator=g)
        elif o['kind'] == 'bn':
            C = o['C']
            p = dict(gamma=torch.rand(C, generator=g) + 0.5, beta=0.1 * torch.randn(C, generator=g), rm0=0.1 * torch.randn(C, generator=g),
                     rv0=torch.rand(C, generator=g) + 0.5)
        out.append(p)
    return out


def inputs(stack, name, seed=0):
    """(x0 fp32 [n, 32], dy fp32 of the stack's result)"""
    lv, _ = geometry(stack, name)
    g = torch.Generator().manual_seed(9000 + 100 * sorted(STACKS).index(stack) + SCENES[stack].index(name) + 1000 * seed)
    last = STACKS[stack][-1]
    return torch.randn(len(lv[0][2]), 32, generator=g), torch.randn(len(lv[-1][2]), last.get('C', last.get('cout')), generator=g)


# ---------------------------------------------------------------------------------------------------------------- one operation, differentiable
def conv_expr(x, w, g, pairs=None):
    """sum over the pairs of W[:, t, :] x[source row] into the destination rows (no bias)"""
    wk = w.reshape(w.shape[0], -1, w.shape[-1])
    y = torch.zeros(g.n_dst, w.shape[0], dtype=x.dtype)
    for t, (s, d) in enumerate(g.pairs if pairs is None else pairs):
        if len(s):
            y = y.index_add(0, d, x[s] @ wk[:, t, :].t())
    return y


def _window(x, g, fill):
    """[n_out, K, C] values of every window (``fill`` at absent cells) and the [n_out, K] presence mask"""
    tab = SP.table(g.sp, g.n_dst, 'out').long()
    have = tab >= 0
    v = x[tab.clamp(min=0)]
    return torch.where(have[:, :, None], v, torch.full((), fill, dtype=x.dtype)), have


def pool_expr(x, g, mode):
    if not g.n_dst:
        return x.new_zeros(0, x.shape[1]) + 0.0 * x.sum()
    if mode == 'maxpool':
        return _window(x, g, float('-inf'))[0].max(1)[0]
    v, have = _window(x, g, 0.0)
    return v.sum(1) / have.sum(1, keepdim=True).to(x.dtype)


def join_expr(a, b, g):
    pa, pb = (g.rows_a >= 0)[:, None], (g.rows_b >= 0)[:, None]
    ga = a[g.rows_a.clamp(min=0).long()] if len(a) else a.new_zeros(len(pa), a.shape[1])
    gb = b[g.rows_b.clamp(min=0).long()] if len(b) else b.new_zeros(len(pb), b.shape[1])
    return torch.where(pa & pb, ga + gb, torch.where(pa, ga, gb))


def bn_expr(x, gamma, beta, relu):
    """training-mode batch norm (+ ReLU), differentiable; -> (y, pre-activation, mean, biased variance)"""
    m = x.mean(0)
    var = ((x - m) ** 2).mean(0)
    pre = (x - m) / torch.sqrt(var + EPS) * gamma + beta
    return (torch.relu(pre) if relu else pre), pre, m, var


def _vjp(y, ins, dy):
    if not y.requires_grad:                     # no pair reaches any input (an empty level): the result does not depend on them
        return [torch.zeros_like(t) for t in ins]
    gs = torch.autograd.grad(y, ins, dy, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for t, g in zip(ins, gs)]


def _bn_case(x, dy, p):
    f = lambda t: t.detach().float().numpy()
    return SimpleNamespace(n=x.shape[0], C=x.shape[1], x=f(x), dy=None if dy is None else f(dy), gamma=f(p['gamma']), beta=f(p['beta']),
                           rm0=f(p['rm0']), rv0=f(p['rv0']))


def eval_rows(p):
    """(scale, shift, invstd) by the fp32 torch expressions of ``SparseBatchNorm._eval_rows``"""
    istd = torch.rsqrt(p['rv0'] + EPS)
    scale = p['gamma'] * istd
    return scale, p['beta'] - p['rm0'] * scale, istd


# ---------------------------------------------------------------------------------------------------------------- a stack on the CPU
def emulate(stack, name, dtype=torch.float32, training=True, fault=None, prm=None, x0=None, dy=None):
    """The stack evaluated on the CPU in ``dtype`` with the same pair-list sums, as a run.  float32: what an fp32 implementation gives
    (batch norm through ``_bn_edges.emulate_forward`` / ``emulate_backward``, the restatement of the kernels; bias gradient with fp64
    accumulation); float64: the chained float64 references.  ``fault`` = (name, operation) plants a bug:
      'reuse_pairs'   a convolution run over the pairs of the FIRST layer with its indice_key (the level that key was built for)
      'relu_no_grad'  a bare ReLU whose input gets no gradient
      'row_dropped'   norm statistics with the last row left out
      'bias_lonely'   the bias missing on the rows without pairs"""
    ops = STACKS[stack]
    lv, geo = geometry(stack, name)
    prm = params(stack) if prm is None else prm
    x0d, dyd = inputs(stack, name)
    x0, dy = (x0d if x0 is None else x0).to(dtype), (dyd if dy is None else dy).to(dtype)
    f32 = dtype == torch.float32
    bad = lambda what, i: fault is not None and fault == (what, i)
    tens, recs, back = [x0], [], []
    for i, o in enumerate(ops):
        kind, g = o['kind'], geo[i]
        p = {k: v.to(dtype) for k, v in prm[i].items()}
        xs = [tens[t] for t in o['src']]
        rec = dict(kind=kind, src=list(o['src']), x=xs, level=lv[i + 1], params={k: p[k] for k in ('w', 'b', 'gamma', 'beta') if k in p}, pgrads={})
        if kind in CONV_KINDS:
            pairs = None
            if bad('reuse_pairs', i):
                first = next(j for j, q in enumerate(ops) if q['kind'] == kind and q['key'] == o['key'])
                pairs = [(s[(s < g.n_src) & (d < g.n_dst)], d[(s < g.n_src) & (d < g.n_dst)]) for s, d in geo[first].pairs]
            lonely = conv_expr(torch.ones(g.n_src, 1, dtype=dtype), torch.ones(1, len(g.pairs), 1, dtype=dtype), g)[:, :1] == 0

            def f(x, w, b=None, i=i, g=g, pairs=pairs, lonely=lonely):
                y = conv_expr(x, w, g, pairs)
                if b is None:
                    return y
                return y + (torch.where(lonely, torch.zeros((), dtype=dtype), b[None, :]) if bad('bias_lonely', i) else b)
            ins = [xs[0], p['w']] + ([p['b']] if 'b' in p else [])

            def bw(dy, f=f, ins=ins):
                ins = [t.detach().requires_grad_() for t in ins]
                gs = _vjp(f(*ins), ins, dy)
                out = dict(w=gs[1])
                if len(ins) == 3:
                    out['b'] = dy.double().sum(0).to(dtype)
                return [gs[0]], out
            y = f(*ins)
        elif kind in ('maxpool', 'avgpool'):
            def bw(dy, x=xs[0], g=g, kind=kind):
                x = x.detach().requires_grad_()
                return _vjp(pool_expr(x, g, kind), [x], dy), {}
            y = pool_expr(xs[0], g, kind)
        elif kind == 'relu':
            def bw(dy, x=xs[0], i=i):
                return [None if bad('relu_no_grad', i) else torch.where(x > 0, dy, torch.zeros((), dtype=dtype))], {}
            y = torch.where(xs[0] > 0, xs[0], torch.zeros((), dtype=dtype))
        elif kind == 'prune':
            rec['keep'] = g.keep

            def bw(dy, x=xs[0], g=g):
                return [SS.prune_reference(x, g.keep, dy)[1]], {}
            y = xs[0][g.keep]
        elif kind == 'add':
            def bw(dy, g=g):
                return [SS.take_reference(dy, g.into_a), SS.take_reference(dy, g.into_b)], {}
            y = join_expr(xs[0], xs[1], g)
        else:
            y, bw = _emulate_bn(rec, o, p, xs[0], dtype, training, bad('row_dropped', i))
        rec['y'] = y.detach()
        tens.append(rec['y'])
        recs.append(rec)
        back.append(bw)
    grads = {len(ops): dy}
    for i in reversed(range(len(ops))):
        if i + 1 not in grads:
            continue
        dxs, recs[i]['pgrads'] = back[i](grads[i + 1])
        for t, dx in zip(ops[i]['src'], dxs):
            if dx is not None:
                grads[t] = dx if t not in grads else grads[t] + dx
    return dict(records=recs, grads=grads, x0=x0)


def _emulate_bn(rec, o, p, x, dtype, training, drop_row):
    relu, n = o['relu'], x.shape[0]
    rec.update(relu=relu, training=training, rm0=p['rm0'], rv0=p['rv0'], rm1=p['rm0'], rv1=p['rv0'])
    zeros = lambda: dict(gamma=torch.zeros_like(p['gamma']), beta=torch.zeros_like(p['beta']))
    if not training:
        scale, shift, istd = eval_rows(p)
        rec.update(scale=scale, shift=shift)
        pre = x * scale + shift
        y = torch.relu(pre) if relu else pre

        def bw(dy):
            g = torch.where(y > 0, dy, torch.zeros((), dtype=dtype)) if relu else dy
            xh = (x - p['rm0']) * istd
            return [scale * g], dict(gamma=(g.double() * xh.double()).sum(0).to(dtype), beta=g.double().sum(0).to(dtype))
        return y, bw
    if not n:
        return x, lambda dy: ([torch.zeros_like(x)], zeros())
    if dtype == torch.float32:
        c = _bn_case(x, None, p)
        fw = BE.emulate_forward(c, relu, False, 'row_dropped' if drop_row else None)
        rec.update(rm1=torch.from_numpy(fw.rm), rv1=torch.from_numpy(fw.rv))

        def bw(dy):
            c.dy = dy.numpy()
            b = BE.emulate_backward(c, fw, relu, False, False)
            return [torch.from_numpy(b.dx)], dict(gamma=torch.from_numpy(b.dgamma), beta=torch.from_numpy(b.dbeta))
        return torch.from_numpy(np.ascontiguousarray(fw.y)), bw
    y, _, m, var = bn_expr(x, p['gamma'], p['beta'], relu)
    rec.update(rm1=(1 - MOM) * p['rm0'] + MOM * m, rv1=(1 - MOM) * p['rv0'] + MOM * var * (n / (n - 1) if n > 1 else 1.0))

    def bw(dy):
        ins = [t.detach().requires_grad_() for t in (x, p['gamma'], p['beta'])]
        gs = _vjp(bn_expr(*ins, relu)[0], ins, dy)
        return [gs[0]], dict(gamma=gs[1], beta=gs[2])
    return y, bw


# ---------------------------------------------------------------------------------------------------------------- the checker
def _d(t):
    return torch.as_tensor(t).detach().double().cpu()


def _np64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _conv_reference(o, g, rec, dy, operands):
    """-> ({name: (reference, bound)} for y and, with dy, dw / db, [(dx reference, bound, None)], lonely rows)"""
    x, w = _d(rec['x'][0]).requires_grad_(), _d(rec['params']['w']).requires_grad_()
    b = _d(rec['params']['b']) if 'b' in rec['params'] else None
    one_x, one_w = torch.ones(g.n_src, 1, dtype=torch.float64, requires_grad=True), torch.ones(1, *w.shape[1:4], 1, dtype=torch.float64, requires_grad=True)
    ax, aw = x.detach().abs().requires_grad_(), w.detach().abs().requires_grad_()
    y, Ly, Sy = conv_expr(x, w, g), conv_expr(one_x, one_w, g), conv_expr(ax, aw, g)
    cin, cout = w.shape[-1], w.shape[0]
    by = cg.bound(Ly.detach() * cin, Sy.detach(), operands)
    yr = y.detach()
    if b is not None:             # one more fp32 rounding, of a value bounded by S + |b|
        yr, by = yr + b, by + U * (Sy.detach() + b.abs())
    out, dxs = dict(y=(yr, by)), [None]
    if dy is not None:
        dyd = _d(dy)
        (dx, dw), (Lx, Lw), (Sx, Sw) = _vjp(y, [x, w], dyd), _vjp(Ly, [one_x, one_w], torch.ones_like(Ly)), _vjp(Sy, [ax, aw], dyd.abs())
        dxs = [(dx, cg.bound(Lx.round() * cout, Sx, operands), None)]
        out['dw'] = (dw, cg.bound(Lw.round().expand_as(Sw), Sw, operands))
        if b is not None:
            out['db'] = T.bias_grad_reference(dy.detach().cpu())
    return out, dxs, (Ly.detach()[:, 0] == 0)


def _bn_reference(o, rec, dy):
    """-> ({name: (got, reference, bound)} in numpy, dx entry or None)"""
    p, x, y = rec['params'], rec['x'][0].detach().cpu(), rec['y'].detach().cpu()
    relu, n = rec['relu'], x.shape[0]
    f = lambda t: t.detach().cpu().float().numpy()
    c = _bn_case(x, dy, dict(p, rm0=rec['rm0'], rv0=rec['rv0']))
    mask = (f(y) > 0) if relu else None
    out, dx = {}, None
    if rec['training'] and n:
        r = BE.stats_ref(c)
        yr, yb = BE.y_ref(c, r, relu)
        out = dict(y=(f(y), yr, yb), running_mean=(f(rec['rm1']), r.rm, r.b_rm), running_var=(f(rec['rv1']), r.rv, r.b_rv))
        if dy is not None:
            b = BE.bwd_ref(c, r, mask, False)
            out.update(dgamma=(f(rec['pgrads']['gamma']), b.dgamma, b.b_dgamma), dbeta=(f(rec['pgrads']['beta']), b.dbeta, b.b_dbeta))
            dx = (_np64(b.dx), _np64(b.b_dx), None)
    elif rec['training']:          # no rows: nothing normalised, the running statistics untouched, zero gradients exact zeros
        same = lambda a, b: (f(a), f(b).astype(np.float64), np.zeros(c.C))
        out = dict(running_mean=same(rec['rm1'], rec['rm0']), running_var=same(rec['rv1'], rec['rv0']))
        if dy is not None:
            out.update(dgamma=(f(rec['pgrads']['gamma']), np.zeros(c.C), np.zeros(c.C)), dbeta=(f(rec['pgrads']['beta']), np.zeros(c.C), np.zeros(c.C)))
            dx = (torch.zeros(0, c.C, dtype=torch.float64),) * 2 + (None,)
    else:
        s, sh = f(rec['scale']).astype(np.float64), f(rec['shift']).astype(np.float64)
        xs = c.x.astype(np.float64) * s
        yr = np.maximum(xs + sh, 0.0) if relu else xs + sh
        out = dict(y=(f(y), yr, U * (np.abs(xs) + np.abs(yr))), running_mean=(f(rec['rm1']), c.rm0.astype(np.float64), np.zeros(c.C)),
                   running_var=(f(rec['rv1']), c.rv0.astype(np.float64), np.zeros(c.C)))
        if dy is not None and n:
            dxr, dxb = BE.eval_bwd_ref(f(rec['scale']), c.dy, mask, None)
            dx = (_np64(dxr), _np64(dxb), None)
            istd = 1.0 / np.sqrt(c.rv0.astype(np.float64) + BE.EPS)
            r = SimpleNamespace(m=c.rm0.astype(np.float64), istd=istd, s=c.gamma.astype(np.float64) * istd, dm64=0.0, rvar=0.0)
            b = BE.bwd_ref(c, r, mask, False)
            out.update(dgamma=(f(rec['pgrads']['gamma']), b.dgamma, b.b_dgamma), dbeta=(f(rec['pgrads']['beta']), b.dbeta, b.b_dbeta))
    return out, dx


def check(stack, name, run, operands='fp32'):
    """-> (ratios {'<kind>.<quantity>': largest err / bound}, failures [text]).  A run passes when ``failures`` is empty."""
    ops = STACKS[stack]
    lv, geo = geometry(stack, name)
    recs, grads = run['records'], run['grads']
    ratios, fails, shared = {}, [], {}
    readers = consumers(ops)

    def ratio(i, what, r):
        key = f"{ops[i]['kind']}.{what}"
        ratios[key] = max(ratios.get(key, 0.0), r)
        if not r <= 1.0:
            fails.append(f"record {i} ({ops[i]['kind']}): bound: {what} err / bound = {r:.3g}")

    def exact(i, what, got, ref):
        ok = got is not None and SS.same(got, ref)
        ratio(i, what, 0.0 if ok else float('inf'))

    if len(recs) != len(ops):
        return ratios, [f'{len(recs)} records for {len(ops)} operations']
    for t in range(len(ops) + 1):
        if grads.get(t) is None:
            fails.append(f'no gradient: tensor {t} ' + ('(the stack input)' if t == 0 else f"(output of record {t - 1}, {ops[t - 1]['kind']})") + ' received none')
    for i, (o, g, rec) in enumerate(zip(ops, geo, recs)):
        kind = o['kind']
        if rec['kind'] != kind or list(rec['src']) != list(o['src']):
            fails.append(f"record {i}: is {rec['kind']} of {rec['src']}, the stack has {kind} of {o['src']}")
            continue
        # ---- the chain: what the operation received is what its producer returned; its level is the tracked level
        for j, t in enumerate(o['src']):
            prev = run['x0'] if t == 0 else recs[t - 1]['y']
            if not SS.same(rec['x'][j], prev):
                fails.append(f'record {i} ({kind}): chain: input {j} is not bit-equal to tensor {t} as it was produced')
        B, shape, coords = rec['level']
        rB, rshape, rcoords = lv[i + 1]
        c = torch.as_tensor(coords).detach().cpu()
        if int(B) != rB or [int(s) for s in shape] != list(rshape) or c.dtype != torch.int32 or c.shape != rcoords.shape or not torch.equal(c, rcoords):
            fails.append(f'record {i} ({kind}): level: indices / spatial_shape / batch_size differ from the tracked level '
                         f'({tuple(c.shape)} rows in {list(shape)} x {B}, tracked {tuple(rcoords.shape)} in {list(rshape)} x {rB})')
            continue
        y, x = rec['y'].detach().cpu(), [t.detach().cpu() for t in rec['x']]
        if y.shape[0] != len(rcoords) or y.dtype != torch.float32:
            fails.append(f'record {i} ({kind}): level: {tuple(y.shape)} {y.dtype} features on a level of {len(rcoords)} rows')
            continue
        dy = grads.get(i + 1)
        dy = None if dy is None else dy.detach().cpu()
        missing = [k for k in rec['params'] if rec['pgrads'].get(k) is None]
        for pname in missing:
            fails.append(f'record {i} ({kind}): no gradient: parameter {pname} has none')
        dy_params = None if missing else dy     # the parameter checks need every gradient
        dxs = [None] * len(o['src'])
        if kind in CONV_KINDS:
            out, dxs, lonely = _conv_reference(o, g, rec, dy_params, operands)
            got = dict(y=y, dw=rec['pgrads'].get('w'), db=rec['pgrads'].get('b'))
            for q, (ref, bnd) in out.items():
                ratio(i, q, cg.excess(got[q].reshape(ref.shape), ref, bnd))
            if bool(lonely.any()):          # a row without pairs: exactly the bias (or +-0)
                want = rec['params']['b'].detach().cpu().expand(int(lonely.sum()), -1) if 'b' in rec['params'] else torch.zeros(int(lonely.sum()), y.shape[1])
                ratio(i, 'y_without_pairs', 0.0 if torch.equal(y[lonely], want) else float('inf'))
            if dy is not None and dy_params is None:
                dxs = _conv_reference(o, g, dict(rec, pgrads={}), dy, operands)[1]
        elif kind == 'bn':
            out, dx = _bn_reference(o, rec, dy_params)
            for q, (got, ref, bnd) in out.items():
                ratio(i, q, BE.margin(got, ref, bnd))
            dxs = [dx]
        elif kind == 'maxpool':
            yr, arg = SP.max_forward(x[0], g.sp, g.n_dst)
            exact(i, 'y', y, yr)
            if dy is not None:
                dxs = [SP.max_backward(dy, arg, g.sp, g.n_src) + (None,)]
        elif kind == 'avgpool':
            yr, _, yb = SP.avg_forward(x[0], g.sp, g.n_dst)
            ratio(i, 'y', SP.excess(y, yr, yb))
            if dy is not None:
                dxs = [SP.avg_backward(dy, g.sp, g.n_src, g.n_dst) + (None,)]
        elif kind == 'relu':
            ok = bool(torch.isfinite(x[0]).all()) and torch.equal(y, torch.relu(x[0]))
            ratio(i, 'y', 0.0 if ok else float('inf'))
            if dy is not None:
                r = torch.where(x[0] > 0, dy, torch.zeros(()))
                dxs = [(r.double(), torch.zeros_like(r, dtype=torch.float64), r)]
        elif kind == 'prune':
            keep = torch.as_tensor(rec['keep']).cpu()
            if not torch.equal(keep, g.keep):
                fails.append(f'record {i} (prune): the mask differs from the one the coordinates give')
                continue
            yr, dxr = SS.prune_reference(x[0], keep, dy)
            exact(i, 'y', y, yr)
            if dy is not None:
                dxs = [(dxr.double(), torch.zeros_like(dxr, dtype=torch.float64), dxr)]
        elif kind == 'add':
            exact(i, 'y', y, SS.join_reference(x[0], g.rows_a, x[1], g.rows_b))
            if dy is not None:
                rs = [SS.take_reference(dy, g.into_a), SS.take_reference(dy, g.into_b)]
                dxs = [(r.double(), torch.zeros_like(r, dtype=torch.float64), r) for r in rs]
        # ---- dx: against the gradient that reached the input tensor; a tensor with several readers holds their sum
        for t, e in zip(o['src'], dxs):
            if e is None or grads.get(t) is None:
                continue
            if len(readers[t]) > 1:
                shared.setdefault(t, []).append((i, e))
            elif e[2] is not None:
                exact(i, 'dx', grads[t], e[2])
            else:
                ratio(i, 'dx', cg.excess(grads[t], e[0], e[1]))
    for t, parts in shared.items():
        if len(parts) != len(readers[t]):
            continue                            # a reader without dy: reported as a missing gradient
        ref = sum(e[0] for _, e in parts)
        bnd = sum(e[1] for _, e in parts) + (len(parts) - 1) * U * ref.abs()
        r = cg.excess(grads[t], ref, bnd)
        ratios['shared.dx'] = max(ratios.get('shared.dx', 0.0), r)
        if not r <= 1.0:
            fails.append(f'tensor {t}, read by records {[i for i, _ in parts]}: bound: summed dx err / bound = {r:.3g}')
    return ratios, fails
