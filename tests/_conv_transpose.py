"""Sparse transposed convolution and the bias of the sparse convolution layers: configurations, a brute-force reference of the output set
and the pair lists written straight from the definition, float64 dense references, the rounding bounds, and the value kinds of the
bias-gradient tests.  Case builders and checkers only: plain CPU tensors, no test functions, no device use.
tests/test_conv_transpose_cpu.py checks the checker, tests/test_gpu_conv_transpose.py runs the kernels.

Definition, per axis: out_dim = (in_dim - 1) s - 2 p + d (k - 1) + q + 1 (torch's rule); output cell o is active iff an active input i
and a tap t in [0, k) give o = i s - p + t d on all three axes with 0 <= o < out_dim; rows in lexicographic (b, x, y, z) order; offset
index = (t0 k1 + t1) k2 + t2, the order of the weight layout [C_out, k0, k1, k2, C_in], taps not flipped.
y[o] = sum over the pairs (i, t) of W[:, t, :] x[i] = ``F.conv_transpose3d(x, W.permute(4, 0, 1, 2, 3), stride, padding, output_padding,
dilation=dilation)`` sampled at the active rows; the dense result is exactly zero at every other cell.

The pair lists are kept as ``(new-level rows, layer-input rows)`` per offset -- (pair_in, pair_out) of the ``Rulebook`` the layer runs in
mode 'inv'.  A second, independent derivation (``forward_lists``): ``_conv_general.brute`` on the forward geometry (k, s, p, d) built FROM
the output set, restricted to the layer's input rows.

Bounds.  Convolution: ``_conv_geometry.bound`` unchanged, L from the dense expression on ones, S from it on absolute values.
Bias forward: the bits of the fp32 y + b.  Bias gradient: fp64 accumulation of n terms in any fixed order, then one rounding to fp32:
|db - ref| <= 2^-24 |ref| + (1 + 2^-24) gamma64_n sum|dy|, gamma64_n = n 2^-53 / (1 - n 2^-53), plus one fp32 subnormal.  The reference
is torch's float64 column sum (blocked pairwise: its own error grows with log n, far inside the n 2^-53 term).
"""
import numpy as np
import torch
import torch.nn.functional as F

import _conv_general as cgn
import _conv_geometry as cg

# name -> (kernel, stride, padding, output_padding, dilation); ints or triples
CONFIGS = {
    'k2s2p0': (2, 2, 0, 0, 1),                                        # the U-Net's up-sampling as a true transposed layer: 8 outputs per input
    'k3s2p1q1': (3, 2, 1, 1, 1),                                      # the common decoder layer: exact doubling
    'k3s2p1q0': (3, 2, 1, 0, 1),
    'k3s2p0': (3, 2, 0, 0, 1),
    'k3s1p1': (3, 1, 1, 0, 1),
    'k3s3p1q2': (3, 3, 1, 2, 1),                                      # gaps
    'k3s2p2d2q1': (3, 2, 2, 1, 2),
    'k3s2p2': (3, 2, 2, 0, 1),                                        # padding at the reach d (k - 1): crop at both ends, a corner row keeps one tap
    'k321s121p100q010': ((3, 2, 1), (1, 2, 1), (1, 0, 0), (0, 1, 0), 1),      # K = 6
    'k122s2p0': ((1, 2, 2), 2, 0, 0, 1),                              # K = 4
    'k1s2p0q1': (1, 2, 0, 1, 1),                                      # K = 1
}
BEYOND = (3, 2, 3, 0, 1)          # padding one past the reach d (k - 1): input rows on the low faces have no pair (geometry tests only)
SCENES = cgn.SCENES
FULL_GRID_SCENES = ['line_x_65', 'block5_odd_extent', 'empty_middle_scene']
CHANNELS = [(16, 32), (32, 64), (64, 96), (160, 192)]

scene = cgn.scene


def geom(cfg):
    """(k, s, p, q, d) as triples"""
    return tuple(cgn._t3(v) for v in (CONFIGS[cfg] if isinstance(cfg, str) else cfg))


def layer_args(cfg):
    k, s, p, q, d = CONFIGS[cfg] if isinstance(cfg, str) else cfg
    return dict(kernel_size=k, stride=s, padding=p, output_padding=q, dilation=d)


def out_shape(shape, cfg):
    k, s, p, q, d = geom(cfg)
    return tuple((int(shape[a]) - 1) * s[a] - 2 * p[a] + d[a] * (k[a] - 1) + q[a] + 1 for a in range(3))


def _taps(k):
    return [(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]


_GEO = {}


def brute(cfg, name, flip=False, drop_q=False):
    """(out_coords int32 [n_out, 4] canonical, out_shape, K x (new-level rows, layer-input rows) int32) of configuration ``cfg`` on
    scene ``name``, from the definition: every (input row, tap) marks its output cell and is a pair of that tap's list.
    ``flip`` / ``drop_q``: the two sabotaged variants of the checker's own check (taps in reversed order; output padding forgotten)."""
    key = (cfg, name, flip, drop_q)
    if key in _GEO:
        return _GEO[key]
    _, B, shape, coords = scene(name)
    k, s, p, q, d = geom(cfg)
    oshape = out_shape(shape, cfg)
    if drop_q:
        oshape = tuple(oshape[a] - q[a] for a in range(3))
    rows = [tuple(int(v) for v in r) for r in coords.tolist()]
    taps = _taps(k)
    hits = []                                                        # (tap index, input row, output cell)
    for ti, t in enumerate(taps):
        for i, r in enumerate(rows):
            o = tuple(r[1 + a] * s[a] - p[a] + t[a] * d[a] for a in range(3))
            if all(0 <= o[a] < oshape[a] for a in range(3)):
                hits.append((len(taps) - 1 - ti if flip else ti, i, (r[0],) + o))
    out = sorted({h[2] for h in hits})                                # lexicographic on (b, x, y, z) == canonical
    row_of = {c: j for j, c in enumerate(out)}
    pairs = []
    for ti in range(len(taps)):
        mine = sorted((i, row_of[c]) for tj, i, c in hits if tj == ti)
        pairs.append((np.asarray([j for _, j in mine], np.int32), np.asarray([i for i, _ in mine], np.int32)))
    _GEO[key] = (torch.tensor(out, dtype=torch.int32).reshape(-1, 4), oshape, pairs)
    return _GEO[key]


def forward_lists(cfg, name):
    """The same lists by another road: ``_conv_general.brute`` of the FORWARD layer (k, s, p, d) on the output set as its input level --
    every (forward output row, tap) looks its input cell up -- restricted to the forward output cells that are rows of the transposed
    layer's input, and renumbered to those rows."""
    _, B, shape, coords = scene(name)
    k, s, p, q, d = geom(cfg)
    oc, oshape, _ = brute(cfg, name)
    fwd = (k, s, p, d, False)
    real, tag = cgn.scene, f'convt::{cfg}::{name}'
    cgn.scene = lambda n: (tag, B, oshape, oc) if n == tag else real(n)
    try:
        foc, foshape, fpairs = cgn.brute(fwd, tag)
    finally:
        cgn.scene = real
    row_of = {tuple(r): i for i, r in enumerate(coords.tolist())}
    to_row = np.asarray([row_of.get(tuple(r), -1) for r in foc.tolist()], np.int64).reshape(-1)
    out = []
    for pi, po in fpairs:                                             # (forward input = new-level rows, forward output rows)
        keep = to_row[po] >= 0 if len(po) else np.zeros(0, bool)
        out.append((pi[keep].astype(np.int32), to_row[po][keep].astype(np.int32)))
    return out


def same_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- dense references
def dense_full(x, w, cfg, name):
    """x [n, Cin] on the scene's rows, w [Cout, k0, k1, k2, Cin] -> the dense [B, Cout, X', Y', Z'] result"""
    _, B, shape, coords = scene(name)
    k, s, p, q, d = geom(cfg)
    return F.conv_transpose3d(cg._scatter(x, coords, B, shape), w.permute(4, 0, 1, 2, 3), stride=s, padding=p, output_padding=q, dilation=d)


def dense_convt(x, w, cfg, name):
    oc, oshape, _ = brute(cfg, name)
    y = dense_full(x, w, cfg, name)
    assert tuple(y.shape[2:]) == tuple(oshape), (cfg, name, y.shape, oshape)
    return cg._sample(y, oc)


def off_set_is_zero(x, w, cfg, name) -> bool:
    """the dense result is exactly zero at every cell that is not an active output row"""
    y = dense_full(x, w, cfg, name).clone()
    c = brute(cfg, name)[0].long()
    y[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = 0
    return bool((y == 0).all())


def n_rows(cfg, name):
    """(source rows, destination rows)"""
    return len(scene(name)[3]), len(brute(cfg, name)[0])


def make_inputs(cfg, name, cin, cout, seed):
    """float32 CPU inputs with a wide dynamic range, as ``_conv_general.make_inputs``, and a bias"""
    ns, nd = n_rows(cfg, name)
    g = torch.Generator().manual_seed(seed)
    k = geom(cfg)[0]

    def wide(n, c):
        return torch.randn(n, c, generator=g) * torch.exp(torch.randn(n, c, generator=g) * 2.0)
    return dict(x=wide(ns, cin), w=torch.randn(cout, *k, cin, generator=g) * 0.1, add=torch.randn(nd, cout, generator=g), go=wide(nd, cout),
                b=torch.randn(cout, generator=g))


def _run(x, w, add, go, cfg, name):
    x, w, add = [t.detach().clone().requires_grad_() for t in (x, w, add)]
    y = dense_convt(x, w, cfg, name) + add
    y.backward(go)
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(y=y.detach(), dx=zero(x), dw=zero(w), dadd=zero(add))


def reference(inp, cfg, name):
    return _run(*[inp[q].double() for q in ('x', 'w', 'add', 'go')], cfg, name)


def product_counts(cfg, name):
    ns, nd = n_rows(cfg, name)
    k = geom(cfg)[0]
    one = lambda *s: torch.ones(*s, dtype=torch.float64)
    r = _run(one(ns, 1), one(1, *k, 1), torch.zeros(nd, 1, dtype=torch.float64), one(nd, 1), cfg, name)
    return dict(y=r['y'][:, 0].round(), dx=r['dx'][:, 0].round(), dw=r['dw'].reshape(-1).round())


def magnitudes(inp, cfg, name):
    return _run(*[inp[q].double().abs() for q in ('x', 'w', 'add', 'go')], cfg, name)


_CASES = {}


def case(cfg, name, cin, cout):
    """inputs, float64 reference (db = column sums of go included), both bounds and the pair counts: computed once per process, shared and
    never written to"""
    key = (cfg, name, cin, cout)
    if key not in _CASES:
        seed = ((cin * 1000 + cout) * 100 + list(CONFIGS).index(cfg)) * 100 + SCENES.index(name) + 7
        inp = make_inputs(cfg, name, cin, cout, seed)
        cnt, S = product_counts(cfg, name), magnitudes(inp, cfg, name)
        k = geom(cfg)[0]
        Ls = dict(y=cnt['y'][:, None] * cin, dx=cnt['dx'][:, None] * cout, dw=cnt['dw'].reshape(1, *k, 1).expand_as(S['dw']), dadd=0.0)
        bnd = {o: {q: cg.bound(Ls[q], S[q], o) for q in Ls} for o in ('fp32', 'bf16')}
        _CASES[key] = dict(inp=inp, ref=reference(inp, cfg, name), bound=bnd, counts=cnt)
    return _CASES[key]


def pair_sum(inp, cfg, name, dtype=torch.float64, pairs=None):
    """y, dx, dw, dadd from pair lists (default: the brute-force ones): per-offset gather, matrix product, index_add"""
    pairs = brute(cfg, name)[2] if pairs is None else pairs
    ns, nd = n_rows(cfg, name)
    x, w, add = [inp[q].to(dtype).clone().requires_grad_() for q in ('x', 'w', 'add')]
    wk = w.reshape(w.shape[0], -1, w.shape[-1])
    y = torch.zeros(nd, w.shape[0], dtype=dtype)
    for t, (new_rows, in_rows) in enumerate(pairs):
        if len(in_rows):
            y = y.index_add(0, torch.as_tensor(new_rows, dtype=torch.long), x[torch.as_tensor(in_rows, dtype=torch.long)] @ wk[:, t, :].t())
    y = y + add
    y.backward(inp['go'].to(dtype))
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(y=y.detach(), dx=zero(x), dw=zero(w), dadd=zero(add))


# ---------------------------------------------------------------------------------------------------------------- biased layers
def layer_case(dense, inp, cin, cout):
    """A layer with a bias against float64: ``dense(x, w)`` is the differentiable dense expression of the layer without its bias
    ([n_src, cin], [cout, k.., cin] -> [n_dst, cout]).  -> (ref, bound) dicts over y, dx, dw, db.  y = fl(conv + b) is one more rounding
    of a value bounded by S + |b|: (L + 9) 2^-24 (S + |b|); dx and dW do not see the bias; db is the column sum of the output gradient
    (``bias_grad_reference``)."""
    def run(x, w, b, go):
        x, w, b = [t.detach().clone().requires_grad_() for t in (x, w, b)]
        y = dense(x, w) + b
        y.backward(go)
        zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
        return dict(y=y.detach(), dx=zero(x), dw=zero(w), db=zero(b))
    args = [inp[q].double() for q in ('x', 'w', 'b', 'go')]
    ref, S = run(*args), run(*[a.abs() for a in args])
    one = lambda *s: torch.ones(*s, dtype=torch.float64)
    cnt = run(one(len(inp['x']), 1), one(1, *inp['w'].shape[1:4], 1), torch.zeros(1, dtype=torch.float64), one(len(inp['go']), 1))
    bnd = dict(y=(cnt['y'].round() * cin + 9.0) * cg.U32 * S['y'], dx=cg.bound(cnt['dx'].round() * cout, S['dx']),
               dw=cg.bound(cnt['dw'].round().expand_as(S['dw']), S['dw']), db=bias_grad_reference(inp['go'])[1])
    return ref, bnd


# ---------------------------------------------------------------------------------------------------------------- bias gradient
BIAS_KINDS = ['normal', 'integer', 'offset_mean', 'dominant_row', 'cancelling']
BIAS_WIDTHS = [32, 96, 160, 512]


def bias_rows(rows_per_wg, step):
    """row counts of the bias tests: 1; one below / at / above the first pass's rows per workgroup; one below / at / above the point
    where the second pass needs more than one step (``step`` partials per step)"""
    edge = rows_per_wg * step
    return [1, rows_per_wg - 1, rows_per_wg, rows_per_wg + 1, edge - 1, edge, edge + 1]


def bias_values(kind, n, C, seed=0):
    """dy float32 [n, C] of one value kind"""
    g = torch.Generator().manual_seed(1000 * BIAS_KINDS.index(kind) + 7 * C + n % 997 + seed)
    if kind == 'normal':
        return torch.randn(n, C, generator=g)
    if kind == 'integer':                      # |sum| <= 8 n < 2^24 up to 65 537 rows: every partial sum is exact in fp32, db is bit-equal
        return torch.randint(-8, 9, (n, C), generator=g).float()
    if kind == 'offset_mean':                  # |mean| >> spread
        return 1000.0 + 1e-3 * torch.randn(n, C, generator=g)
    if kind == 'dominant_row':
        v = torch.randn(n, C, generator=g)
        v[n // 2] *= 1e8
        return v
    assert kind == 'cancelling'                # +a, e, -a triples: a plain fp32 running sum loses the bits of e below ulp(a) in every triple
    v = 0.5 + torch.rand(n, C, generator=g)
    a = 1e4 * (1.0 + torch.rand(n // 3, C, generator=g))
    v[0:3 * (n // 3):3] = a
    v[2:3 * (n // 3):3] = -a
    return v


def bias_grad_reference(dy):
    """(float64 column sums, the bound of the module docstring)"""
    d = dy.double()
    n = d.shape[0]
    ref, S = d.sum(0), d.abs().sum(0)
    gamma = n * 2.0 ** -53 / (1.0 - n * 2.0 ** -53)
    return ref, 2.0 ** -24 * ref.abs() + (1.0 + 2.0 ** -24) * gamma * S + 2.0 ** -149


def running_sum_fp32(dy):
    """the plain fp32 running sum over the rows, in row order (what the kernel must NOT be)"""
    s = np.zeros(dy.shape[1], np.float32)
    for r in dy.numpy():
        s = (s + r).astype(np.float32)
    return torch.from_numpy(s)
