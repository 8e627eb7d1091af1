"""General sparse-convolution geometry (kernel extents 1..3 per axis, stride, padding, dilation): the layer configurations, a brute-force
numpy reference of the output set and the pair lists written straight from the definition, the float64 dense references of y, dx, dW
and the addend gradient, and the elementwise rounding bound of tests/_conv_geometry.py on top of them.  Case builders and checkers only:
plain CPU tensors, no test functions, no device use.  tests/test_conv_general_cpu.py checks the checker, tests/test_gpu_conv_general.py
runs the kernels.

Definition (spconv's), per axis: out_dim = floor((in_dim + 2 p - d (k - 1) - 1) / s) + 1; output cell o is active iff an active input i
and a tap t in [0, k) satisfy i + p = o s + t d on all three axes with 0 <= o < out_dim; offset index = (t0 k1 + t1) k2 + t2, the order
of the weight layout [C_out, k0, k1, k2, C_in].  A submanifold layer has stride 1, padding d (k - 1) / 2 and output set = input set.

References.  Forward: ``F.conv3d(stride, padding, dilation)`` on the scattered grid, sampled at the output rows, weights permuted as in
``_conv_geometry.dense_down``.  Inverse layer (z on the OUTPUT rows -> the input rows, weights [C_out, k0, k1, k2, C_z]):
inverse(z)[i, co] = sum over the pairs (i, o) of offset t of W[co, t, cz] z[o, cz] -- the vector-Jacobian product of that same dense
convolution with the weight axes swapped, V = W.permute(4, 1, 2, 3, 0), taken by autograd with ``create_graph`` so that the gradients
of the inverse layer come from autograd on the same expression too.

Bound: ``_conv_geometry.bound`` unchanged, with L from the same expression on ones and S from the same expression on absolute values.
"""
import numpy as np
import torch
import torch.nn.functional as F

import _conv_geometry as cg

# name -> (kernel, stride, padding, dilation, submanifold); ints or triples
CONFIGS = {
    'k3s2p1': (3, 2, 1, 1, False),                                   # the common strided layer
    'k3s2p0': (3, 2, 0, 1, False),                                   # edge drop, possibly empty output
    'k3s1p1': (3, 1, 1, 1, False),                                   # regular convolution: the output set grows
    'k2s2p0': (2, 2, 0, 1, False),                                   # must equal the existing down rulebook
    'k2s1p0': (2, 1, 0, 1, False),
    'k331s221p110': ((3, 3, 1), (2, 2, 1), (1, 1, 0), 1, False),     # K = 9
    'k122s2p0': ((1, 2, 2), 2, 0, 1, False),                         # K = 4
    'k321s121p100': ((3, 2, 1), (1, 2, 1), (1, 0, 0), 1, False),     # K = 6, mixed
    'k1s2p0': (1, 2, 0, 1, False),                                   # K = 1
    'k3s3p1': (3, 3, 1, 1, False),                                   # stride above the kernel's reach leaves gaps
    'k3s2p2d2': (3, 2, 2, 2, False),                                 # dilation
    'subm_k3d2': (3, 1, 0, 2, True),                                 # dilated submanifold
    'subm_k133': ((1, 3, 3), 1, 0, 1, True),                         # K = 9 submanifold
}
SUBM_K3 = (3, 1, 0, 1, True)                                         # the existing SubM layer (carve-out), for the equality checks

SCENES = [f'line_{a}_{n}' for a in 'xz' for n in (31, 32, 33, 63, 64, 65)] + [
    'block4', 'block5', 'block_in_corner_0', 'block_in_far_corner', 'two_scenes_same_coords', 'empty_middle_scene', 'block5_odd_extent',
    'block_odd_mixed_extent', 'single_voxel']


def _t3(v):
    return (int(v),) * 3 if isinstance(v, int) else tuple(int(a) for a in v)


def geom(cfg):
    """(k, s, p, d) as triples and the submanifold flag, with the submanifold layer's effective stride and padding filled in"""
    k, s, p, d, subm = CONFIGS[cfg] if isinstance(cfg, str) else cfg
    k, s, p, d = _t3(k), _t3(s), _t3(p), _t3(d)
    if subm:
        s, p = (1, 1, 1), tuple(d[a] * (k[a] - 1) // 2 for a in range(3))
    return k, s, p, d, bool(subm)


def layer_args(cfg):
    """constructor keywords of the layer of this configuration"""
    k, s, p, d, subm = CONFIGS[cfg] if isinstance(cfg, str) else cfg
    return dict(kernel_size=k, dilation=d) if subm else dict(kernel_size=k, stride=s, padding=p, dilation=d)


def scene(name):
    kind = 'subm' if name == 'single_voxel' else 'down'
    return cg.geometry(kind, name)


def out_shape(shape, cfg):
    k, s, p, d, subm = geom(cfg)
    return tuple((int(shape[a]) + 2 * p[a] - d[a] * (k[a] - 1) - 1) // s[a] + 1 for a in range(3))


_GEO = {}


def brute(cfg, name):
    """(out_coords int32 [n_out, 4] canonical, out_shape, K x (in_rows, out_rows) int32) of configuration ``cfg`` on scene ``name``,
    from the definition: every (input row, tap) marks its output cell; every (output row, tap) looks its input cell up"""
    key = (cfg if isinstance(cfg, str) else tuple(map(str, cfg)), name)
    if key in _GEO:
        return _GEO[key]
    _, B, shape, coords = scene(name)
    k, s, p, d, subm = geom(cfg)
    oshape = tuple(shape) if subm else out_shape(shape, cfg)
    rows = [tuple(int(v) for v in r) for r in coords.tolist()]
    taps = [(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])]
    if subm:
        out = list(rows)
    else:
        cells = set()
        for r in rows:
            for t in taps:
                v = [r[1 + a] + p[a] - t[a] * d[a] for a in range(3)]
                if all(v[a] >= 0 and v[a] % s[a] == 0 and v[a] // s[a] < oshape[a] for a in range(3)):
                    cells.add((r[0], v[0] // s[0], v[1] // s[1], v[2] // s[2]))
        out = sorted(cells)                                    # lexicographic on (b, x, y, z) == canonical
    row_of = {r: i for i, r in enumerate(rows)}
    pairs = []
    for t in taps:
        pi, po = [], []
        for j, o in enumerate(out):
            i = row_of.get((o[0],) + tuple(o[1 + a] * s[a] - p[a] + t[a] * d[a] for a in range(3)))
            if i is not None:
                pi.append(i)
                po.append(j)
        pairs.append((np.asarray(pi, np.int32), np.asarray(po, np.int32)))
    oc = torch.tensor(out, dtype=torch.int32).reshape(-1, 4)
    _GEO[key] = (oc, oshape, pairs)
    return _GEO[key]


# ---------------------------------------------------------------------------------------------------------------- dense references
def dense_forward(x, w, cfg, name):
    """x [n_in, Cin], w [Cout, k0, k1, k2, Cin] -> [n_out, Cout] at the output rows of ``brute``"""
    _, B, shape, coords = scene(name)
    k, s, p, d, subm = geom(cfg)
    oc, oshape, _ = brute(cfg, name)
    y = F.conv3d(cg._scatter(x, coords, B, shape), w.permute(0, 4, 1, 2, 3), stride=s, padding=p, dilation=d)
    assert tuple(y.shape[2:]) == tuple(oshape), (cfg, name, y.shape, oshape)
    return cg._sample(y, oc)


def dense_inverse(z, w, cfg, name):
    """z [n_out, Cz] on the output rows, w [Cout, k0, k1, k2, Cz] -> [n_in, Cout]: the input gradient of ``dense_forward`` with the
    weight axes swapped, under the grad-output z"""
    _, B, shape, coords = scene(name)
    u = torch.zeros(len(coords), w.shape[0], dtype=z.dtype, requires_grad=True)
    f = dense_forward(u, w.permute(4, 1, 2, 3, 0), cfg, name)
    if f.numel() == 0:
        return torch.zeros(len(coords), w.shape[0], dtype=z.dtype) + 0.0 * (z.sum() + w.sum())
    return torch.autograd.grad(f, u, grad_outputs=z, create_graph=True)[0]


def n_rows(mode, cfg, name):
    """(source rows, destination rows)"""
    n, n2 = len(scene(name)[3]), len(brute(cfg, name)[0])
    return (n, n2) if mode == 'fwd' else (n2, n)


def make_inputs(mode, cfg, name, cin, cout, seed):
    """float32 CPU inputs with a wide dynamic range, as ``_conv_geometry.make_inputs``"""
    ns, nd = n_rows(mode, cfg, name)
    g = torch.Generator().manual_seed(seed)
    k = geom(cfg)[0]

    def wide(n, c):
        return torch.randn(n, c, generator=g) * torch.exp(torch.randn(n, c, generator=g) * 2.0)
    return dict(x=wide(ns, cin), w=torch.randn(cout, *k, cin, generator=g) * 0.1, add=torch.randn(nd, cout, generator=g), go=wide(nd, cout))


def _run(mode, x, w, add, go, cfg, name):
    x, w, add = [t.detach().clone().requires_grad_() for t in (x, w, add)]
    y = (dense_forward if mode == 'fwd' else dense_inverse)(x, w, cfg, name) + add
    y.backward(go)
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(y=y.detach(), dx=zero(x), dw=zero(w), dadd=zero(add))


def reference(mode, inp, cfg, name):
    return _run(mode, *[inp[k].double() for k in ('x', 'w', 'add', 'go')], cfg, name)


def product_counts(mode, cfg, name):
    """per-row / per-offset pair counts from the dense expression on ones: dict(y [n_dst], dx [n_src], dw [K]) float64"""
    ns, nd = n_rows(mode, cfg, name)
    k = geom(cfg)[0]
    one = lambda *s: torch.ones(*s, dtype=torch.float64)
    r = _run(mode, one(ns, 1), one(1, *k, 1), torch.zeros(nd, 1, dtype=torch.float64), one(nd, 1), cfg, name)
    return dict(y=r['y'][:, 0].round(), dx=r['dx'][:, 0].round(), dw=r['dw'].reshape(-1).round())


def magnitudes(mode, inp, cfg, name):
    return _run(mode, *[inp[k].double().abs() for k in ('x', 'w', 'add', 'go')], cfg, name)


_CASES = {}


def case(mode, cfg, name, cin, cout):
    """inputs, float64 reference, both bounds and the pair counts of ``mode`` ('fwd' / 'inv') with weights [cout, k.., cin]: computed once
    per process, shared and never written to"""
    key = (mode, cfg, name, cin, cout)
    if key not in _CASES:
        seed = ((cin * 1000 + cout) * 100 + list(CONFIGS).index(cfg)) * 100 + SCENES.index(name) + (50 if mode == 'inv' else 0)
        inp = make_inputs(mode, cfg, name, cin, cout, seed)
        cnt, S = product_counts(mode, cfg, name), magnitudes(mode, inp, cfg, name)
        k = geom(cfg)[0]
        Ls = dict(y=cnt['y'][:, None] * cin, dx=cnt['dx'][:, None] * cout, dw=cnt['dw'].reshape(1, *k, 1).expand_as(S['dw']), dadd=0.0)
        bnd = {o: {q: cg.bound(Ls[q], S[q], o) for q in Ls} for o in ('fp32', 'bf16')}
        _CASES[key] = dict(inp=inp, ref=reference(mode, inp, cfg, name), bound=bnd, counts=cnt)
    return _CASES[key]


def pair_sum(mode, inp, cfg, name, dtype=torch.float64, pairs=None):
    """y, dx, dw, dadd from the brute-force pair lists: per-offset gather, matrix product, index_add (the checker of the checker)"""
    _, _, ref_pairs = brute(cfg, name)
    pairs = ref_pairs if pairs is None else pairs
    ns, nd = n_rows(mode, cfg, name)
    x, w, add = [inp[q].to(dtype).clone().requires_grad_() for q in ('x', 'w', 'add')]
    wk = w.reshape(w.shape[0], -1, w.shape[-1])
    y = torch.zeros(nd, w.shape[0], dtype=dtype)
    for t, (pi, po) in enumerate(pairs):
        src, dst = (pi, po) if mode == 'fwd' else (po, pi)
        if len(src):
            y = y.index_add(0, torch.as_tensor(dst, dtype=torch.long), x[torch.as_tensor(src, dtype=torch.long)] @ wk[:, t, :].t())
    y = y + add
    y.backward(inp['go'].to(dtype))
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(y=y.detach(), dx=zero(x), dw=zero(w), dadd=zero(add))
