"""Degenerate level geometries for the sparse convolutions (unidet3d_amd/csrc/spconv*.hip), their float64 dense references and the
elementwise rounding bound the kernels are held to.  Case builders and checkers only: plain CPU tensors, no test functions, no
device use.  tests/test_conv_geometry_cpu.py checks the checker (references against the oracle, the bound against sabotaged
results), tests/test_gpu_conv_geometry.py runs the kernels.

A geometry is ``(name, B, spatial_shape, coords)``: coords int32 [n, 4] = (batch, x, y, z), built from integers, unique and in
canonical order (ascending ((b*X + x)*Y + y)*Z + z).

References.  ``dense_subm`` / ``dense_down`` / ``dense_inverse`` scatter the rows into a dense float64 grid, run ``F.conv3d(padding=1)``
/ ``F.conv3d(stride=2)`` / ``F.conv_transpose3d(stride=2)`` with the weight permutations of tests/test_oracle_identities.py and sample the
result at the active sites.  They are differentiable: gradients come from autograd on the same expression (``reference``).

Bound.  For one output element let S = sum_i |x_i| |w_i| + |addend| and L its own number of products.
  * fp32 results (native fp32 MFMAs and three-plane products alike): a sum of L terms accumulated in fp32 in ANY order is within
    (L - 1) u S of the exact sum to first order (u = 2**-24; every partial sum is bounded by S); adding the addend is one more
    rounding.  The three-plane form drops the plane products pl_i * pl_j with i + j >= 3, which lie below 2**-23 of a product
    (three 8-bit planes: the dropped part of x w is below 2**-24 |x| |w| twice over) -- two more units of u S; the remaining slack of
    the constant 8 covers the second-order terms.  Bound: (L + 8) * 2**-24 * S.
  * bf16 operands: each operand is rounded to 8 significant bits, round to nearest even: relative error d <= u / (1 + u), u = 2**-8.
    Two roundings per product: (1 + d)**2 - 1 <= (2 u + 3 u**2) / (1 + u)**2 < 2 u = 2**-7 of |x| |w| -- no first-order slack is
    left, results may come close to it.  Products of bf16 numbers are exact in fp32 and are accumulated in fp32 as above.
    Bound: (2**-7 + L * 2**-24) * S.
The same form holds for dx (operands dy and w) and dW (operands dy and x; L = the pair count of the element's offset).  Where
S == 0 the bound is 0: the kernel's value must be exactly 0.0.  S is computed by running the same dense convolution on |x|, |w| --
its autograd gradients under the grad-output |dy| are exactly the S of dx and dW -- and L by running it on ones.
"""
import numpy as np
import torch
import torch.nn.functional as F

LINE_LENGTHS = (31, 32, 33, 63, 64, 65, 127, 128, 129)         # ragged and exact 32- and 64-row tiles
U32 = 2.0 ** -24
UB16 = 2.0 ** -7


# ---------------------------------------------------------------------------------------------------------------- geometries
def _canon(rows, B, shape):
    c = np.unique(np.asarray(rows, np.int64).reshape(-1, 4), axis=0)             # lexicographic on (b, x, y, z) == canonical
    assert c[:, 0].min() >= 0 and c[:, 0].max() < B
    assert (c[:, 1:] >= 0).all() and (c[:, 1:] < np.asarray(shape)[None]).all()
    return torch.from_numpy(c.astype(np.int32))


def _block(b, lo, ext):
    ext = (ext,) * 3 if isinstance(ext, int) else ext
    return [(b, lo[0] + i, lo[1] + j, lo[2] + k) for i in range(ext[0]) for j in range(ext[1]) for k in range(ext[2])]


def _case(name, B, shape, rows):
    return name, B, tuple(int(s) for s in shape), _canon(rows, B, shape)


def _line_extent(L):
    return 136 if L > 65 else (72 if L > 33 else 40)


def _lines():
    out = []
    for L in LINE_LENGTHS:
        E = _line_extent(L)
        out.append(_case(f'line_x_{L}', 1, (E, 3, 3), [(0, 2 + i, 1, 1) for i in range(L)]))
        out.append(_case(f'line_z_{L}', 1, (3, 3, E), [(0, 1, 1, 3 + i) for i in range(L)]))
    return out


def _common():
    """lines, blocks and batches: used for the SubM and for the strided / inverse convolutions"""
    out = _lines()
    out.append(_case('block4', 1, (8, 8, 8), _block(0, (2, 3, 1), 4)))                                      # exactly 64 rows
    out.append(_case('block4_plus_detached', 1, (12, 8, 8), _block(0, (2, 3, 1), 4) + [(0, 9, 1, 6)]))
    out.append(_case('block5', 1, (8, 8, 8), _block(0, (1, 2, 1), 5)))                                      # interior: all 27 taps
    out.append(_case('block_in_corner_0', 1, (8, 8, 8), _block(0, (0, 0, 0), 3)))
    out.append(_case('block_in_far_corner', 2, (7, 6, 5), _block(0, (4, 3, 2), 3) + _block(1, (4, 3, 2), 3)))   # shape - 1 on every axis
    out.append(_case('two_scenes_same_coords', 2, (8, 8, 8), _block(0, (2, 2, 2), 3) + _block(1, (2, 2, 2), 3)))
    out.append(_case('empty_middle_scene', 3, (8, 8, 8), _block(0, (1, 1, 1), 3) + _block(2, (3, 2, 4), (2, 3, 2))))
    return out


def _subm_only():
    out = [_case('single_voxel', 1, (8, 8, 8), [(0, 3, 4, 5)]),
           _case('two_voxels_apart', 1, (8, 8, 8), [(0, 1, 1, 1), (0, 5, 4, 3)])]                             # only the centre offset has pairs
    for a, name in enumerate('xyz'):
        p = [0, 3, 4, 2]
        q = list(p); q[1 + a] += 1
        out.append(_case(f'adjacent_{name}', 1, (8, 8, 8), [tuple(p), tuple(q)]))
    # 3-D checkerboards of an 8 x 8 x 8 region, no face neighbour in either: (x + y + z) even leaves the twelve edge offsets only,
    # (x + y + z) divisible by three leaves six edge offsets (+1, -1, 0) and the two corner offsets +-(1, 1, 1)
    for m, name in ((2, 'checkerboard8'), (3, 'checkerboard8_mod3')):
        out.append(_case(name, 1, (10, 10, 10),
                         [(0, 1 + i, 1 + j, 1 + k) for i in range(8) for j in range(8) for k in range(8) if (i + j + k) % m == 0]))
    return out


def _down_only():
    out = []
    for k in range(8):
        out.append(_case(f'child_{k}', 1, (8, 8, 8), [(0, 2 + (k >> 2), 4 + ((k >> 1) & 1), 2 + (k & 1))]))
    out.append(_case('full_cell', 1, (8, 8, 8), _block(0, (2, 4, 2), 2)))
    out.append(_case('block5_odd_extent', 2, (5, 5, 5), _block(0, (0, 0, 0), 5) + _block(1, (0, 0, 0), 5)))   # the layer at 4 has no parent
    out.append(_case('block5_even_extent', 1, (6, 6, 6), _block(0, (0, 0, 0), 5)))
    out.append(_case('block_odd_mixed_extent', 1, (9, 6, 7), _block(0, (5, 1, 3), (4, 4, 4))))
    return out


_CACHE = {}


def geometries(kind='subm'):
    """kind 'subm': the cases of the 3x3x3 submanifold convolution; 'down': those of the strided / inverse pair"""
    if kind not in _CACHE:
        _CACHE[kind] = (_subm_only() if kind == 'subm' else _down_only()) + _common()
        names = [g[0] for g in _CACHE[kind]]
        assert len(set(names)) == len(names)
    return _CACHE[kind]


def geometry(kind, name):
    return next(g for g in geometries(kind) if g[0] == name)


def is_line_or_block(name):
    return name.startswith('line_') or name in ('block4', 'block4_plus_detached', 'block5')


def down_coords(coords, shape):
    """coarser level of a stride-2 convolution: the unique parents that lie inside floor(shape / 2), canonical order"""
    oshape = tuple(int(s) // 2 for s in shape)
    c = coords.long().clone()
    c[:, 1:] >>= 1
    ok = (c[:, 1:] < torch.tensor(oshape)[None]).all(1)
    if not bool(ok.any()):
        return torch.zeros(0, 4, dtype=torch.int32), oshape
    return torch.unique(c[ok], dim=0).int(), oshape


# ---------------------------------------------------------------------------------------------------------------- dense references
def _scatter(feats, coords, B, shape):
    c = coords.long()
    d = feats.new_zeros(B, *shape, feats.shape[1])
    return d.index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), feats).permute(0, 4, 1, 2, 3)


def _sample(d, coords):
    c = coords.long()
    return d[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]


def dense_subm(x, w, coords, B, shape):
    """SubMConv3d(k=3): x [n, Cin], w [Cout, 3, 3, 3, Cin] -> [n, Cout] at the rows of ``coords``"""
    return _sample(F.conv3d(_scatter(x, coords, B, shape), w.permute(0, 4, 1, 2, 3), padding=1), coords)


def dense_down(x, w, coords, B, shape):
    """SparseConv3d(k=2, s=2): x [n, Cin], w [Cout, 2, 2, 2, Cin] -> [n_out, Cout] at the rows of ``down_coords(coords, shape)``"""
    oc, oshape = down_coords(coords, shape)
    d = F.conv3d(_scatter(x, coords, B, shape), w.permute(0, 4, 1, 2, 3), stride=2)
    assert tuple(d.shape[2:]) == oshape
    return _sample(d, oc)


def dense_inverse(z, w, coords, B, shape):
    """SparseInverseConv3d(k=2) on the pairs of the strided convolution of ``coords``: z [n_out, Cz] on ``down_coords(coords, shape)``,
    w [Cout, 2, 2, 2, Cz] -> [n, Cout] at the rows of ``coords``; a row whose parent lies outside floor(shape / 2) receives nothing"""
    oc, oshape = down_coords(coords, shape)
    d = F.conv_transpose3d(_scatter(z, oc, B, oshape), w.permute(4, 0, 1, 2, 3), stride=2)
    c = coords.long()
    inb = (c[:, 1:] < 2 * torch.tensor(oshape)[None]).all(1)
    out = z.new_zeros(len(c), w.shape[0])
    return out.index_put((inb.nonzero().flatten(),), _sample(d, coords[inb]))


DENSE = dict(subm=dense_subm, down=dense_down, inv=dense_inverse)
KSIZE = dict(subm=3, down=2, inv=2)


def n_rows(op, coords, shape):
    """(source rows, destination rows) of ``op`` on this geometry"""
    n, n2 = len(coords), len(down_coords(coords, shape)[0])
    return dict(subm=(n, n), down=(n, n2), inv=(n2, n))[op]


def make_inputs(op, coords, shape, cin, cout, seed):
    """float32 CPU inputs of one case: features and gradients with a wide dynamic range, weights, an addend"""
    ns, nd = n_rows(op, coords, shape)
    g = torch.Generator().manual_seed(seed)
    k = KSIZE[op]

    def wide(n, c):
        return torch.randn(n, c, generator=g) * torch.exp(torch.randn(n, c, generator=g) * 2.0)
    return dict(x=wide(ns, cin), w=torch.randn(cout, k, k, k, cin, generator=g) * 0.1, add=torch.randn(nd, cout, generator=g), go=wide(nd, cout))


def _run(op, x, w, add, go, coords, B, shape):
    x, w, add = [t.detach().clone().requires_grad_() for t in (x, w, add)]
    y = DENSE[op](x, w, coords, B, shape) + add
    y.backward(go)
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return dict(y=y.detach(), dx=zero(x), dw=zero(w), dadd=zero(add))


def reference(op, inp, coords, B, shape):
    """float64 y, dx, dw, dadd of ``op`` (+ addend) on the inputs of ``make_inputs``"""
    return _run(op, *[inp[k].double() for k in ('x', 'w', 'add', 'go')], coords, B, shape)


def product_counts(op, coords, B, shape):
    """per-row / per-offset pair counts, from the dense convolution on ones: dict(y [n_dst], dx [n_src], dw [k^3]) float64"""
    ns, nd = n_rows(op, coords, shape)
    k = KSIZE[op]
    one = lambda *s: torch.ones(*s, dtype=torch.float64)
    r = _run(op, one(ns, 1), one(1, k, k, k, 1), torch.zeros(nd, 1, dtype=torch.float64), one(nd, 1), coords, B, shape)
    return dict(y=r['y'][:, 0].round(), dx=r['dx'][:, 0].round(), dw=r['dw'].reshape(-1).round())


def magnitudes(op, inp, coords, B, shape):
    """S of every element of y, dx, dw, dadd: the same dense convolution on |x|, |w|, |addend| under the grad-output |dy|"""
    return _run(op, *[inp[k].double().abs() for k in ('x', 'w', 'add', 'go')], coords, B, shape)


def bound(L, S, operands='fp32'):
    """elementwise rounding bound (module docstring): fp32 results (L + 8) 2**-24 S, bf16 operands (2**-7 + L 2**-24) S"""
    L = torch.as_tensor(L, dtype=torch.float64)
    if operands == 'fp32':
        return (L + 8.0) * U32 * S
    assert operands == 'bf16'
    return (UB16 + L * U32) * S


def bounds(op, inp, coords, B, shape, operands='fp32'):
    """bound of every element of y, dx, dw, dadd for this case"""
    cnt, S = product_counts(op, coords, B, shape), magnitudes(op, inp, coords, B, shape)
    cout, cin = inp['w'].shape[0], inp['w'].shape[-1]
    Lw = cnt['dw'].reshape(1, *inp['w'].shape[1:4], 1)
    return dict(y=bound(cnt['y'][:, None] * cin, S['y'], operands), dx=bound(cnt['dx'][:, None] * cout, S['dx'], operands),
                dw=bound(Lw.expand_as(S['dw']), S['dw'], operands), dadd=bound(0.0, S['dadd'], operands), counts=cnt)


def excess(got, ref, bnd):
    """largest err / bound over the elements (0 / 0 = 0; anything over a zero bound, or a non-finite value, = inf)"""
    got = torch.as_tensor(got).detach().double().cpu()
    assert got.shape == ref.shape == bnd.shape, (got.shape, ref.shape, bnd.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)            # x / 0 = inf, nan stays nan
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float('inf')))
    return float(torch.nan_to_num(ratio, nan=float('inf'), posinf=float('inf')).max())


_CASES = {}


def case(op, name, cin, cout):
    """inputs, float64 reference and both bounds of ``op`` with cin -> cout channels on geometry ``name``: computed once per process,
    shared by every test that needs them and never written to.  -> dict(inp, ref, bound={'fp32': ..., 'bf16': ...}, counts)"""
    key = (op, name, cin, cout)
    if key not in _CASES:
        kind = 'subm' if op == 'subm' else 'down'
        _, B, shape, coords = geometry(kind, name)
        gi = [g[0] for g in geometries(kind)].index(name)
        inp = make_inputs(op, coords, shape, cin, cout, seed=(cin * 1000 + cout) * 100 + gi)
        cnt, S = product_counts(op, coords, B, shape), magnitudes(op, inp, coords, B, shape)
        Ls = dict(y=cnt['y'][:, None] * cin, dx=cnt['dx'][:, None] * cout, dw=cnt['dw'].reshape(1, *inp['w'].shape[1:4], 1).expand_as(S['dw']), dadd=0.0)
        bnd = {o: {k: bound(Ls[k], S[k], o) for k in Ls} for o in ('fp32', 'bf16')}
        _CASES[key] = dict(inp=inp, ref=reference(op, inp, coords, B, shape), bound=bnd, counts=cnt)
    return _CASES[key]
