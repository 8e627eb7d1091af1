"""Per-scene operations on sparse tensors (``topk_mask`` / ``prune_topk``, ``global_pool``; csrc/sparse_scene.hip): scene builders, score
and value kinds, and the references, written straight from the definitions of include/u3d.h section S3.  Plain CPU code: numpy / torch
on the host, no test functions, no device use.  tests/test_scene_ops_cpu.py checks the checker, tests/test_gpu_scene_ops.py runs the
kernels.

Everything but the average's forward is compared bit for bit (``same``).  The average's forward has the one bound of this file
(``avg_bound``): an fp64 sum in some fixed order, one division, one rounding to fp32."""
import numpy as np
import torch

SCORE_KINDS = ['equal', 'two', 'low_byte', 'high_byte', 'negative', 'special', 'random', 'block_tie', 'scene_tie']
VALUE_KINDS = ['randn', 'integer', 'ties', 'nan_inf', 'negative']
NAN_ROW_COL = (lambda n, C: (n // 2, C // 2))            # where 'nan_inf' puts its NaN; the +inf sits one row and one column before it


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(got, ref) -> bool:
    """bit for bit, shape and dtype included"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    return torch.equal(bits(got), bits(ref)) if got.dtype == torch.float32 else torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------------------------- scenes
def grid_for(sizes):
    """a cubic grid whose cell count covers the largest scene"""
    s = 4
    while s ** 3 < max(max(sizes), 1):
        s *= 2
    return [s, s, s]


def coords_of(sizes, shape=None, seed=None):
    """int32 [n, 4] = (b, x, y, z) in canonical order: scene b has sizes[b] voxels -- the first cells of the grid, or (seed) a random
    sorted subset of its cells"""
    shape = shape or grid_for(sizes)
    X, Y, Z = shape
    g = np.random.default_rng(seed) if seed is not None else None
    out = []
    for b, nb in enumerate(sizes):
        cells = np.arange(nb) if g is None else np.sort(g.choice(X * Y * Z, size=nb, replace=False))
        out.append(np.stack([np.full(nb, b), cells // (Y * Z), cells // Z % Y, cells % Z], 1))
    c = np.concatenate(out) if out else np.zeros((0, 4))
    return torch.from_numpy(c.astype(np.int32)).reshape(-1, 4)


def ref_offsets(coords, B):
    """offsets[b] = the first row whose batch index is >= b, offsets[B] = n"""
    b = coords[:, 0].tolist()
    return [next((i for i, v in enumerate(b) if v >= s), len(b)) for s in range(B)] + [len(b)]


# ---------------------------------------------------------------------------------------------------------------- top-k
def rank_keys(scores, largest=True):
    """uint32 [n]: the order-preserving integer image of the score bits -- every NaN the one largest key, -0.0 = +0.0, denormals kept;
    ``largest=False`` reverses the numbers and leaves the NaNs on top"""
    u = scores.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    u = np.where(u == 0x80000000, 0, u)
    k = np.where((u & 0x80000000) != 0, ~u & 0xffffffff, u | 0x80000000)
    if not largest:
        k = ~k & 0xffffffff
    return np.where(nan, 0xffffffff, k).astype(np.uint64)


def per_scene_k(k, B):
    return [k] * B if isinstance(k, int) else list(k)


def ref_topk_mask(scores, offsets, k, largest=True):
    """torch.bool [n]: scene b keeps the first min(k_b, n_b) rows of a Python sort on (key descending, row ascending)"""
    key = rank_keys(scores.reshape(-1), largest).tolist()
    mask = torch.zeros(len(key), dtype=torch.bool)
    for b, kb in enumerate(per_scene_k(k, len(offsets) - 1)):
        order = sorted(range(offsets[b], offsets[b + 1]), key=lambda i: (-key[i], i))
        mask[order[:kb]] = True
    return mask


def torch_sort_mask(scores, offsets, k):
    """the same mask for ``largest=True`` from ``torch.sort(descending=True, stable=True)`` on the CPU, which puts NaN first, breaks ties by
    index and treats +-0 as equal: the second opinion on ``ref_topk_mask``"""
    mask = torch.zeros(scores.numel(), dtype=torch.bool)
    for b, kb in enumerate(per_scene_k(k, len(offsets) - 1)):
        lo, hi = offsets[b], offsets[b + 1]
        order = torch.sort(scores.reshape(-1)[lo:hi], descending=True, stable=True).indices
        mask[lo + order[:kb]] = True
    return mask


def _from_bits(a):
    return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


def scores(kind, n, offsets, seed=0, block=256):
    """fp32 [n] of one kind.  'block_tie' / 'scene_tie' put a run of equal values across row ``block`` / across every scene boundary, a
    few rows above it and the rest below: a k just above the count of the high rows cuts the run."""
    g = np.random.default_rng(seed)
    if kind == 'equal':
        return torch.full((n,), 0.5)
    if kind == 'two':
        return torch.from_numpy(np.where(g.random(n) < 0.5, 0.25, 0.75).astype(np.float32))
    if kind == 'low_byte':                                         # only the last radix pass can tell them apart
        return _from_bits(0x3f000000 + g.integers(0, 256, n))
    if kind == 'high_byte':                                        # only the first can (positive and finite: bit 23 is clear)
        return _from_bits((g.integers(0, 128, n) << 24) | 0x00123456)
    if kind == 'negative':
        return torch.from_numpy((-g.random(n) - 0.1).astype(np.float32))
    if kind == 'random':
        return torch.from_numpy(g.standard_normal(n).astype(np.float32))
    if kind == 'special':
        pool = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x00000001,
                         0x80000001, 0x00000064, 0x007fffff, 0x807fffff, 0x00800000, 0x3f800000, 0xbf800000, 0x7f7fffff, 0xff7fffff], dtype=np.uint32)
        return _from_bits(pool[g.integers(0, len(pool), n)])
    if kind not in ('block_tie', 'scene_tie'):
        raise KeyError(kind)
    s = (g.random(n) * 0.5).astype(np.float32)                     # below the run
    marks = [block] if kind == 'block_tie' else [o for o in offsets[1:-1]]
    for m in marks:
        s[max(m - 6, 0):min(m + 7, n)] = 1.0
    s[g.integers(0, n, max(n // 50, 1))] = 2.0
    return torch.from_numpy(s)


def k_values(sizes):
    """the k of the issue: 0, 1, n_b - 1, n_b, n_b + 1 (per scene), a per-scene list, and the half that cuts runs of ties"""
    return [0, 1, [max(s - 1, 0) for s in sizes], list(sizes), [s + 1 for s in sizes], [(3 * b + 2) % (s + 2) for b, s in enumerate(sizes)],
            [s // 2 for s in sizes]]


def compact_reference(mask):
    """(kept int32 [n_keep], pos int32 [n]) of a mask"""
    kept = torch.nonzero(mask)[:, 0].int()
    pos = torch.full((len(mask),), -1, dtype=torch.int32)
    pos[kept.long()] = torch.arange(len(kept), dtype=torch.int32)
    return kept, pos


# ---------------------------------------------------------------------------------------------------------------- pooling
def values(kind, n, C, offsets, seed=0):
    """fp32 [n, C] of one kind; 'integer' makes the average's fp64 sums exact; 'nan_inf' has ONE NaN and ONE +inf"""
    g = np.random.default_rng(seed)
    if kind == 'randn':
        x = g.standard_normal((n, C))
    elif kind == 'integer':
        x = g.integers(-64, 65, (n, C))
    elif kind == 'ties':
        x = g.standard_normal((n, C))
        x[:, 0] = 1.5                                              # a column of ties: the first row of every scene wins
        x[:, C - 1] = np.where(np.arange(n) % 3 == 1, 0.0, -0.0)   # +-0.0 tie as well
    elif kind == 'nan_inf':
        x = g.standard_normal((n, C))
    elif kind == 'negative':
        x = -np.abs(g.standard_normal((n, C))) - 1.0               # a maximum that starts from 0 shows here
    else:
        raise KeyError(kind)
    x = torch.from_numpy(x.astype(np.float32))
    if kind == 'nan_inf' and n:
        r, c = NAN_ROW_COL(n, C)
        x[r, c] = float('nan')
        x[max(r - 1, 0), max(c - 1, 0)] = float('inf')
    return x


def take_max_walk(col):
    """sparse_pool.hip's take_max over one column, row by row: (value, row)"""
    h, a = None, -1
    for i, v in enumerate(col):
        if a < 0 or v > h or (v != v and h == h):
            h, a = v, i
    return h, a


def ref_global_max(x, offsets):
    """(y fp32 [B, C], arg int32 [B, C]): np.argmax returns the first NaN if there is one, else the first maximal element -- take_max's
    rule (``take_max_walk`` is the definition; tests/test_scene_ops_cpu.py compares the two); an empty scene gives +0.0 and -1"""
    B, C = len(offsets) - 1, x.shape[1]
    xn = x.numpy()
    y, arg = np.zeros((B, C), np.float32), np.full((B, C), -1, np.int32)
    for b in range(B):
        lo, hi = offsets[b], offsets[b + 1]
        if hi > lo:
            a = np.argmax(xn[lo:hi], axis=0)
            arg[b] = lo + a
            y[b] = xn[lo + a, np.arange(C)]
    return torch.from_numpy(y), torch.from_numpy(arg)


def ref_global_max_bwd(dy, arg, n):
    """dx[i, c] = dy[b, c] where arg[b, c] == i, else +0.0"""
    B, C = dy.shape
    dx = torch.zeros(n, C, dtype=torch.float32)
    for b in range(B):
        cols = torch.nonzero(arg[b] >= 0)[:, 0]
        dx[arg[b, cols].long(), cols] = dy[b, cols]
    return dx


def ref_global_avg(x, offsets, dtype=np.longdouble):
    """[B, C] in ``dtype`` (np.float64 or np.longdouble), NOT rounded to fp32: sum / n_b, 0 for an empty scene"""
    B, C = len(offsets) - 1, x.shape[1]
    xn = x.numpy().astype(dtype)
    y = np.zeros((B, C), dtype)
    for b in range(B):
        lo, hi = offsets[b], offsets[b + 1]
        if hi > lo:
            y[b] = xn[lo:hi].sum(0) / dtype(hi - lo)
    return y


def avg_bound(x, offsets, y_ref):
    """elementwise: 2^-24 |y_ref| + n_b 2^-52 mean|x| + 2^-149 -- the rounding to fp32, the fp64 sum in any order, the smallest denormal"""
    B, C = len(offsets) - 1, x.shape[1]
    bound = np.zeros((B, C), np.longdouble)
    xa = np.abs(x.numpy().astype(np.longdouble))
    for b in range(B):
        lo, hi = offsets[b], offsets[b + 1]
        m = xa[lo:hi].mean(0) if hi > lo else 0
        bound[b] = np.longdouble(2) ** -24 * np.abs(y_ref[b]) + (hi - lo) * np.longdouble(2) ** -52 * m + np.longdouble(2) ** -149
    return bound


def avg_check(y, x, offsets):
    """(ok, largest err / bound) of a device result y fp32 [B, C]; a NaN / inf must sit exactly where the reference has one"""
    ref = ref_global_avg(x, offsets)
    got = y.detach().cpu().numpy().astype(np.longdouble)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isnan(ref), np.isnan(got)) or not np.array_equal(ref[~fin & ~np.isnan(ref)], got[~fin & ~np.isnan(ref)]):
        return False, float('inf')
    with np.errstate(invalid='ignore'):
        err, bound = np.abs(got - ref)[fin], avg_bound(x, offsets, np.where(fin, ref, 0))[fin]
    ratio = float((err / bound).max()) if err.size else 0.0
    return bool((err <= bound).all()), ratio


def ref_global_avg_bwd(dy, offsets, n):
    """dx[i, c] = dy[b, c] * inv_b, inv_b = 1.0f / (float)n_b, each product rounded on its own (fp32 arithmetic throughout)"""
    dx = torch.zeros(n, dy.shape[1], dtype=torch.float32)
    for b in range(len(offsets) - 1):
        lo, hi = offsets[b], offsets[b + 1]
        if hi > lo:
            inv = np.float32(1.0) / np.float32(hi - lo)
            dx[lo:hi] = torch.from_numpy((dy[b].numpy() * inv).astype(np.float32))
    return dx
