"""Shared cases of the LayerNorm edge tests (tests/test_ln_edges_cpu.py, tests/test_gpu_ln_edges.py): the kernels of csrc/norm.hip
(layer_norm_fwd_k<1 | 2 | 4>, layer_norm_bwd_k<1 | 2 | 4>, layer_norm_reduce_k) behind u3d_layer_norm_fwd[_b16], u3d_layer_norm_bwd[_b16],
u3d_layer_norm_bwd_sum, u3d_layer_norm_ws_bytes and the LayerNorm half of u3d_ln_linear.  Inputs, float64 references, acceptance bounds
and a host model of the kernels in fp32 numpy; nothing here touches a GPU.

Widths (WIDTHS): a lane owns the float4 columns lane, lane + 64, ... (`slots`), the template is picked from nv = ceil(C / 4 / 64) ->
<1>, <2>, <4> (nv = 3 runs <4> with an empty slot).  The list holds every fill state of the slots: one slot partly filled (4 .. 252), full
(256), a second slot with one float4 (260), half (384), all but one (508), full (512), a third (516, 640, 768), a fourth (772, 1020,
1024); C % 64 != 0 makes a workgroup of layer_norm_reduce_k straddle the dgamma / dbeta boundary.  Row counts: the forward grid is
ceil(M / 4) workgroups of four waves; the backward grid is nb = ln_blocks(M) = min(cap, ceil(M / 4)), cap = 512 (1024 from M = 65536),
restated below -- if the restatement drifts from norm.hip the lists only lose sharpness, no check becomes wrong.  NB_EDGES are the
edges of the three loops of layer_norm_reduce_k in nb (16 waves, the four-way unrolled `b + 48 < nb; b += 64`, the tail `b += 16`).

Value kinds (KINDS); s = x + res is the normalised row:
  ints    forward: x, res integers in [-2, 2], so s and its row sum S are exact and the mean must equal float32(S) / float32(C) BIT
          FOR BIT (the kernel divides, it does not multiply by a reciprocal).  Backward: the kernel is GIVEN stats = (mean 0, rstd 1),
          s in [-4, 4], dy, dy2, dy3 integers in [-4, 4], gamma in {+-1, +-2}: xh = s and d xh are exact integers, dgamma and dbeta
          integer sums below 2^24 -- bit for bit at every M: the guard against a lost, doubled or misattributed row that no
          rounding bound gives at M = 65537;
  randn   2 randn + 0.5;
  offset  row mean from {-100, 100, 1000}, std 0.1 (|mean| >> std);
  const   every other row equal to one of {0, 3.7, -1e3, 1e-20} (x = res = half the value: the sum is exact), ordinary rows between:
          var = 0, rstd = 1 / sqrt(eps);
  big     sigma = 1e4;
  spike   one element 1e6, the rest 1e-3 randn;
  tiny    1e-20 randn: the squares underflow, var flushes to 0, rstd = fl(1 / sqrt(eps)).
gamma is drawn from +-[0.5, 1.5] ({+-1, +-2} for `ints`); channel 1 and the last channel have gamma = 0, channel 1 also beta = 0 (y
exactly 0 there).  EPS is the fp32 number 1e-5 the entry points receive.  Domain limit: |s - mean| near 1e19 overflows the fp32 sum of
squares, as in any fp32 LayerNorm; no kind goes there.

Bounds.  u = 2^-24 (fp32, round to nearest), first order in u, coefficients rounded up.  Every comparison is elementwise
error / bound <= 1, and exactly 0 where the bound is 0 (`margin`).
  sum_out  bit for bit float32(x) + float32(res); every later reference starts from that fp32 s.
  mean     against the float64 row mean m:  |m' - m| <= (C + 1) u A1,  A1 = mean |s|  (an fp32 sum of C terms in any order, one division).
  rstd     against 1 / sqrt(var + eps) in float64, var about the true mean.  dm = the mean bound,
             dvar = (C + 4) u (var + dm^2) + dm^2 + C 2^-126      (the last term: one flushed square per element)
             relative bound  dvar / (2 (var + eps)) + 4u.
           Of the 4u one is fl(var' + eps), up to two are rsqrtf -- which compiles to a bare v_rsq_f32; that the instruction is good
           to 1 ulp is what AMD's ISA manual is understood to specify, an ASSUMPTION here, not verified -- and one is spare.  This is
           the only check that rests on the accuracy of rsqrtf.
  y        against the float64 formula on the DEVICE'S OWN (mean', rstd') read back from `stats`: y2 = (s - m') r' gamma + beta,
             bound  u (5 |(s - m') r' gamma| + |y2|)
           (one rounding each for the subtraction, two products and the addition, separate or contracted, one spare): independent
           of rsqrtf, and tight -- the host model sits close under the coefficient-4 form.
  backward against float64 on the inputs the kernel is given: s, stats, gamma, d = fl(fl(dy + dy2) + dy3) (restated in fp32 in the
           kernel's fixed order).  xh = (s - m) r, g = d gamma, mg = mean g, mgx = mean g xh, t = g - mg - xh mgx:
             dmg = (C + 1) u mean|g|,   dmgx = (C + 4) u mean|g xh|
             dx       r (u |g| + dmg + |xh| dmgx + 3u |xh mgx| + u |g - mg| + u |t|) + 2u |r t|
             dbeta    M u sum_rows |d|                  (an fp32 sum of exact terms in any order)
             dgamma   (M + 3) u sum_rows |d xh|         (terms that carry 3u each)
At large M the dgamma / dbeta bounds are worst-case bounds a single lost row stays inside (test_ln_edges_cpu.py asserts this): there
only the `ints` kind guards, which is why every shape runs with it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

F32, F64, LD = np.float32, np.float64, np.longdouble
U = 2.0 ** -24
EPS = float(F32(1e-5))
OK, EINVAL, EUNSUPPORTED = 0, -1, -3                    # include/u3d.h
KINDS = ('ints', 'randn', 'offset', 'const', 'big', 'spike', 'tiny')
WIDTHS = (4, 8, 36, 60, 64, 100, 252, 256, 260, 384, 508, 512, 516, 640, 768, 772, 1020, 1024)
REFUSED_WIDTHS = {0: EINVAL, -4: EINVAL, 2: EUNSUPPORTED, 6: EUNSUPPORTED, 1028: EUNSUPPORTED}
EVERY_M_WIDTHS = (36, 772)                              # M in 1 .. 9, every value
KIND_ROWS = (5, 131)                                    # a ragged last workgroup | 33 workgroups, the last with three waves
NB_EDGES = (1, 2, 15, 16, 17, 47, 48, 49, 63, 64, 65, 111, 112, 113, 127, 128, 129, 511, 512)
NB_WIDTHS = (64, 36)                                    # 36: a reduce workgroup straddles dgamma / dbeta
CAPPED_ROWS = (2049, 2053, 4096 + 2, 65535, 65536, 65537)
CAPPED_WIDE = ((2049, 1024), (2049, 516))
SUM_WIDTHS = (64, 384, 772)                             # one width of each template
CONST_VALUES = (0.0, 3.7, -1e3, 1e-20)
OFFSET_MEANS = (-100.0, 100.0, 1000.0)
_RES_SCALE = dict(randn=0.5, offset=0.01, const=0.5, big=1e3, spike=1e-4, tiny=1e-21)


# ============================================================================================================ grids (norm.hip)
def template(C):
    """the NV of the kernel instance norm.hip launches at width C"""
    nv = -(-(C // 4) // 64)
    return 1 if nv == 1 else 2 if nv == 2 else 4


def ln_blocks(M):
    """norm.hip ln_blocks (U3D_LN_BLOCKS unset): workgroups of the backward pass = rows of per-workgroup partials"""
    cap = 1024 if M >= 65536 else 512
    return int(min(cap, max(1, -(-M // 4))))


def ws_bytes(M, C):
    return ln_blocks(M) * 2 * C * 4 + 256


def nb_rows():
    """M = 4 nb and 4 nb - 3: nb workgroups, the last full / with one row"""
    return sorted({m for nb in NB_EDGES for m in (4 * nb, 4 * nb - 3)})


# ============================================================================================================ cases
def _seed(kind, M, C):
    return [KINDS.index(kind), int(M), int(C), 20251]


def make_case(kind, M, C):
    rng = np.random.default_rng(_seed(kind, M, C))
    if kind == 'ints':
        x = rng.integers(-2, 3, (M, C)).astype(F32)
        res = rng.integers(-2, 3, (M, C)).astype(F32)
        dy, dy2, dy3 = (rng.integers(-4, 5, (M, C)).astype(F32) for _ in range(3))
        gamma = (rng.integers(1, 3, C) * rng.choice([-1, 1], C)).astype(F32)
    else:
        z = rng.standard_normal((M, C))
        if kind in ('randn', 'const'):
            t = 2 * z + 0.5
        elif kind == 'offset':
            t = np.asarray(OFFSET_MEANS)[rng.integers(0, 3, M)][:, None] + 0.1 * z
        elif kind == 'big':
            t = 1e4 * z
        elif kind == 'spike':
            t = 1e-3 * z
            if M:
                t[np.arange(M), rng.integers(0, C, M)] = 1e6
        elif kind == 'tiny':
            t = 1e-20 * z
        else:
            raise ValueError(kind)
        res = (_RES_SCALE[kind] * rng.standard_normal((M, C))).astype(F32)
        x = (t - res.astype(F64)).astype(F32)
        if kind == 'const':                              # rows 0, 2, 4, ...: x = res = v / 2, the sum is exactly float32(v)
            rows = np.arange(0, M, 2)
            half = (np.asarray(CONST_VALUES, F32) / F32(2))[(rows // 2) % 4]
            x[rows] = half[:, None]
            res[rows] = half[:, None]
        dy, dy2, dy3 = (rng.standard_normal((M, C)).astype(F32) for _ in range(3))
        gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F32)
    beta = (0.1 * rng.standard_normal(C)).astype(F32)
    gamma[1] = 0.0
    beta[1] = 0.0
    gamma[C - 1] = 0.0
    return SimpleNamespace(kind=kind, M=M, C=C, x=x, res=res, gamma=gamma, beta=beta, dy=dy, dy2=dy2, dy3=dy3)


def row_sum_in(c, with_res=True):
    """the fp32 row the kernel normalises: float32(x) + float32(res) (one IEEE addition: the device must return these bits)"""
    return c.x + c.res if with_res else c.x


def unit_stats(M):
    """stats = (mean 0, rstd 1) for every row: what the `ints` backward passes"""
    st = np.zeros((M, 2), F32)
    st[:, 1] = 1.0
    return st


def grad_sum(dy, dy2=None, dy3=None):
    """fl(fl(dy + dy2) + dy3) in fp32, the kernel's fixed order; a missing term is skipped"""
    d = dy
    if dy2 is not None:
        d = d + dy2
    if dy3 is not None:
        d = d + dy3
    return np.asarray(d, F32)


# ============================================================================================================ references
def fwd_ref(s):
    """float64 row statistics of the fp32 rows s [M, C] and their bounds"""
    M, C = s.shape
    sl = s.astype(LD)
    m = sl.sum(1) / C
    var = (((sl - m[:, None]) ** 2).sum(1) / C).astype(F64)
    m = m.astype(F64)
    a1 = np.abs(s.astype(F64)).sum(1) / C
    r = SimpleNamespace(M=M, C=C, m=m, var=var, a1=a1, S=s.astype(F64).sum(1))
    r.b_mean = (C + 1) * U * a1
    dm = r.b_mean
    r.dvar = (C + 4) * U * (var + dm ** 2) + dm ** 2 + C * 2.0 ** -126
    r.rstd = 1.0 / np.sqrt(var + EPS)
    r.b_rstd = r.rstd * (r.dvar / (2 * (var + EPS)) + 4 * U)
    return r


def exact_mean(s):
    """`ints`: float32(S) / float32(C), one correctly rounded fp32 division of two exact numbers"""
    S = s.astype(F64).sum(1)
    assert np.all(np.abs(S) < 2 ** 24)
    return S.astype(F32) / F32(s.shape[1])


def const_row_rstd(v, mean_dev, C):
    """rows whose C elements all equal v, and the mean m' the device (or the model) wrote for them: every element gives the same
    a = fl(v - m') (u), a^2 (u), the sum of C equal terms ((C - 1) u), the division (u): var' = q (1 + (C + 3) u), q = (v - m')^2, up
    to one flushed square per element -> (1 / sqrt(q + eps), its bound with the 4u of the rstd check)"""
    q = (np.asarray(v, F64) - np.asarray(mean_dev, F64)) ** 2
    ref = 1.0 / np.sqrt(q + EPS)
    return ref, ref * (((C + 4) * U * q + C * 2.0 ** -126) / (2 * (q + EPS)) + 4 * U)


def y_ref(s, stats, gamma, beta, coeff=5):
    """y in float64 from the stats the device (or the model) wrote: -> (y2 [M, C], bound)"""
    st = np.asarray(stats, F64).reshape(-1, 2)
    p = (s.astype(F64) - st[:, :1]) * st[:, 1:2] * gamma.astype(F64)[None, :]
    y2 = p + beta.astype(F64)[None, :]
    return y2, U * (coeff * np.abs(p) + np.abs(y2))


def bwd_ref(s, stats, gamma, d):
    """float64 gradients from the inputs the kernel is given (s [M, C], stats [M, 2], gamma [C], the summed gradient d [M, C], all
    fp32): -> namespace(dx, dgamma, dbeta, b_dx, b_dgamma, b_dbeta)"""
    M, C = s.shape
    st = np.asarray(stats, F64).reshape(-1, 2)
    m, r = st[:, :1], st[:, 1:2]
    d = d.astype(F64)
    xh = (s.astype(F64) - m) * r
    g = d * gamma.astype(F64)[None, :]
    mg = g.sum(1, keepdims=True) / C
    mgx = (g * xh).sum(1, keepdims=True) / C
    t = g - mg - xh * mgx
    o = SimpleNamespace(dx=r * t, dgamma=(d * xh).sum(0), dbeta=d.sum(0))
    dmg = (C + 1) * U * np.abs(g).sum(1, keepdims=True) / C
    dmgx = (C + 4) * U * np.abs(g * xh).sum(1, keepdims=True) / C
    ra = np.abs(r)
    o.b_dx = (ra * (U * np.abs(g) + dmg + np.abs(xh) * dmgx + 3 * U * np.abs(xh * mgx) + U * np.abs(g - mg) + U * np.abs(t))
              + 2 * U * np.abs(r * t))
    o.b_dbeta = M * U * np.abs(d).sum(0)
    o.b_dgamma = (M + 3) * U * np.abs(d * xh).sum(0)
    return o


def margin(got, ref, bound):
    """worst |got - ref| / bound; an element with bound 0 must be equal"""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.broadcast_to(np.asarray(bound, F64), np.shape(ref))
    if ref.size == 0:
        return 0.0
    err = np.abs(got - ref)
    if not np.all(np.isfinite(err)):
        return float('inf')
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(q.max())


def forward_margins(s, got, gamma, beta):
    """worst error / bound of the forward outputs `got` (.stats [M, 2], .y [M, C]) for the fp32 rows s"""
    r = fwd_ref(s)
    st = np.asarray(got.stats).reshape(-1, 2)
    y2, yb = y_ref(s, st, gamma, beta)
    return dict(mean=margin(st[:, 0], r.m, r.b_mean), rstd=margin(st[:, 1], r.rstd, r.b_rstd), y=margin(got.y, y2, yb))


def backward_margins(ref, got):
    return dict(dx=margin(got.dx, ref.dx, ref.b_dx), dgamma=margin(got.dgamma, ref.dgamma, ref.b_dgamma),
                dbeta=margin(got.dbeta, ref.dbeta, ref.b_dbeta))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


# ============================================================================================================ bf16
def bf16_bits(a, truncate=False):
    """the bf16 bit patterns (uint16) of finite fp32 values: round to nearest, ties to even -- or, `truncate`, the planted fault"""
    b = np.ascontiguousarray(a, F32).view(np.uint32)
    if truncate:
        return (b >> np.uint32(16)).astype(np.uint16)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


# ============================================================================================================ host model (fp32)
ORDERS = ('seq', 'pairwise', 'lanes')


def row_sums(v, order, skip_last_slot=False):
    """fp32 sum along the rows of v [M, C] in one of three orders: 'seq' left to right, 'pairwise' (numpy's), 'lanes' = the kernel's
    (lane l adds (a + b) + (c + d) of its float4 columns l, l + 64, ..., then the six steps of the xor shuffle tree).
    `skip_last_slot`: the planted fault of a lane loop that stops before the partly filled last slot"""
    v = np.ascontiguousarray(v, F32)
    M, C = v.shape
    if order == 'seq':
        return np.cumsum(v, axis=1, dtype=F32)[:, -1]
    if order == 'pairwise':
        return v.sum(axis=1, dtype=F32)
    c4 = C // 4
    nv = -(-c4 // 64)
    p = np.zeros((M, nv * 256), F32)
    p[:, :C] = v
    p = p.reshape(M, nv, 64, 4)
    q = (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])
    acc = np.zeros((M, 64), F32)
    for i in range(nv - 1 if skip_last_slot and c4 % 64 else nv):
        acc = acc + q[:, i]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def model_forward(c, with_res=True, order='lanes', fault=None):
    """layer_norm_fwd_k in fp32 numpy (rsqrt correctly rounded) -> namespace(s, stats, y, y16 bits).  `fault`: a planted bug"""
    C = c.C
    s = row_sum_in(c, with_res)
    cf = F32(C)
    if fault == 'mean_short':                            # the last float4 never reaches the sum
        z = s.copy()
        z[:, C - 4:] = 0
        mean = row_sums(z, order) / cf
    else:
        mean = row_sums(s, order, skip_last_slot=fault == 'skip_last_slot') / cf
    dl = s - mean[:, None]
    var = row_sums(dl * dl, order) / (F32(C - 1) if fault == 'var_c_minus_1' else cf)
    ve = var if fault == 'no_eps' else var + F32(EPS)
    with np.errstate(divide='ignore'):
        rstd = (1.0 / np.sqrt(ve.astype(F64))).astype(F32)
    stats = np.stack([mean, rstd], 1) if s.shape[0] else np.zeros((0, 2), F32)
    used = np.roll(stats, -1, axis=0) if fault == 'neighbour_stats' else stats
    with np.errstate(invalid='ignore', over='ignore'):
        y = ((s - used[:, :1]) * used[:, 1:2]) * c.gamma[None, :] + c.beta[None, :]
    return SimpleNamespace(s=s, stats=stats, y=y, y16=bf16_bits(y, truncate=fault == 'bf16_trunc'))


def _partials(terms, nb):
    """layer_norm_bwd_k's per-workgroup partial rows [nb, C] of the per-row terms [M, C]: wave w of workgroup b adds rows 4 b + w,
    4 b + w + 4 nb, ... in turn, then the four waves are added in order"""
    M, C = terms.shape
    trips = max(1, -(-M // (4 * nb)))
    p = np.zeros((trips * nb * 4, C), F32)
    p[:M] = terms
    p = p.reshape(trips, nb, 4, C)
    acc = np.zeros((nb, 4, C), F32)
    for k in range(trips):
        acc = acc + p[k]
    t = np.zeros((nb, C), F32)
    for w in range(4):
        t = t + acc[:, w]
    return t


def _reduce(part, twice=None):
    """layer_norm_reduce_k over the partial rows [nb, C]: 16 waves stride the rows, four accumulators in the unrolled loop, one in
    the tail, (v0 + v1) + (v2 + v3), then the 16 wave sums in order.  `twice`: that partial row is added a second time (planted)"""
    nb, C = part.shape
    total = np.zeros(C, F32)
    for w in range(16):
        v = [np.zeros(C, F32) for _ in range(4)]
        b = w
        while b + 48 < nb:
            for a in range(4):
                v[a] = v[a] + part[b + 16 * a]
                if twice is not None and b + 16 * a == twice:
                    v[a] = v[a] + part[twice]
            b += 64
        while b < nb:
            v[0] = v[0] + part[b]
            if twice is not None and b == twice:
                v[0] = v[0] + part[b]
            b += 16
        total = total + ((v[0] + v[1]) + (v[2] + v[3]))
    return total


def model_backward(s, stats, gamma, dy, dy2=None, dy3=None, order='lanes', fault=None, twice=None):
    """layer_norm_bwd_k + layer_norm_reduce_k in fp32 numpy -> namespace(d, dx, dx16 bits, dgamma, dbeta).  order 'lanes' also
    follows the kernels' row order for dgamma / dbeta (workgroup partials, strided reduce); 'seq' / 'pairwise' add the rows so"""
    M, C = s.shape
    d = grad_sum(dy, dy3, dy2) if fault == 'dy3_first' else grad_sum(dy, dy2, dy3)
    st = np.asarray(stats, F32).reshape(-1, 2)
    if fault == 'neighbour_stats':
        st = np.roll(st, -1, axis=0)
    mean, rstd = st[:, :1], st[:, 1:2]
    cf = F32(C)
    xh = (s - mean) * rstd
    g = d * gamma[None, :]
    mg = (row_sums(g, order) / cf)[:, None]
    mgx = (row_sums(g * xh, order) / cf)[:, None]
    dx = rstd * ((g - mg) - xh * mgx)
    tg, tb = d * xh, d.copy()
    if fault == 'row_skipped' and M:
        tg[M // 2] = 0
        tb[M // 2] = 0
    if order == 'lanes':
        nb = ln_blocks(M)
        dgamma, dbeta = _reduce(_partials(tg, nb), twice), _reduce(_partials(tb, nb), twice)
    elif order == 'seq':
        dgamma = np.cumsum(tg, axis=0, dtype=F32)[-1] if M else np.zeros(C, F32)
        dbeta = np.cumsum(tb, axis=0, dtype=F32)[-1] if M else np.zeros(C, F32)
    else:
        dgamma, dbeta = np.ascontiguousarray(tg.T).sum(axis=1, dtype=F32), np.ascontiguousarray(tb.T).sum(axis=1, dtype=F32)
    if fault == 'swapped':
        dgamma, dbeta = dbeta, dgamma
    if fault == 'straddle_shift':                        # a reduce workgroup takes its column from the lane, not from j % C (C % 64 != 0)
        dgamma = np.roll(dgamma, 64 % C)
    return SimpleNamespace(d=d, dx=dx, dx16=bf16_bits(dx, truncate=fault == 'bf16_trunc'), dgamma=dgamma, dbeta=dbeta)
