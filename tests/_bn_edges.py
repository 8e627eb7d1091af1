"""Shared cases of the batch-norm edge tests (tests/test_bn_edges_cpu.py, tests/test_gpu_bn_edges.py): the kernels of csrc/bn.hip
(bn_reduce_k<0 / 1>, bn_partials_k, bn_sum_k, bn_finalize_k, bn_apply_k, bn_bwd_apply_k) behind u3d_bn_forward / _backward and the
split entry points u3d_bn_stats / _finalize / _apply / _bwd_stats / _bwd_apply.  Inputs, float64 / longdouble references and
acceptance bounds; nothing here touches a GPU.

Widths: every divisibility class of lpr = C / 4 against the 256 lanes of a workgroup (WIDTHS).  Row counts: the edges of the two
grid formulas of bn.hip (`bn_grid`, `ew_grid`), restated below as stats_grid / ew_grid -- if the restatement drifts from bn.hip the
lists only lose sharpness, no check becomes wrong.  Value kinds (KINDS):
  ints    integers in [-4, 4] (dy likewise): sum x, sum x^2 and sum dy are integers below 2^53, so the fp64 `sums` vector and dbeta
          must equal the integer result BIT FOR BIT at every n -- the guard against a lost or doubled row that no rounding bound at
          large n gives;
  randn   2 randn + 0.5;
  offset  per-channel mean from {-100, 100, 1000}, std 0.1 (|mean| >> std: the cancellation in E[x^2] - mean^2);
  const   the whole column equal to one of {0, 3.7, -1e3, 1e-20}: the variance clamps at 0, invstd = 1 / sqrt(eps);
  big     sigma = 1e4.
gamma is drawn from +-[0.5, 1.5]; channel 1 and the last channel have gamma = 0, channel 1 also beta = 0 (pre-activation exactly 0).
eps and momentum are the fp32 numbers the entry points receive (EPS, MOM): they are parameters of the operation, not rounded by it.

References: mean and variance by the two-pass formula in longdouble; y, running statistics, dgamma, dbeta, dx by the float64 formulas
of training-mode batch norm.  The gradients take the ReLU mask as an argument: the tests pass the DEVICE's own decisions (y > 0), so
no element has to be left out of a comparison.

Bounds.  u = 2^-24 (fp32, round to nearest), g64(k) = k 2^-53 (k fp64 operations in any order), n rows.  First order in u; the
coefficients are rounded up where the text says so.  Notation: m = mean, E2 = E[x^2], A1 = mean |x|, s = gamma / sqrt(var + eps).

  sums      S1 = sum x and S2 = sum x^2 are fp64 sums of exact terms (an fp32 value and the 48-bit product of two):
            |dS1| <= g64(n) sum|x|, |dS2| <= g64(n) sum x^2, whatever the order (per lane, per workgroup, shuffle tree).
  mean      m' = S1 / n in fp64, then rounded to fp32:  |dm64| <= g64(n + 4) A1,   |dm| <= u |m| + g64(n + 4) A1.
  var       var' = S2 / n - m'^2:  g64(n + 1) E2 from S2, 2 |m| |dm64| <= g64(n + 1) (m^2 + E2) from m'^2 (|m| A1 <= (m^2 + E2) / 2),
            two roundings of the size of E2 + m^2:   dvar = 2 g64(n + 4) (E2 + m^2).  The clamp at 0 only moves var' towards var >= 0.
  invstd    (float)(1 / sqrt(var' + eps)):  relative u + rv,  rv = dvar / (2 (var + eps)).
  scale     fl(gamma invstd): relative 2u + rv.
  shift     fl(beta - fl(mean_f scale)):  mean_f scale carries 4u |m s| (u of mean_f, 2u of scale, u of the product) + rv |m s| +
            |s| g64(n + 4) A1; the subtraction u |shift|.  Written as the x = 0 case of y below:
            u (5 |m s| + 2 |beta| + |shift|) + |m s| rv + |s| g64(n + 4) A1.
  y         fl(x scale + shift), separate or fused multiply-add: x scale carries 3u |x s| + rv |x s| -- the rv parts of x scale and
            mean_f scale are the SAME relative error of scale, so they combine to |x - m| |s| rv --, the addition u |y|:
              u (4 |x s| + 5 |m s| + 2 |beta| + |y|) + |x - m| |s| rv + |s| g64(n + 4) A1
            (4 for 3 and 2 |beta| for |beta|: room for the second-order terms).  ReLU is 1-Lipschitz: the same bound after it.
            With |mean| / std = 1e4 the u |m s| terms alone are ~1e-3: a property of the scale / shift form.
  running   fl(fl(1 - mom) r + mom v), v = mean_f or (float) of the unbiased variance var' n / (n - 1) (n = 1: var' itself), with
            a = (1 - mom) r, b = mom v:   u (3 |a| + 3 |b| + |a + b|) + mom dv,   dv = g64(n + 4) A1 or dvar n / (n - 1).
  backward  g = dy where the mask holds, else 0.  xhat' = fl(fl(x - mean_f) invstd_f) = xhat + c + r_i with the SYSTEMATIC part
            |c| <= invstd (u |m| + g64(n + 4) A1) (the rounding of the mean, the same for every row) and |r_i| <= (4u + rv) |xhat_i|
            (subtraction u, invstd u + rv, product u, one spare).
  sums'     A = sum g (fp64 of exact terms): dA = g64(n + 4) sum|g|;  B = sum g xhat':
            dB = |c| |sum g| + (4u + rv + g64(n + 4)) sum|g xhat|.
  dbeta     (float) A: dA + u |A|.     dgamma   (float) B: dB + u |B|.
  dx        fl(scale (fl(g - m1) - fl(xhat' m2))) [+ addend], m1 = (float)(A / n), m2 = (float)(B / n):
            dm1 = dA / n + u |m1|,  dm2 = dB / n + u |m2|,  t = g - m1 - xhat m2,  dx0 = s t:
              |s| (dm1 + u |g - m1| + |m2| (|c| + (4u + rv) |xhat|) + |xhat| dm2 + u |xhat m2| + u |t|) + (3u + rv) |dx0|
            (+ u |dx0 + addend| for the addition of the addend, separate or fused).
  eval bwd  zero sums, count 1: m1 = m2 = 0, dx = fl(scale g) [+ addend]: u |scale g| (+ u |scale g + addend|), against the
            device's own fp32 scale.
  partials  u3d_bn_stats from per-tile sums [n_tiles][2][C] (fp32): an fp64 sum of n_tiles exact terms per column:
            g64(n_tiles + 4) sum|p|; integer-valued partials come out exact.
  const     n copies of a value v: every partial sum j v is exact (24 + 29 bits); j v^2 is exact when (odd part of the mantissa
            of v^2) n < 2^53 -- then var' = 0 exactly and invstd = fl(1 / sqrt(eps)); else dvar as above with E2 = m^2 = v^2.
At large n the random-value bounds are worst-case bounds a single lost row stays inside (test_bn_edges_cpu.py prints this): there
only the `ints` kind guards, which is why every shape runs with it."""
from __future__ import annotations

from fractions import Fraction
from types import SimpleNamespace

import numpy as np

F32, F64, LD = np.float32, np.float64, np.longdouble
U = 2.0 ** -24
EPS = float(F32(1e-4))
MOM = float(F32(0.1))
EINVAL = -1
KINDS = ('ints', 'randn', 'offset', 'const', 'big')
WIDTHS = (4, 8, 16, 32, 36, 64, 96, 100, 128, 160, 260, 288, 320, 384, 508, 512)
REFUSED_WIDTHS = (0, 2, 6, 516)
EVERY_N_WIDTHS = (36, 508)                       # every n in 1 .. 70, `ints`
LARGE_ROWS = {32: 131073, 64: 65537, 512: 8193}  # 256 * 16 * rpb + 1: the first row count with the statistics grid capped
PARTIAL_WIDTHS = (32, 96, 128, 160, 288, 512)    # 2C: 64 | 192 | 256 | 256 + 64 | 256 + 256 + 64 | 4 x 256
SHADOW_WIDTHS = (32, 64, 96, 160, 288, 512)
CONST_VALUES = (0.0, 3.7, -1e3, 1e-20)
OFFSET_MEANS = (-100.0, 100.0, 1000.0)


def g64(k):
    return np.asarray(k, F64) * 2.0 ** -53


# ============================================================================================================ grids (bn.hip)
def rpb(C):
    """rows per workgroup pass of bn_reduce_k (bn.hip: rpb = 256 / lpr, lpr = C / 4)"""
    return 256 // (C // 4)


def stats_grid(n, C):
    """bn.hip bn_grid: ceil(n / (16 rpb)) workgroups, 1 .. 256"""
    return int(min(256, max(1, -(-n // (rpb(C) * 16)))))


def ew_grid(n, C):
    """bn.hip ew_grid: ceil(n C / 4 / 256) workgroups, 1 .. 4096"""
    return int(min(4096, max(1, -(-(n * (C // 4)) // 256))))


def partials_rpp(C):
    return 1 if 2 * C >= 256 else 256 // (2 * C)


def partials_grid(n_tiles, C):
    """bn.hip bn_partials_grid: ceil(n_tiles / (16 rpp)) workgroups, 1 .. 128"""
    return int(min(128, max(1, -(-n_tiles // (partials_rpp(C) * 16)))))


def row_edges(C):
    r = rpb(C)
    return sorted({n for n in (1, 2, r - 1, r, r + 1, 16 * r, 16 * r + 1, 64 * r - 1, 64 * r + 1) if n > 0})


def tile_edges(C):
    """n_tiles around bn_partials_k's loop edges: one pass, the two-loads loop and its tail with one workgroup (2 rpp +- 1) and with
    the capped grid (2 * 128 * rpp +- 1), the 16-tiles-per-thread edge, the first count with the grid capped"""
    r = partials_rpp(C)
    return sorted({t for t in (1, 2, 2 * r - 1, 2 * r + 1, 16 * r - 1, 16 * r + 1, 2 * 128 * r - 1, 2 * 128 * r + 1, 128 * 16 * r + 1) if t > 0})


# ============================================================================================================ cases
def _seed(kind, n, C):
    return [KINDS.index(kind), int(n), int(C), 20250]


def make_case(kind, n, C):
    rng = np.random.default_rng(_seed(kind, n, C))
    if kind == 'ints':
        x = rng.integers(-4, 5, (n, C)).astype(F32)
        dy = rng.integers(-4, 5, (n, C)).astype(F32)
        addend = rng.integers(-4, 5, (n, C)).astype(F32)
    else:
        if kind == 'randn':
            x = 2 * rng.standard_normal((n, C)) + 0.5
        elif kind == 'offset':
            x = np.asarray(OFFSET_MEANS)[rng.integers(0, 3, C)][None, :] + 0.1 * rng.standard_normal((n, C))
        elif kind == 'const':
            x = np.broadcast_to(np.asarray(CONST_VALUES)[(np.arange(C) + rng.integers(0, 4)) % 4][None, :], (n, C))
        elif kind == 'big':
            x = 1e4 * rng.standard_normal((n, C))
        else:
            raise ValueError(kind)
        x = np.ascontiguousarray(x, dtype=F32)
        dy = rng.standard_normal((n, C)).astype(F32)
        addend = rng.standard_normal((n, C)).astype(F32)
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F32)
    beta = (0.1 * rng.standard_normal(C)).astype(F32)
    gamma[1] = 0.0
    beta[1] = 0.0
    gamma[C - 1] = 0.0
    rm0 = rng.standard_normal(C).astype(F32)
    rv0 = rng.uniform(0.5, 2.0, C).astype(F32)
    return SimpleNamespace(kind=kind, n=n, C=C, x=x, dy=dy, addend=addend, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0)


def partials_case(kind, n_tiles, C):
    """synthetic [n_tiles][2][C] fp32 per-tile sums: integers ('ints': exact in fp64 whatever the order) or randn"""
    rng = np.random.default_rng(_seed(kind, n_tiles, C) + [1])
    if kind == 'ints':
        return rng.integers(-64, 65, (n_tiles, 2, C)).astype(F32)
    return (8 * rng.standard_normal((n_tiles, 2, C))).astype(F32)


def partials_ref(p):
    pl = p.astype(LD)
    return pl.sum(0).astype(F64).reshape(-1), g64(p.shape[0] + 4) * np.abs(pl).sum(0).astype(F64).reshape(-1)


# ============================================================================================================ references
def stats_ref(c):
    """two-pass mean / variance in longdouble and what the bounds need: -> namespace of float64 [C] rows"""
    n = c.n
    xl = c.x.astype(LD)
    s1 = xl.sum(0)
    m = s1 / n
    d = xl - m
    var = (d * d).sum(0) / n
    s2 = (xl * xl).sum(0)
    r = SimpleNamespace(n=n, m=m.astype(F64), var=var.astype(F64), s1=s1.astype(F64), s2=s2.astype(F64), e2=(s2 / n).astype(F64),
                        a1=(np.abs(xl).sum(0) / n).astype(F64))
    r.istd = (1 / np.sqrt(var + LD(EPS))).astype(F64)
    g, b = c.gamma.astype(F64), c.beta.astype(F64)
    r.s = g * r.istd
    r.shift = b - r.m * r.s
    r.unb = r.var * n / (n - 1) if n > 1 else r.var
    r.rm = (1 - MOM) * c.rm0.astype(F64) + MOM * r.m
    r.rv = (1 - MOM) * c.rv0.astype(F64) + MOM * r.unb
    # ---- bounds
    r.dvar = 2 * g64(n + 4) * (r.e2 + r.m ** 2)
    r.rvar = 0.5 * r.dvar / (r.var + EPS)
    r.dm64 = g64(n + 4) * r.a1
    ms = np.abs(r.m * r.s)
    r.b_sums = np.concatenate([g64(n) * np.abs(xl).sum(0).astype(F64), g64(n) * r.s2])
    r.b_mean = U * np.abs(r.m) + r.dm64
    r.b_istd = r.istd * (U + r.rvar)
    r.b_scale = np.abs(r.s) * (2 * U + r.rvar)
    r.b_shift = U * (5 * ms + 2 * np.abs(b) + np.abs(r.shift)) + ms * r.rvar + np.abs(r.s) * r.dm64
    a, bm, bv = (1 - MOM) * c.rm0.astype(F64), MOM * r.m, MOM * r.unb
    r.b_rm = U * (3 * np.abs(a) + 3 * np.abs(bm) + np.abs(a + bm)) + MOM * r.dm64
    a = (1 - MOM) * c.rv0.astype(F64)
    r.b_rv = U * (3 * np.abs(a) + 3 * np.abs(bv) + np.abs(a + bv)) + MOM * r.dvar * (n / (n - 1) if n > 1 else 1.0)
    return r


def y_ref(c, r, relu):
    """-> (y float64 [n, C], bound)"""
    x = c.x.astype(F64)
    pre = x * r.s + r.shift
    y = np.maximum(pre, 0.0) if relu else pre
    b = (U * (4 * np.abs(x * r.s) + 5 * np.abs(r.m * r.s) + 2 * np.abs(c.beta.astype(F64)) + np.abs(y))
         + np.abs(x - r.m) * np.abs(r.s) * r.rvar + np.abs(r.s) * r.dm64)
    return y, b


def const_invstd(c):
    """`const` kind: (1 / sqrt(eps), tolerance [C]) -- fp32 rounding alone where n v^2 is exact in fp64 (module docstring)"""
    v = c.x[0].astype(F64)
    tol = np.empty(c.C)
    for j, vj in enumerate(v):
        num = Fraction(float(vj)) ** 2
        odd = num.numerator
        while odd and odd % 2 == 0:
            odd //= 2
        exact = odd * c.n < 2 ** 53
        tol[j] = 0.0 if exact else 0.5 * 2 * float(g64(c.n + 4)) * 2 * float(vj) ** 2 / EPS
    ref = 1.0 / np.sqrt(EPS)
    return ref, ref * (U + tol)


def bwd_ref(c, r, mask, with_addend, n_total=None):
    """float64 gradients of training-mode batch norm (+ ReLU with the given decisions `mask`: bool [n, C] or None = no ReLU).
    -> namespace(dx, dgamma, dbeta, sums [2C], b_dx, b_dgamma, b_dbeta, b_sums [2C])"""
    n = c.n
    x, dy = c.x.astype(F64), c.dy.astype(F64)
    g = dy if mask is None else np.where(mask, dy, 0.0)
    xh = (x - r.m) * r.istd
    A, B = g.sum(0), (g * xh).sum(0)
    m1, m2 = A / n, B / n
    t = g - m1 - xh * m2
    dx0 = r.s * t
    o = SimpleNamespace(dgamma=B, dbeta=A, sums=np.concatenate([A, B]))
    cc = r.istd * (U * np.abs(r.m) + r.dm64)                    # systematic part of the xhat error
    rel = 4 * U + r.rvar
    dA = g64(n + 4) * np.abs(g).sum(0)
    dB = cc * np.abs(A) + (rel + g64(n + 4)) * np.abs(g * xh).sum(0)
    o.b_sums = np.concatenate([dA, dB])
    o.b_dbeta = dA + U * np.abs(A)
    o.b_dgamma = dB + U * np.abs(B)
    dm1, dm2 = dA / n + U * np.abs(m1), dB / n + U * np.abs(m2)
    o.b_dx = (np.abs(r.s) * (dm1 + U * np.abs(g - m1) + np.abs(m2) * (cc + rel * np.abs(xh)) + np.abs(xh) * dm2 + U * np.abs(xh * m2) + U * np.abs(t))
              + (3 * U + r.rvar) * np.abs(dx0))
    o.dx = dx0
    if with_addend:
        o.dx = dx0 + c.addend.astype(F64)
        o.b_dx = o.b_dx + U * np.abs(o.dx)
    return o


def eval_bwd_ref(scale32, dy, mask, addend):
    """zero sums, count 1: dx = scale dy' (+ addend) against the fp32 scale the kernel was given"""
    g = dy.astype(F64) if mask is None else np.where(mask, dy.astype(F64), 0.0)
    p = scale32.astype(F64)[None, :] * g
    if addend is None:
        return p, U * np.abs(p)
    return p + addend.astype(F64), U * np.abs(p) + U * np.abs(p + addend.astype(F64))


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


# ============================================================================================================ shadows
def fragment_order(C):
    """index [C]: shadow[:, j] = y[:, index[j]] (bn.hip at store_shadow: inside each 32-channel group the 16 bytes at byte 16 q hold
    channels 4q .. 4q + 3 and 16 + 4q .. 16 + 4q + 3)"""
    idx = np.empty(C, np.int64)
    for g in range(C // 32):
        for q in range(4):
            for j in range(4):
                idx[32 * g + 8 * q + j] = 32 * g + 4 * q + j
                idx[32 * g + 8 * q + 4 + j] = 32 * g + 16 + 4 * q + j
    return idx


# ============================================================================================================ fp32 restatement
def _f(a):
    return np.asarray(a, F32)


def _fma(a, b, c, fused):
    """fl(a b + c) in fp32: separate multiply and add, or one rounding (the fp64 product of two fp32 numbers is exact; the fp64 sum
    is rounded once more to fp32 -- double rounding, a restatement and not the instruction)"""
    if fused:
        return _f(a.astype(F64) * b.astype(F64) + c.astype(F64))
    return _f(_f(a * b) + c)


def emulate_forward(c, relu, fused, fault=None):
    """numpy restatement of bn_reduce_k<0> + bn_sum_k + bn_apply_k.  `fault`: a planted bug (test_bn_edges_cpu.py)"""
    n, C = c.n, c.C
    x = c.x
    xs = x[:-1] if fault == 'row_dropped' else x
    s1 = xs.astype(F64).sum(0)
    if fault == 'fp32_mean':
        s1 = np.cumsum(xs, axis=0, dtype=F32)[-1].astype(F64)
    s2 = (xs.astype(F64) * xs.astype(F64)).sum(0)
    m = s1 / n
    var = np.maximum(s2 / n - m * m, 0.0)
    istd = _f(1.0 / np.sqrt(var + F64(EPS)))
    mf = _f(m)
    sc = _f(c.gamma * istd)
    beta = -c.beta if fault == 'beta_sign' else c.beta
    sf = _fma(-mf, sc, beta, fused)
    sc_a, sf_a = sc, sf
    if fault == 'last_group':
        sc_a, sf_a = sc.copy(), sf.copy()
        sc_a[C - 4:], sf_a[C - 4:] = sc[C - 8:C - 4], sf[C - 8:C - 4]
    pre = _fma(x, np.broadcast_to(sc_a, x.shape), np.broadcast_to(sf_a, x.shape), fused)
    y = np.maximum(pre, F32(0)) if relu else pre
    unb = var * n / (n - 1) if n > 1 else var
    om, mom = F32(1) - F32(MOM), F32(MOM)
    rm = _f(_f(om * c.rm0) + _f(mom * mf))
    rv = _f(_f(om * c.rv0) + _f(mom * _f(unb)))
    return SimpleNamespace(sums=np.concatenate([s1, s2]), mean=mf, istd=istd, scale=sc, shift=sf, y=y, pre=pre, rm=rm, rv=rv)


def emulate_backward(c, fw, relu, with_addend, fused, fault=None):
    """numpy restatement of bn_reduce_k<1> + bn_sum_k + bn_bwd_apply_k on the restated forward `fw`"""
    n = c.n
    x = c.x
    if relu:
        mask = fw.pre >= 0 if fault == 'mask_ge' else fw.pre > 0
        g = np.where(mask, c.dy, F32(0))
    else:
        g = c.dy
    xh = _f(_f(x - fw.mean) * fw.istd)
    A = g.astype(F64).sum(0)
    B = (g.astype(F64) * xh.astype(F64)).sum(0)
    inv = 1.0 / (n + 1 if fault == 'count_off_by_one' else n)
    m1, m2 = _f(A * inv), _f(B * inv)
    t1 = _f(g - m1)
    t = _fma(-xh, np.broadcast_to(m2, xh.shape), t1, fused)
    o = _f(fw.scale * t)
    if with_addend:
        o = _fma(np.broadcast_to(fw.scale, t.shape), t, c.addend, fused) if fused else _f(o + c.addend)
    return SimpleNamespace(sums=np.concatenate([A, B]), dbeta=_f(A), dgamma=_f(B), dx=o)


def forward_margins(c, r, got, relu):
    """worst error / bound of every forward output of a device (or restated) run `got` against the references"""
    yr, yb = y_ref(c, r, relu)
    return dict(mean=margin(got.mean, r.m, r.b_mean), invstd=margin(got.istd, r.istd, r.b_istd), scale=margin(got.scale, r.s, r.b_scale),
                shift=margin(got.shift, r.shift, r.b_shift), y=margin(got.y, yr, yb), running_mean=margin(got.rm, r.rm, r.b_rm),
                running_var=margin(got.rv, r.rv, r.b_rv), sums=margin(got.sums, np.concatenate([r.s1, r.s2]), r.b_sums))


def backward_margins(ref, got):
    return dict(dx=margin(got.dx, ref.dx, ref.b_dx), dgamma=margin(got.dgamma, ref.dgamma, ref.b_dgamma),
                dbeta=margin(got.dbeta, ref.dbeta, ref.b_dbeta), sums=margin(got.sums, ref.sums, ref.b_sums))
