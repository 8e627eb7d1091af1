"""Shared cases of the varlen-attention edge tests (tests/test_attn_edges_cpu.py, tests/test_gpu_attn_edges.py): the flash kernels of
csrc/attn.hip (attn_fwd_k, attn_bwd_dq_k, attn_bwd_dkv_k: native fp32 MFMA) and csrc/attn_x3.hip (attn_fwd_x3_k, attn_bwd_dq_x3_k,
attn_bwd_dkv_x3_k: bf16 planes, NW = 4 | 8 waves) with attn_delta_k and the work decode of csrc/attn_common.h, behind the
u3d_attn_varlen_{fwd,bwd}{,_drop}{,_bf16,_b16} entry points.  Cases, float64 references, acceptance bounds, an fp32 restatement of the
device arithmetic with planted faults, a restatement of the work decode; nothing here touches a GPU.

Flows (FLOWS): native (fp32 math 'mfma', head_dim 32 only) | x3 (three bf16 planes per fp32 operand, the default) | bf16_operands (fp32
tensors, one bf16 plane) | bf16_tensors (bf16 qkv / dout / out / dqkv).  The two bf16 flows receive RNE-rounded inputs and are compared
with the float64 result of those.

Scene layouts (LAYOUTS): one row | 64-key tile edges | 128-row edges (a workgroup of eight waves) | one row in the fourth tile | empty
scenes around a short one and eleven key tiles, the last one holding 60 keys | empty scenes first | empty scenes last.

Value kinds (KINDS); q, k, v per head, dout drawn like v:
  randn    1.5 randn;
  peaked   q and k times 4: logits reach +-200;
  shift    k plus a per-head constant vector of +-8: every score of a row moves by q . c, the softmax does not;
  rising   q = |randn|, k = 0.1 randn + 0.5 (key index // 64): the row maximum rises in every key tile, alpha is strictly inside (0, 1);
  voffset  v plus 1e3: dS = P (dP - delta) cancels;
  tiny     q times 1e-3: near-uniform rows;
  group    THE EXACT KIND.  Every key j of a scene has a group g(j) < G <= head_dim and k_j = 32 e_dim(g(j)); every query i has a group and
           q_i = 32 e_dim(g(i)); v and dout are integers in +-{1 .. 4}.  All of it is exact in bf16 and under the three-plane split.
           In-group scores are formed from identical operands -- bit-identical ties at 1024 scale (181 nats at head_dim 32, 128 at 64) --
           and off-group scores are exactly 0, so exp2 returns exactly 0 for them once the row maximum is the tie: p is exactly 1 on the
           group and 0 elsewhere, l == |G| exactly, O is an integer sum and out_i = fl(O fl(1 / |G|)): two roundings.  Groups (_groups):
           scenes of at most 16 rows and of 64 rows have G = 1 (the uniform row, l = n; 64: a power of two, bit-exact); otherwise
           G = min(head_dim, round(n / 16)) >= 2, one group of a single key (G >= 3), and the LATE group, whose keys are the last
           min(8, keys of the last tile) keys of the scene -- a power of two or a single key -- while queries 0 and 3 (first tile) and
           n - 1 belong to it: before the last tile such a query has m = 0 and has accumulated every key with p = 1; the alpha = 0 step
           must wipe o, ol and l exactly.  Every query's group has a key.

References: float64 softmax attention per scene and head, out, lse = logsumexp, and the float64 formulas of its gradient (dV = P^T dO,
dP = dO V^T, delta = rowsum(dO . O), dS = P . (dP - delta), dQ = scale dS K, dK = scale dS^T Q; tests/test_attn_edges_cpu.py holds them
against torch.autograd).  `scale` is the fp32 number the entry point receives: a parameter of the operation, not rounded by it.  The
`group` forward reference is the closed form: per group the float64 sum of v over |G|, lse = 1024 scale + log |G|.

Bounds.  Elementwise, first order in u = 2^-24.  g2(k) = gamma2(k) of tests/_gemm_edges.py: k accumulated MFMA terms at ONE fp32 ulp each
(that module's convention: nothing documents how the MFMA accumulator rounds), and 2^-22 of the absolute product for the dropped cross
terms of the three-plane form (x3 only; `c3` below).  Notation per scene and head: n rows, T = ceil(n / 64) key tiles, hd = head_dim,
s_ij = scale q_i . k_j,  A_i = max_j scale sum_d |q_id k_jd|,  p = softmax.
  score     e_s(i) = (g2(hd + 6) + c3) A_i: hd products of one score; + 6: the rounding of scale log2(e), of q scale log2(e) (or of the
            score times scale log2(e), bf16 tensors), the subtraction of the maximum, the conversion of units; two spare.
            bf16 operands: + r16 A_i (q scale log2(e) is rounded to bf16).  r16 = 2^-8 is the unit roundoff of bf16: eight significand
            bits, half an ulp is up to 2^-8 of the value (2^-9 is only its average over a binade -- the `group` scores, ONE rounded
            number times 1024, are off by 1.65 x 2^-9 of their size at head_dim 32, on the device and in the restatement alike).
  out       (2 e_s(i) + g2(64 + 2T + 8) + c3 + r16) sum_j p_ij |v_jd|.  2 e_s: the score of the element and the scores under the
            normaliser.  64: the products of one key tile; 2T: alpha and the rescaling, once per tile; 8: exp2 of p, the row sum, l's
            own rescaling, 1 / l, the final product, the join of the low-order accumulator, two spare.  (The accumulation over the T
            tiles is counted as ONE tile's 64 terms: sharper than the worst case g2(64 T), which rounding errors of either sign do not
            approach -- the CPU test prints how far inside the restated arithmetic stays.)  + r16 in the bf16 flows: the probabilities
            are rounded to bf16 for the P V product.
  lse       e_s(i) + u (|lse_i| + 2 max_j |s_ij| + 4) + g2(T + 70): m ln2 (the constant, the product) and the final sum at the size of
            lse and of the maximum; log l: 64 terms of a tile's row sum, T rescalings, exp2 and __logf.
  backward  the recomputed probabilities carry the relative error eps_i = 2 e_s(i) + 4u (|lse_i| + max_j |s_ij|) + 16u (lse log2(e),
            the recomputed score, the subtraction, exp2) and the absolute error 2^-126: fp32 flushes what float64 keeps as 1e-79.
  dS        E_ij = eps_i |dS_ij| + p_ij (g2(hd + 4) + c3) (sum_d |dout_id| |v_jd| + sum_d |dout_id| (|out_id| + b_out_id))
                   + 2^-126 (1 + sum_d |dout_id| |v_jd| + sum_d |dout_id| (|out_id| + b_out_id))
            (delta's share of b_out enters at the size of the roundings already counted: b_out is itself a few u of sum p |v|.)
            bf16 flows: + p_ij sum_d |dout_id| b_out_id IN FULL -- delta is formed from the device's out, which carries the bf16
            roundings of the probabilities (and of the store, bf16 tensors): 2^-8 of sum p |v|, not a few u.  With v = 1e3 + noise
            this term is the whole error of dq and dk; without it the restated bf16 arithmetic leaves the dq bound 24 times.
  dq        scale (sum_j E_ij |k_jd| + (g2(n + 8) + c3 + r16) sum_j |dS_ij| |k_jd|); r16: dS is rounded to bf16 for the product.
  dk        the same with q in place of k and the sum over i; bf16 operands: 2 r16 (dS and q scale log2(e) are both rounded).
  dv        sum_i (eps_i + g2(n + 8) + c3 + r16) p_ij |dout_id| + 2^-126 sum_i |dout_id|.
  bf16 tensors: every stored element (out, dq, dk, dv) adds half a bf16 ulp of the fp32 value it was rounded from (half_ulp_bf16).
None of the coefficients comes from a measurement.

`group` acceptance (group_forward_margin, group_zero_masks): |out - closed form| <= 2 fp32 ulp of the closed form (+ half a bf16 ulp,
bf16 tensors), so a power-of-two group is bit-exact; lse under the lse bound; with dropout at p = 0.5 (1 / (1 - p) = 2 exactly) out is
2 (integer sum over the kept group keys) fl(1 / |G|) under the same 2 ulp, exactly 0 where every group key is dropped; in the backward
pass the off-group probabilities are exactly 0, so every element of dq and dk outside the group's own dim, and every element of dk / dv
of a key whose group has no query, is exactly 0 (the float64 softmax has 1e-77 there); the other elements are held to the bounds above.

The restated arithmetic (emulate) is plain fp32: log2-unit scores, 64-key tiles, online maximum, alpha, l, o (1 / l), lse = m ln2 + log l,
the backward p = exp2(s - lse log2(e)), delta from the restated out; the bf16 flows round where the kernels do.  FAULTS are the switches
of tests/test_attn_edges_cpu.py.  Six of them leave a bound or the `group` acceptance by factors of 100 and more; a truncating bf16
store moves an element by less than one bf16 ulp where half of one is allowed, so it fails the acceptance by a factor below 2 -- in
more than a tenth of the elements that need rounding (that test counts them)."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from _gemm_edges import U, gamma2, half_ulp_bf16, margin, rne

FLOWS = ('native', 'x3', 'bf16_operands', 'bf16_tensors')
PLANE_FLOWS = FLOWS[1:]
FLOW_MATH = {'native': 'mfma', 'x3': 'bf16x3', 'bf16_operands': None, 'bf16_tensors': None}          # precision.fp32_math the flow needs
FLOW_SUFFIX = {'native': '', 'x3': '', 'bf16_operands': '_bf16', 'bf16_tensors': '_b16'}             # u3d_attn_varlen_{fwd,bwd}<suffix>
FLOW_HD = {'native': (32,), 'x3': (32, 64), 'bf16_operands': (32, 64), 'bf16_tensors': (32, 64)}
FLOW_HDS = tuple((f, hd) for f in FLOWS for hd in FLOW_HD[f])
LAYOUTS = ((1,), (63, 64, 65), (127, 128, 129), (193,), (0, 5, 0, 700), (0, 0, 5), (5, 0, 0))
KINDS = ('randn', 'peaked', 'shift', 'rising', 'voffset', 'tiny', 'group')
RANDOM_KINDS = KINDS[:6]
FAULTS = ('mask_last_key', 'no_o_rescale', 'no_l_rescale', 'dq_skip_last_key', 'dkv_skip_last_query', 'lse_log2', 'bf16_trunc')
OUTPUTS = ('out', 'lse', 'dq', 'dk', 'dv')
LOG2E, LN2 = np.float32(1.44269504088896340736), np.float32(0.69314718055994530942)
TINY = 2.0 ** -126
R16 = 2.0 ** -8
# decode edges: (H, lens); head_dim 64 only where the third entry says so
_rs = np.random.default_rng(1764)
DECODE_CASES = (
    (1, (65,), None),
    (3, (5, 0, 70), None),
    (5, (17, 64, 1), None),
    (1, tuple(int(v) for v in np.concatenate([[0, 1, 3, 64, 65], _rs.choice([0, 1, 3, 64, 65], 12)])), None),          # 17 scenes
    (2, tuple({2: 3, 9: 65, 16: 1, 31: 64, 32: 17}.get(b, 0) for b in range(33)), None),                                 # 33 scenes, 28 empty
    (16, (65, 3), 64),
)
MAXLEN_LENS = (65, 129)
MAXLEN_OVER = (130, 192, 256, 257, 4096)


def scale_of(hd):
    """the fp32 number the entry points receive"""
    return float(np.float32(1.0 / math.sqrt(hd)))


# ============================================================================================================ work decode (attn_common.h)
def attn_tiles(max_len, tile_rows):
    return (max_len + tile_rows - 1) // tile_rows


def attn_grid(H, B, n_tiles):
    return ((H * B + 7) // 8) * 8 * n_tiles


def attn_decode(block, H, B, n_tiles):
    """(scene, head, tile) of workgroup `block`; scene >= B: a padding workgroup"""
    x, j = block & 7, block >> 3
    hb = (j // n_tiles) * 8 + x
    return hb // H, hb % H, j % n_tiles


# ============================================================================================================ cases
def _groups(n, hd, rng):
    """(group of every key [n], group of every query [n], G); module docstring"""
    if n <= 16 or n == 64:
        return np.zeros(n, np.int64), np.zeros(n, np.int64), 1
    G = min(hd, max(2, int(round(n / 16))))
    last = n - 64 * ((n - 1) // 64)
    nl = min(8, last)
    ng = G - 2 if G >= 3 else 1                                   # general groups 0 .. ng - 1
    gk = np.full(n, -1, np.int64)
    gk[n - nl:] = G - 1                                           # the late group
    if G >= 3:
        gk[1] = G - 2                                             # the group of one key
    rest = rng.permutation(np.flatnonzero(gk < 0))
    gk[rest] = np.arange(rest.size) % ng
    gq = rng.integers(0, ng, n)
    gq[[0, 3, n - 1]] = G - 1
    if G >= 3:
        gq[5] = G - 2
    return gk, gq, G


def _seed(kind, lens, H, hd):
    return [KINDS.index(kind), int(H), int(hd), 977] + [int(v) for v in lens]


@functools.lru_cache(maxsize=None)
def make_case(kind, lens, H, hd, bf16=False):
    """qkv fp32 [n, 3 H hd] (q | k | v, heads side by side), dout fp32 [n, H hd]; bf16: both RNE-rounded (they stay fp32 tensors).
    `group`: groups[scene][head] = (gk, gq, G, dim [G])"""
    rng = np.random.default_rng(_seed(kind, lens, H, hd))
    n, D = int(sum(lens)), H * hd
    groups = None
    if kind == 'group':
        q, k = np.zeros((n, H, hd), np.float32), np.zeros((n, H, hd), np.float32)
        v = (rng.integers(1, 5, (n, H, hd)) * rng.choice([-1, 1], (n, H, hd))).astype(np.float32)
        do = (rng.integers(1, 5, (n, H, hd)) * rng.choice([-1, 1], (n, H, hd))).astype(np.float32)
        groups, o = [], 0
        for ln in lens:
            per_head = []
            for h in range(H):
                gk, gq, G = _groups(ln, hd, rng)
                dim = (np.arange(G) + 5 * h) % hd
                k[o + np.arange(ln), h, dim[gk]] = 32.0
                q[o + np.arange(ln), h, dim[gq]] = 32.0
                per_head.append((gk, gq, G, dim))
            groups.append(per_head)
            o += ln
    else:
        q, k, v, do = [1.5 * rng.standard_normal((n, H, hd)) for _ in range(4)]
        if kind == 'peaked':
            q, k = 4 * q, 4 * k
        elif kind == 'shift':
            k = k + 8.0 * rng.choice([-1.0, 1.0], (1, H, hd))
        elif kind == 'rising':
            idx = np.concatenate([np.arange(ln) for ln in lens]) if n else np.zeros(0)
            q = np.abs(q / 1.5)
            k = 0.1 * k / 1.5 + 0.5 * (idx // 64)[:, None, None]
        elif kind == 'voffset':
            v = v + 1e3
        elif kind == 'tiny':
            q = 1e-3 * q
        elif kind != 'randn':
            raise ValueError(kind)
    qkv = torch.from_numpy(np.concatenate([np.asarray(t, np.float32).reshape(n, D) for t in (q, k, v)], 1))
    dout = torch.from_numpy(np.asarray(do, np.float32).reshape(n, D))
    if bf16:
        qkv, dout = rne(qkv), rne(dout)
    return SimpleNamespace(kind=kind, lens=tuple(lens), H=H, hd=hd, n=n, D=D, qkv=qkv, dout=dout, groups=groups, bf16=bf16)


def flow_case(kind, lens, H, hd, flow):
    return make_case(kind, tuple(lens), H, hd, flow in ('bf16_operands', 'bf16_tensors'))


def _heads(c):
    """yields (row offset, rows, head, q, k, v, dout) float32 views of one (scene, head)"""
    o = 0
    for ln in c.lens:
        for h in range(c.H):
            sl = slice(h * c.hd, (h + 1) * c.hd)
            x = c.qkv[o:o + ln]
            yield o, ln, h, x[:, sl], x[:, c.D:][:, sl], x[:, 2 * c.D:][:, sl], c.dout[o:o + ln, sl]
        o += ln


def _blank(c):
    z = lambda: torch.zeros(c.n, c.D, dtype=torch.float64)
    return SimpleNamespace(out=z(), lse=torch.zeros(c.H, c.n, dtype=torch.float64), dq=z(), dk=z(), dv=z())


# ============================================================================================================ references and bounds
def _scene_ref(q, k, v, do, scale, flow, keep=None, rinv=1.0):
    """float64 attention of one (scene, head) and its gradient with the elementwise bounds of the module docstring: ten [n, hd] / [n]
    tensors.  keep (float64 [n, n] of 0 / 1) and rinv: dropout on the probabilities (forward reference only)"""
    q, k, v, do = q.double(), k.double(), v.double(), do.double()
    n, hd = q.shape
    T = -(-n // 64)
    c3 = 2.0 ** -22 if flow == 'x3' else 0.0
    b16 = flow in ('bf16_operands', 'bf16_tensors')
    r16 = R16 if b16 else 0.0
    S, aS = scale * (q @ k.t()), scale * (q.abs() @ k.abs().t())
    A, smax = aS.max(1).values, S.abs().max(1).values
    e_s = (float(gamma2(hd + 6)) + c3 + (R16 if flow == 'bf16_operands' else 0.0)) * A
    lse = torch.logsumexp(S, 1)
    P = torch.exp(S - lse[:, None])
    Pd = P if keep is None else P * keep * rinv
    out, aout = Pd @ v, Pd @ v.abs()
    b_out = (2 * e_s + float(gamma2(64 + 2 * T + 8)) + c3 + r16)[:, None] * aout
    b_lse = e_s + U * (lse.abs() + 2 * smax + 4) + float(gamma2(T + 70))
    h_out = torch.zeros_like(out)
    if flow == 'bf16_tensors':
        h_out = half_ulp_bf16(out.abs() + b_out)
        b_out = b_out + h_out
    eps = 2 * e_s + 4 * U * (lse.abs() + smax) + 16 * U
    dP, adP = do @ v.t(), do.abs() @ v.abs().t()
    delta = (do * out).sum(1)
    adelta = (do.abs() * (out.abs() + b_out)).sum(1)
    dS = P * (dP - delta[:, None])
    w = adP + adelta[:, None]
    E = eps[:, None] * dS.abs() + P * (float(gamma2(hd + 4)) + c3) * w + TINY * (1 + w)
    if b16:
        E = E + P * (do.abs() * b_out).sum(1)[:, None]
    gn = float(gamma2(n + 8)) + c3 + r16
    dq, b_dq = scale * (dS @ k), scale * (E @ k.abs() + gn * (dS.abs() @ k.abs()))
    gk_ = gn + (R16 if flow == 'bf16_operands' else 0.0)
    dk, b_dk = scale * (dS.t() @ q), scale * (E.t() @ q.abs() + gk_ * (dS.abs().t() @ q.abs()))
    dv = P.t() @ do
    b_dv = ((eps + gn)[:, None] * P).t() @ do.abs() + TINY * do.abs().sum(0)[None, :]
    if flow == 'bf16_tensors':
        b_dq, b_dk, b_dv = [b + half_ulp_bf16(g.abs() + b) for g, b in ((dq, b_dq), (dk, b_dk), (dv, b_dv))]
    return SimpleNamespace(out=out, lse=lse, dq=dq, dk=dk, dv=dv, b_out=b_out, b_lse=b_lse, b_dq=b_dq, b_dk=b_dk, b_dv=b_dv)


def reference(c, flow, mask=None, p=0.0):
    """float64 (out [n, D], lse [H, n], dq, dk, dv [n, D]) and b_<name>, the bounds of `flow`.  mask (uint8 / bool [H, n, n], packed rows,
    1 = kept) with p: dropout on the probabilities -- only out and lse (and their bounds) are meaningful then"""
    r = _blank(c)
    for nm in OUTPUTS:
        setattr(r, 'b_' + nm, torch.zeros_like(getattr(r, nm)))
    sc = scale_of(c.hd)
    for o, ln, h, q, k, v, do in _heads(c):
        if ln == 0:
            continue
        keep = None if mask is None else mask[h, o:o + ln, o:o + ln].double()
        s = _scene_ref(q, k, v, do, sc, flow, keep, 1.0 / (1.0 - p))
        sl = slice(h * c.hd, (h + 1) * c.hd)
        for nm in ('out', 'dq', 'dk', 'dv'):
            getattr(r, nm)[o:o + ln, sl] = getattr(s, nm)
            getattr(r, 'b_' + nm)[o:o + ln, sl] = getattr(s, 'b_' + nm)
        r.lse[h, o:o + ln], r.b_lse[h, o:o + ln] = s.lse, s.b_lse
    return r


@functools.lru_cache(maxsize=None)
def cached_reference(kind, lens, H, hd, flow):
    return reference(flow_case(kind, lens, H, hd, flow), flow)


def margins(r, got):
    """worst error / bound of every output `got` has"""
    return {nm: margin(getattr(got, nm), getattr(r, nm), getattr(r, 'b_' + nm)) for nm in OUTPUTS if getattr(got, nm, None) is not None}


def split_dqkv(dqkv, D):
    return dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]


# ============================================================================================================ the exact kind
def ulp32(x):
    """one fp32 ulp at magnitude x (float64 tensor): 2^(floor(log2 |x|) - 23), 0 at 0"""
    return half_ulp_bf16(x) * 2.0 ** -15


def group_closed(c, mask=None):
    """closed form of the `group` forward pass: float64 (out [n, D], lse [H, n], group size of every query [H, n]).  mask (uint8 / bool
    [H, n, n], 1 = kept): dropout at p = 0.5 -- 2 (sum over the kept group keys) / |G|"""
    out = torch.zeros(c.n, c.D, dtype=torch.float64)
    lse = torch.zeros(c.H, c.n, dtype=torch.float64)
    size = torch.zeros(c.H, c.n, dtype=torch.float64)
    s = 1024.0 * scale_of(c.hd)
    o = 0
    for ln, per_head in zip(c.lens, c.groups):
        for h, (gk, gq, G, dim) in enumerate(per_head):
            if ln == 0:
                continue
            sl = slice(h * c.hd, (h + 1) * c.hd)
            member = torch.from_numpy(gq[:, None] == gk[None, :]).double()                # [query, key]
            cnt = member.sum(1)
            w = member if mask is None else 2.0 * member * mask[h, o:o + ln, o:o + ln].double()
            out[o:o + ln, sl] = (w @ c.qkv[o:o + ln, 2 * c.D:][:, sl].double()) / cnt[:, None]
            lse[h, o:o + ln] = s + torch.log(cnt)
            size[h, o:o + ln] = cnt
        o += ln
    return out, lse, size


def group_forward_margin(c, flow, out, mask=None):
    """worst |out - closed form| / (2 fp32 ulp of the closed form [+ half a bf16 ulp]); inf where an element with tolerance 0 differs"""
    ref, _, _ = group_closed(c, mask)
    tol = 2 * ulp32(ref)
    if flow == 'bf16_tensors':
        tol = tol + half_ulp_bf16(ref.abs() + tol)
    return margin(out, ref, tol)


def group_zero_masks(c):
    """bool [n, D] each: the elements of dq, dk, dv that must be exactly 0 (module docstring)"""
    zq, zk, zv = [torch.ones(c.n, c.D, dtype=torch.bool) for _ in range(3)]
    zv[:] = False
    o = 0
    for ln, per_head in zip(c.lens, c.groups):
        for h, (gk, gq, G, dim) in enumerate(per_head):
            if ln == 0:
                continue
            rows = torch.arange(o, o + ln)
            zq[rows, h * c.hd + torch.from_numpy(dim[gq])] = False
            has_q = np.isin(gk, gq)
            zk[rows[has_q], h * c.hd + torch.from_numpy(dim[gk[has_q]])] = False
            zv[o + np.flatnonzero(~has_q), h * c.hd:(h + 1) * c.hd] = True
        o += ln
    return zq, zk, zv


def group_backward_margins(c, r, dq, dk, dv):
    """the backward acceptance of `group`: (number of non-zero elements where exact zeros are due, margins of the other elements)"""
    zq, zk, zv = group_zero_masks(c)
    bad = sum(int((g[z] != 0).sum()) for g, z in ((dq, zq), (dk, zk), (dv, zv)))
    m = {}
    for nm, g, z in (('dq', dq, zq), ('dk', dk, zk), ('dv', dv, zv)):
        m[nm] = margin(g[~z], getattr(r, nm)[~z], getattr(r, 'b_' + nm)[~z])
    return bad, m


def late_groups(c):
    """[(scene, head, first key of the late group, first key of the last tile, late-group queries below 64)] of the multi-tile scenes with G > 1"""
    res = []
    for b, (ln, per_head) in enumerate(zip(c.lens, c.groups)):
        for h, (gk, gq, G, dim) in enumerate(per_head):
            if ln > 64 and G > 1:
                keys = np.flatnonzero(gk == G - 1)
                res.append((b, h, int(keys.min()), 64 * ((ln - 1) // 64), np.flatnonzero(gq[:64] == G - 1)))
    return res


# ============================================================================================================ fp32 restatement
def trunc_bf16(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _emulate_scene(q, k, v, do, scale, flow, fault):
    f = torch.float32
    n, hd = q.shape
    tensors, b16 = flow == 'bf16_tensors', flow in ('bf16_operands', 'bf16_tensors')
    rnd = rne if b16 else (lambda t: t)
    store = (trunc_bf16 if fault == 'bf16_trunc' else rne) if tensors else (lambda t: t)
    c = torch.tensor(np.float32(scale) * LOG2E)
    qs = q if tensors else rnd(q * c)

    def scores(keys):
        s = qs @ keys.t()
        return s * c if tensors else s
    m, l, o = torch.full((n,), -math.inf, dtype=f), torch.zeros(n, dtype=f), torch.zeros(n, hd, dtype=f)
    T = -(-n // 64)
    for kt in range(T):
        ks, vs = k[64 * kt:64 * kt + 64], v[64 * kt:64 * kt + 64]
        s = scores(ks)
        if fault == 'mask_last_key' and kt == T - 1:
            s[:, -1] = -math.inf
        m_new = torch.maximum(m, s.max(1).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - m_new[:, None])
        l = (l if fault == 'no_l_rescale' else l * alpha) + p.sum(1)
        if fault != 'no_o_rescale':
            o = o * alpha[:, None]
        o = o + rnd(p) @ vs
        m = m_new
    out = store(o * (1.0 / l)[:, None])
    lse = m + torch.log2(l) if fault == 'lse_log2' else m * torch.tensor(LN2) + torch.log(l)
    delta = (do * out).sum(1)
    p = torch.exp2(scores(k) - (lse * torch.tensor(LOG2E))[:, None])
    dS = p * (do @ v.t() - delta[:, None])
    dSq = dS.clone()
    if fault == 'dq_skip_last_key':
        dSq[:, -1] = 0
    dq = (rnd(dSq) @ k) * np.float32(scale)
    if fault == 'dkv_skip_last_query':
        p, dS = p.clone(), dS.clone()
        p[-1], dS[-1] = 0, 0
    dk = (rnd(dS).t() @ q) * np.float32(scale) if tensors else (rnd(dS).t() @ qs) * torch.tensor(LN2)
    dv = rnd(p).t() @ do
    return SimpleNamespace(out=out, lse=lse, dq=store(dq), dk=store(dk), dv=store(dv))


def emulate(c, flow, fault=None):
    """the restated device arithmetic on a case: float64 copies of the fp32 (bf16) results, laid out like `reference`"""
    r = _blank(c)
    sc = scale_of(c.hd)
    for o, ln, h, q, k, v, do in _heads(c):
        if ln == 0:
            continue
        s = _emulate_scene(q.contiguous(), k.contiguous(), v.contiguous(), do.contiguous(), sc, flow, fault)
        sl = slice(h * c.hd, (h + 1) * c.hd)
        for nm in ('out', 'dq', 'dk', 'dv'):
            getattr(r, nm)[o:o + ln, sl] = getattr(s, nm).double()
        r.lse[h, o:o + ln] = s.lse.double()
    return r
