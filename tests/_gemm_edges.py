"""Shared cases of the decoder-GEMM edge tests (tests/test_gemm_edges_cpu.py, tests/test_gpu_gemm_edges.py): the NT kernels
(csrc/gemm.hip gemm_nt_k / gemm_nt_x3_k, csrc/gemm_b16.hip gemm_nt_b16_k) with their six epilogues, the TN kernels (gemm_tn_k,
gemm_tn_x3_k, gemm_tn_bf16_k, gemm_tn_b16_k) with their row splits and the fixed-order reduce.

Shapes are chosen THROUGH the host-only plan queries (include/u3d.h u3d_gemm_*_plan: the function the launch itself takes its decision
from), so every list below is known to run the (kernel, tile, split situation) it is meant for; a shape whose plan is not the wanted
one raises.  Two value kinds: 'exact' (integers in [-2, 2]: every product and partial sum is an integer below 2^24, exact in bf16 and
under the three-plane split, so EVERY kernel form must return the integer result bit for bit) and 'randn' (sigma 1, weights 0.1).
References are float64; the acceptance bounds are rounding bounds of the operation, none of them comes from a measurement:

  * product bound: gamma_2(n + 4) * abs_ref, gamma_2(k) = k 2u / (1 - k 2u) with 2u = 2^-23 per accumulated term (Higham, Accuracy and
    Stability of Numerical Algorithms, 3.1, with ONE ULP instead of half an ulp per term: nothing in this project documents how the
    MFMA accumulator rounds, and one ulp a term also covers an accumulator that truncates); n = K for NT, M for TN (any split of the
    rows and any order of the reduce is a summation of the same M terms); + 4: the low-order tile's final add, the bias, the addend,
    the reduce's last level.  abs_ref is the same expression over absolute values, bias and addend included;
  * three-plane kernels: + 2^-22 abs_ref, the dropped cross terms m.l + l.m + l.l (csrc/u3d_common.h at split3_pair);
  * bf16 operands / bf16 tensors: compared with the float64 product of the RNE-rounded operands under the same bound; a bf16 C adds
    half a bf16 ulp of the fp32 value it was rounded from;
  * column sums: gamma(M) * sum |A| with u = 2^-24 (VALU additions, round to nearest);
  * GELU: `pre` is held to the product bound; the activation to 1e-5 of the largest reference element (the project's criterion for
    gelu_f, tests/test_gpu_kernels.py test_mlp_fused_epilogues_fwd_bwd), against float64 GELU of the device's own pre / aux.
The random-value bounds are worst-case bounds and grow with the depth: gamma_2(M + 4) of a TN product over M ~ 16k rows is 2e-3 of
abs_ref, which a single lost or doubled row stays inside (tests/test_gemm_edges_cpu.py prints this).  At large M only the 'exact' kind
guards against single-row losses, which is why every shape runs with both kinds.
Nothing here touches a GPU."""
from __future__ import annotations

import ctypes as C
import math
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24
KINDS = ('exact', 'randn')
NATIVE, X3, B16 = 0, 1, 2                         # include/u3d.h U3D_GEMM_NATIVE / _X3 / _B16
BF16_OPERANDS = 16                                # include/u3d.h U3D_BF16_OPERANDS
A16, B16F, C16 = 1, 2, 4                          # include/u3d.h U3D_A_BF16 / U3D_B_BF16 / U3D_C_BF16
EINVAL, EUNSUPPORTED = -1, -3
GELU_TOL = 1e-5
TILES = ((128, 128), (128, 64), (64, 64))
# kernel form -> (fp32 math mode it needs or None, kernel family, K-step, the tiles the dispatcher can give it)
NT_FORMS = {
    'native': ('mfma', NATIVE, 16, TILES),        # gemm_nt_k
    'x3': ('bf16x3', X3, 32, TILES[1:]),          # gemm_nt_x3_k<.., WP = false>
    'x3_planes': ('bf16x3', X3, 32, TILES[1:]),   # gemm_nt_x3_k<.., WP = true>: W passed as planes of u3d_weight_planes_batch
    'bf16op': (None, B16, 32, TILES),             # gemm_nt_b16_k<.., false, false> on gemm.hip's tile choice (U3D_BF16_OPERANDS)
    'b16': (None, B16, 32, TILES),                # gemm_nt_b16_k through u3d_gemm_nt_b16: its own tile choice, four dtype combinations
}
TN_FORMS = {
    'native': ('mfma', NATIVE, 16, (64, 128)),    # gemm_tn_k<64> / <128>
    'x3': ('bf16x3', X3, 32, (64, 128)),          # gemm_tn_x3_k<64, 64> / <128, 64>
    'bf16op': (None, B16, 32, (128,)),            # gemm_tn_bf16_k
    'b16': (None, B16, 32, (128,)),               # gemm_tn_b16_k, four dtype combinations
}
NT16_FLAGS = (0, A16, C16, A16 | C16)
TN16_FLAGS = (0, A16, B16F, A16 | B16F)
# epilogues of the fp32-tensor entry points: epi -> (entry point, act); u3d_ffn_fwd runs 1 / 2 followed by 0
EPI_ENTRY = {0: ('u3d_gemm_nt', 0), 1: ('u3d_linear_act', 1), 2: ('u3d_linear_act', 2), 3: ('u3d_linear_dact', 1),
             4: ('u3d_linear_dact', 2), 5: ('u3d_gemm_nt_add', 0)}


def gamma2(k):
    """k 2u / (1 - k 2u): k accumulated terms at one fp32 ulp each"""
    ku = np.asarray(k, np.float64) * 2 * U
    return ku / (1.0 - ku)


def gamma(k):
    ku = np.asarray(k, np.float64) * U
    return ku / (1.0 - ku)


def rne(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> the fp32 value of its bf16 rounding (round to nearest even: torch's conversion)"""
    return t.float().to(torch.bfloat16).float()


def half_ulp_bf16(mag: torch.Tensor) -> torch.Tensor:
    """half a bf16 ulp at magnitude `mag` (float64): 2^(floor(log2 mag) - 8), 0 at 0"""
    m = mag.double().abs()
    e = torch.floor(torch.log2(torch.where(m > 0, m, torch.ones_like(m))))
    return torch.where(m > 0, torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 8), torch.zeros_like(m))


# ============================================================================================================ plan queries
@contextmanager
def math_mode(mode):
    from unidet3d_amd import precision as P
    if mode is None:
        yield
    else:
        with P.fp32_math(mode):
            yield


def _lib():
    from unidet3d_amd import _lib as L
    return L.lib()


def nt_plan(M, N, K, flags=0):
    """(status, kernel family, tile_m, tile_n) of a u3d_gemm_nt-family call under the CURRENT fp32 math mode"""
    k, a, b = C.c_int(-1), C.c_int(0), C.c_int(0)
    rc = _lib().u3d_gemm_nt_plan(M, N, K, flags, C.byref(k), C.byref(a), C.byref(b))
    return rc, k.value, a.value, b.value


def nt16_plan(M, N, K, epi=0, flags=0):
    a, b = C.c_int(0), C.c_int(0)
    rc = _lib().u3d_gemm_nt_b16_plan(M, N, K, epi, flags, C.byref(a), C.byref(b))
    return rc, B16, a.value, b.value


@dataclass(frozen=True)
class TnPlan:
    rc: int
    kernel: int
    tile_n: int
    tile_k: int
    splits: int
    rows_per_split: int
    M: int

    @property
    def used(self):
        """splits that hold at least one row"""
        return -(-self.M // self.rows_per_split)

    @property
    def empty(self):
        return self.splits - self.used

    @property
    def last_rows(self):
        """rows of the last split that holds any"""
        return self.M - (self.used - 1) * self.rows_per_split


def tn_plan(M, N, K, bf=0) -> TnPlan:
    k, a, b, s, r = C.c_int(-1), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    rc = _lib().u3d_gemm_tn_plan(M, N, K, bf, C.byref(k), C.byref(a), C.byref(b), C.byref(s), C.byref(r))
    return TnPlan(rc, k.value, a.value, b.value, s.value, max(r.value, 1), M)


def tn16_plan(M, N, K, flags=0) -> TnPlan:
    a, b, s, r = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    rc = _lib().u3d_gemm_tn_b16_plan(M, N, K, flags, C.byref(a), C.byref(b), C.byref(s), C.byref(r))
    return TnPlan(rc, B16, a.value, b.value, s.value, max(r.value, 1), M)


def nt_form_plan(form, M, N, K, epi=0, flags=0):
    """plan of `form` at a shape, under the math mode the form needs"""
    mode = NT_FORMS[form][0]
    with math_mode(mode):
        if form == 'b16':
            return nt16_plan(M, N, K, epi, flags)
        return nt_plan(M, N, K, BF16_OPERANDS if form == 'bf16op' else 0)


def tn_form_plan(form, M, N, K, flags=0) -> TnPlan:
    with math_mode(TN_FORMS[form][0]):
        if form == 'b16':
            return tn16_plan(M, N, K, flags)
        return tn_plan(M, N, K, 1 if form == 'bf16op' else 0)


def _need_nt(form, tile, shapes):
    """the shapes, after checking that each one runs `form` on `tile`"""
    fam = NT_FORMS[form][1]
    for M, N, K in shapes:
        got = nt_form_plan(form, M, N, K)
        if got != (0, fam, *tile):
            raise AssertionError(f'NT {form}: shape {(M, N, K)} is planned as {got}, wanted kernel {fam} on tile {tile}')
    return list(shapes)


# ============================================================================================================ NT shape lists
def _sweeps(TM, TN_, K):
    """an M sweep at one ragged N and an N sweep at one ragged M (not the cross product)"""
    ms = sorted({1, 31, 32, 33, TM // 2, TM // 2 + 1, TM - 1, TM, TM + 1, 2 * TM + 1})
    ns = sorted({1, 4, 19, 31, 32, 33, TN_ // 2 + 1, TN_ - 1, TN_, TN_ + 1, 2 * TN_ + 2})
    return [(m, 19, K) for m in ms] + [(33, n, K) for n in ns]


# tiles the cost models pick only at size: the smallest shapes that select them (evaluated with the queries; K = 32 keeps the float64
# reference cheap).  (M, N): ragged rows with full columns, ragged both, ragged columns.
_BIG = {
    ('native', (128, 128)): [(3201, 1024), (3199, 1000), (3073, 1021)],
    ('native', (128, 64)): [(1153, 1024), (1151, 1000)],
    ('bf16op', (128, 128)): [(3201, 1024), (3199, 1000), (3073, 1021)],
    ('bf16op', (128, 64)): [(1153, 1024), (1151, 1000)],
    ('x3', (128, 64)): [(1153, 1024), (4097, 19)],
    ('x3_planes', (128, 64)): [(1153, 1024), (4097, 19)],
    ('b16', (128, 128)): [(4097, 1024), (4095, 1000)],
    ('b16', (128, 64)): [(2049, 1024), (32769, 20)],
}


def nt_tile_shapes(form, tile):
    """[(M, N, K)] that run `form` on `tile`: the literal sweeps for 64 x 64, the smallest selecting shapes for the large tiles"""
    K = 32
    if tile == (64, 64):
        shapes = _sweeps(64, 64, K)
        if form == 'b16':                         # a bf16 C needs an even N: the M sweep once more at N = 20 (its row-pair stores at odd M)
            shapes += [(m, 20, k) for m, n, k in shapes if n == 19]
        return _need_nt(form, tile, shapes)
    return _need_nt(form, tile, [(M, N, K) for M, N in _BIG[(form, tile)]])


def nt_ragged_shape(form, tile):
    """one shape of the tile that is ragged in rows AND columns, more than one workgroup (the epilogue tests)"""
    if tile == (64, 64):
        return _need_nt(form, tile, [(65, 66, 32)])[0]
    M, N = {(128, 128): {'b16': (4095, 1000)}.get(form, (3199, 1000)),
            (128, 64): {'b16': (2049, 1000)}.get(form, (1151, 1000))}[tile]
    return _need_nt(form, tile, [(M, N, 32)])[0]


def nt_k_steps(form):
    """one to five K-steps of the form's kernel: prologue only, the peeled step, the loop body once, twice, three times"""
    ks = NT_FORMS[form][2]
    return _need_nt(form, (64, 64), [(65, 33, ks * i) for i in range(1, 6)])


ROUTE_KS = (16, 48, 80)                            # K = 16 (mod 32) under bf16x3 silently takes the native kernel
GRID_WGS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17)  # every remainder of xcd_swizzle


def nt_grid_shapes(form):
    """g workgroups of 64 x 64 (two column tiles where g is even), ragged in both directions"""
    out = []
    for g in GRID_WGS:
        rows, cols = (g // 2, 2) if g % 2 == 0 else (g, 1)
        out.append((64 * (rows - 1) + 5, 64 * (cols - 1) + 40, 32))
    return _need_nt(form, (64, 64), out)


# ============================================================================================================ TN shape lists
TN_ROWS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
TN_SMALL_N = (4, 20, 60, 64, 68, 132)
TN_SMALL_K = (4, 36, 64, 68, 132)
TN_BIG = ((512, 512), (1024, 256), (516, 772))    # 16+ tiles of 128 x 128: the 128 tiles of gemm_tn_k / gemm_tn_x3_k
TN_LAST_SPLIT_ONE_ROW = (513, 641, 1025)          # at N = K = 64
TN_LAST_EMPTY = (2049, 512, 768)
TN_CAP = (32769, 64, 64)                          # 256 splits (the cap), many of them wholly past M


def _r8(v, q):
    return -(-v // q) * q


def tn_tile_shapes(form, T, flags=0):
    """[(M, N, K)] that run `form` with output tiles of T rows.  N / K are rounded up to the granule a bf16 operand needs."""
    qa, qb = (8 if flags & A16 else 4), (8 if flags & B16F else 4)
    if T == 128 and form in ('native', 'x3'):
        shapes = [(65, _r8(n, qa), _r8(k, qb)) for n, k in TN_BIG]
    else:
        shapes = [(33, _r8(n, qa), _r8(68, qb)) for n in TN_SMALL_N] + [(33, _r8(20, qa), _r8(k, qb)) for k in TN_SMALL_K]
    for s in shapes:
        p = tn_form_plan(form, *s, flags=flags)
        if p.rc != 0 or p.tile_n != T or p.kernel != TN_FORMS[form][1]:
            raise AssertionError(f'TN {form}: shape {s} is planned as {p}, wanted tile {T}')
    return shapes


def tn_row_shapes(form, flags=0):
    """one split with one and two trips and ragged trips; last split of one row; empty splits; the cap of 256 splits"""
    qa, qb = (8 if flags & A16 else 4), (8 if flags & B16F else 4)
    out = [(m, _r8(20, qa), _r8(36, qb)) for m in TN_ROWS]
    out += [(m, 64, 64) for m in TN_LAST_SPLIT_ONE_ROW]
    out += [TN_LAST_EMPTY, TN_CAP]
    for s in out:
        p = tn_form_plan(form, *s, flags=flags)
        if p.rc != 0:
            raise AssertionError(f'TN {form}: shape {s} is refused ({p.rc})')
    return out


# ============================================================================================================ inputs
def _seed(*v):
    s = 0
    for x in v:
        s = (s * 1_000_003 + int(x)) % (2 ** 31 - 1)
    return s


def _vals(rng, kind, shape, sigma=1.0):
    if kind == 'exact':
        return torch.from_numpy(rng.integers(-2, 3, shape).astype(F32))
    return torch.from_numpy((rng.standard_normal(shape) * sigma).astype(F32))


@dataclass
class NtCase:
    kind: str
    M: int
    N: int
    K: int
    A: torch.Tensor                               # fp32 [M, K]
    W: torch.Tensor                               # fp32 [N, K]
    bias: torch.Tensor                            # fp32 [N]
    aux: torch.Tensor                             # fp32 [M, N]: addend (epi 5), GELU pre-activation (4); relu(aux) is the ReLU output (3)


def nt_case(kind, M, N, K) -> NtCase:
    rng = np.random.default_rng(_seed(1, KINDS.index(kind), M, N, K))
    return NtCase(kind, M, N, K, _vals(rng, kind, (M, K)), _vals(rng, kind, (N, K), 0.1), _vals(rng, kind, (N,)),
                  _vals(rng, kind, (M, N)))


@dataclass
class TnCase:
    kind: str
    M: int
    N: int
    K: int
    A: torch.Tensor                               # fp32 [M, N]
    B: torch.Tensor                               # fp32 [M, K]


def tn_case(kind, M, N, K) -> TnCase:
    rng = np.random.default_rng(_seed(2, KINDS.index(kind), M, N, K))
    return TnCase(kind, M, N, K, _vals(rng, kind, (M, N)), _vals(rng, kind, (M, K)))


# ============================================================================================================ references
def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def nt_operands(case: NtCase, bf16: bool, aux_bf16: bool = False):
    """float64 (A, W, bias, aux) as the kernel form sees them: A and W RNE-rounded for a bf16 form (bias stays fp32)"""
    A, W = (rne(case.A), rne(case.W)) if bf16 else (case.A, case.W)
    aux = rne(case.aux) if aux_bf16 else case.aux
    return A.double(), W.double(), case.bias.double(), aux.double()


def nt_ref(case: NtCase, epi: int, with_bias: bool = True, bf16: bool = False, aux_bf16: bool = False):
    """(ref, abs_ref, factor) float64 [M, N].  ref is what the product bound applies to: the result for epi 0, 1, 3, 5, `pre` for
    epi 2, the product BEFORE the gelu' factor for epi 4 (factor = gelu'(aux), else None)."""
    A, W, b, aux = nt_operands(case, bf16, aux_bf16)
    return nt_epilogue_ref(A @ W.t(), A.abs() @ W.abs().t(), b, aux, epi, with_bias)


def nt_epilogue_ref(acc, aacc, b, aux, epi: int, with_bias: bool = True):
    """nt_ref from the float64 products A W^T and |A| |W|^T (on any device: a test that runs many epilogues on one large case forms
    the products once)"""
    if with_bias and epi in (0, 1, 2):
        acc, aacc = acc + b, aacc + b.abs()
    if epi == 1:
        acc = acc.clamp(min=0)
    elif epi == 3:
        keep = (aux.clamp(min=0) > 0).double()
        acc, aacc = acc * keep, aacc * keep
    elif epi == 5:
        acc, aacc = acc + aux, aacc + aux.abs()
    return acc, aacc, (gelu_grad64(aux) if epi == 4 else None)


def nt_bound(abs_ref, K, x3: bool):
    return (float(gamma2(K + 4)) + (2.0 ** -22 if x3 else 0.0)) * abs_ref


def tn_ref(case: TnCase, a_bf16: bool = False, b_bf16: bool = False):
    """(C [N, K], abs C, column sums of A [N], sum |A| [N]) float64; the column sums come from the unrounded fp32 A"""
    A = (rne(case.A) if a_bf16 else case.A).double()
    B = (rne(case.B) if b_bf16 else case.B).double()
    return A.t() @ B, A.abs().t() @ B.abs(), case.A.double().sum(0), case.A.double().abs().sum(0)


def tn_bound(abs_ref, M, x3: bool):
    return (float(gamma2(M + 4)) + (2.0 ** -22 if x3 else 0.0)) * abs_ref


def colsum_bound(abs_sum, M):
    return float(gamma(M)) * abs_sum


def margin(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """worst error / bound (tests/_segments.py margin): inf when an element with bound 0 is not met exactly or is not finite"""
    g = got.double()
    err = (g - ref).abs()
    if not bool(torch.isfinite(g).all()) or bool(((err > bound) & (bound == 0)).any()):
        return float('inf')
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def max_norm_ratio(got, ref) -> float:
    """the criterion of the workload-shaped tests (tests/_parity.py rel): largest error over the largest reference element"""
    return float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-12))


# ============================================================================================================ emulation (numpy fp32)
def split3(x: np.ndarray):
    """csrc/u3d_common.h split3_pair as restated in tests/test_bf16x3_split_cpu.py"""
    x = x.astype(F32)
    h = ((x.view(np.uint32) + np.uint32(0x8000)) & np.uint32(0xffff0000)).view(F32)
    r1 = (x - h).astype(F32)
    m = (r1.view(np.uint32) & np.uint32(0xffff0000)).view(F32)
    return h, m, (r1 - m).astype(F32)


def _seq_dot(P, Q, x3=False):
    """out[i, j] = sum_t P[t, i] Q[t, j], one fp32 rounding per product and per addition, t ascending.  x3: the six plane products
    of the three-plane kernels -- h.h into the main accumulator, the five low-order ones into a second one, added at the end."""
    P, Q = P.astype(F32), Q.astype(F32)
    acc = np.zeros((P.shape[1], Q.shape[1]), F32)
    if not x3:
        for t in range(P.shape[0]):
            acc = acc + P[t][:, None] * Q[t][None, :]
        return acc
    lo = np.zeros_like(acc)
    ph, pm, pl = split3(P)
    qh, qm, ql = split3(Q)
    for t in range(P.shape[0]):
        for a, b in ((ph, ql), (pm, qm), (pl, qh), (ph, qm), (pm, qh)):
            lo = lo + a[t][:, None] * b[t][None, :]
        acc = acc + ph[t][:, None] * qh[t][None, :]
    return acc + lo


def nt_emulate(case: NtCase, epi: int, family: int, with_bias=True, c_bf16=False) -> torch.Tensor:
    """fp32 sequential sums over k, then the epilogue in fp32 (epi 0, 1, 3, 5; the GELU epilogues share epi 0's arithmetic up to
    `pre`).  family B16: operands RNE-rounded first."""
    A, W = case.A, case.W
    if family == B16:
        A, W = rne(A), rne(W)
    acc = _seq_dot(A.numpy().T.copy(), W.numpy().T.copy(), family == X3)
    if with_bias and epi in (0, 1, 2):
        acc = acc + case.bias.numpy()[None, :]
    aux = (rne(case.aux) if c_bf16 else case.aux).numpy()
    if epi == 1:
        acc = np.maximum(acc, F32(0))
    elif epi == 3:
        acc = np.where(np.maximum(aux, 0) > 0, acc, F32(0))
    elif epi == 5:
        acc = acc + aux
    out = torch.from_numpy(acc.astype(F32))
    return rne(out) if c_bf16 else out


def tn_emulate(case: TnCase, plan: TnPlan, family: int, a_bf16=False, b_bf16=False):
    """(C, column sums): per split an fp32 sequential sum over its rows, then the reduce's order -- four interleaved running sums
    over the splits, the tail into the first, (v0 + v1) + (v2 + v3)"""
    A = rne(case.A) if (family == B16 or a_bf16) else case.A
    B = rne(case.B) if (family == B16 or b_bf16) else case.B
    A, B, A32 = A.numpy(), B.numpy(), case.A.numpy()
    S, rps = plan.splits, plan.rows_per_split
    parts, sums = [], []
    for s in range(S):
        lo, hi = min(case.M, s * rps), min(case.M, (s + 1) * rps)
        parts.append(_seq_dot(A[lo:hi], B[lo:hi], family == X3))
        cs = np.zeros(case.N, F32)
        for r in range(lo, hi):
            cs = cs + A32[r]
        sums.append(cs)

    def reduce(ps):
        v = [np.zeros_like(ps[0]) for _ in range(4)]
        s = 0
        while s + 4 <= S:
            for u in range(4):
                v[u] = v[u] + ps[s + u]
            s += 4
        while s < S:
            v[0] = v[0] + ps[s]
            s += 1
        return (v[0] + v[1]) + (v[2] + v[3])
    return torch.from_numpy(reduce(parts)), torch.from_numpy(reduce(sums))


# ============================================================================================================ mutants
def nt_mutants(case: NtCase, tile, kstep: int, bf16=False):
    """Plausible wrong results in float64: (name, epi it is a wrong result of, wrong [M, N]).  A mutant that would not alter this
    case (no ragged tile, one K-step ...) is not yielded."""
    TM, TN_ = tile
    A, W, b, aux = nt_operands(case, bf16)
    M, N, K = case.M, case.N, case.K
    ref = A @ W.t() + b
    if K > kstep:
        yield 'last_k_step_dropped', 0, ref - A[:, K - kstep:] @ W[:, K - kstep:].t()
    if M % TM >= 2:
        w = ref.clone()
        w[M - 1] = w[M - 2]
        yield 'last_row_of_ragged_row_tile_repeats_the_row_before', 0, w
    w = ref.clone()
    for j in range(0, N, 32):
        w[:, j:j + 32] += b[j] - b[j:j + 32]
    yield 'bias_of_the_first_column_of_a_32_column_block', 0, w
    n0 = N // TN_ * TN_
    if 0 < n0 < N:
        w = ref.clone()
        w[:, n0:] = A @ W[:N - n0].t() + b[n0:]
        yield 'ragged_column_tile_reads_w_rows_of_tile_0', 0, w
    flat = torch.cat([aux.flatten(), torch.zeros(M, dtype=torch.float64)])
    idx = (torch.arange(M)[:, None] * (N + 1) + torch.arange(N)[None, :])
    yield 'aux_row_stride_n_plus_1', 5, A @ W.t() + flat[idx]


def tn_mutants(case: TnCase, plan: TnPlan, trip: int):
    """(name, wrong C [N, K] or None, wrong column sums [N] or None) in float64, built on the plan's splits"""
    A, B = case.A.double(), case.B.double()
    M, S, rps, used = case.M, plan.splits, plan.rows_per_split, plan.used
    ref = A.t() @ B

    def rows_prod(idx):
        idx = torch.as_tensor(idx, dtype=torch.int64)
        return A[idx].t() @ B[idx]
    drop = []
    for s in range(used):
        lo, hi = s * rps, min(M, (s + 1) * rps)
        drop += list(range(lo + (hi - lo - 1) // trip * trip, hi))
    yield 'last_trip_of_every_split_dropped', ref - rows_prod(drop), None
    lo = (used - 1) * rps
    if (M - lo) % trip:
        yield 'ragged_rows_of_the_last_split_dropped', ref - rows_prod(list(range(lo + (M - lo) // trip * trip, M))), None
    if used > 1:
        yield 'first_row_of_the_next_split_counted_twice', ref + rows_prod([s * rps for s in range(1, used)]), None
        s = used // 2
        yield 'one_split_left_out_of_the_reduce', ref - rows_prod(list(range(s * rps, min(M, (s + 1) * rps)))), None
    tail0 = (S - S % 4) * rps
    if S % 4 and tail0 < M:
        yield 'reduce_tail_left_out', ref - rows_prod(list(range(tail0, M))), None
    yield 'column_sums_miss_the_last_split', None, A.sum(0) - A[lo:].sum(0)


# ============================================================================================================ small kernels
TRANSPOSE_SHAPES = ((1, 1), (31, 33), (32, 32), (33, 65), (256, 19))
TRANSPOSE_BATCH = ((33, 65), (1, 40), (64, 32))
PLANES_BATCH = (8, 2056, 264)                     # values per matrix (multiples of 8): one thread, nine blocks (ragged), two blocks
GELU_SIZES = (4, 1020, 1024, 1028)
GELU16_SIZES = (8, 2040, 2048, 2056)              # the bf16 passes take 8 values per thread: around one block of 256 threads
AUTOGRAD_N = (1, 5, 17, 33, 47)
AUTOGRAD_K = (16, 48, 80)


def planes_ref(w: torch.Tensor) -> torch.Tensor:
    """int16 [3, n]: the bit patterns of the three bf16 planes of an fp32 tensor (numpy split3)"""
    h, m, l = split3(w.numpy().reshape(-1))
    return torch.from_numpy(np.stack([(p.view(np.uint32) >> np.uint32(16)).astype(np.uint16).view(np.int16) for p in (h, m, l)]))
