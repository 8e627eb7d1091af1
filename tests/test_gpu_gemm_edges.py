"""The decoder GEMMs (csrc/gemm.hip, csrc/gemm_b16.hip) at every tile, K-step, epilogue and split edge, through the C ABI: every
NT kernel form on every tile its dispatcher can choose (M and N sweeps around the tile, the smallest shapes that select the large
tiles, one to five K-steps, every remainder of the XCD swizzle, all epilogues with and without bias, W passed as pre-split planes),
every TN kernel form (tiles, one and two ragged trips, a last split of one row, empty splits, the cap of 256 splits, the reduce's
four-way unroll and tail, column sums, the four dtype combinations), the small kernels next to them, and dense.linear / dense.mlp at
the widths that run the zero-padding of the reduction depth.

Shapes, float64 references, bounds and their derivations come from tests/_gemm_edges.py (checked on the host by
tests/test_gemm_edges_cpu.py); which kernel and tile a shape runs is what the host plan queries report.  Every call: the outputs lie
in an allocation with N_GUARD sentinel rows behind them (untouched afterwards) and are pre-filled with NaN (finite afterwards), the
operands have NaN rows behind their last row, the TN workspace is NaN, integer-valued cases match bit for bit, random ones are inside
the elementwise bound, a second run gives the same bits and the inputs are unchanged."""
import numpy as np
import pytest
import torch

import _gemm_edges as GE
from _parity import log_errors

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = -12288.0                                 # exact in bf16
N_GUARD = 8
NAN = float('nan')
BF = torch.bfloat16


def _in(t, dtype=torch.float32):
    """device copy of a 1-D / 2-D operand with N_GUARD rows of NaN behind its last row, in one allocation"""
    t = t.to(dtype)
    full = torch.full((t.shape[0] + N_GUARD, *t.shape[1:]), NAN, dtype=dtype, device=DEV)
    full[:t.shape[0]] = t.to(DEV)
    return full


def _out(rows, cols, dtype=torch.float32):
    full = torch.full((rows + N_GUARD, cols), GUARD, dtype=dtype, device=DEV)
    full[:rows] = NAN
    return full


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same(a, b):
    """bitwise, NaN included"""
    return torch.equal(_bits(a), _bits(b))


def _guard_ok(full, rows):
    return bool((full[rows:] == GUARD).all()) and bool(torch.isfinite(full[:rows].float()).all())


# ============================================================================================================ NT through the C ABI
def _planes(w_full, N, K):
    """bf16 [3 * N * K] (+ sentinel tail) planes of W, written by u3d_weight_planes_batch"""
    from unidet3d_amd import _lib as L
    n = N * K
    pl = torch.full((3 * n + 64,), GUARD, dtype=BF, device=DEV)
    desc = torch.tensor([[w_full.data_ptr(), pl.data_ptr(), n // 8, 0]], dtype=torch.int64, device=DEV)
    L.call('u3d_weight_planes_batch', L.ptr(desc), 1, (n // 8 + 255) // 256, L.stream())
    assert bool((pl[3 * n:] == GUARD).all())
    return pl


def _run_nt(form, case, epi, with_bias=True, flags=0):
    """-> (C [M, N], pre [M, N] or None) device views after the checks every call gets"""
    from unidet3d_amd import _lib as L
    M, N, K = case.M, case.N, case.K
    a16, c16 = form == 'b16' and bool(flags & GE.A16), form == 'b16' and bool(flags & GE.C16)
    A, W = _in(case.A, BF if a16 else torch.float32), _in(case.W)
    bias = _in(case.bias) if with_bias and epi in (0, 1, 2) else None
    aux_host = case.aux.clamp(min=0) if epi == 3 else case.aux
    aux = _in(aux_host, BF if (c16 and epi == 3) else torch.float32) if epi >= 3 else None
    keep = [t.clone() for t in (A, W) + ((bias,) if bias is not None else ()) + ((aux,) if aux is not None else ())]
    outs = []
    with GE.math_mode(GE.NT_FORMS[form][0]):
        planes = _planes(W, N, K) if form == 'x3_planes' else None
        for _ in range(2):
            Cf = _out(M, N, BF if c16 else torch.float32)
            pre = _out(M, N) if epi == 2 else None
            s = L.stream()
            if form == 'b16':
                L.call('u3d_gemm_nt_b16', L.ptr(A), L.ptr(W), L.ptr(bias), epi, L.ptr(aux), L.ptr(Cf), flags, M, N, K, 0.0, s)
            else:
                f = GE.BF16_OPERANDS if form == 'bf16op' else 0
                name, act = GE.EPI_ENTRY[epi]
                if epi == 0 and f == 0:
                    L.call('u3d_gemm_nt', L.ptr(A), L.ptr(W), L.ptr(bias), L.ptr(Cf), M, N, K, L.ptr(planes), 0.0, s)
                elif epi in (0, 1, 2):
                    L.call('u3d_linear_act', L.ptr(A), L.ptr(W), L.ptr(bias), epi | f, L.ptr(pre), L.ptr(Cf), M, N, K, L.ptr(planes), 0.0, s)
                elif epi in (3, 4):
                    L.call('u3d_linear_dact', L.ptr(A), L.ptr(W), L.ptr(aux), act | f, L.ptr(Cf), M, N, K, L.ptr(planes), 0.0, s)
                else:
                    L.call('u3d_gemm_nt_add', L.ptr(A), L.ptr(W), L.ptr(aux), f, L.ptr(Cf), M, N, K, L.ptr(planes), 0.0, s)
            what = (form, (M, N, K), epi, with_bias, flags, case.kind)
            assert _guard_ok(Cf, M), ('C: guard rows touched or interior not finite', what)
            assert pre is None or _guard_ok(pre, M), ('pre: guard rows touched or interior not finite', what)
            outs.append((Cf[:M], None if pre is None else pre[:M]))
    assert _same(outs[0][0], outs[1][0]) and (outs[0][1] is None or _same(outs[0][1], outs[1][1])), ('second run differs', what)
    now = (A, W) + ((bias,) if bias is not None else ()) + ((aux,) if aux is not None else ())
    assert all(_same(x, y) for x, y in zip(keep, now)), ('an input was modified', what)
    return outs[0]


_PRODUCTS = {}


def _nt_ref_dev(case, epi, with_bias, bf16, aux_bf16):
    """GE.nt_ref on the device; the float64 products of a case are formed once (on the host) and shared by its epilogues"""
    key = (case.kind, case.M, case.N, case.K, bf16)
    if key not in _PRODUCTS:
        if len(_PRODUCTS) >= 4:
            _PRODUCTS.clear()
        A, W, _, _ = GE.nt_operands(case, bf16)
        _PRODUCTS[key] = ((A @ W.t()).to(DEV), (A.abs() @ W.abs().t()).to(DEV))
    acc, aacc = _PRODUCTS[key]
    aux = (GE.rne(case.aux) if aux_bf16 else case.aux).to(DEV).double()
    return GE.nt_epilogue_ref(acc, aacc, case.bias.to(DEV).double(), aux, epi, with_bias)


def _check_nt(form, case, epi, with_bias=True, flags=0):
    """runs the call and compares on the device; -> worst error / bound (0 for an exact case, which must match bit for bit).
    Epilogue 4 (C = acc * gelu'(aux)) is the exception: the product before the gelu' factor is not observable, so the whole result is
    held to (product bound) * |gelu'(aux)| + 1e-5 of the largest reference element -- in effect the GELU max-norm criterion, also for
    the integer-valued case (its product bound is 0, gelu' is not an integer).  The product itself is held elementwise and bit for bit
    by the five other epilogues on the same shapes."""
    a16, c16 = form == 'b16' and bool(flags & GE.A16), form == 'b16' and bool(flags & GE.C16)
    family = GE.NT_FORMS[form][1]
    C, pre = _run_nt(form, case, epi, with_bias, flags)
    ref, aref, factor = _nt_ref_dev(case, epi, with_bias, family == GE.B16, c16 and epi == 3)
    bound = GE.nt_bound(aref, case.K, family == GE.X3) if case.kind == 'randn' else torch.zeros_like(aref)
    what = (form, (case.M, case.N, case.K), epi, with_bias, flags, case.kind)
    if epi == 2:                                   # pre by the product bound; the activation against float64 GELU of the device's pre
        m = GE.margin(pre, ref, bound)
        act = GE.gelu64(pre)
        assert float((C.double() - act).abs().max()) <= GE.GELU_TOL * float(act.abs().max()), ('gelu', what)
    elif epi == 4:                                 # the product by its bound times |gelu'(aux)|, gelu' itself by the GELU criterion
        full = ref * factor
        m = GE.margin(C, full, bound * factor.abs() + GE.GELU_TOL * float(full.abs().max()))
    elif c16:
        if case.kind == 'exact':
            m = 0.0 if torch.equal(C.float(), GE.rne(ref.float())) else float('inf')
        else:
            m = GE.margin(C.float(), ref, bound + GE.half_ulp_bf16(ref.abs() + bound))
    else:
        m = GE.margin(C, ref, bound)
    print('gemm_edges nt', what, 'worst error / bound', m)
    assert m <= 1.0, (what, m)
    return m


def _nt_tiles():
    return [(form, tile) for form, (_, _, _, tiles) in GE.NT_FORMS.items() for tile in tiles]


def _ids(v):
    return '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize('form,tile', _nt_tiles(), ids=lambda v: _ids(v))
def test_nt_every_tile_row_and_column_edge(form, tile):
    """M and N sweeps around the tile (64 x 64), the smallest shapes that select it (large tiles); plain product with bias.  The b16
    form runs its four dtype combinations (a bf16 C needs an even N; on the large tiles one combination per shape and value kind, all
    four between them -- test_nt_b16_every_epilogue_and_dtype_combination runs every one on every tile).  x3_planes must also give the bits of the in-flight split."""
    worst = 0.0
    for i, (M, N, K) in enumerate(GE.nt_tile_shapes(form, tile)):
        for j, kind in enumerate(GE.KINDS):
            case = GE.nt_case(kind, M, N, K)
            every = GE.NT16_FLAGS if tile == (64, 64) else (GE.NT16_FLAGS[(2 * i + j) % 4],)      # large tiles: the four combinations in turn
            for flags in (every if form == 'b16' else (0,)):
                if flags & GE.C16 and N % 2:
                    continue
                worst = max(worst, _check_nt(form, case, 0, True, flags))
            if form == 'x3_planes':
                assert _same(_run_nt('x3_planes', case, 0)[0], _run_nt('x3', case, 0)[0]), ('planes differ from the in-flight split', M, N, K, kind)
    log_errors('gemm_edges_nt_tiles', dict(form=form, tile=list(tile), worst_error_over_bound=worst))


@pytest.mark.parametrize('form', list(GE.NT_FORMS))
def test_nt_k_steps_and_every_grid_remainder(form):
    """one to five K-steps (prologue only, the peeled step, the loop body once, twice, three times) and 1 .. 9, 15, 16, 17
    workgroups: every remainder of xcd_swizzle"""
    worst = 0.0
    for M, N, K in GE.nt_k_steps(form) + GE.nt_grid_shapes(form):
        for kind in GE.KINDS:
            case = GE.nt_case(kind, M, N, K)
            for flags in ((0, GE.A16) if form == 'b16' else (0,)):          # an fp32 and a bf16 A are staged by different code
                worst = max(worst, _check_nt(form, case, 0, True, flags))
            if form == 'x3_planes':
                assert _same(_run_nt('x3_planes', case, 0)[0], _run_nt('x3', case, 0)[0]), (M, N, K, kind)
    log_errors('gemm_edges_nt_k_steps_grids', dict(form=form, worst_error_over_bound=worst))


def test_nt_k_16_mod_32_takes_the_native_kernel_under_the_three_plane_mode():
    """the route check: under bf16x3, K in {16, 48, 80} must give the bits of the same call under mfma"""
    worst = 0.0
    for K in GE.ROUTE_KS:
        for kind in GE.KINDS:
            case = GE.nt_case(kind, 65, 33, K)
            for epi in (0, 5):
                with GE.math_mode('bf16x3'):
                    assert GE.nt_plan(65, 33, K)[1] == GE.NATIVE
                assert _same(_run_nt('x3', case, epi)[0], _run_nt('native', case, epi)[0]), (K, kind, epi)
                worst = max(worst, _check_nt('native', case, epi))
    log_errors('gemm_edges_nt_route_k16', dict(worst_error_over_bound=worst))


@pytest.mark.parametrize('form,tile', [ft for ft in _nt_tiles() if ft[0] != 'b16'], ids=lambda v: _ids(v))
def test_nt_every_epilogue_on_every_tile(form, tile):
    """all six epilogues through u3d_gemm_nt / u3d_linear_act / u3d_linear_dact / u3d_gemm_nt_add at a shape of the tile that is
    ragged in rows and columns, with and without bias"""
    M, N, K = GE.nt_ragged_shape(form, tile)
    worst = {}
    for kind in GE.KINDS:
        case = GE.nt_case(kind, M, N, K)
        for epi in range(6):
            for with_bias in ((True, False) if epi <= 2 else (False,)):
                m = _check_nt(form, case, epi, with_bias)
                worst[epi] = max(worst.get(epi, 0.0), m)
                if form == 'x3_planes':
                    assert _same(_run_nt('x3_planes', case, epi, with_bias)[0], _run_nt('x3', case, epi, with_bias)[0]), (epi, with_bias, kind)
    log_errors('gemm_edges_nt_epilogues', dict(form=form, tile=list(tile), worst_error_over_bound={str(k): v for k, v in worst.items()}))


@pytest.mark.parametrize('tile', GE.TILES, ids=lambda v: _ids(v))
def test_nt_b16_every_epilogue_and_dtype_combination(tile):
    """u3d_gemm_nt_b16 at epi {0, 1, 3, 5} x flags {0, A, C, A | C} where the header allows the combination (epi 5 is fp32 out)"""
    M, N, K = GE.nt_ragged_shape('b16', tile)
    worst = {}
    for kind in GE.KINDS:
        case = GE.nt_case(kind, M, N, K)
        for epi in (0, 1, 3, 5):
            for flags in GE.NT16_FLAGS:
                if epi == 5 and flags & GE.C16:
                    continue
                for with_bias in ((True, False) if epi == 0 else (True,)):
                    m = _check_nt('b16', case, epi, with_bias, flags)
                    worst[f'{epi}/{flags}'] = max(worst.get(f'{epi}/{flags}', 0.0), m)
    log_errors('gemm_edges_nt_b16_epilogues', dict(tile=list(tile), worst_error_over_bound=worst))


def _run_ffn(form, c1, c2, act):
    """u3d_ffn_fwd twice on guarded tensors -> (H or None, A, Z) on the host; guards, same bits on the second run, inputs unchanged"""
    from unidet3d_amd import _lib as L
    M, d_in, hid, d_out = c1.M, c1.K, c1.N, c2.N
    f = GE.BF16_OPERANDS if form == 'bf16op' else 0
    ins = [_in(c1.A), _in(c1.W), _in(c1.bias), _in(c2.W), _in(c2.bias)]
    keep = [t.clone() for t in ins]
    X, W1, b1, W2, b2 = ins
    runs = []
    with GE.math_mode(GE.NT_FORMS[form][0]):
        p1, p2 = (_planes(W1, hid, d_in), _planes(W2, d_out, hid)) if form == 'x3_planes' else (None, None)
        for _ in range(2):
            H, A, Z = (_out(M, hid) if act == 2 else None), _out(M, hid), _out(M, d_out)
            L.call('u3d_ffn_fwd', L.ptr(X), L.ptr(W1), L.ptr(b1), L.ptr(W2), L.ptr(b2), act | f, L.ptr(H), L.ptr(A), L.ptr(Z), M, d_in,
                   hid, d_out, L.ptr(p1), L.ptr(p2), 0.0, L.stream())
            assert _guard_ok(A, M) and _guard_ok(Z, M) and (H is None or _guard_ok(H, M)), (form, c1.kind, act)
            runs.append((None if H is None else H[:M], A[:M], Z[:M]))
    assert all(x is None or _same(x, y) for x, y in zip(*runs)), ('second run differs', form, c1.kind, act)
    assert all(_same(x, y) for x, y in zip(keep, ins)), ('an input was modified', form, c1.kind, act)
    return runs[0]


@pytest.mark.parametrize('form', ['native', 'x3', 'x3_planes', 'bf16op'])
def test_ffn_fwd_chains_two_products(form):
    """u3d_ffn_fwd: act(X W1^T + b1) in H (GELU pre-activation) / A, then A W2^T + b2 in Z.  Z is compared with the float64 product
    of the device's own A, so each product is held to its own bound.  With pre-split planes for W1 and W2 the three results must be
    the bits of the in-flight split."""
    M, d_in, hid, d_out = 65, 32, 96, 33
    family = GE.NT_FORMS[form][1]
    worst = 0.0
    for kind in GE.KINDS:
        c1, c2 = GE.nt_case(kind, M, hid, d_in), GE.nt_case(kind, M, d_out, hid)
        for act in (1, 2):
            H, A, Z = _run_ffn(form, c1, c2, act)
            if form == 'x3_planes':
                assert all(x is None or _same(x, y) for x, y in zip((H, A, Z), _run_ffn('x3', c1, c2, act))), ('planes differ', kind, act)
            ref, aref, _ = GE.nt_ref(c1, act, bf16=family == GE.B16)
            zero = kind == 'exact'
            b1d = torch.zeros_like(aref) if zero else GE.nt_bound(aref, d_in, family == GE.X3)
            if act == 1:
                m1 = GE.margin(A.cpu(), ref, b1d)
            else:
                m1 = GE.margin(H.cpu(), ref, b1d)
                g = GE.gelu64(H.cpu())
                assert float((A.cpu().double() - g).abs().max()) <= GE.GELU_TOL * float(g.abs().max())
            c2d = GE.NtCase(kind, M, d_out, hid, A.cpu(), c2.W, c2.bias, c2.aux)
            ref2, aref2, _ = GE.nt_ref(c2d, 0, bf16=family == GE.B16)
            exact2 = zero and act == 1             # integer A only behind the ReLU
            m2 = GE.margin(Z.cpu(), ref2, torch.zeros_like(aref2) if exact2 else GE.nt_bound(aref2, hid, family == GE.X3))
            print('gemm_edges ffn', form, kind, act, 'worst error / bound', m1, m2)
            assert m1 <= 1.0 and m2 <= 1.0, (form, kind, act, m1, m2)
            worst = max(worst, m1, m2)
    log_errors('gemm_edges_ffn', dict(form=form, worst_error_over_bound=worst))

# ============================================================================================================ TN through the C ABI
def _run_tn(form, case, colsum, flags=0):
    from unidet3d_amd import _lib as L
    M, N, K = case.M, case.N, case.K
    a16, b16 = form == 'b16' and bool(flags & GE.A16), form == 'b16' and bool(flags & GE.B16F)
    A, B = _in(case.A, BF if a16 else torch.float32), _in(case.B, BF if b16 else torch.float32)
    keep = (A.clone(), B.clone())
    lib = L.lib()
    nbytes = lib.u3d_gemm_tn_b16_ws_bytes(M, N, K) if form == 'b16' else lib.u3d_gemm_tn_ws_bytes(M, N, K)
    outs = []
    what = (form, (M, N, K), colsum, flags, case.kind)
    with GE.math_mode(GE.TN_FORMS[form][0]):
        for _ in range(2):
            ws = torch.full(((nbytes + 3) // 4,), NAN, dtype=torch.float32, device=DEV)
            dW, db = _out(N, K), (_out(N, 1) if colsum else None)
            if form == 'b16':
                L.call('u3d_gemm_tn_b16', L.ptr(A), L.ptr(B), L.ptr(dW), L.ptr(db), flags, M, N, K, L.ptr(ws), 0.0, L.stream())
            else:
                L.call('u3d_gemm_tn_bf16' if form == 'bf16op' else 'u3d_gemm_tn', L.ptr(A), L.ptr(B), L.ptr(dW), L.ptr(db), M, N, K,
                       L.ptr(ws), 0.0, L.stream())
            assert _guard_ok(dW, N), ('dW: guard rows touched or interior not finite', what)
            assert db is None or _guard_ok(db, N), ('column sums: guard touched or not finite', what)
            outs.append((dW[:N], None if db is None else db[:N, 0]))
    assert _same(outs[0][0], outs[1][0]) and (not colsum or _same(outs[0][1], outs[1][1])), ('second run differs', what)
    assert _same(keep[0], A) and _same(keep[1], B), ('an input was modified', what)
    return outs[0]


def _check_tn(form, case, colsum, flags=0):
    a16, b16 = form == 'b16' and bool(flags & GE.A16), form == 'b16' and bool(flags & GE.B16F)
    family = GE.TN_FORMS[form][1]
    if a16 or b16:                                 # a bf16 TENSOR holds the rounded values: they are the operand, column sums included
        case = GE.TnCase(case.kind, case.M, case.N, case.K, GE.rne(case.A) if a16 else case.A, GE.rne(case.B) if b16 else case.B)
    dW, db = _run_tn(form, case, colsum, flags)
    ref, aref, sref, asum = GE.tn_ref(case, family == GE.B16, family == GE.B16)
    ref, aref = ref.to(DEV), aref.to(DEV)
    zero = case.kind == 'exact'
    m = GE.margin(dW, ref, torch.zeros_like(aref) if zero else GE.tn_bound(aref, case.M, family == GE.X3))
    ms = 0.0
    if colsum:
        ms = GE.margin(db.cpu(), sref, torch.zeros_like(asum) if zero else GE.colsum_bound(asum, case.M))
    what = (form, (case.M, case.N, case.K), colsum, flags, case.kind)
    print('gemm_edges tn', what, 'worst error / bound', m, 'column sums', ms)
    assert m <= 1.0 and ms <= 1.0, (what, m, ms)
    return m, ms


def _tn_tiles():
    return [(form, T) for form, (_, _, _, tiles) in GE.TN_FORMS.items() for T in tiles]


@pytest.mark.parametrize('form,T', _tn_tiles())
def test_tn_every_tile_edge(form, T):
    """N and K around the tile (full, ragged, more than one tile, a single float4), with and without the column sums; the b16 form
    in its four dtype combinations"""
    worst, worst_cs = 0.0, 0.0
    for flags in (GE.TN16_FLAGS if form == 'b16' else (0,)):
        for i, (M, N, K) in enumerate(GE.tn_tile_shapes(form, T, flags)):
            for kind in GE.KINDS:
                m, ms = _check_tn(form, GE.tn_case(kind, M, N, K), (i + GE.KINDS.index(kind)) % 2 == 0, flags)
                worst, worst_cs = max(worst, m), max(worst_cs, ms)
    log_errors('gemm_edges_tn_tiles', dict(form=form, tile=T, worst_error_over_bound=worst, column_sums=worst_cs))


@pytest.mark.parametrize('form', list(GE.TN_FORMS))
def test_tn_every_row_split_situation(form):
    """one split with one and two trips and ragged trips; a last split of one row at split counts that are no multiple of 4 or 8;
    empty splits (whose partial must be written as zero: the workspace is NaN); the cap of 256 splits.  With the column sums; the
    b16 form in its four dtype combinations (integer values in all four, random values with both operands fp32 and both bf16)."""
    worst, worst_cs = 0.0, 0.0
    for flags in (GE.TN16_FLAGS if form == 'b16' else (0,)):
        for M, N, K in GE.tn_row_shapes(form, flags):
            for kind in GE.KINDS:
                if kind == 'randn' and (flags in (GE.A16, GE.B16F) or (M > 2048 and flags)):
                    continue
                m, ms = _check_tn(form, GE.tn_case(kind, M, N, K), True, flags)
                worst, worst_cs = max(worst, m), max(worst_cs, ms)
    _check_tn(form, GE.tn_case('exact', 129, 64, 64), False)
    log_errors('gemm_edges_tn_rows', dict(form=form, worst_error_over_bound=worst, column_sums=worst_cs))


# ============================================================================================================ refused arguments
def test_refused_arguments_return_the_documented_status_and_write_nothing():
    from unidet3d_amd import _lib as L
    lib = L.lib()
    s = L.stream()
    a = torch.ones(64, 64, device=DEV)
    h = torch.ones(64, 64, dtype=BF, device=DEV)
    out = torch.full((64 + N_GUARD, 64), GUARD, device=DEV)
    ws = torch.full((1 << 16,), GUARD, device=DEV)
    p = L.ptr
    for mode in ('mfma', 'bf16x3'):
        with GE.math_mode(mode):
            assert lib.u3d_gemm_nt(p(a), p(a), None, p(out), 0, 64, 64, None, 0.0, s) == GE.EINVAL
            assert lib.u3d_gemm_nt(p(a), p(a), None, p(out), 4, 4, 8, None, 0.0, s) == GE.EUNSUPPORTED
            assert lib.u3d_gemm_nt(p(a), p(a), None, p(out), 4, 4, 24, None, 0.0, s) == GE.EUNSUPPORTED
            assert lib.u3d_linear_act(p(a), p(a), None, GE.BF16_OPERANDS, None, p(out), 4, 4, 16, None, 0.0, s) == GE.EUNSUPPORTED
            assert lib.u3d_linear_act(p(a), p(a), None, 2, None, p(out), 4, 4, 16, None, 0.0, s) == GE.EINVAL            # GELU without pre
            assert lib.u3d_linear_dact(p(a), p(a), None, 1, p(out), 4, 4, 16, None, 0.0, s) == GE.EINVAL                 # mask without aux
            assert lib.u3d_gemm_tn(p(a), p(a), p(out), None, 0, 4, 4, p(ws), 0.0, s) == GE.EINVAL
            assert lib.u3d_gemm_tn(p(a), p(a), p(out), None, 8, 6, 4, p(ws), 0.0, s) == GE.EUNSUPPORTED
            assert lib.u3d_gemm_tn_bf16(p(a), p(a), p(out), None, 8, 4, 6, p(ws), 0.0, s) == GE.EUNSUPPORTED
    assert lib.u3d_gemm_nt_b16(p(a), p(a), None, 0, None, p(out), 0, 0, 64, 64, 0.0, s) == GE.EINVAL
    assert lib.u3d_gemm_nt_b16(p(a), p(a), None, 0, None, p(out), 0, 4, 4, 16, 0.0, s) == GE.EUNSUPPORTED
    assert lib.u3d_gemm_nt_b16(p(a), p(a), None, 0, None, p(out), GE.C16, 4, 5, 32, 0.0, s) == GE.EUNSUPPORTED             # odd N, bf16 C
    assert lib.u3d_gemm_nt_b16(p(a), p(a), None, 5, p(a), p(out), GE.C16, 4, 4, 32, 0.0, s) == GE.EUNSUPPORTED            # epi 5, bf16 C
    assert lib.u3d_gemm_nt_b16(p(a), p(a), None, 2, None, p(out), 0, 4, 4, 32, 0.0, s) == GE.EINVAL
    assert lib.u3d_gemm_tn_b16(p(h), p(a), p(out), None, GE.A16, 8, 12, 8, p(ws), 0.0, s) == GE.EUNSUPPORTED
    assert lib.u3d_gemm_tn_b16(p(a), p(h), p(out), None, GE.B16F, 8, 8, 12, p(ws), 0.0, s) == GE.EUNSUPPORTED
    assert lib.u3d_gemm_tn_b16(p(a), p(a), p(out), None, 0, 0, 8, 8, p(ws), 0.0, s) == GE.EINVAL
    assert lib.u3d_gelu_fwd(p(a), p(out), 6, s) == GE.EINVAL and lib.u3d_transpose(p(a), p(out), 0, 4, s) == GE.EINVAL
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()) and bool((ws == GUARD).all())
    log_errors('gemm_edges_refused_arguments', dict(outputs_untouched=True))


# ============================================================================================================ small kernels
@pytest.mark.parametrize('R,Cc', GE.TRANSPOSE_SHAPES)
def test_transpose(R, Cc):
    from unidet3d_amd import _lib as L
    src = torch.from_numpy(np.random.default_rng(R * 100 + Cc).standard_normal((R, Cc)).astype(np.float32))
    a, out = _in(src), _out(Cc, R)
    L.call('u3d_transpose', L.ptr(a), L.ptr(out), R, Cc, L.stream())
    assert _guard_ok(out, Cc) and torch.equal(out[:Cc].cpu(), src.t().contiguous())
    log_errors('gemm_edges_transpose', dict(R=R, C=Cc, equal=True))


def test_transpose_batch_and_weight_planes_batch():
    """three matrices of different sizes in one launch each: transposes equal the plain transpose, planes are the bits of the numpy
    split (tests/test_bf16x3_split_cpu.py); nothing is written behind any destination"""
    from unidet3d_amd import _lib as L
    rng = np.random.default_rng(5)
    srcs = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in GE.TRANSPOSE_BATCH]
    ins, outs, rows, blocks = [], [], [], 0
    for t in srcs:
        R, Cc = t.shape
        ins.append(_in(t)), outs.append(_out(Cc, R))
        rows.append([ins[-1].data_ptr(), outs[-1].data_ptr(), R, Cc, blocks])
        blocks += ((R + 31) // 32) * ((Cc + 31) // 32)
    desc = torch.tensor(rows, dtype=torch.int64, device=DEV)
    L.call('u3d_transpose_batch', L.ptr(desc), len(rows), blocks, L.stream())
    for t, o in zip(srcs, outs):
        assert _guard_ok(o, t.shape[1]) and torch.equal(o[:t.shape[1]].cpu(), t.t().contiguous()), t.shape
    vals = [torch.from_numpy((rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 3)).astype(np.float32)) for n in GE.PLANES_BATCH]
    ins, outs, rows, blocks = [], [], [], 0
    for v in vals:
        n = v.numel()
        ins.append(_in(v.view(-1, 8)))
        outs.append(torch.full((3 * n + 64,), GUARD, dtype=BF, device=DEV))
        rows.append([ins[-1].data_ptr(), outs[-1].data_ptr(), n // 8, blocks])
        blocks += (n // 8 + 255) // 256
    desc = torch.tensor(rows, dtype=torch.int64, device=DEV)
    L.call('u3d_weight_planes_batch', L.ptr(desc), len(rows), blocks, L.stream())
    for v, o in zip(vals, outs):
        n = v.numel()
        assert bool((o[3 * n:] == GUARD).all()), n
        assert torch.equal(o[:3 * n].view(torch.int16).cpu().view(3, n), GE.planes_ref(v)), n
    log_errors('gemm_edges_transpose_planes_batch', dict(transposes=[list(s) for s in GE.TRANSPOSE_BATCH], planes=list(GE.PLANES_BATCH), equal=True))


@pytest.mark.parametrize('n', GE.GELU_SIZES)
def test_stand_alone_gelu_passes(n):
    from unidet3d_amd import _lib as L
    rng = np.random.default_rng(n)
    h = torch.from_numpy((rng.standard_normal(n) * 2).astype(np.float32))
    da = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    hd, dad = _in(h.view(-1, 1)), _in(da.view(-1, 1))
    a, dh = _out(n, 1), _out(n, 1)
    L.call('u3d_gelu_fwd', L.ptr(hd), L.ptr(a), n, L.stream())
    L.call('u3d_gelu_bwd', L.ptr(dad), L.ptr(hd), L.ptr(dh), n, L.stream())
    assert _guard_ok(a, n) and _guard_ok(dh, n)
    ra, rd = GE.gelu64(h), da.double() * GE.gelu_grad64(h)
    ea = float((a[:n, 0].cpu().double() - ra).abs().max()) / (GE.GELU_TOL * float(ra.abs().max()))
    ed = float((dh[:n, 0].cpu().double() - rd).abs().max()) / (GE.GELU_TOL * float(rd.abs().max()))
    print('gemm_edges gelu', n, 'worst error / tolerance', ea, ed)
    assert ea <= 1.0 and ed <= 1.0, (n, ea, ed)
    log_errors('gemm_edges_gelu', dict(n=n, worst_error_over_bound=max(ea, ed)))


@pytest.mark.parametrize('n', GE.GELU16_SIZES)
def test_stand_alone_gelu_passes_bf16(n):
    """the bf16 passes (8 values per thread): fp32 arithmetic on the bf16 values, one rounding on the way out; one thread, a ragged
    last block on either side of a block edge"""
    from unidet3d_amd import _lib as L
    rng = np.random.default_rng(16 + n)
    hb = GE.rne(torch.from_numpy((rng.standard_normal(n) * 2).astype(np.float32)))
    db = GE.rne(torch.from_numpy(rng.standard_normal(n).astype(np.float32)))
    hd, dad = _in(hb.view(-1, 1), BF), _in(db.view(-1, 1), BF)
    a, dh = _out(n, 1, BF), _out(n, 1, BF)
    L.call('u3d_gelu_fwd_b16', L.ptr(hd), L.ptr(a), n, L.stream())
    L.call('u3d_gelu_bwd_b16', L.ptr(dad), L.ptr(hd), L.ptr(dh), n, L.stream())
    assert _guard_ok(a, n) and _guard_ok(dh, n)
    worst = 0.0
    for got, ref in ((a, GE.gelu64(hb)), (dh, db.double() * GE.gelu_grad64(hb))):
        tol = GE.GELU_TOL * float(ref.abs().max())
        m = GE.margin(got[:n, 0].cpu().float(), ref, tol + GE.half_ulp_bf16(ref.abs() + tol))
        assert m <= 1.0, (n, m)
        worst = max(worst, m)
    log_errors('gemm_edges_gelu_b16', dict(n=n, worst_error_over_bound=worst))


# ============================================================================================================ autograd
FLOWS = ('fp32-mfma', 'fp32-bf16x3', 'bf16-operands')


def _pb(aref, depth, three):
    """the product bound gamma_2(depth + 4) * abs_ref (+ 2^-22 abs_ref where the three-plane kernel runs) with the TRUE reduction
    depth: zero padding of the depth adds exact zero terms and no rounding"""
    return (float(GE.gamma2(depth + 4)) + (2.0 ** -22 if three else 0.0)) * aref


def _x3_nt(x3, depth, q=16):
    """the three-plane NT kernel runs when the mode is bf16x3 and the (padded) reduction depth is a multiple of 32"""
    return x3 and (depth + q - 1) // q * q % 32 == 0


@pytest.mark.parametrize('flow', FLOWS)
def test_dense_linear_at_widths_that_are_zero_padded(flow):
    """dense.linear forward, dX, dW, db at N in {1, 5, 17, 33, 47} x K in {16, 48, 80}: N is zero-padded to 4 (dW's TN product) and to
    16 / 32 (dX's reduction depth), K to 32 under bf16 operands.  Zero padding adds exact zero terms, so the bounds are those of the
    unpadded depth: gamma_2(K + 4) for y, gamma_2(N + 4) for dX, gamma_2(M + 4) for dW.  (The bf16-activation flow needs every
    reduction depth % 32 == 0 and never applies at these K.)"""
    from unidet3d_amd import dense, precision as P
    bf = flow == 'bf16-operands'
    x3 = flow == 'fp32-bf16x3'
    M = 70
    worst = 0.0
    for N in GE.AUTOGRAD_N:
        for K in GE.AUTOGRAD_K:
            for kind in GE.KINDS:
                c = GE.nt_case(kind, M, N, K)
                dy = GE.nt_case(kind, M, N, 16).aux
                x = c.A.to(DEV).requires_grad_(True)
                w = c.W.to(DEV).requires_grad_(True)
                b = c.bias.to(DEV).requires_grad_(True)
                with P.fp32_math('mfma' if flow == 'fp32-mfma' else 'bf16x3'), P.operands('bf16' if bf else 'fp32'):
                    y = dense.linear(x, w, b)
                    y.backward(dy.to(DEV))
                torch.cuda.synchronize()
                r = (lambda t: GE.rne(t).double()) if bf else (lambda t: t.double())
                zero = kind == 'exact'
                checks = {
                    'y': (y, r(c.A) @ r(c.W).t() + c.bias.double(), r(c.A).abs() @ r(c.W).abs().t() + c.bias.double().abs(), K,
                          _x3_nt(x3, K)),
                    'dx': (x.grad, r(dy) @ r(c.W), r(dy).abs() @ r(c.W).abs(), N, _x3_nt(x3, N)),
                    'dw': (w.grad, r(dy).t() @ r(c.A), r(dy).abs().t() @ r(c.A).abs(), M, x3),
                }
                for name, (got, ref, aref, depth, three) in checks.items():
                    m = GE.margin(got.detach().cpu(), ref, torch.zeros_like(aref) if zero else _pb(aref, depth, three))
                    assert m <= 1.0, (flow, N, K, kind, name, m)
                    worst = max(worst, m)
                sref, asum = dy.double().sum(0), dy.double().abs().sum(0)
                m = GE.margin(b.grad.cpu(), sref, torch.zeros_like(asum) if zero else GE.colsum_bound(asum, M))
                assert m <= 1.0, (flow, N, K, kind, 'db', m)
                worst = max(worst, m)
    print('gemm_edges autograd linear', flow, 'worst error / bound', worst)
    log_errors('gemm_edges_autograd_linear', dict(flow=flow, worst_error_over_bound=worst))


def _mlp_random_stages(flow, act, M, hid, N, K):
    """dense.mlp forward + backward with random values, every stage against float64 of the stage's OWN inputs: the hidden tensors the
    Function saved (a, and the GELU pre-activation h) are read back from the graph node, so each product is held to its own bound
    with its true depth.  The hidden gradient dh is not observable: its float64 value is formed from the device's a / h, its error
    bound e_dh = (product bound at depth N) * |act'| (+ the 1e-5 GELU criterion), and dX, dW1, db1 carry e_dh through |W1|, |x| and
    the column sum next to their own product bound.  -> worst error / bound"""
    from unidet3d_amd import dense, precision as P
    x3 = flow == 'fp32-bf16x3'
    c1, c2 = GE.nt_case('randn', M, hid, K), GE.nt_case('randn', M, N, hid)
    ts = [t.to(DEV).requires_grad_(True) for t in (c1.A, c1.W, c1.bias, c2.W, c2.bias)]
    dz = c2.aux
    with P.fp32_math('mfma' if flow == 'fp32-mfma' else 'bf16x3'):
        z = dense.mlp(*ts, act)
        saved = z.grad_fn.saved_tensors
        a_dev, h_dev = saved[3].detach().cpu(), (None if saved[4] is None else saved[4].detach().cpu())
        z.backward(dz.to(DEV))
    torch.cuda.synchronize()
    x, W1, b1, W2, b2, dz64 = c1.A.double(), c1.W.double(), c1.bias.double(), c2.W.double(), c2.bias.double(), dz.double()
    got = dict(z=z.detach().cpu(), dx=ts[0].grad.cpu(), dw1=ts[1].grad.cpu(), db1=ts[2].grad.cpu(), dw2=ts[3].grad.cpu(), db2=ts[4].grad.cpu())
    margins = {}
    # forward: x W1^T + b1 (depth K), the activation, a W2^T + b2 (depth hid) on the device's own a
    pre, apre = x @ W1.t() + b1, x.abs() @ W1.abs().t() + b1.abs()
    e_pre = _pb(apre, K, _x3_nt(x3, K))
    if act == 'relu':
        margins['a'] = GE.margin(a_dev, pre.clamp(min=0), e_pre)
    else:
        margins['h'] = GE.margin(h_dev, pre, e_pre)
        g = GE.gelu64(h_dev)
        margins['a'] = GE.margin(a_dev, g, torch.full_like(g, GE.GELU_TOL * float(g.abs().max())))
    a = a_dev.double()
    margins['z'] = GE.margin(got['z'], a @ W2.t() + b2, _pb(a.abs() @ W2.abs().t() + b2.abs(), hid, _x3_nt(x3, hid)))
    # backward of the second Linear: both operands are known exactly
    margins['dw2'] = GE.margin(got['dw2'], dz64.t() @ a, _pb(dz64.abs().t() @ a.abs(), M, x3))
    margins['db2'] = GE.margin(got['db2'], dz64.sum(0), GE.colsum_bound(dz64.abs().sum(0), M))
    # the hidden gradient: (dz W2) * act' from the device's own a / h
    fac = (a_dev > 0).double() if act == 'relu' else GE.gelu_grad64(h_dev)
    dh = (dz64 @ W2) * fac
    e_dh = _pb(dz64.abs() @ W2.abs(), N, _x3_nt(x3, N)) * fac.abs()
    if act == 'gelu':
        e_dh = e_dh + GE.GELU_TOL * float(dh.abs().max())
    adh = dh.abs() + e_dh
    margins['dw1'] = GE.margin(got['dw1'], dh.t() @ x, _pb(adh.t() @ x.abs(), M, x3) + e_dh.t() @ x.abs())
    margins['db1'] = GE.margin(got['db1'], dh.sum(0), GE.colsum_bound(adh.sum(0), M) + e_dh.sum(0))
    margins['dx'] = GE.margin(got['dx'], dh @ W1, _pb(adh @ W1.abs(), hid, _x3_nt(x3, hid)) + e_dh @ W1.abs())
    for name, m in margins.items():
        assert m <= 1.0, (flow, act, N, K, name, m)
    return max(margins.values())


@pytest.mark.parametrize('flow', FLOWS[:2])
def test_dense_mlp_at_widths_that_are_zero_padded(flow):
    """dense.mlp (d_in = K, hidden 48, d_out = N) forward and backward.  ReLU with integer values: every intermediate is an integer,
    the mask is the reference's, so the result and all five gradients must match float64 bit for bit.  ReLU and GELU with random
    values: the result and all five gradients by the elementwise bounds, stage by stage (_mlp_random_stages) -- this runs the hidden
    gradient through the activation on a dz zero-padded from N to 16.  (Under bf16 operands dense.mlp needs d_in % 32 == 0, which
    none of these K is.)"""
    from unidet3d_amd import dense, precision as P
    M, hid = 70, 48
    worst = {'relu': 0.0, 'gelu': 0.0}
    for N in GE.AUTOGRAD_N:
        for K in GE.AUTOGRAD_K:
            c1, c2 = GE.nt_case('exact', M, hid, K), GE.nt_case('exact', M, N, hid)
            ts = [t.to(DEV).requires_grad_(True) for t in (c1.A, c1.W, c1.bias, c2.W, c2.bias)]
            with P.fp32_math('mfma' if flow == 'fp32-mfma' else 'bf16x3'):
                z = dense.mlp(*ts, 'relu')
                z.backward(c2.aux.to(DEV))
            torch.cuda.synchronize()
            ts64 = [t.detach().cpu().double().requires_grad_(True) for t in ts]
            z64 = torch.relu(ts64[0] @ ts64[1].t() + ts64[2]) @ ts64[3].t() + ts64[4]
            z64.backward(c2.aux.double())
            assert torch.equal(z.detach().cpu().double(), z64.detach()), (flow, N, K, 'z')
            for name, t, t64 in zip(('dx', 'dw1', 'db1', 'dw2', 'db2'), ts, ts64):
                assert torch.equal(t.grad.cpu().double(), t64.grad), (flow, N, K, name)
            for act in ('relu', 'gelu'):
                worst[act] = max(worst[act], _mlp_random_stages(flow, act, M, hid, N, K))
    print('gemm_edges autograd mlp', flow, 'worst error / bound', worst)
    log_errors('gemm_edges_autograd_mlp', dict(flow=flow, worst_error_over_bound=worst))


