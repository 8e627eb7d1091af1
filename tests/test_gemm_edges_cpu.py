"""Host-side checks of tests/_gemm_edges.py, the helper behind tests/test_gpu_gemm_edges.py: its float64 references agree with
torch, a numpy emulation of the kernels' arithmetic (fp32 sequential sums, the three-plane split of tests/test_bf16x3_split_cpu.py,
RNE rounding to bf16) stays inside every acceptance bound, every mutant is rejected, and the shape lists reach every (kernel, tile)
instantiation and every split situation -- as reported by the host-only plan queries (include/u3d.h u3d_gemm_*_plan), i.e. by the
function the launches take their decision from.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gemm_edges as GE


# ============================================================================================================ 1. references
def test_references_agree_with_torch_float64():
    c = GE.nt_case('randn', 37, 21, 48)
    A, W, b, aux = (t.double() for t in (c.A, c.W, c.bias, c.aux))
    lin = F.linear(A, W, b)
    assert torch.allclose(GE.nt_ref(c, 0)[0], lin, rtol=1e-13, atol=1e-13)
    assert torch.allclose(GE.nt_ref(c, 0, with_bias=False)[0], F.linear(A, W), rtol=1e-13, atol=1e-13)
    assert torch.allclose(GE.nt_ref(c, 1)[0], F.relu(lin), rtol=1e-13, atol=1e-13)
    assert torch.allclose(GE.nt_ref(c, 2)[0], lin, rtol=1e-13, atol=1e-13)                       # `pre`
    assert torch.allclose(GE.gelu64(lin), F.gelu(lin), rtol=1e-12, atol=1e-14)
    assert torch.allclose(GE.nt_ref(c, 5)[0], F.linear(A, W) + aux, rtol=1e-13, atol=1e-13)
    # epi 3 / 4: the input gradient through the activation, by autograd (A plays dY, W the transposed weight)
    for epi, act in ((3, F.relu), (4, F.gelu)):
        h = aux.clone().requires_grad_(True)
        act(h).backward(F.linear(A, W))
        ref, _, factor = GE.nt_ref(c, epi)
        assert torch.allclose(ref * (factor if factor is not None else 1.0), h.grad, rtol=1e-11, atol=1e-13), epi
    t = GE.tn_case('randn', 45, 20, 36)
    x = t.B.double()
    w = torch.zeros(20, 36, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(20, dtype=torch.float64, requires_grad=True)
    F.linear(x, w, bias).backward(t.A.double())                                                  # dW = dY^T X, db = column sums of dY
    cref, _, sref, _ = GE.tn_ref(t)
    assert torch.allclose(cref, w.grad, rtol=1e-13, atol=1e-13) and torch.allclose(sref, bias.grad, rtol=1e-13, atol=1e-13)
    # the bf16 forms: operands rounded to nearest even first (numpy restatement of the rounding against torch's)
    v = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    bits = v.view(np.uint32)
    r = ((bits + np.uint32(0x7fff) + ((bits >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)
    assert np.array_equal(GE.rne(torch.from_numpy(v)).numpy(), r)
    assert torch.equal(GE.half_ulp_bf16(torch.tensor([1.0, 1.5, 2.0, 0.0, -3.0])), torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0.0, 2.0 ** -7],
                                                                                              dtype=torch.float64))


# ============================================================================================================ 2. bounds
NT_EMU = [('native', GE.NATIVE), ('x3', GE.X3), ('bf16op', GE.B16)]


@pytest.mark.parametrize('form,family', NT_EMU)
def test_nt_emulation_stays_inside_the_bound(form, family):
    """fp32 sequential sums over k (six plane products under the split; RNE-rounded operands): worst error / bound on the randn
    cases of the K-step, grid and 64 x 64 sweep lists; the exact cases come out bit for bit."""
    worst, worst_c16 = 0.0, 0.0
    shapes = GE.nt_k_steps(form) + GE.nt_grid_shapes(form)[:6] + GE.nt_tile_shapes(form, (64, 64))[-4:]
    for M, N, K in shapes:
        for kind in GE.KINDS:
            c = GE.nt_case(kind, M, N, K)
            for epi in (0, 1, 3, 5):
                ref, aref, _ = GE.nt_ref(c, epi, bf16=family == GE.B16)
                got = GE.nt_emulate(c, epi, family)
                if kind == 'exact':
                    assert torch.equal(got.double(), ref), (form, M, N, K, epi)
                    continue
                m = GE.margin(got, ref, GE.nt_bound(aref, K, family == GE.X3))
                worst = max(worst, m)
                assert m <= 1.0, (form, M, N, K, epi, m)
            if family == GE.B16 and kind == 'randn' and N % 2 == 0:                              # a bf16 C: + half a bf16 ulp
                ref, aref, _ = GE.nt_ref(c, 0, bf16=True)
                b = GE.nt_bound(aref, K, False)
                m = GE.margin(GE.nt_emulate(c, 0, family, c_bf16=True), ref, b + GE.half_ulp_bf16(ref.abs() + b))
                worst_c16 = max(worst_c16, m)
                assert m <= 1.0, (form, M, N, K, 'bf16 C', m)
    print(f'gemm_edges emulation NT {form}: worst error / bound {worst:.4f}, bf16 C {worst_c16:.4f}')


@pytest.mark.parametrize('form,family', NT_EMU)
def test_tn_emulation_stays_inside_the_bound(form, family):
    worst, worst_cs = 0.0, 0.0
    shapes = [(m, 20, 36) for m in GE.TN_ROWS] + [(m, 64, 64) for m in GE.TN_LAST_SPLIT_ONE_ROW]
    if form == 'native':
        shapes.append((2049, 64, 64))
    for M, N, K in shapes:
        plan = GE.tn_form_plan(form, M, N, K)
        for kind in GE.KINDS:
            c = GE.tn_case(kind, M, N, K)
            ref, aref, sref, asum = GE.tn_ref(c, family == GE.B16, family == GE.B16)
            got, cs = GE.tn_emulate(c, plan, family)
            if kind == 'exact':
                assert torch.equal(got.double(), ref) and torch.equal(cs.double(), sref), (form, M, N, K)
                continue
            m, ms = GE.margin(got, ref, GE.tn_bound(aref, M, family == GE.X3)), GE.margin(cs, sref, GE.colsum_bound(asum, M))
            worst, worst_cs = max(worst, m), max(worst_cs, ms)
            assert m <= 1.0 and ms <= 1.0, (form, M, N, K, m, ms)
    print(f'gemm_edges emulation TN {form}: worst error / bound {worst:.4f}, column sums {worst_cs:.4f}')


# ============================================================================================================ 3. mutants
def _nt_rejected(c, wrong, epi, family, kind):
    ref, aref, _ = GE.nt_ref(c, epi, bf16=family == GE.B16)
    if kind == 'exact':
        return not torch.equal(wrong, ref)
    return GE.margin(wrong, ref, GE.nt_bound(aref, c.K, family == GE.X3)) > 1.0


@pytest.mark.parametrize('kind', GE.KINDS)
def test_every_nt_mutant_is_rejected(kind):
    seen = set()
    for form, family in NT_EMU:
        ks = GE.NT_FORMS[form][2]
        for tile, (M, N, K) in (((64, 64), (65, 66, 2 * ks)), ((64, 64), (129, 33, 3 * ks)), ((128, 64), (131, 70, 2 * ks)),
                                ((128, 128), (259, 130, 2 * ks))):
            c = GE.nt_case(kind, M, N, K)
            for name, epi, wrong in GE.nt_mutants(c, tile, ks, family == GE.B16):
                assert _nt_rejected(c, wrong, epi, family, kind), (form, tile, (M, N, K), name)
                seen.add(name)
    assert len(seen) == 5, seen


def _tn_rejected(c, plan, wrong, wrong_cs, family, kind):
    ref, aref, sref, asum = GE.tn_ref(c)
    if wrong is not None:
        return (not torch.equal(wrong, ref)) if kind == 'exact' else GE.margin(wrong, ref, GE.tn_bound(aref, c.M, family == GE.X3)) > 1.0
    return (not torch.equal(wrong_cs, sref)) if kind == 'exact' else GE.margin(wrong_cs, sref, GE.colsum_bound(asum, c.M)) > 1.0


@pytest.mark.parametrize('kind', GE.KINDS)
def test_every_tn_mutant_is_rejected(kind):
    seen = set()
    for form in ('native', 'x3'):
        family, trip = GE.TN_FORMS[form][1], GE.TN_FORMS[form][2]
        for M, N, K in [(33, 20, 36), (129, 20, 36), (513, 64, 64), (641, 64, 64), (1025, 64, 64), (2049, 64, 64)]:
            c, plan = GE.tn_case(kind, M, N, K), GE.tn_form_plan(form, M, N, K)
            for name, wrong, wrong_cs in GE.tn_mutants(c, plan, trip):
                assert _tn_rejected(c, plan, wrong, wrong_cs, family, kind), (form, (M, N, K), plan, name)
                seen.add(name)
    assert len(seen) == 6, seen


def test_what_the_max_norm_criterion_sees_of_the_mutants_at_16001_rows():
    """The workload-shaped tests compare by max |error| / max |reference| < 1e-5 at M ~ 16k.  This prints, for every mutant at
    M = 16001, that ratio and the error over the elementwise bound, and asserts what decides the matter at that size: the
    integer-valued case rejects every one of them by inequality.
    With random values the max-norm ratio rejects every one of them too (one wrong or lost row of 16001 is far above 1e-5 of the
    largest element); what it cannot do is say which rows.  The random-value elementwise bound grows with M, and at this size the
    mutants that lose a single row stay inside it -- the printed lines show which -- so at large M the integer-valued kind is
    what guards against them (tests/_gemm_edges.py header)."""
    M = 16001
    rows = []
    c, cx = GE.nt_case('randn', M, 66, 64), GE.nt_case('exact', M, 66, 64)
    for (name, epi, wrong), (_, _, wrong_x) in zip(GE.nt_mutants(c, (128, 64), 32), GE.nt_mutants(cx, (128, 64), 32)):
        ref, aref, _ = GE.nt_ref(c, epi)
        assert _nt_rejected(cx, wrong_x, epi, GE.X3, 'exact'), name
        rows.append(('nt', name, GE.max_norm_ratio(wrong, ref), GE.margin(wrong, ref, GE.nt_bound(aref, c.K, True))))
    for form in ('native', 'x3'):
        family, trip = GE.TN_FORMS[form][1], GE.TN_FORMS[form][2]
        t, tx, plan = GE.tn_case('randn', M, 64, 64), GE.tn_case('exact', M, 64, 64), GE.tn_form_plan(form, M, 64, 64)
        ref, aref, sref, asum = GE.tn_ref(t)
        for (name, wrong, wrong_cs), (_, wx, wx_cs) in zip(GE.tn_mutants(t, plan, trip), GE.tn_mutants(tx, plan, trip)):
            assert _tn_rejected(tx, plan, wx, wx_cs, family, 'exact'), (form, name)
            if wrong is not None:
                rows.append((f'tn {form}', name, GE.max_norm_ratio(wrong, ref), GE.margin(wrong, ref, GE.tn_bound(aref, M, family == GE.X3))))
            else:
                rows.append((f'tn {form}', name, GE.max_norm_ratio(wrong_cs, sref), GE.margin(wrong_cs, sref, GE.colsum_bound(asum, M))))
    for where, name, r, m in rows:
        print(f'M = {M}: {where:10s} {name:52s} max-norm ratio {r:.2e} ({"ACCEPTED" if r < 1e-5 else "rejected"} at 1e-5), '
              f'error / elementwise bound {m:.2e}; exact values: rejected')


# ============================================================================================================ 4. coverage
def test_shape_lists_reach_every_kernel_tile_and_split_situation():
    """Every (kernel form, tile) the dispatchers can choose is reached by a shape list (the list builders raise when a plan is not
    the wanted one), and the TN row lists hold every split situation: one split, a last split of one row with split counts that are
    no multiple of 4 (three-plane) and of 8 (native), an empty last split, the cap of 256 splits with empty ones."""
    for form, (_, _, _, tiles) in GE.NT_FORMS.items():
        for tile in tiles:
            shapes = GE.nt_tile_shapes(form, tile)
            assert shapes, (form, tile)
            print(f'NT {form:10s} tile {tile[0]:3d} x {tile[1]:3d}: {len(shapes)} shapes, e.g. {shapes[0]}, ragged {GE.nt_ragged_shape(form, tile)}')
        assert len(GE.nt_k_steps(form)) == 5 and len(GE.nt_grid_shapes(form)) == len(GE.GRID_WGS)
    for flags in GE.NT16_FLAGS:                                                                   # the b16 tiles do not depend on the dtypes
        for tile in GE.TILES:
            M, N, K = GE.nt_ragged_shape('b16', tile)
            assert GE.nt16_plan(M, N, K, 0, flags) == (0, GE.B16, *tile), (flags, tile)
    # K = 16 (mod 32) under the three-plane mode takes the native kernel, K = 0 (mod 32) the three-plane one
    with GE.math_mode('bf16x3'):
        assert all(GE.nt_plan(65, 33, k)[1] == GE.NATIVE for k in GE.ROUTE_KS)
        assert all(GE.nt_plan(65, 33, k)[1] == GE.X3 for k in (32, 64, 96))
    for form, (_, _, _, tiles) in GE.TN_FORMS.items():
        for T in tiles:
            for flags in (GE.TN16_FLAGS if form == 'b16' else (0,)):
                shapes = GE.tn_tile_shapes(form, T, flags)
                print(f'TN {form:10s} tile {T:3d} flags {flags}: {shapes}')
        situations = {}
        for s in GE.tn_row_shapes(form):
            p = GE.tn_form_plan(form, *s)
            assert p.rc == 0 and p.rows_per_split % 16 == 0 and p.splits * p.rows_per_split >= s[0] and 1 <= p.used <= p.splits <= 256, (form, s, p)
            key = ('one split' if p.splits == 1 else f'{p.splits} splits, last holds {p.last_rows} rows' +
                   (f', {p.empty} empty' if p.empty else ''))
            situations[s] = key
            print(f'TN {form:10s} {s}: {key} ({p.rows_per_split} rows per split)')
        plans = {s: GE.tn_form_plan(form, *s) for s in situations}
        assert all(plans[(m, 20, 36)].splits == 1 for m in (1, 15, 16, 17, 31, 32, 33, 63, 64))
        assert plans[GE.TN_CAP].splits == 256 and plans[GE.TN_CAP].empty > 0, plans[GE.TN_CAP]
        assert [plans[(m, 64, 64)].last_rows for m in GE.TN_LAST_SPLIT_ONE_ROW] == [1, 1, 1]
        counts = [plans[(m, 64, 64)].splits for m in GE.TN_LAST_SPLIT_ONE_ROW]
        if form == 'native':
            assert counts == [9, 11, 17] and plans[GE.TN_LAST_EMPTY].empty > 0
        elif form == 'bf16op':
            assert counts == [9, 11, 17] and plans[GE.TN_LAST_EMPTY].empty > 0
        else:
            assert counts == [5, 6, 9]
        if form == 'x3':
            assert plans[GE.TN_CAP].rows_per_split == 160 and plans[GE.TN_CAP].empty == 51 and plans[GE.TN_LAST_EMPTY].empty > 0
        if form == 'b16':                                                                         # 17 splits of 128 rows: the last one holds ONE row
            assert (plans[GE.TN_LAST_EMPTY].splits, plans[GE.TN_LAST_EMPTY].last_rows) == (17, 1)


def test_plan_queries_return_the_status_of_the_launch():
    import ctypes
    from unidet3d_amd import _lib as L
    l = L.lib()
    for mode in ('mfma', 'bf16x3'):
        with GE.math_mode(mode):
            assert GE.nt_plan(0, 4, 16)[0] == GE.EINVAL and GE.nt_plan(4, 0, 16)[0] == GE.EINVAL and GE.nt_plan(4, 4, 0)[0] == GE.EINVAL
            assert GE.nt_plan(4, 4, 16, 3)[0] == GE.EINVAL                                       # an unknown flag
            assert GE.nt_plan(4, 4, 8)[0] == GE.EUNSUPPORTED and b'multiple of 16' in l.u3d_last_error()
            assert GE.nt_plan(4, 4, 16, GE.BF16_OPERANDS)[0] == GE.EUNSUPPORTED and b'multiple of 32' in l.u3d_last_error()
            assert GE.tn_plan(0, 4, 4).rc == GE.EINVAL
            assert GE.tn_plan(5, 6, 8).rc == GE.EUNSUPPORTED and GE.tn_plan(5, 8, 6, 1).rc == GE.EUNSUPPORTED
    assert GE.nt16_plan(4, 4, 16)[0] == GE.EUNSUPPORTED and GE.nt16_plan(0, 4, 32)[0] == GE.EINVAL
    assert GE.nt16_plan(4, 4, 32, 2)[0] == GE.EINVAL and GE.nt16_plan(4, 4, 32, 0, 2)[0] == GE.EINVAL
    assert GE.nt16_plan(4, 5, 32, 0, GE.C16)[0] == GE.EUNSUPPORTED and GE.nt16_plan(4, 4, 32, 5, GE.C16)[0] == GE.EUNSUPPORTED
    assert GE.nt16_plan(4, 5, 32, 5, GE.A16)[0] == 0
    assert GE.tn16_plan(5, 12, 8, GE.A16).rc == GE.EUNSUPPORTED and GE.tn16_plan(5, 8, 12, GE.B16F).rc == GE.EUNSUPPORTED
    assert GE.tn16_plan(5, 12, 12, 0).rc == 0 and GE.tn16_plan(5, 8, 8, 4).rc == GE.EINVAL
    assert l.u3d_gemm_nt_plan(65, 33, 32, 0, None, None, None) == 0                              # NULL outputs are allowed
    r = ctypes.c_int64(0)
    assert l.u3d_gemm_tn_plan(129, 64, 64, 0, None, None, None, None, ctypes.byref(r)) == 0 and r.value > 0
