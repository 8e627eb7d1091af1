"""Host-side checks of tests/_bn_edges.py, the helper behind tests/test_gpu_bn_edges.py: its float64 references agree with torch's
batch norm in float64, a numpy restatement of the device arithmetic of csrc/bn.hip (fp64 sums, fp32 everything else, multiply-add
separate or fused) stays inside every acceptance bound for every value kind, every planted fault leaves the bounds (or the exact
`ints` comparison), and the case lists reach the grid and loop edges they are meant for.  No GPU."""
import numpy as np
import pytest
import torch

import _bn_edges as BE

SAMPLE = [(1, 32), (2, 36), (7, 4), (33, 64), (70, 508), (257, 100), (1025, 160), (4097, 32), (65537, 8)]


# ============================================================================================================ 1. references
@pytest.mark.parametrize('relu', [0, 1])
def test_references_agree_with_torch_float64(relu):
    c = BE.make_case('randn', 57, 36)
    r = BE.stats_ref(c)
    bn = torch.nn.BatchNorm1d(c.C, eps=BE.EPS, momentum=BE.MOM).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c.gamma).double()); bn.bias.copy_(torch.from_numpy(c.beta).double())
        bn.running_mean.copy_(torch.from_numpy(c.rm0).double()); bn.running_var.copy_(torch.from_numpy(c.rv0).double())
    x = torch.from_numpy(c.x).double().requires_grad_()
    y = bn(x)
    y = torch.relu(y) if relu else y
    (y * torch.from_numpy(c.dy).double()).sum().backward()
    yr, _ = BE.y_ref(c, r, relu)
    kw = dict(rtol=1e-12, atol=1e-12)
    assert np.allclose(yr, y.detach().numpy(), **kw)
    assert np.allclose(r.rm, bn.running_mean.numpy(), **kw) and np.allclose(r.rv, bn.running_var.numpy(), **kw)
    b = BE.bwd_ref(c, r, (yr > 0) if relu else None, False)
    assert np.allclose(b.dx, x.grad.numpy(), **kw) and np.allclose(b.dgamma, bn.weight.grad.numpy(), **kw)
    assert np.allclose(b.dbeta, bn.bias.grad.numpy(), **kw)
    ba = BE.bwd_ref(c, r, (yr > 0) if relu else None, True)
    assert np.allclose(ba.dx, x.grad.numpy() + c.addend.astype(np.float64), **kw) and bool((ba.b_dx > b.b_dx).all())
    one = BE.stats_ref(BE.make_case('randn', 1, 8))                       # n = 1: the biased variance (0) goes into running_var
    assert bool((one.var == 0).all()) and bool((one.unb == 0).all())


def test_case_lists_reach_the_edges_they_name():
    assert [BE.rpb(C) for C in (4, 32, 36, 100, 260, 508, 512)] == [256, 32, 28, 10, 3, 2, 2]
    for C in BE.WIDTHS:
        assert C % 4 == 0 and 4 <= C <= 512
        r, e = BE.rpb(C), BE.row_edges(C)
        assert {1, 2, r + 1, 16 * r + 1, 64 * r + 1} <= set(e)
        assert BE.stats_grid(16 * r, C) == 1 and BE.stats_grid(16 * r + 1, C) == 2 and BE.stats_grid(64 * r + 1, C) == 5
        assert max(e) * C <= 70000                                     # small: every kind and both relu settings run at each
    assert {256 % (C // 4) == 0 for C in BE.WIDTHS} == {True, False}   # full and idle-lane workgroups
    for C, n in BE.LARGE_ROWS.items():
        assert BE.stats_grid(n - 1, C) == 256 and -(-(n - 1) // (BE.rpb(C) * 16)) == 256 and -(-n // (BE.rpb(C) * 16)) == 257
        assert n * C * 4 <= 17 * 2 ** 20
    assert BE.ew_grid(8192, 512) == 4096 and -(-(8193 * 128) // 256) > 4096          # 8193 rows of 512: past the apply grid's cap
    for C in BE.PARTIAL_WIDTHS:
        t = BE.tile_edges(C)
        assert BE.partials_grid(max(t) - 1, C) == 128 and -(-max(t) // (BE.partials_rpp(C) * 16)) == 129
    assert [(2 * C) // 256 + (1 if (2 * C) % 256 else 0) for C in BE.PARTIAL_WIDTHS] == [1, 1, 1, 2, 3, 4]      # column chunks
    idx = BE.fragment_order(64)
    assert sorted(idx.tolist()) == list(range(64)) and idx[:8].tolist() == [0, 1, 2, 3, 16, 17, 18, 19] and idx[40:44].tolist() == [36, 37, 38, 39]
    c = BE.make_case('const', 5, 8)
    assert bool((c.x == c.x[0]).all()) and c.gamma[1] == 0 and c.beta[1] == 0 and c.gamma[-1] == 0 and bool((c.gamma[2:-1] != 0).all())
    assert bool((BE.make_case('randn', 9, 64).gamma < 0).any())


# ============================================================================================================ 2. bounds
@pytest.mark.parametrize('kind', BE.KINDS)
def test_restated_device_arithmetic_stays_inside_every_bound(kind):
    worst = {}
    for n, C in SAMPLE:
        c = BE.make_case(kind, n, C)
        r = BE.stats_ref(c)
        for fused in (False, True):
            for relu in (0, 1):
                fw = BE.emulate_forward(c, relu, fused)
                ms = BE.forward_margins(c, r, fw, relu)
                if kind == 'ints':
                    assert np.array_equal(fw.sums, np.concatenate([r.s1, r.s2])), (n, C)
                if kind == 'const':
                    ref, tol = BE.const_invstd(c)
                    assert bool((np.abs(fw.istd.astype(np.float64) - ref) <= tol).all()), (n, C)
                mask = (fw.y > 0) if relu else None
                for with_addend in (False, True):
                    bw = BE.emulate_backward(c, fw, relu, with_addend, fused)
                    b = BE.bwd_ref(c, r, mask, with_addend)
                    mb = BE.backward_margins(b, bw)
                    if kind == 'ints':
                        assert np.array_equal(bw.sums[:C], b.sums[:C]) and np.array_equal(bw.dbeta.astype(np.float64), b.dbeta), (n, C)
                    ms.update({('dx_addend' if with_addend and k == 'dx' else k if k != 'sums' else 'bwd_sums'): v for k, v in mb.items()})
                    for k, v in ms.items():
                        worst[k] = max(worst.get(k, 0.0), v)
                        assert v <= 1.0, (kind, n, C, fused, relu, with_addend, k, v)
    print(f'bn_edges restatement {kind}: worst error / bound', {k: round(v, 4) for k, v in worst.items()})


# ============================================================================================================ 3. planted faults
def _run(c, relu, fault_f=None, fault_b=None, with_addend=False, fused=True):
    r = BE.stats_ref(c)
    fw = BE.emulate_forward(c, relu, fused, fault=fault_f)
    ms = BE.forward_margins(c, r, fw, relu)
    mask = (fw.y > 0) if relu else None                                # as on the device: the reference takes the forward's own mask
    bw = BE.emulate_backward(c, fw, relu, with_addend, fused, fault=fault_b)
    b = BE.bwd_ref(c, r, mask, with_addend)
    ms.update({'b_' + k: v for k, v in BE.backward_margins(b, bw).items()})
    return ms, fw, bw, r, b


def test_planted_faults_leave_the_bounds():
    # ---- one row dropped from the sums: outside the bounds at small n; at large n only the exact comparison of `ints` notices
    ms, *_ = _run(BE.make_case('randn', 70, 36), 1, fault_f='row_dropped')
    print('planted: one row dropped, randn n = 70: mean', ms['mean'], 'y', ms['y'], 'sums', ms['sums'])
    assert ms['mean'] > 1 and ms['y'] > 1 and ms['sums'] > 1
    c = BE.make_case('ints', 65537, 8)
    ms, fw, _, r, _ = _run(c, 1, fault_f='row_dropped')
    exact = np.array_equal(fw.sums, np.concatenate([r.s1, r.s2]))
    print('planted: one row dropped, ints n = 65537: y', ms['y'], 'mean', ms['mean'], 'sums bit-exact', exact)
    assert not exact and ms['sums'] > 1
    cr = BE.make_case('randn', 65537, 8)
    ms, *_ = _run(cr, 1, fault_f='row_dropped')
    print('planted: one row dropped, randn n = 65537: y', ms['y'], 'scale', ms['scale'], '(what a value bound alone gives at large n)')
    # ---- mean accumulated in fp32
    ms, *_ = _run(BE.make_case('offset', 65537, 8), 0, fault_f='fp32_mean')
    print('planted: fp32 mean, offset n = 65537: mean', ms['mean'], 'y', ms['y'])
    assert ms['mean'] > 1 and ms['y'] > 1
    # ---- the last 4-column group takes the neighbouring group's scale / shift
    ms, *_ = _run(BE.make_case('randn', 33, 64), 0, fault_f='last_group')
    print('planted: last column group from its neighbour: y', ms['y'])
    assert ms['y'] > 1
    # ---- shift with the wrong sign of beta
    ms, *_ = _run(BE.make_case('randn', 33, 64), 1, fault_f='beta_sign')
    print('planted: wrong sign of beta: shift', ms['shift'], 'y', ms['y'])
    assert ms['shift'] > 1 and ms['y'] > 1
    # ---- ReLU mask from >= 0: channel 1 (gamma = beta = 0) and the all-zero columns with beta ... have pre-activation exactly 0
    c = BE.make_case('const', 33, 64)
    ms, fw, *_ = _run(c, 1, fault_b='mask_ge')
    assert bool((fw.pre[:, 1] == 0).all())
    print('planted: mask from >= 0, const: dbeta', ms['b_dbeta'], 'bwd sums', ms['b_sums'])
    assert ms['b_dbeta'] > 1 and ms['b_sums'] > 1
    # ---- the row count off by one in backward
    ms, *_ = _run(BE.make_case('randn', 70, 36), 1, fault_b='count_off_by_one')
    print('planted: backward count n + 1, n = 70: dx', ms['b_dx'])
    assert ms['b_dx'] > 1
    ms, *_ = _run(BE.make_case('randn', 4097, 32), 0, fault_b='count_off_by_one', with_addend=True)
    print('planted: backward count n + 1, n = 4097, addend: dx', ms['b_dx'])
    assert ms['b_dx'] > 1
    # ---- and none of them planted: inside
    ms, *_ = _run(BE.make_case('randn', 70, 36), 1)
    assert max(ms.values()) <= 1.0, ms


def test_scale_shift_form_at_large_mean_over_std():
    """y = x scale + shift at |mean| / std = 1e4 carries ~u |mean| |scale| of absolute error: inside the bound, and far
    above what the same data gives once centred -- a property of the form, measured here on the restatement"""
    c = BE.make_case('offset', 4097, 32)
    r = BE.stats_ref(c)
    fw = BE.emulate_forward(c, 0, True)
    yr, yb = BE.y_ref(c, r, 0)
    err = np.abs(fw.y.astype(np.float64) - yr).max(0)
    big = np.abs(r.m) > 500
    print('scale / shift form, offset kind: worst |error| of y at |mean| = 1000:', err[big & (c.gamma != 0)].max(), 'at |mean| = 100:',
          err[~big & (c.gamma != 0)].max(), 'error / bound', BE.margin(fw.y, yr, yb))
    assert BE.margin(fw.y, yr, yb) <= 1.0
    assert 1e-5 < err[big & (c.gamma != 0)].max() < 5e-3
