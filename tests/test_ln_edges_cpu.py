"""Host-side checks of tests/_ln_edges.py, the helper behind tests/test_gpu_ln_edges.py: its float64 references agree with torch's
layer norm in float64, the case lists reach the template, lane-slot and loop edges of csrc/norm.hip they are meant for, a host model
of the kernels in fp32 numpy (three summation orders, the kernels' own among them) stays inside every acceptance bound for every
value kind and width, and every planted fault is rejected by the check named next to it.  No GPU."""
import numpy as np
import pytest
import torch

import _ln_edges as LE


def _fwd_bwd(c, order='lanes', with_res=True, fault_f=None, fault_b=None, twice=None, ints_bwd=None):
    """model forward, then model backward on the model's own s and stats (`ints`: on the unit stats the GPU test passes)"""
    with np.errstate(invalid='ignore', over='ignore'):      # a planted fault may put an infinity into the statistics
        fw = LE.model_forward(c, with_res, order, fault=fault_f)
        ints = c.kind == 'ints' if ints_bwd is None else ints_bwd
        stats = LE.unit_stats(c.M) if ints else fw.stats
        bw = LE.model_backward(fw.s, stats, c.gamma, c.dy, c.dy2, c.dy3, order, fault=fault_b, twice=twice)
        ref = LE.bwd_ref(fw.s, stats, c.gamma, LE.grad_sum(c.dy, c.dy2, c.dy3))
        ms = LE.forward_margins(fw.s, fw, c.gamma, c.beta)
        ms.update(LE.backward_margins(ref, bw))
    return ms, fw, bw, ref


def _ints_exact(bw, ref):
    return np.array_equal(bw.dgamma.astype(np.float64), ref.dgamma) and np.array_equal(bw.dbeta.astype(np.float64), ref.dbeta)


# ============================================================================================================ 1. references
@pytest.mark.parametrize('C', [36, 260])
def test_references_agree_with_torch_float64(C):
    c = LE.make_case('randn', 23, C)
    s = LE.row_sum_in(c)
    r = LE.fwd_ref(s)
    d = LE.grad_sum(c.dy, c.dy2, c.dy3)
    so = torch.from_numpy(s).double().requires_grad_()
    w, b = torch.from_numpy(c.gamma).double().requires_grad_(), torch.from_numpy(c.beta).double().requires_grad_()
    yo = torch.nn.functional.layer_norm(so, (C,), w, b, LE.EPS)
    yo.backward(torch.from_numpy(d).double())
    stats = np.stack([r.m, r.rstd], 1)
    y2, _ = LE.y_ref(s, stats, c.gamma, c.beta)
    kw = dict(rtol=1e-12, atol=1e-12)
    assert np.allclose(y2, yo.detach().numpy(), **kw)
    ref = LE.bwd_ref(s, stats, c.gamma, d)                 # float64 stats in: np.asarray(..., F64) keeps them
    assert np.allclose(ref.dx, so.grad.numpy(), **kw) and np.allclose(ref.dgamma, w.grad.numpy(), **kw) and np.allclose(ref.dbeta, b.grad.numpy(), **kw)


def test_case_lists_reach_the_edges_they_name():
    assert [LE.template(C) for C in (4, 256, 260, 512, 516, 768, 772, 1024)] == [1, 1, 2, 2, 4, 4, 4, 4]
    fill = {(-(-(C // 4) // 64), (C // 4) % 64 == 0) for C in LE.WIDTHS}         # (slots in use, last slot full)
    assert fill == {(n, f) for n in (1, 2, 3, 4) for f in (False, True)}
    assert {260, 508, 772, 1020} <= set(LE.WIDTHS) and all(C % 4 == 0 and 4 <= C <= 1024 for C in LE.WIDTHS)
    assert any(C % 64 for C in LE.NB_WIDTHS) and any(C % 64 == 0 for C in LE.NB_WIDTHS)
    assert [LE.ln_blocks(M) for M in (0, 1, 4, 5, 2048, 2049, 65535, 65536, 65537)] == [1, 1, 1, 2, 512, 512, 512, 1024, 1024]
    assert LE.ws_bytes(0, 64) == 2 * 64 * 4 + 256 and LE.ws_bytes(65536, 64) == 1024 * 2 * 64 * 4 + 256
    for nb in LE.NB_EDGES:
        assert LE.ln_blocks(4 * nb) == nb and LE.ln_blocks(4 * nb - 3) == nb
    # the loops of layer_norm_reduce_k in nb: wave w is idle below nb = w + 1; the unrolled loop runs once from nb = 49 (wave 0) to
    # 64 (wave 15), twice from 113; the tail runs 0 .. 3 times
    unrolled = lambda nb, w: len(range(w, max(nb - 48, w), 64))            # noqa: E731
    assert [unrolled(nb, 0) for nb in (48, 49, 112, 113, 512)] == [0, 1, 1, 2, 8] and [unrolled(nb, 15) for nb in (63, 64, 127, 128)] == [0, 1, 1, 2]
    assert {15, 16, 17, 47, 48, 49, 63, 64, 65, 111, 112, 113, 127, 128, 129} <= set(LE.NB_EDGES)
    assert max(LE.nb_rows()) == 2048 and min(LE.nb_rows()) == 1
    for M in LE.CAPPED_ROWS:                                                       # the row-stride loop takes a ragged last trip
        assert -(-M // 4) > LE.ln_blocks(M) or M in (65535,)
    assert LE.ln_blocks(65535) == 512 and -(-65535 // (4 * 512)) == 32 and LE.ln_blocks(65537) == 1024
    # value kinds
    c = LE.make_case('const', 9, 64)
    s = LE.row_sum_in(c)
    for i, v in zip(range(0, 9, 2), (0.0, 3.7, -1e3, 1e-20, 0.0)):
        assert bool((s[i] == np.float32(v)).all())
    assert not bool((s[1] == s[1, 0]).all())
    assert c.gamma[1] == 0 and c.beta[1] == 0 and c.gamma[-1] == 0 and bool((c.gamma[2:-1] != 0).all())
    c = LE.make_case('ints', 65537, 64)
    s = LE.row_sum_in(c)
    assert float(np.abs(s).max()) == 4 and set(np.unique(np.abs(c.gamma))) == {0.0, 1.0, 2.0}
    d = LE.grad_sum(c.dy, c.dy2, c.dy3).astype(np.float64)
    assert float(np.abs(d * s).sum(0).max()) < 2 ** 24 and float(np.abs(d).sum(0).max()) < 2 ** 24     # every partial sum is exact
    c = LE.make_case('randn', 131, 64)
    assert not LE.same_bits(LE.grad_sum(c.dy, c.dy2, c.dy3), LE.grad_sum(c.dy, c.dy3, c.dy2))              # the order of the sum shows
    c = LE.make_case('tiny', 5, 64)
    s = LE.row_sum_in(c)
    assert float(((s - s.mean(1, keepdims=True)) ** 2).max()) < 2.0 ** -126                                 # the squares underflow
    c = LE.make_case('spike', 5, 64)
    assert bool((np.abs(LE.row_sum_in(c)).max(1) > 9e5).all())
    c = LE.make_case('offset', 131, 64)
    assert {round(float(v), -1) for v in LE.row_sum_in(c).mean(1)} == {-100.0, 100.0, 1000.0}
    assert LE.bf16_bits(np.array([1.0, 1.00390625, 1.01171875, -3.0e38], np.float32)).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xFF62]


def test_bf16_restatement_is_torch_round_to_nearest_even():
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-20, 20, 4096), [0.0, -0.0, 1.00390625, 1.01171875]]).astype(np.float32)
    t = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(LE.bf16_bits(a), t)
    assert not np.array_equal(LE.bf16_bits(a, truncate=True), t)


# ============================================================================================================ 2. bounds
@pytest.mark.parametrize('kind', LE.KINDS)
def test_host_model_stays_inside_every_bound(kind):
    """A condition, not a measurement: the model's three summation orders at every width, with and without the residual."""
    worst = {}
    for C in LE.WIDTHS:
        for M in (5, 131) if C in (64, 260, 772) else (5,):
            c = LE.make_case(kind, M, C)
            for order in LE.ORDERS:
                for with_res in (True, False):
                    ms, fw, bw, ref = _fwd_bwd(c, order, with_res)
                    y4 = LE.margin(fw.y, *LE.y_ref(fw.s, fw.stats, c.gamma, c.beta, coeff=4))
                    worst['y_coeff4'] = max(worst.get('y_coeff4', 0.0), y4)
                    if kind == 'ints':
                        assert LE.same_bits(fw.stats[:, 0], LE.exact_mean(fw.s)), (C, M, order)
                        assert _ints_exact(bw, ref), (C, M, order)
                    if kind == 'tiny':
                        assert np.allclose(fw.stats[:, 1], 1 / np.sqrt(LE.EPS), rtol=4 * LE.U, atol=0), (C, M, order)
                    if kind == 'const':
                        rows = slice(0, M, 2)
                        cr, cb = LE.const_row_rstd(fw.s[rows, 0], fw.stats[rows, 0], C)
                        assert LE.margin(fw.stats[rows, 1], cr, cb) <= 1.0, (C, M, order)
                    assert bool((fw.y[:, 1] == 0).all()) and LE.same_bits(fw.y[:, -1], np.broadcast_to(c.beta[-1], (M,)).copy())
                    for k, v in ms.items():
                        worst[k] = max(worst.get(k, 0.0), v)
                        assert v <= 1.0, (kind, C, M, order, with_res, k, v)
    print(f'ln_edges host model {kind}: worst error / bound', {k: round(v, 4) for k, v in worst.items()})
    assert worst['y_coeff4'] <= 1.0                      # the bound in use (5) keeps one rounding spare


@pytest.mark.parametrize('M,C', [(4 * 49, 36), (4 * 113 - 3, 64), (2049, 64), (2049, 516)])
def test_host_model_in_the_kernels_row_order_is_exact_on_integers(M, C):
    c = LE.make_case('ints', M, C)
    ms, fw, bw, ref = _fwd_bwd(c)
    assert max(ms.values()) <= 1.0, ms
    assert _ints_exact(bw, ref)
    c = LE.make_case('randn', M, C)
    ms, *_ = _fwd_bwd(c)
    assert max(ms.values()) <= 1.0, ms


# ============================================================================================================ 3. planted faults
def test_planted_forward_faults_are_rejected():
    # ---- mean over the row without its last float4: the mean check (and the exact mean of `ints`)
    ms, *_ = _fwd_bwd(LE.make_case('randn', 5, 64), fault_f='mean_short')
    print('planted: last float4 left out of the mean, randn C = 64: mean', ms['mean'])
    assert ms['mean'] > 1
    c = LE.make_case('ints', 9, 1024)
    _, fw, *_ = _fwd_bwd(c, fault_f='mean_short')
    assert not LE.same_bits(fw.stats[:, 0], LE.exact_mean(fw.s))
    # ---- variance divided by C - 1: the rstd check, at the widest row too (relative 1 / 2C against ~C u / 2)
    for C in (64, 1024):
        ms, *_ = _fwd_bwd(LE.make_case('randn', 5, C), fault_f='var_c_minus_1')
        print('planted: var / (C - 1), C =', C, ': rstd', ms['rstd'], 'y', ms['y'])
        assert ms['rstd'] > 1 and ms['mean'] <= 1 and ms['y'] <= 1          # y is checked on the device's own stats: only rstd sees it
    # ---- eps omitted: the rstd check on the constant rows
    ms, fw, *_ = _fwd_bwd(LE.make_case('const', 9, 64), fault_f='no_eps')
    print('planted: no eps, const: rstd', ms['rstd'])
    assert ms['rstd'] > 1
    # ---- the partly filled last lane slot skipped: the mean check
    for C in (260, 772):
        for kind in ('randn', 'ints'):
            ms, fw, *_ = _fwd_bwd(LE.make_case(kind, 5, C), fault_f='skip_last_slot')
            print('planted: last lane slot skipped, C =', C, kind, ': mean', ms['mean'])
            assert ms['mean'] > 1
        assert not LE.same_bits(fw.stats[:, 0], LE.exact_mean(fw.s))
    # ---- y from the neighbouring row's statistics: the y check
    ms, *_ = _fwd_bwd(LE.make_case('randn', 5, 64), fault_f='neighbour_stats')
    print('planted: y from the next row`s stats: y', ms['y'])
    assert ms['y'] > 1 and ms['mean'] <= 1 and ms['rstd'] <= 1
    # ---- bf16 by truncation: the bit comparison with the rounded fp32 result
    fw = LE.model_forward(LE.make_case('randn', 5, 64), fault='bf16_trunc')
    good = torch.from_numpy(fw.y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert not np.array_equal(fw.y16, good) and np.array_equal(LE.model_forward(LE.make_case('randn', 5, 64)).y16, good)


def test_planted_backward_faults_are_rejected():
    # ---- one row left out of dgamma / dbeta at M = 65537: ONLY the exact comparison of `ints` notices
    c = LE.make_case('ints', 65537, 64)
    ms, _, bw, ref = _fwd_bwd(c, fault_b='row_skipped')
    assert not _ints_exact(bw, ref)
    ms0, _, bw0, _ = _fwd_bwd(c)
    assert _ints_exact(bw0, ref) and max(ms0.values()) <= 1
    cr = LE.make_case('randn', 65537, 64)
    ms, *_ = _fwd_bwd(cr, fault_b='row_skipped')
    print('planted: one row skipped, randn M = 65537: dgamma', ms['dgamma'], 'dbeta', ms['dbeta'], '(what a value bound alone gives at large M)')
    assert ms['dgamma'] <= 1 and ms['dbeta'] <= 1
    ms, *_ = _fwd_bwd(LE.make_case('randn', 5, 64), fault_b='row_skipped')          # at small M the bounds do
    assert ms['dgamma'] > 1 and ms['dbeta'] > 1
    # ---- one partial row added twice in the reduce, at the first nb with one / two trips of the unrolled loop
    for nb, tw in ((49, 48), (113, 112)):
        c = LE.make_case('ints', 4 * nb, 36)
        _, _, bw, ref = _fwd_bwd(c, twice=tw)
        assert not _ints_exact(bw, ref), nb
        _, _, bw, ref = _fwd_bwd(c)
        assert _ints_exact(bw, ref), nb
        ms, *_ = _fwd_bwd(LE.make_case('randn', 4 * nb, 36), twice=tw)
        print('planted: partial row', tw, 'added twice, nb =', nb, ': randn dgamma', ms['dgamma'], 'dbeta', ms['dbeta'])
        assert ms['dgamma'] > 1 or ms['dbeta'] > 1
    # ---- dgamma and dbeta swapped; dgamma shifted by the C % 64 straddle: the bounds and the exact comparison
    for fault in ('swapped', 'straddle_shift'):
        for kind in ('randn', 'ints'):
            ms, _, bw, ref = _fwd_bwd(LE.make_case(kind, 131, 36), fault_b=fault)
            print('planted:', fault, kind, ': dgamma', ms['dgamma'], 'dbeta', ms['dbeta'])
            assert ms['dgamma'] > 1
            assert kind != 'ints' or not _ints_exact(bw, ref)
    # ---- bf16 by truncation
    c = LE.make_case('randn', 5, 64)
    fw = LE.model_forward(c)
    bw = LE.model_backward(fw.s, fw.stats, c.gamma, c.dy, fault='bf16_trunc')
    assert not np.array_equal(bw.dx16, torch.from_numpy(bw.dx).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    # ---- dy3 added before dy2: the bit comparison with the plain backward fed the sum in the kernel's order (the bounds, referred
    # to that same sum, stay inside: a one-ulp matter)
    c = LE.make_case('randn', 131, 64)
    fw = LE.model_forward(c)
    plain = LE.model_backward(fw.s, fw.stats, c.gamma, LE.grad_sum(c.dy, c.dy2, c.dy3))
    good = LE.model_backward(fw.s, fw.stats, c.gamma, c.dy, c.dy2, c.dy3)
    bad = LE.model_backward(fw.s, fw.stats, c.gamma, c.dy, c.dy2, c.dy3, fault='dy3_first')
    assert LE.same_bits(good.dx, plain.dx) and LE.same_bits(good.dgamma, plain.dgamma) and LE.same_bits(good.dbeta, plain.dbeta)
    assert not LE.same_bits(bad.d, plain.d) and not LE.same_bits(bad.dx, plain.dx)
    # ---- a neighbour row's stats: the dx check
    for kind in ('randn', 'offset'):
        ms, *_ = _fwd_bwd(LE.make_case(kind, 131, 64), fault_b='neighbour_stats')
        print('planted: backward reads the next row`s stats,', kind, ': dx', ms['dx'], 'dgamma', ms['dgamma'])
        assert ms['dx'] > 1
    # ---- and none planted: inside
    ms, *_ = _fwd_bwd(LE.make_case('randn', 131, 36))
    assert max(ms.values()) <= 1.0, ms
