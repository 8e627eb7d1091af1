"""csrc/criterion.hip on the edge cases of tests/_criterion_edges.py (cost ties around the (topk+1)-th value, predictions equal to /
touching their GT, zero extents and the union clamp, class bookkeeping up to GT 63, saturating logits, scattered class columns,
rotated-box degeneracies) against the fp64 CPU oracle's autograd (oracle/criterion.py, oracle/rotated_iou.py), and the two box-decode
kernels against an fp64 restatement of PredBBox + _bbox_pred_to_bbox."""
import pytest
import torch

import _criterion_edges as E
import _parity as PA
import test_criterion_edges_cpu as EC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name', E.CASES)
def test_fused_criterion_edge_case_matches_fp64_oracle(name):
    """``MODELS.build(cfg)`` on the ``_packed`` head outputs with ``fused = True`` (the kernel: ``_can_fuse`` is asserted) and again with
    ``fused = False`` (tensor ops on the device): loss and the gradients w.r.t. the packed logits / boxes against the fp64 oracle.
    Bounds as in test_gpu_ref_golden.py: loss 2e-6, gradients 2e-5 (axis-aligned), 1e-4 / 1e-3 (class / box, batches with rotated boxes).
    One block cannot meet them in any fp32 evaluation (test_criterion_edges_cpu.MEASURED): rotated_edges scene 1, headings 0 against
    pi/2 -- fp32 oracle against fp64 oracle 2.26e-2 on its box gradient, bound 4 x that = 9.1e-2; the kernel measures 2.26e-2 there
    as well (it takes the fp32 oracle's corner), and every other block of the case keeps the bounds above."""
    case, o64 = E.build(name)
    o32 = EC.oracle32(name)
    for fused in (True, False):
        loss, dcls, dbox, crit, pred, insts = EC.run_product(case, DEV, fused, True, scale=1.3)
        rec = EC.check_errors(case, loss, dcls, dbox, o64, o32, f'criterion_edges_{name}_{"fused" if fused else "tensor_ops"}')
        PA.log_errors(f'criterion_edges_{name}_{"fused" if fused else "tensor_ops"}', rec)


def _al64(x):
    return (x + 63) & ~63


@pytest.mark.parametrize('name', E.CASES)
def test_fused_criterion_matched_sets_targets_and_foreign_columns(name):
    """u3d_criterion_packed through the C ABI with a workspace of the test's own and output buffers pre-filled with a sentinel: the
    64-bit matched-GT mask of every (layer, query) equals the fp64 oracle's matched set bit for bit (ties at the kth value unmatched,
    bit 63 included), the class target read off it (label of the highest set bit) equals the oracle's, every element of dcls / dbox
    is written, and dcls is exactly 0 in every column a scene does not own."""
    from unidet3d_amd import _lib as L
    from unidet3d_amd.registry import MODELS
    case, o64 = E.build(name)
    crit = MODELS.build(EC.CFG[case['crit']])
    insts = EC.product_insts(case, DEV)
    cls, box = torch.stack(case['cls']).to(DEV).contiguous(), torch.stack(case['box']).to(DEV).contiguous()
    Ln, n_tot, CU = cls.shape
    B, bd, names, cidx = len(insts), box.shape[-1], case['names'], case['cidx']
    idxs = [crit.datasets.index(n) for n in names]
    c1s = [len(c) for c in cidx] if cidx is not None else [CU] * B
    yaw = case['yaw'] or [bd == 7] * B
    g = crit._flat_gt(insts, case['sizes'], DEV, [crit.topk[i] for i in idxs], [crit.datasets_weights[i] for i in idxs], c1s, yaw, cidx, bd)
    assert g is not None
    consts = (float(crit.matcher.costs[0].weight), float(crit.matcher.costs[1].weight), float(crit.non_object_weight),
              float(crit.loss_weight[0]), float(crit.loss_weight[1]))
    SENT = 12345.0
    loss = torch.full((1,), SENT, device=DEV)
    dcls, dbox = torch.full_like(cls, SENT), torch.full_like(box, SENT)
    ws = torch.zeros(L.lib().u3d_criterion_ws_bytes(Ln, B, n_tot, g['G'], g['P']), dtype=torch.uint8, device=DEV)
    L.call('u3d_criterion_packed', L.ptr(cls), L.ptr(box), L.ptr(g['cu']), L.ptr(g['gt_off']), L.ptr(g['labels']), L.ptr(g['boxes']),
           L.ptr(g['qmask']), L.ptr(g['qm_off']), L.ptr(g['meta']), L.ptr(g['scene_w']), L.ptr(g['cidx']), Ln, B, n_tot, CU, bd,
           g['G'], g['P'], g['max_gt'], g['slack'], *consts, L.ptr(loss), L.ptr(dcls), L.ptr(dbox), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    off = _al64(Ln * g['P'] * 4) + _al64(Ln * n_tot * 4) + _al64(Ln * g['G'] * 4)            # cost, logz, kth precede the match masks
    mm = ws[off:off + Ln * n_tot * 8].view(torch.int64).view(Ln, n_tot).cpu()
    dcls, dbox = dcls.cpu(), dbox.cpu()
    assert abs(float(loss) - float(o64['loss'])) < 2e-6 * abs(float(o64['loss']))
    assert not bool((dcls == SENT).any()) and not bool((dbox == SENT).any())
    for l in range(Ln):
        o = 0
        for b, n in enumerate(case['sizes']):
            labels, want = case['gt'][b]['labels'], o64['matched'][l][b]
            bits = mm[l, o:o + n]
            got = torch.stack([(bits >> j) & 1 for j in range(len(labels))], 1).bool() if len(labels) else torch.zeros(n, 0, dtype=torch.bool)
            assert torch.equal(got, want), (name, l, b, (got != want).nonzero().tolist())
            assert bool(((bits >> len(labels)) == 0).all()) if len(labels) < 64 else True       # no bit beyond the scene's GTs
            last = (got * torch.arange(1, len(labels) + 1)).amax(1) - 1 if len(labels) else torch.full((n,), -1)
            n_cls = E.N_CLS[names[b]]
            target = torch.where(last >= 0, labels[last.clamp(min=0)] if len(labels) else last, n_cls)
            assert torch.equal(target, o64['target'][l][b])
            own = cidx[b] if cidx is not None else list(range(CU))
            rows = dcls[l, o:o + n]
            # the one-hot position of the class gradient: softmax - onehot is negative at the target only (where the row's
            # softmax has not saturated to exactly 1 at the target, which the cost-free read above covers)
            neg = rows[:, own] < 0
            assert bool((neg.sum(1) <= 1).all()) and bool((neg.float().argmax(1)[neg.any(1)] == target[neg.any(1)]).all())
            foreign = [c for c in range(CU) if c not in own]
            assert float(rows[:, foreign].abs().max()) == 0 if foreign else True
            if bd == 7 and not yaw[b]:
                assert float(dbox[l, o:o + n, 6].abs().max()) == 0                                  # a heading column the scene does not use
            o += n
    if name == 'scattered_columns':
        assert cidx is not None and all(len(set(range(CU)) - set(c)) > 0 for c in cidx)


# ---------------------------------------------------------------------------------------------------------------- box decode
def _decode_ref(raw, cen, yaw_rows, dof):
    """PredBBox.decode (exp of the six face distances) + _bbox_pred_to_bbox, restated: rows with a heading -> (centre, w = S / (1 + q),
    l = w q, size_z, atan2(r6, r7) / 2) with S = e0 + e1 + e2 + e3, q = exp(|(r6, r7)|); rows without -> (centre, size[, 0])"""
    e = torch.exp(raw[:, :6])
    centre = cen + (e[:, 1::2] - e[:, 0::2]) / 2
    size = e[:, 0::2] + e[:, 1::2]
    if dof == 6:
        return torch.cat((centre, size), 1)
    S = e[:, 0] + e[:, 1] + e[:, 2] + e[:, 3]
    q = torch.exp(torch.sqrt(raw[:, 6] ** 2 + raw[:, 7] ** 2))
    alpha = 0.5 * torch.atan2(raw[:, 6], raw[:, 7])
    rot = torch.cat((centre, (S / (1 + q))[:, None], (S / (1 + q) * q)[:, None], size[:, 2:3], alpha[:, None]), 1)
    if yaw_rows is None:
        return rot
    return torch.where(yaw_rows.bool()[:, None], rot, torch.cat((centre, size, torch.zeros_like(alpha)[:, None]), 1))


def _decode_inputs(M):
    """raw [M, 8], centres [M, 3], upstream gradient seeds; the first rows are the edge rows (cycled when M is small), the last row is
    a +-20 row so that the tail of the last block is not a quiet one"""
    g = torch.Generator().manual_seed(M)
    raw = torch.randn(M, 8, generator=g)
    cen = torch.rand(M, 3, generator=g) * 4
    special = [
        lambda r: r.__setitem__(slice(6, 8), 0.0),                              # 0: r6 = r7 = 0 (even row)
        lambda r: r.__setitem__(slice(6, 8), 0.0),                              # 1: r6 = r7 = 0 (odd row)
        lambda r: (r.__setitem__(7, 0.0), r.__setitem__(6, 0.75)),              # 2: r7 = 0, r6 != 0
        lambda r: (r.__setitem__(7, 0.0), r.__setitem__(6, -1.5)),              # 3: the same on an odd row, r6 < 0
        lambda r: r.__setitem__(slice(0, 8), torch.tensor([20., -20, 20, -20, -20, 20, 20, -20])),     # 4: +-20
        lambda r: r.__setitem__(4, 88.5),                                       # 5: expf still finite (2.7e38)
        lambda r: r.__setitem__(1, 88.5),                                       # 6: the same inside S = e0 + .. + e3
        lambda r: (r.__setitem__(0, -104.0), r.__setitem__(3, -104.0)),         # 7: the size underflows towards 0
    ]
    for i in range(min(M, len(special))):
        special[i](raw[i])
    if M > len(special):
        raw[M - 1] = torch.tensor([-20., 20, -20, 20, 20, -20, -20, 20])
    up = (torch.rand(M, 7, generator=g) - 0.5) * 0.5                             # |.| <= 1/4: e * de stays finite on the 88.5 rows
    return raw, cen, up


def _check_rows(got, ref64, ref32, what):
    """1e-6 of the row's largest reference entry on finite outputs; an infinity sits where the fp32 restatement has it"""
    got, ref64 = got.double().cpu(), ref64.double()
    inf32 = torch.isinf(ref32)
    assert torch.equal(torch.isinf(got) & inf32, inf32) and torch.equal(got[inf32], ref32.double()[inf32]), what
    fin = torch.isfinite(ref32) & torch.isfinite(ref64)
    assert bool(torch.isfinite(got[fin]).all()), what
    scale = torch.where(fin, ref64.abs(), torch.zeros_like(ref64)).amax(1, keepdim=True)
    err = torch.where(fin, (got - ref64).abs(), torch.zeros_like(ref64)) / scale.clamp(min=1e-30)
    assert float(err.max()) <= 1e-6, (what, float(err.max()), err.argmax())
    return float(err.max())


@pytest.mark.parametrize('M', [1, 255, 257, 1000])
@pytest.mark.parametrize('form', ['six', 'none', 'zeros', 'alternating'])
def test_box_decode_kernels_match_fp64_restatement(M, form):
    """_BoxDecodeFn ('six') and _BoxDecode7Fn with ``yaw_rows`` None / all zero / alternating, forward and backward, against the fp64
    restatement; M around the 256-thread block.  Rows with r6 = r7 = 0: torch's own backward is 0 * inf = NaN there (sqrt and atan2 at
    the origin); the kernel's documented answer is a ZERO heading gradient (box_decode7_bwd_k's rho2 > 0 guard), which this test pins."""
    from unidet3d_amd.encoder import _BoxDecode7Fn, _BoxDecodeFn
    raw, cen, up = _decode_inputs(M)
    dof = 6 if form == 'six' else 7
    yaw = dict(six=None, none=None, zeros=torch.zeros(M, dtype=torch.uint8), alternating=(torch.arange(M) % 2 == 0).to(torch.uint8))[form]
    up = up[:, :dof]
    refs = {}
    for dt in (torch.float64, torch.float32):
        r = raw.detach().clone().to(dt).requires_grad_()
        out = _decode_ref(r, cen.to(dt), yaw, dof)
        (out * up.to(dt)).sum().backward()
        refs[dt] = (out.detach(), r.grad)
    has_yaw = torch.ones(M, dtype=torch.bool) if (dof == 7 and yaw is None) else (yaw.bool() if dof == 7 else torch.zeros(M, dtype=torch.bool))
    rho0 = (raw[:, 6] == 0) & (raw[:, 7] == 0) & has_yaw
    for dt in refs:                                                               # the pinned answer replaces torch's NaN on those rows
        assert bool(torch.isnan(refs[dt][1][rho0][:, 6:]).all())
        refs[dt][1][rho0, 6:] = 0.0
    r = raw.detach().clone().to(DEV).requires_grad_()
    yd = yaw.to(DEV) if yaw is not None else None
    out = _BoxDecodeFn.apply(r, cen.to(DEV)) if dof == 6 else _BoxDecode7Fn.apply(r, cen.to(DEV), yd)
    (out * up.to(DEV)).sum().backward()
    assert out.shape == (M, dof) and r.grad.shape == (M, 8)
    e_f = _check_rows(out.detach(), refs[torch.float64][0], refs[torch.float32][0], 'forward')
    e_b = _check_rows(r.grad, refs[torch.float64][1], refs[torch.float32][1], 'backward')
    g = r.grad.cpu()
    assert float(g[rho0][:, 6:].abs().max()) == 0 if bool(rho0.any()) else True
    assert float(g[~has_yaw][:, 6:].abs().max()) == 0 if bool((~has_yaw).any()) else True    # no heading: its raw columns get no gradient
    if M == 1000 and form == 'alternating':
        PA.log_errors('box_decode_edges', dict(forward=e_f, backward=e_b))
