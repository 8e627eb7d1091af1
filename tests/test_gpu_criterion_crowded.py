"""csrc/criterion.hip on scenes with more than 64 ground-truth boxes (tests/_criterion_crowded.py): multi-word match masks and the
pair-parallel cost kernel against the fp64 CPU oracle's autograd, the masks themselves bit for bit through the C ABI, the entry
point's size checks, run-to-run determinism, and one small batch through ``UniDet3D.loss`` with the kernel against the tensor-op
formulation."""
import ctypes

import numpy as np
import pytest
import torch

import _criterion_crowded as C
import _criterion_edges as E
import _parity as PA
import test_criterion_edges_cpu as EC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U3D_OK, U3D_EUNSUPPORTED = 0, -3


@pytest.mark.parametrize('name', C.CASES)
def test_fused_criterion_crowded_case_matches_fp64_oracle(name):
    """``fused = True`` (the kernel: ``_can_fuse`` is asserted by ``EC.run_product`` and ``_loss_fused`` must not decline) and
    ``fused = False`` (tensor ops on the device) against the fp64 oracle under the bounds of test_gpu_criterion_edges.py: loss 2e-6,
    gradients 2e-5 per block (axis-aligned batches), 1e-4 / 1e-3 (class / box) for crowded_mixed with its rotated scene.  No block
    needs a measured bound (``C.MEASURED`` is empty: test_criterion_crowded_cpu.py holds the fp32 oracle to 1e-4 on every block)."""
    case, o64 = C.build(name)
    o32 = C.oracle32(name)
    for fused in (True, False):
        loss, dcls, dbox, crit, pred, insts = EC.run_product(case, DEV, fused, True, scale=1.3)
        if fused:
            assert crit._can_fuse(pred, insts, case['names'])
            assert crit._loss_fused(pred['_packed'], insts, case['names']) is not None
        tag = f'criterion_crowded_{name}_{"fused" if fused else "tensor_ops"}'
        PA.log_errors(tag, C.check_errors(case, loss, dcls, dbox, o64, o32, tag))


def _al64(x):
    return (x + 63) & ~63


def _abi_args(case, g, cls, box, loss, dcls, dbox, ws, **over):
    from unidet3d_amd import _lib as L
    crit = over.pop('crit')
    consts = (float(crit.matcher.costs[0].weight), float(crit.matcher.costs[1].weight), float(crit.non_object_weight),
              float(crit.loss_weight[0]), float(crit.loss_weight[1]))
    Ln, n_tot, CU = cls.shape
    v = dict(L=Ln, B=g['B'], n_tot=n_tot, CU=CU, BD=box.shape[-1], G=g['G'], P=g['P'], max_gt=g['max_gt'], slack=g['slack'])
    v.update(over)
    return (L.ptr(cls), L.ptr(box), L.ptr(g['cu']), L.ptr(g['gt_off']), L.ptr(g['labels']), L.ptr(g['boxes']), L.ptr(g['qmask']),
            L.ptr(g['qm_off']), L.ptr(g['meta']), L.ptr(g['scene_w']), L.ptr(g['cidx']), v['L'], v['B'], v['n_tot'], v['CU'], v['BD'],
            v['G'], v['P'], v['max_gt'], v['slack'], *consts, L.ptr(loss), L.ptr(dcls), L.ptr(dbox), L.ptr(ws), L.stream())


@pytest.mark.parametrize('name', C.CASES)
def test_fused_criterion_multi_word_masks_targets_and_foreign_columns(name):
    """u3d_criterion_packed through the C ABI with a workspace of the test's own and sentinel-filled outputs: every word of every
    (layer, query) match mask equals the fp64 oracle's matched set bit for bit -- hence no bit at or beyond the scene's GT count in any
    word --, the class target read off the highest set bit equals the oracle's, every element of dcls / dbox is written, and the
    foreign class columns and an unused heading column are exactly 0."""
    from unidet3d_amd import _lib as L
    case, o64 = C.build(name)
    crit, insts, g = C.flat_gt(case, DEV)
    assert g is not None and g['max_gt'] > 64
    cls, box = torch.stack(case['cls']).to(DEV).contiguous(), torch.stack(case['box']).to(DEV).contiguous()
    Ln, n_tot, CU = cls.shape
    bd, names, cidx = box.shape[-1], case['names'], case['cidx']
    yaw = case['yaw'] or [bd == 7] * g['B']
    W = (g['max_gt'] + 63) // 64
    SENT = 12345.0
    loss = torch.full((1,), SENT, device=DEV)
    dcls, dbox = torch.full_like(cls, SENT), torch.full_like(box, SENT)
    nbytes = L.lib().u3d_criterion_ws_bytes_gt(Ln, g['B'], n_tot, g['G'], g['P'], g['max_gt'])
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    L.call('u3d_criterion_packed', *_abi_args(case, g, cls, box, loss, dcls, dbox, ws, crit=crit))
    torch.cuda.synchronize()
    off = _al64(Ln * g['P'] * 4) + _al64(Ln * n_tot * 4) + _al64(Ln * g['G'] * 4)            # cost, logz, kth precede the match words
    mm = ws[off:off + Ln * n_tot * W * 8].view(torch.int64).view(Ln, n_tot, W).cpu()
    dcls, dbox = dcls.cpu(), dbox.cpu()
    assert abs(float(loss) - float(o64['loss'])) < 2e-6 * abs(float(o64['loss']))
    assert not bool((dcls == SENT).any()) and not bool((dbox == SENT).any())
    for l in range(Ln):
        o = 0
        for b, n in enumerate(case['sizes']):
            labels, want = case['gt'][b]['labels'], o64['matched'][l][b]
            words = mm[l, o:o + n]
            assert torch.equal(words, C.match_words(want, W)), (name, l, b)                    # all W words, bits past the GT count included
            bits = torch.stack([(words[:, j >> 6] >> (j & 63)) & 1 for j in range(W * 64)], 1).bool()
            assert not bool(bits[:, len(labels):].any())
            last = (bits * torch.arange(1, W * 64 + 1)).amax(1) - 1
            n_cls = E.N_CLS[names[b]]
            target = torch.where(last >= 0, labels[last.clamp(min=0, max=max(len(labels) - 1, 0))] if len(labels) else last, n_cls)
            assert torch.equal(target, o64['target'][l][b])
            own = cidx[b] if cidx is not None else list(range(CU))
            rows = dcls[l, o:o + n]
            neg = rows[:, own] < 0                                                               # softmax - onehot is negative at the target only
            assert bool((neg.sum(1) <= 1).all()) and bool((neg.float().argmax(1)[neg.any(1)] == target[neg.any(1)]).all())
            foreign = [c for c in range(CU) if c not in own]
            assert float(rows[:, foreign].abs().max()) == 0 if foreign else True
            if bd == 7 and not yaw[b]:
                assert float(dbox[l, o:o + n, 6].abs().max()) == 0
            o += n
    if name == 'crowded_last_bit':
        for l in range(Ln):
            assert mm[l, 5].tolist() == [1 - (1 << 63), 1 - (1 << 63)] and mm[l, 9].tolist() == [0, 1]     # bits 0 and 63 of both words; bit 64
            want = o64['dbox'][l][5]
            assert float((dbox[l, 5].double() - want).abs().max()) < 2e-5 * float(o64['dbox'][l][:30].abs().max())


def test_entry_point_takes_65_gts_and_refuses_a_scene_beyond_32_bit_indexing():
    """max_gt = 65 is U3D_OK (it was U3D_EUNSUPPORTED).  A scene whose n_b * g_b cannot be indexed in 32 bits is refused with
    U3D_EUNSUPPORTED and a message before anything is launched: the sizes are passed as integers over the same tiny real buffers, and
    the sentinel-filled outputs stay untouched."""
    from unidet3d_amd import _lib as L
    g_ = E._gen(11)
    case = E._pack('sixty_five', 'scannet', [E._random_scene(g_, 'scannet', 12, 65)], g_)
    crit, insts, g = C.flat_gt(case, DEV)
    assert g is not None and g['max_gt'] == 65
    cls, box = torch.stack(case['cls']).to(DEV).contiguous(), torch.stack(case['box']).to(DEV).contiguous()
    SENT = 12345.0
    loss = torch.full((1,), SENT, device=DEV)
    dcls, dbox = torch.full_like(cls, SENT), torch.full_like(box, SENT)
    lib = L.lib()
    ws = torch.zeros(lib.u3d_criterion_ws_bytes_gt(2, 1, 12, 65, 12 * 65, 65), dtype=torch.uint8, device=DEV)
    # one scene of 70 000 queries x 40 000 GTs = 2.8e9 entries > 2^31 - 1
    rc = lib.u3d_criterion_packed(*_abi_args(case, g, cls, box, loss, dcls, dbox, ws, crit=crit, n_tot=70_000, G=40_000, P=70_000 * 40_000,
                                             max_gt=40_000))
    torch.cuda.synchronize()
    assert rc == U3D_EUNSUPPORTED
    msg = lib.u3d_last_error().decode()
    assert '32-bit' in msg and '40000' in msg and '70000' in msg, msg
    assert float(loss) == SENT and bool((dcls == SENT).all()) and bool((dbox == SENT).all())
    assert lib.u3d_criterion_ws_bytes_gt(2, 1, 12, 65, 12 * 65, 65) > lib.u3d_criterion_ws_bytes(2, 1, 12, 65, 12 * 65)
    rc = lib.u3d_criterion_packed(*_abi_args(case, g, cls, box, loss, dcls, dbox, ws, crit=crit))
    torch.cuda.synchronize()
    assert rc == U3D_OK, lib.u3d_last_error().decode()
    assert bool(torch.isfinite(loss).all()) and float(loss) != SENT and not bool((dcls == SENT).any()) and not bool((dbox == SENT).any())
    assert isinstance(rc, int) and ctypes.sizeof(ctypes.c_int) == 4


def test_fused_criterion_crowded_mixed_is_deterministic():
    """no atomics, fixed reduction order: two runs give bit-identical loss, dcls and dbox"""
    case, _ = C.build('crowded_mixed')
    a = EC.run_product(case, DEV, True, True)
    b = EC.run_product(case, DEV, True, True)
    assert torch.equal(a[0], b[0])
    for l in range(case['L']):
        assert torch.equal(a[1][l], b[1][l]) and torch.equal(a[2][l], b[2][l])


def test_model_loss_with_a_crowded_scene_fused_against_tensor_ops():
    """Two synthetic ScanNet rooms of 3 000 / 4 000 points through ``UniDet3D.loss`` (0.05 m voxels, two decoder layers, the shapes of
    ``smoke()``); the first room holds 80 annotated objects.  Both rooms stay below ``query_thr`` = 3 000 superpoints (asserted), so no
    random query selection separates the two passes.  ``criterion.fused = True`` (asserted to have run the kernel) against
    ``False``: loss within 1e-3 relative, every parameter gradient within 1e-3 (max-norm relative) and the flat gradient's cosine
    >= ``PA.COS_MIN`` with a relative L2 error below 1e-3 -- the bounds tests/_parity.py holds a full-model gradient to (``compare``: loss 1e-3, ``grad_tol`` 1e-3,
    ``COS_MIN``)."""
    from _detw import fill_state_dict
    from unidet3d_amd.config import build_model, scannet_model_cfg
    from unidet3d_amd.data import make_batch_inputs
    from unidet3d_amd.synthetic import make_scene
    cfg = scannet_model_cfg(voxel_size=0.05)
    cfg['decoder']['num_layers'] = 2
    model = fill_state_dict(build_model(cfg), tag0=3000, scale=0.06).to(DEV).train()
    scenes = [make_scene(31, n_points=3_000, n_furniture=80), make_scene(32, n_points=4_000)]
    assert all(int(sc.superpoints.max()) + 1 <= cfg['query_thr'] for sc in scenes)
    assert int(np.bincount(scenes[0].instance_mask[scenes[0].instance_mask >= 0], minlength=80).min()) > 0
    inputs, samples = make_batch_inputs(scenes, DEV)
    calls = []
    orig = model.criterion._loss_fused
    model.criterion._loss_fused = lambda *a, **k: calls.append(orig(*a, **k)) or calls[-1]
    res = {}
    for fused in (True, False):
        model.criterion.fused = fused
        model.zero_grad(set_to_none=True)
        loss = model.loss(inputs, samples)['det_loss']
        loss.backward()
        res[fused] = (float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
    assert len(calls) == 1 and calls[0] is not None                                  # the kernel took the 80-GT batch
    (lf, gf), (lt, gt) = res[True], res[False]
    assert set(gf) == set(gt) and all(bool(torch.isfinite(v).all()) for v in gf.values())
    keys = sorted(gt)
    stats = PA.flat_gradient_stats({'fused': gf}, gt, keys)['fused']
    worst = max(PA.rel(gf[k], gt[k]) for k in keys)
    rec = dict(loss_rel=abs(lf - lt) / abs(lt), grad_max_rel=worst, cos=stats['cos'], l2_rel=stats['l2_rel'])
    print('criterion_crowded_model', rec)
    PA.log_errors('criterion_crowded_model', rec)
    assert rec['loss_rel'] < 1e-3 and worst < 1e-3 and stats['cos'] >= PA.COS_MIN and stats['l2_rel'] < 1e-3, rec
