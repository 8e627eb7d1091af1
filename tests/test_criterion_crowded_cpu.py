"""The crowded cases of tests/_criterion_crowded.py (more than 64 GTs in a scene) pinned on the CPU: the builders are deterministic
and admissible, the cases exercise what they are for (matches beyond GT 63, bits 64 and 128, queries with matches in two words),
the fp32 oracle agrees with the fp64 oracle, the tensor-op formulations agree with the fp64 oracle, and the host-side packing
(``UniDet3DCriterion._flat_gt``) no longer refuses such a batch.

fp32 oracle against fp64 oracle, measured here (max over the (layer, scene) blocks; loss relative):
  crowded_single    loss 6.5e-8, dcls 2.2e-7, dbox 3.1e-7
  crowded_mixed     loss 6.2e-9, dcls 1.0e-7, dbox 1.6e-6 (the rotated ARKitScenes scene; the other blocks <= 7.2e-7)
  crowded_last_bit  loss 6.3e-8, dcls 1.0e-7, dbox 3.1e-7
Every block is far inside the GPU bounds (2e-5; 1e-4 / 1e-3 with rotated boxes), so ``C.MEASURED`` is empty: no bound of
tests/test_gpu_criterion_crowded.py is widened."""
import pytest
import torch

import _criterion_crowded as C
import _criterion_edges as E
import test_criterion_edges_cpu as EC
import test_ref_golden_cpu as R


@pytest.mark.parametrize('name', C.CASES)
def test_builders_are_deterministic_and_admissible(name):
    case, o64 = C.build(name)
    assert not E.margin_violations(case, o64) and E.all_finite(case, o64)
    again, _ = C.BUILDERS[name]()
    assert again['sizes'] == case['sizes'] and again.get('seed') == case.get('seed') and again.get('repair_rounds') == case.get('repair_rounds')
    for l in range(case['L']):
        assert torch.equal(again['cls'][l], case['cls'][l]) and torch.equal(again['box'][l], case['box'][l])
    for a, b in zip(again['gt'], case['gt']):
        assert all(torch.equal(a[k], b[k]) for k in ('labels', 'boxes', 'qmask'))
    assert case['L'] == 2 and all(n <= 70 for n in case['sizes'])
    want = dict(crowded_single=[65, 129, 0, 64], crowded_mixed=[70, 200, 3], crowded_last_bit=[128, 3])[name]
    assert [len(g['labels']) for g in case['gt']] == want
    if name == 'crowded_single':
        assert 0 < case['repair_rounds'] < C.REPAIR_ROUNDS
    if name == 'crowded_mixed':
        assert case['BD'] == 7 and case['yaw'] == [True, False, False] and all(len(set(range(case['CU'])) - set(c)) > 0 for c in case['cidx'])


@pytest.mark.parametrize('name', C.CASES)
def test_fp32_oracle_agrees_with_fp64_oracle(name):
    """same matcher decisions and class targets; per-block gradient errors printed and held to 1e-4 (no measured bound is needed)"""
    case, o64 = C.build(name)
    o32 = C.oracle32(name)
    assert E.all_finite(case, o32) and EC.same_matched(o32, o64)
    for l in range(case['L']):
        for t32, t64 in zip(o32['target'][l], o64['target'][l]):
            assert torch.equal(t32, t64)
    e32 = EC.scene_errors(case, o32['dcls'], o32['dbox'], o64)
    e_l = abs(float(o32['loss']) - float(o64['loss'])) / abs(float(o64['loss']))
    print(f'{name}: fp32 oracle vs fp64 oracle: loss {e_l:.2e}', e32)
    assert e_l < 2e-6
    assert all(e[0] < 1e-4 and e[1] < 1e-4 for (l, b), e in e32.items() if (name, b) not in C.MEASURED)
    assert not C.MEASURED


def test_crowded_cases_exercise_multi_word_masks():
    """read off the fp64 oracle's matched sets"""
    case, o = C.build('crowded_single')
    for l in range(2):
        m = o['matched'][l][1]                                              # the 129-GT scene: three words
        assert m.shape == (70, 129)
        per_word = [m[:, 64 * w:64 * (w + 1)].any(1) for w in range(3)]
        assert int(m[:, 64:].sum()) > 0                                     # matched pairs beyond GT 63
        assert int(m[:, 64].sum()) > 0 and int(m[:, 128].sum()) > 0         # bit 0 of word 1, the single bit of word 2
        assert int((per_word[0] & per_word[1]).sum()) > 0                   # queries whose matches span two words
        assert int(o['matched'][l][0][:, 64].sum()) > 0                     # the 65-GT scene: its one GT past the word
        assert o['matched'][l][2].shape == (30, 0) and o['matched'][l][3].shape == (33, 64) and int(o['matched'][l][3][:, 63].sum()) > 0
    case, o = C.build('crowded_mixed')
    for l in range(2):
        assert int(o['matched'][l][0][:, 64:].sum()) > 0                    # rotated pairs in the second word
        assert all(int(o['matched'][l][1][:, 64 * w:64 * (w + 1)].sum()) > 0 for w in range(4))      # 200 GTs: four words in use
    case, o = C.build('crowded_last_bit')
    labels = case['gt'][0]['labels']
    assert len({int(labels[j]) for j in (0, 63, 64, 127)}) == 4
    for l in range(2):
        m = o['matched'][l][0]
        assert m[5].nonzero().flatten().tolist() == [0, 63, 64, 127] and int(o['target'][l][0][5]) == int(labels[127]) == 9
        assert m[9].nonzero().flatten().tolist() == [64] and int(o['target'][l][0][9]) == int(labels[64]) == 2


def test_last_bit_box_gradient_is_the_sum_over_the_four_matched_gts():
    """d loss / d box of query 5 = lw_box / (scenes with matches * matched pairs of the scene) * sum over GT 0, 63, 64, 127 of
    d DIoU(query 5, GT) / d box, evaluated with the oracle's own loss function in fp64"""
    from oracle import criterion as oc
    case, o = C.build('crowded_last_bit')
    lw_box = R.SCANNET_CRIT['loss_weight'][1]
    for l in range(2):
        n_has = sum(1 for m in o['matched'][l] if bool(m.any()))
        cnt = int(o['matched'][l][0].sum())
        q = case['box'][l][5].double().clone().requires_grad_()
        gtb = case['gt'][0]['boxes'][[0, 63, 64, 127]].double()
        oc.axis_aligned_diou_loss(oc.bbox_to_loss(q[None].expand(4, -1)), oc.bbox_to_loss(gtb)).sum().backward()
        want = q.grad * lw_box / (n_has * cnt)
        assert float((o['dbox'][l][5] - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize('name', C.CASES)
def test_tensor_op_paths_match_fp64_oracle_on_crowded_cases(name):
    """the per-scene loop and, for the single-dataset cases, the batched ``_loss_packed`` on CPU tensors: the formulations the kernel
    is tested against keep the bounds of ``C.check_errors`` on these shapes"""
    case, o64 = C.build(name)
    ran = []
    for packed in (False, True):
        loss, dcls, dbox, crit, pred, insts = EC.run_product(case, 'cpu', False, packed)
        if packed and not crit._can_pack(pred, insts, case['names']):
            continue
        ran.append(packed)
        C.check_errors(case, loss, dcls, dbox, o64, C.oracle32(name), f'{name} packed={packed}')
    assert ran == ([False] if case['cidx'] is not None else [False, True])


@pytest.mark.parametrize('name,max_gt', [('crowded_single', 129), ('crowded_mixed', 200), ('crowded_last_bit', 128)])
def test_flat_gt_packs_a_crowded_batch(name, max_gt):
    """the host-side packing hands a batch with more than 64 GTs in a scene to the kernel (it returned None before)"""
    case, _ = C.build(name)
    crit, insts, g = C.flat_gt(case, 'cpu')
    assert isinstance(g, dict) and g['max_gt'] == max_gt
    gs = [len(x['labels']) for x in case['gt']]
    assert g['G'] == sum(gs) and g['P'] == sum(n * k for n, k in zip(case['sizes'], gs)) and g['B'] == len(gs)
    assert g['gt_off'].tolist() == [sum(gs[:b]) for b in range(len(gs) + 1)]
    assert g['labels'].shape == (g['G'],) and g['boxes'].shape == (g['G'], case['BD']) and g['qmask'].numel() == g['P']
    assert g['slack'] >= 0


def test_flat_gt_still_refuses_too_few_queries():
    """the remaining condition: a scene with GT but fewer than topk + 1 queries goes to the per-scene path (None)"""
    g = E._gen(5)
    case = E._pack('few', 'scannet', [E._random_scene(g, 'scannet', 6, 70), E._random_scene(g, 'scannet', 20, 3)], g)
    assert C.flat_gt(case, 'cpu')[2] is None


def test_workspace_size_grows_with_the_mask_words():
    from unidet3d_amd import _lib
    l = _lib.lib()
    L, B, n, G, P = 2, 3, 100, 300, 100 * 300
    base = l.u3d_criterion_ws_bytes(L, B, n, G, P)
    assert l.u3d_criterion_ws_bytes_gt(L, B, n, G, P, 0) == l.u3d_criterion_ws_bytes_gt(L, B, n, G, P, 64) == base
    al = lambda x: (x + 63) & ~63
    for max_gt, W in ((65, 2), (128, 2), (129, 3), (300, 5)):
        assert l.u3d_criterion_ws_bytes_gt(L, B, n, G, P, max_gt) - base == al(L * n * 8 * W) - al(L * n * 8)
    assert l.u3d_criterion_ws_bytes_gt(L, B, n, G, P, -1) < 0
