"""The conditions the device-evaluation tests (tests/test_gpu_eval_device.py) rely on, checked on the host: the cases of
tests/_eval_cases.py keep every IoU away from the thresholds and from each other, the parallel "first qualifying claimant" rule
equals the sequential walk of ``evaluation.eval_det_cls``, and packing annotations into flat arrays round-trips."""
import numpy as np
import pytest
import torch

import _eval_cases as EC

CASES = EC.build_cases()
MATCH = {}


def match(name):
    if name not in MATCH:
        MATCH[name] = EC.host_match(CASES[name])
    return MATCH[name]


def test_cases_cover_the_list():
    assert set(CASES) == {'a', 'b', 'c', 'd', 'h', 'a_rot', 'b_rot', 'c_rot', 'd_rot', 'h_rot', 'e', 'f', 'g'}
    f = CASES['f']
    lab = np.concatenate([l for _, _, l in f.dt])
    assert len(f.dt) == 40 and (lab == 1).sum() == 3000 and (lab == 0).sum() == 37
    from unidet3d_amd import _lib
    assert len(f.gt[0][1]) > _lib.lib().u3d_eval_gt_chunk()              # an image with more ground truths than one LDS chunk
    g = CASES['g']
    assert {(d[0].shape[1], t[0].shape[1]) for d, t in zip(g.dt, g.gt)} == {(6, 7), (7, 6), (7, 7)}


@pytest.mark.parametrize('name', sorted(CASES))
def test_ious_are_closed_form_and_clear_of_the_thresholds(name):
    m = match(name)
    known = np.array(sorted(EC.IOU_OF_SHIFT.values()))
    for d, p in enumerate(m['pairs']):
        # every same-class IoU is one of the lattice values (size and position are exact in fp32 up to rounding)
        assert np.abs(p[:, None].astype(np.float64) - known[None]).min(1).max(initial=0.0) < 1e-4, (name, d, p)
        for thr in EC.THRESHOLDS:
            assert (np.abs(p - thr) > 1e-3).all(), (name, d, p)
        if len(p) >= 2:
            top = np.sort(p)[::-1][:2]
            assert top[0].tobytes() == top[1].tobytes() or top[0] - top[1] >= 1e-3, (name, d, top)
    if not CASES[name].tied:
        keys = list(zip(m['label'].tolist(), m['score'].tolist()))
        assert len(set(keys)) == len(keys), name
    else:
        assert len(set(zip(m['label'].tolist(), m['score'].tolist()))) < len(m['label'])


@pytest.mark.parametrize('name', sorted(n for n in CASES if n.endswith('_rot') or n == 'g'))
def test_fp64_reference_of_the_rotated_pairs_is_the_closed_form(name):
    """The fp64 value the GPU test measures both fp32 paths against.  Box centres are rounded to fp32 (ulp 4e-6 at 32 m) on boxes of
    about 1 m, and d IoU / d shift <= 2: the inputs themselves move an IoU by up to 1e-5 from the lattice value."""
    m = match(name)
    r = EC.iou64_of_best(CASES[name], m)
    ok = ~np.isnan(r)
    assert ok.sum() >= 2 and np.array_equal(ok, (m['jmax'] >= 0) & ~m['aligned'])
    known = np.array(sorted(EC.IOU_OF_SHIFT.values()))
    assert np.abs(r[ok][:, None] - known[None]).min(1).max() < 2e-5


def _walk(score, iou_max, jmax, thr):
    """the sequential greedy walk of eval_det_cls on a STABLE order (the definition of the result for tied scores)"""
    order = np.argsort(-score, kind='stable')
    taken, tp = set(), np.zeros(len(order), bool)
    for r, d in enumerate(order):
        if iou_max[d] > thr and jmax[d] not in taken:
            tp[r] = True
            taken.add(jmax[d])
    return tp


@pytest.mark.parametrize('name', sorted(CASES))
def test_first_claimant_rule_equals_the_sequential_reference(name):
    from unidet3d_amd.evaluation import eval_det_cls
    case, m = CASES[name], match(name)
    gl = np.concatenate([l for _, l in case.gt])
    img = np.concatenate([np.full(len(l), i) for i, (_, _, l) in enumerate(case.dt)])
    gt_img = np.concatenate([np.full(len(l), i) for i, (_, l) in enumerate(case.gt)])
    gt_first = np.concatenate([[0], np.cumsum([len(l) for _, l in case.gt])])
    for c in sorted(set(m['label'].tolist())):
        sel = m['label'] == c
        score, iou_max, jmax = m['score'][sel], m['iou_max'][sel], m['jmax'][sel]
        for thr in EC.THRESHOLDS:
            _, tp = EC.first_claimant(score, iou_max, jmax, thr)
            assert np.array_equal(tp, _walk(score, iou_max, jmax, thr)), (name, c, thr)
        if case.tied:
            continue
        # the host function itself: its arguments are per image (index of the ground truth among the image's ones of the class)
        n_gt_img = {}
        for i in set(img[sel].tolist()):
            n_gt_img[i] = 0
        for i, l in zip(gt_img, gl):
            if l == c:
                n_gt_img[int(i)] = n_gt_img.get(int(i), 0) + 1
        local = np.array([int((gl[gt_first[i]:j] == c).sum()) if j >= 0 else 0 for i, j in zip(img[sel], jmax)], np.int64)
        ref = eval_det_cls(img[sel], score, iou_max, local, n_gt_img, EC.THRESHOLDS)
        for thr, (recall, precision, _) in zip(EC.THRESHOLDS, ref):
            _, tp = EC.first_claimant(score, iou_max, jmax, thr)
            r, p = EC.curves(tp, sum(n_gt_img.values()))
            assert np.array_equal(r, recall, equal_nan=True) and np.array_equal(p, precision, equal_nan=True), (name, c, thr)


@pytest.mark.parametrize('name', sorted(n for n in CASES if not CASES[n].tied))
def test_restatement_gives_the_host_dictionary(name):
    from unidet3d_amd.evaluation import indoor_eval
    case = CASES[name]
    gt, dt = EC.annos(case)
    with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            host = indoor_eval(gt, dt, EC.THRESHOLDS, EC.label2cat(case))
    assert EC.same_dict(EC.reference_eval(case, m=match(name)), host, 1e-12) == []
    if name == 'e':
        assert np.isnan(host['c3_AP_0.25']) and np.isnan(host['c3_rec_0.50']) and host['c4_AP_0.25'] == 0 and host['c4_rec_0.25'] == 0
        assert not any(k.startswith('c5_') for k in host) and not any(k.startswith('c1_') for k in host)
    if name in ('a', 'a_rot'):
        assert host['c0_rec_0.50'] == 1 and host['c0_AP_0.50'] == 1 and host['c1_AP_0.50'] == 1      # one true positive first, one false positive behind
    if name in ('b', 'b_rot'):
        assert host['c0_AP_0.25'] == 1 and host['c0_AP_0.50'] == 0.5
    if name in ('c', 'c_rot'):
        assert host['c0_rec_0.25'] == 0.5                                                              # B stays free, X is a false positive


@pytest.mark.parametrize('name', sorted(CASES))
def test_packing_round_trips(name):
    from unidet3d_amd.evaluation import pack_annotations
    case = CASES[name]
    gt, dt = EC.annos(case)
    p = pack_annotations(gt, dt)
    assert all(not t.is_cuda for t in p.values())
    assert p['det_off'].dtype == p['gt_off'].dtype == p['det_labels'].dtype == p['gt_labels'].dtype == torch.int32
    assert p['det_boxes'].shape[1] == p['gt_boxes'].shape[1] == 7 and p['det_boxes'].dtype == torch.float32
    assert p['det_off'].tolist() == np.concatenate([[0], np.cumsum([len(l) for _, _, l in case.dt])]).tolist()
    assert p['gt_off'].tolist() == np.concatenate([[0], np.cumsum([len(l) for _, l in case.gt])]).tolist()
    for i, ((gb, gl), (db, ds, dl)) in enumerate(zip(case.gt, case.dt)):
        d0, d1, g0, g1 = p['det_off'][i], p['det_off'][i + 1], p['gt_off'][i], p['gt_off'][i + 1]
        assert p['det_labels'][d0:d1].tolist() == dl.tolist() and p['gt_labels'][g0:g1].tolist() == gl.tolist()
        assert np.array_equal(p['det_scores'][d0:d1].numpy(), ds)
        for got, want in ((p['det_boxes'][d0:d1].numpy(), db), (p['gt_boxes'][g0:g1].numpy(), gb)):
            assert np.array_equal(got[:, :want.shape[1]], want) and (want.shape[1] == 7 or (got[:, 6] == 0).all())


def test_device_evaluation_refuses_host_tensors():
    from unidet3d_amd import _lib
    from unidet3d_amd.evaluation import DeviceIndoorMetric, indoor_eval_device
    case = CASES['a']
    gt, dt = EC.annos(case)
    with pytest.raises(_lib.U3DError):
        indoor_eval_device(gt, dt, EC.THRESHOLDS, EC.label2cat(case))
    with pytest.raises(_lib.U3DError):
        DeviceIndoorMetric(['x'], [EC.label2cat(case)]).process(gt[0], dict(dt[0], dataset='x'))
