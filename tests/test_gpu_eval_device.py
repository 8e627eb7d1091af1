"""Device evaluation (csrc/evalmap.hip, ``evaluation.indoor_eval_device`` / ``DeviceIndoorMetric``) against the host protocol
(``evaluation.indoor_eval``, itself pinned to the reference by tests/golden/ref_eval.npz) on the cases of tests/_eval_cases.py:
kernel by kernel (match, order, sweep), end to end, on the reference fixture, through the metric class on real ``predict`` outputs,
run-to-run, and the error paths.  tests/test_eval_cases_cpu.py proves on the host what these comparisons assume about the inputs.

DESIGN.md 4.22 describes the kernels; test_match_kernel prints the measured error ratio of the rotated pairs."""
import os
import warnings

import numpy as np
import pytest
import torch

import _eval_cases as EC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = EC.build_cases()
_CACHE = {}


def run(name):
    """Everything the device computes for a case, once: packed inputs, match, order, sweep (with flags), and the host's view."""
    if name not in _CACHE:
        from unidet3d_amd import ops
        from unidet3d_amd.evaluation import pack_annotations
        case = CASES[name]
        gt, dt = EC.annos(case, DEV)
        p = pack_annotations(gt, dt)
        iou_max, jmax, n_gt, n_det = ops.eval_match(p['det_boxes'], p['det_labels'], p['det_off'], p['gt_boxes'], p['gt_labels'], p['gt_off'], case.n_classes)
        perm = ops.eval_order(p['det_scores'], p['det_labels'], case.n_classes)
        ap, rec, flag, cum = ops.eval_sweep(iou_max, jmax, perm, n_gt, n_det, p['gt_boxes'].shape[0], EC.THRESHOLDS, with_flags=True)
        _CACHE[name] = dict(m=EC.host_match(case), gt=gt, dt=dt, iou_max=iou_max.cpu().numpy(), jmax=jmax.cpu().numpy(), n_gt=n_gt.cpu().numpy(),
                            n_det=n_det.cpu().numpy(), perm=perm.cpu().numpy(), ap=ap.cpu().numpy(), rec=rec.cpu().numpy(), flag=flag.cpu().numpy(),
                            cum=cum.cpu().numpy())
    return _CACHE[name]


def host_eval(case, gt, dt):
    from unidet3d_amd.evaluation import indoor_eval
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return indoor_eval(gt, dt, EC.THRESHOLDS, EC.label2cat(case))


@pytest.mark.parametrize('name', sorted(CASES))
def test_match_kernel(name):
    case, r = CASES[name], run(name)
    m = r['m']
    assert np.array_equal(r['jmax'], m['jmax'])
    assert np.array_equal(np.isneginf(r['iou_max']), np.isneginf(m['iou_max']))
    al = m['aligned'] & (m['jmax'] >= 0)
    assert r['iou_max'][al].tobytes() == m['iou_max'][al].tobytes()                    # the axis-aligned formula, bit for bit
    gl = np.concatenate([l for _, l in case.gt])
    assert np.array_equal(r['n_gt'], np.bincount(gl, minlength=case.n_classes)) and np.array_equal(r['n_det'], np.bincount(m['label'], minlength=case.n_classes))
    ref = EC.iou64_of_best(case, m)
    rot = ~np.isnan(ref)
    assert rot.any() == (name.endswith('_rot') or name == 'g')
    if rot.any():
        e_dev, e_host = np.abs(r['iou_max'][rot] - ref[rot]), np.abs(m['iou_max'][rot] - ref[rot])
        print(f'{name}: rotated pairs {rot.sum()}, max error vs fp64: device {e_dev.max():.3e}, host fp32 {e_host.max():.3e}, '
              f'max ratio {(e_dev / np.maximum(e_host, 2.5e-7)).max():.3f} (of the allowed 4)')
        assert (e_dev <= np.maximum(4 * e_host, 1e-6)).all(), (e_dev, e_host)


@pytest.mark.parametrize('name', sorted(CASES))
def test_order_is_the_stable_lexsort(name):
    r = run(name)
    m = r['m']
    want = np.lexsort((np.arange(len(m['score'])), -m['score'], m['label']))
    assert np.array_equal(r['perm'], want)


@pytest.mark.parametrize('name', sorted(CASES))
def test_sweep_flags_and_counts(name):
    case, r = CASES[name], run(name)
    m, perm = r['m'], r['perm']
    lab = m['label'][perm]
    for ti, thr in enumerate(EC.THRESHOLDS):
        for c in sorted(set(lab.tolist())):
            seg = np.nonzero(lab == c)[0]
            assert np.array_equal(seg, np.arange(seg[0], seg[0] + len(seg)))
            d = perm[seg]
            order, tp = EC.first_claimant(m['score'][d], m['iou_max'][d], m['jmax'][d], thr)
            assert np.array_equal(order, np.arange(len(d)))                            # perm is already the stable order inside the class
            assert np.array_equal(r['flag'][ti, seg].astype(bool), tp), (name, c, thr)
            assert np.array_equal(r['cum'][ti, seg], np.cumsum(tp)), (name, c, thr)
            assert np.array_equal(np.arange(1, len(d) + 1) - r['cum'][ti, seg], np.cumsum(~tp))     # the false positives


@pytest.mark.parametrize('name', sorted(CASES))
def test_end_to_end_equals_host(name):
    from unidet3d_amd.evaluation import indoor_eval_device
    case, r = CASES[name], run(name)
    dev = indoor_eval_device(r['gt'], r['dt'], EC.THRESHOLDS, EC.label2cat(case))
    # tied scores: the host's np.argsort is not stable by contract -> the stable restatement (equal to the host elsewhere, CPU test)
    want = EC.reference_eval(case, m=r['m']) if case.tied else host_eval(case, [dict(g) for g in r['gt']], [{k: v.cpu() for k, v in d.items()} for d in r['dt']])
    assert EC.same_dict(dev, want) == [], (dev, want)
    if name == 'e':
        assert np.isnan(dev['c3_AP_0.25']) and dev['c4_AP_0.50'] == 0 and 'c5_AP_0.25' not in dev
    # ground truths that already live on the device give the same numbers
    gt_dev = [dict(gt_bboxes_3d=g['gt_bboxes_3d'].to(DEV), gt_labels_3d=torch.tensor(g['gt_labels_3d'], dtype=torch.int64, device=DEV)) for g in r['gt']]
    assert EC.same_dict(indoor_eval_device(gt_dev, r['dt'], EC.THRESHOLDS, EC.label2cat(case)), dev, 1e-12) == []


def test_reference_fixture():
    from unidet3d_amd.evaluation import indoor_eval_device
    E = np.load(os.path.join(GOLD, 'ref_eval.npz'))
    gt, dt = [], []

    def bottom(b):           # the fixture holds gravity centres; the box class stores bottom-centre rows, as in tests/test_ref_golden_cpu.py
        from unidet3d_amd.structures import DepthInstance3DBoxes
        return DepthInstance3DBoxes(np.concatenate((b, np.zeros((len(b), 1), np.float32)), 1), with_yaw=False, box_dim=7, origin=(0.5, 0.5, 0.5)).tensor

    for i in range(int(E['E.n_img'])):
        gt.append(dict(gt_bboxes_3d=bottom(E[f'E.gt_box{i}']), gt_labels_3d=E[f'E.gt_lab{i}'].tolist()))
        dt.append(dict(labels_3d=torch.from_numpy(E[f'E.dt_lab{i}']).to(DEV), scores_3d=torch.from_numpy(E[f'E.dt_score{i}']).to(DEV),
                       bboxes_3d=bottom(E[f'E.dt_box{i}']).to(DEV)))
    ret = indoor_eval_device(gt, dt, [0.25, 0.5], {i: f'cls{i}' for i in range(int(E['E.n_cls']))})
    keys = sorted(ret)
    assert keys == [str(k) for k in E['E.ret_keys']]
    got = np.array([ret[k] for k in keys])
    assert np.allclose(got, E['E.ret_vals'], rtol=0, atol=1e-6, equal_nan=True), np.abs(got - E['E.ret_vals']).max()


def test_metric_class_on_predict_outputs():
    import unidet3d_amd  # noqa: F401
    import _parity as PA
    from unidet3d_amd import ops
    from unidet3d_amd.config import build_model, scannet_model_cfg
    from unidet3d_amd.data import make_batch_inputs
    from unidet3d_amd.evaluation import DeviceIndoorMetric, IndoorMetric, pack_annotations
    from unidet3d_amd.structures import DepthInstance3DBoxes
    from unidet3d_amd.synthetic import make_scene
    torch.manual_seed(0)
    cfg = scannet_model_cfg(voxel_size=0.05)
    cfg['decoder']['num_layers'] = 3
    model = build_model(cfg).to(DEV).eval()
    scenes = [make_scene(300 + i, n_points=12_000) for i in range(3)]
    classes = [f'c{i}' for i in range(18)]
    inputs, samples = make_batch_inputs(scenes, DEV)
    with torch.no_grad():
        results = model.predict(inputs, samples)                       # the batched path: three scenes in one call
    host, dev = IndoorMetric(['scannet'], [classes]), DeviceIndoorMetric(['scannet'], [classes])
    for sc, res in zip(scenes, results):
        b, keep = PA.scene_boxes(sc)
        ann = dict(gt_bboxes_3d=DepthInstance3DBoxes(torch.from_numpy(b), with_yaw=False, box_dim=6, origin=(0.5, 0.5, 0.5)),
                   gt_labels_3d=[int(x) for x in sc.labels[keep]])
        r = res.pred_instances_3d
        det = dict(bboxes_3d=r.bboxes_3d, scores_3d=r.scores_3d, labels_3d=r.labels_3d, dataset='scannet')
        host.process(ann, det)
        dev.process(ann, det)
    for ann, pred in dev.results:
        assert all(v.is_cuda for v in (ann['gt_bboxes_3d'], ann['gt_labels_3d'], pred['scores_3d'], pred['labels_3d']))
        assert (pred['bboxes_3d'].tensor if hasattr(pred['bboxes_3d'], 'tensor') else pred['bboxes_3d']).is_cuda
    assert sum(len(p['scores_3d']) for _, p in dev.results) > 0
    # the comparison below is only meaningful when no best IoU sits on a threshold: say so instead of passing or skipping
    p = pack_annotations([a for a, _ in dev.results], [q for _, q in dev.results])
    iou_max = ops.eval_match(p['det_boxes'], p['det_labels'], p['det_off'], p['gt_boxes'], p['gt_labels'], p['gt_off'], 18)[0].cpu().numpy()
    for thr in (0.25, 0.5):
        near = np.abs(iou_max[np.isfinite(iou_max)] - thr)
        if near.size and near.min() < 1e-4:
            pytest.fail(f'a best IoU of this predict run lies {near.min():.2e} from the threshold {thr}: host and device may legitimately differ; change the scenes')
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        want = host.compute_metrics()['scannet']
    got = dev.compute_metrics()['scannet']
    assert EC.same_dict(got, want) == [], (got, want)


def test_two_calls_are_bit_identical():
    from unidet3d_amd import ops
    r = run('f')
    case = CASES['f']
    from unidet3d_amd.evaluation import pack_annotations
    p = pack_annotations(r['gt'], r['dt'])
    for _ in range(2):
        iou_max, jmax, n_gt, n_det = ops.eval_match(p['det_boxes'], p['det_labels'], p['det_off'], p['gt_boxes'], p['gt_labels'], p['gt_off'], case.n_classes)
        perm = ops.eval_order(p['det_scores'], p['det_labels'], case.n_classes)
        ap, rec = ops.eval_sweep(iou_max, jmax, perm, n_gt, n_det, p['gt_boxes'].shape[0], EC.THRESHOLDS)
        assert ap.cpu().numpy().tobytes() == r['ap'].tobytes() and rec.cpu().numpy().tobytes() == r['rec'].tobytes()


def test_errors_and_empty_input():
    from unidet3d_amd import _lib
    from unidet3d_amd.evaluation import DeviceIndoorMetric, indoor_eval_device
    case = CASES['a']
    gt, dt = EC.annos(case)                       # host tensors
    with pytest.raises(_lib.U3DError):
        indoor_eval_device(gt, dt, EC.THRESHOLDS, EC.label2cat(case))
    with pytest.raises(_lib.U3DError):
        DeviceIndoorMetric(['x'], [EC.label2cat(case)]).process(gt[0], dict(dt[0], dataset='x'))
    ret = indoor_eval_device([], [], EC.THRESHOLDS, EC.label2cat(case))
    assert set(ret) == {'mAP_0.25', 'mAR_0.25', 'mAP_0.50', 'mAR_0.50'} and all(np.isnan(v) for v in ret.values())
    # images that hold nothing at all: the launch chain runs on zero rows without an error
    gt0 = [dict(gt_bboxes_3d=torch.zeros(0, 7), gt_labels_3d=[])] * 2
    dt0 = [dict(bboxes_3d=torch.zeros(0, 7, device=DEV), scores_3d=torch.zeros(0, device=DEV), labels_3d=torch.zeros(0, dtype=torch.int64, device=DEV))] * 2
    ret = indoor_eval_device(gt0, dt0, EC.THRESHOLDS, EC.label2cat(case))
    assert set(ret) == {'mAP_0.25', 'mAR_0.25', 'mAP_0.50', 'mAR_0.50'} and all(np.isnan(v) for v in ret.values())
    torch.cuda.synchronize()
    metric = DeviceIndoorMetric(['x'], [EC.label2cat(case)])
    assert metric.compute_metrics() == {'x': ret} or all(np.isnan(v) for v in metric.compute_metrics()['x'].values())
