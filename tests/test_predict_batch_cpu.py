"""Host logic of the batched post-processing: the per-scene settings table built from the joint config (no GPU needed)."""
import numpy as np
import pytest

from unidet3d_amd import ops
from unidet3d_amd.config import joint_model_cfg


def test_scene_table_from_the_joint_config():
    cfg = joint_model_cfg()
    datasets = cfg['decoder']['datasets']
    names = ['scannet', 's3dis', 'arkitscenes', '3rscan', 'scannetpp']
    idx = [datasets.index(n) for n in names]
    sts = [ops.postproc_settings(cfg['test_cfg'], d, cfg['fast_nms'], cfg['use_superpoints']) for d in idx]
    n_q = [3000, 500, 0, 1, 20000]
    n_c = [len(cfg['decoder']['datasets_classes'][d]) for d in idx]
    bd = [6, 6, 7, 6, 6]
    meta, fmeta = ops.postproc_scene_table(n_q, n_c, bd, sts)
    assert meta.dtype == np.int32 and meta.shape == (5, ops.PP_META) and fmeta.dtype == np.float32 and fmeta.shape == (5, ops.PP_FMETA)
    assert meta[:, 0].tolist() == n_q and meta[:, 1].tolist() == n_c and meta[:, 2].tolist() == [c + 1 for c in n_c]
    assert meta[:, 3].tolist() == [1000] * 5 and meta[:, 4].tolist() == bd
    assert meta[:, 5].tolist() == [ops.NMS_MODE_BEV, ops.NMS_MODE_ALIGNED3D, ops.NMS_MODE_ROTATED, ops.NMS_MODE_BEV, ops.NMS_MODE_BEV]
    assert meta[:, 6].tolist() == [1, 1, 0, 0, 0]
    assert fmeta[:, 1].tolist() == [np.float32(cfg['test_cfg']['iou_thr'][d]) for d in idx]
    assert fmeta[:, 0].tolist() == [0.0] * 5 and np.all(fmeta[:, 2] == np.float32(0.18)) and np.all(fmeta[:, 3] == np.float32(0.81))
    # output columns as the per-scene path returns them
    assert [ops.postproc_columns(b, s, 3) for b, s in zip(bd, sts)] == [6, 6, 7, 7, 7]
    assert [ops.postproc_columns(b, s, 0) for b, s in zip(bd, sts)] == [6, 6, 7, 6, 6]


def test_scenes_outside_the_kernel_limits_leave_the_chain():
    st = dict(topk=ops.PP_MAX_K + 1, score_thr=0.0, iou_thr=0.5, fast_nms=True, trim=True, low_sp_thr=0.18, up_sp_thr=0.81)
    assert not ops.postproc_batched_ok(10, 18, st)
    assert not ops.postproc_batched_ok(2 ** 20, 2 ** 11, dict(st, topk=1000))
    meta, _ = ops.postproc_scene_table([10, 10], [18, 18], [6, 6], [st, dict(st, topk=1000)])
    assert meta[:, 3].tolist() == [0, 1000] and meta[:, 6].tolist() == [0, 1]
    with pytest.raises(ValueError):
        ops.postproc_scene_table([10], [18], [5], [st])
