"""The two wide backbones end to end through the shared parity harness (tests/_parity.py): the 64-channel five-level U-Net (planes
64 .. 320, tail blocks up to 512 -> 256) and the 32-channel seven-level one (planes 32 .. 224).  Coordinates bit-exact; per-superpoint
features, logits, boxes and loss within the harness's 1e-3 of the CPU oracle; every parameter gradient within ``grad_tol`` = 5e-3 of
the fp64 oracle evaluated on the product's own activation pattern -- the figure tests/test_gpu_model.py uses for a batch whose
deepest levels hold tens of voxels, which is the case for both nets here (4867 voxels at level 1 of (a); 94, 20 and 3 rows at the
three deepest levels of (b))."""
import copy

import pytest
import torch

import _parity as PA
from _detw import fill_state_dict
from oracle import model as om

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _pair(cfg, num_channels):
    """product (cuda:0) and oracle (CPU) of ``cfg`` with identical deterministic weights; _parity.build_pair does not hand
    num_channels to the oracle"""
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd.config import build_model
    prod = build_model(cfg)
    fill_state_dict(prod, tag0=3000, scale=0.06)
    orac = om.ODetector(num_channels=num_channels, backbone=cfg['backbone'], decoder=cfg['decoder'], voxel_size=cfg['voxel_size'])
    res = orac.load_state_dict(prod.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return prod.to(DEV).train(), orac.train()


def _cfg_64x5():
    from unidet3d_amd.config import scannet_model_cfg
    cfg = scannet_model_cfg(num_channels=64, voxel_size=0.05)
    cfg['decoder']['num_layers'] = 1
    return cfg


def _cfg_32x7():
    from unidet3d_amd.config import scannet_model_cfg
    cfg = scannet_model_cfg(num_channels=32, voxel_size=0.03)         # (5 cm voxels leave the seventh level a single voxel: nn.BatchNorm1d refuses it)
    cfg['backbone']['num_planes'] = [32 * (i + 1) for i in range(7)]
    cfg['decoder']['num_layers'] = 1
    return cfg


def _end_to_end(name, cfg, num_channels, scenes, grad_tol):
    from unidet3d_amd.data import make_batch_inputs
    prod, orac = _pair(cfg, num_channels)
    names = ['scannet'] * len(scenes)
    O = PA.oracle_forward(orac, scenes, names)
    run = lambda m: PA.oracle_forward(m, scenes, names)  # noqa: E731
    inputs, samples = make_batch_inputs(scenes, DEV)
    P = PA.product_forward(prod, inputs, samples, relu_masks=True)
    g64m, _ = PA.oracle_fp64_grads_same_activation_pattern(orac, run, P['relu_masks'])
    return PA.compare(name, P, O, prod, orac, None, None, g64m, grad_tol=grad_tol)


def test_64_channel_five_level_backbone_end_to_end():
    """scannet_model_cfg(num_channels=64): planes 64 .. 320, one 10 k-point scene at 5 cm (4867 voxels)"""
    from unidet3d_amd.synthetic import make_scene
    err = _end_to_end('wide_64x5', _cfg_64x5(), 64, [make_scene(40, n_points=10_000)], grad_tol=5e-3)
    assert err['n_voxels'] == 4867


def test_32_channel_seven_level_backbone_end_to_end():
    """num_planes 32 .. 224, two 10 k-point scenes at 3 cm (level rows about 15344, 7604, 2037, 428, 94, 20, 3)"""
    from unidet3d_amd.synthetic import make_scene
    _end_to_end('wide_32x7', _cfg_32x7(), 32, [make_scene(40, n_points=10_000), make_scene(41, n_points=10_000)], grad_tol=5e-3)


def test_64_channel_backbone_with_bf16_operands_stays_close_to_fp32():
    """the 64-channel net under precision.operands('bf16') (bf16 rows as the default has them) against its own fp32 step: the forward
    tolerance of test_gpu_bf16.test_training_step_bf16_operands_stays_close_to_fp32 (loss within 5e-3), every gradient finite;
    the gradient cosines are logged"""
    from unidet3d_amd import precision as P
    from unidet3d_amd.config import build_model
    from unidet3d_amd.data import make_batch_inputs
    from unidet3d_amd.synthetic import make_scene
    base = fill_state_dict(build_model(_cfg_64x5()), tag0=3000, scale=0.06)
    inputs, samples = make_batch_inputs([make_scene(40, n_points=10_000)], DEV)
    res = {}
    for mode in ('fp32', 'bf16'):
        model = copy.deepcopy(base).to(DEV).train()
        with P.operands(mode):
            loss = model.loss(inputs, copy.deepcopy(samples))['det_loss']
            loss.backward()
        grads = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values()), mode
        res[mode] = (float(loss.detach()), grads, model._vb.coords.cpu())
    (l32, g32, c32), (l16, g16, c16) = res['fp32'], res['bf16']
    assert torch.equal(c32, c16) and set(g32) == set(g16)
    cos = lambda a, b: float((a * b).sum() / (a.norm() * b.norm() + 1e-30))  # noqa: E731
    flat32 = torch.cat([g32[n].flatten() for n in sorted(g32)]); flat16 = torch.cat([g16[n].flatten() for n in sorted(g16)])
    rec = dict(loss_fp32=l32, loss_bf16=l16, loss_rel=abs(l16 - l32) / abs(l32), cos_all_grads=cos(flat32, flat16))
    PA.log_errors('wide_64x5_bf16_step_vs_fp32_step', rec)
    print('wide 64x5 bf16 step vs fp32 step:', rec)
    assert rec['loss_rel'] < 5e-3, rec
