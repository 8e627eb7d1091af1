"""Wide backbones without a GPU: the 64-channel five-level and the 32-channel seven-level configs build, their state_dict loads
strictly into the CPU oracle, a first plane the superpoint pooling has no width for is refused by name, and the C entry points keep
the channel contract ({16} u {32, 64, ..., 512} -> {32, 64, ..., 512}) before any HIP call."""
import ctypes

import pytest

from oracle import model as om


def _cfgs():
    from unidet3d_amd.config import scannet_model_cfg
    a = scannet_model_cfg(num_channels=64, voxel_size=0.05)
    b = scannet_model_cfg(num_channels=32, voxel_size=0.03)
    b['backbone']['num_planes'] = [32 * (i + 1) for i in range(7)]
    return [('64x5', 64, a), ('32x7', 32, b)]


@pytest.mark.parametrize('name,num_channels,cfg', _cfgs(), ids=[c[0] for c in _cfgs()])
def test_wide_configs_build_and_load_into_the_oracle(name, num_channels, cfg):
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd.config import build_model
    cfg['decoder']['num_layers'] = 1
    prod = build_model(cfg)
    assert prod.unet.num_planes == cfg['backbone']['num_planes']
    orac = om.ODetector(num_channels=num_channels, backbone=cfg['backbone'], decoder=cfg['decoder'], voxel_size=cfg['voxel_size'])
    res = orac.load_state_dict(prod.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    widest = max(p.shape[0] for k, p in prod.state_dict().items() if k.startswith('unet.') and p.dim() == 5)
    assert widest == max(cfg['backbone']['num_planes'])


@pytest.mark.parametrize('planes', [[48, 96], [96, 192]])
def test_a_first_plane_the_pooling_has_no_width_for_is_refused_by_name(planes):
    from unidet3d_amd._lib import U3DError
    from unidet3d_amd.spconv_unet import SpConvUNet
    with pytest.raises(U3DError, match=r'num_planes\[0\] must be one of \[32, 64, 128, 256\]'):
        SpConvUNet(planes)
    with pytest.raises(U3DError, match='multiple of 32'):
        SpConvUNet(planes)


def test_inner_levels_and_the_deepest_plane_take_any_multiple_of_32():
    from unidet3d_amd._lib import U3DError
    from unidet3d_amd.spconv_unet import SpConvUNet
    assert SpConvUNet([32, 96, 224, 512]).u.u.u.num_planes == [512]
    for planes in ([64, 288, 320], [64, 544], [64, 80]):              # a tail block of 576 channels; beyond 512; not a multiple of 32
        with pytest.raises(U3DError, match='num_planes'):
            SpConvUNet(planes)


def test_channel_contract_of_the_c_entry_points_needs_no_gpu():
    from unidet3d_amd import _lib
    l = _lib.lib()
    R, G = ctypes.c_int(0), ctypes.c_int(0)
    for cs, cd in ((16, 64), (224, 224), (320, 320), (512, 256), (32, 512), (512, 512)):
        assert l.u3d_spconv_plan(cs, cd, 27, 5000, ctypes.byref(R), ctypes.byref(G)) == 0 and R.value in (32, 64), (cs, cd)
    for cs, cd in ((48, 32), (32, 48), (544, 32), (32, 544), (24, 32), (16, 16)):
        assert l.u3d_spconv_plan(cs, cd, 27, 5000, ctypes.byref(R), ctypes.byref(G)) < 0, (cs, cd)
    # the plans of the instantiated widths are what they were
    assert l.u3d_spconv_plan(160, 160, 27, 1400, ctypes.byref(R), ctypes.byref(G)) == 0 and (R.value, G.value) == (64, 9)
    # the partial buffer of the widest weight gradient stays inside the 64 MB budget
    for n in (3, 5000, 400_000):
        assert 0 < l.u3d_spconv_wgrad_ws_bytes(27, n, 512, 256) <= (64 << 20) + 256, n
        T = l.u3d_spconv_wgrad_tile_rows(27, n, 512, 256)
        assert T > 0 and 27 * -(-n // T) * 512 * 256 * 4 + 256 == l.u3d_spconv_wgrad_ws_bytes(27, n, 512, 256)
    # bf16 rows: the workgroup-tile kernel's widths only; the weight gradient from bf16 rows keeps its own list
    assert [l.u3d_spconv_gmm_bf16a_supported(c, 64) for c in (32, 192, 256, 224, 320, 512, 16)] == [1, 1, 1, 0, 0, 0, 0]
    assert l.u3d_spconv_wgrad_rows_supported(320, 320) == 0
    # a weight gradient outside the contract is refused before any HIP call (the pointers are never read)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert l.u3d_spconv_wgrad(p, 10, p, p, p, p, 27, 10, 10, 64, 48, 32, p, p, 0.0, None) == -3
    assert b'no kernel for Cs=48' in l.u3d_last_error()


def test_route_gathers_fp32_rows_where_the_bf16_row_kernel_has_no_width(monkeypatch):
    """sparse._conv_route: bf16 operands with a shadow present take u3d_spconv_gmm_bf16a only at its widths; at 320 source channels
    the launch gathers the fp32 rows (plan of the fp32-row kernels, rows flag off) -- decided in _conv_route and nowhere else"""
    from types import SimpleNamespace
    from unidet3d_amd import precision as P
    from unidet3d_amd import sparse
    for name in ('_CONV_TS', '_CONV_RS', '_CONV_RS_BF16', '_EPILOGUE_STATS'):
        monkeypatch.setattr(sparse, name, False)
    monkeypatch.setattr(sparse, '_plan', lambda Cs, Cd, K, n_dst, rows_kernel=False: (64, 2) if rows_kernel else (32, 1))
    rb = SimpleNamespace(coords=object(), K=27)
    assert sparse._conv_route(192, 320, 1000, rb, P.FMT_BF16, True, False) == ('pairs', P.FMT_BF16, (64, 2, True))
    assert sparse._conv_route(320, 320, 1000, rb, P.FMT_BF16, True, False) == ('pairs', P.FMT_BF16, (32, 1, False))
    assert sparse._conv_route(320, 320, 1000, rb, P.FMT_X3, False, False) == ('pairs', P.FMT_X3, (32, 1, False))
