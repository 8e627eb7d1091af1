"""Check the checker of tests/test_gpu_conv_general.py on the CPU, and the host side of the general sparse-convolution layers: the
brute-force geometry reference of tests/_conv_general.py equals the oracle's two hard-coded rulebooks bit for bit, its lists ascend in
both columns without repeats, the float64 dense references equal a pair-list sum over those lists, a sabotaged result lies outside
the bound; the layer constructors accept and refuse what they document; the C header and the ctypes table carry the new entry points
under the unchanged ABI version."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _conv_general as G
import _conv_geometry as cg
from oracle import sparse_ops as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['u3d_conv_out_shape', 'u3d_conv_mark', 'u3d_conv_rulebook', 'u3d_conv_rulebook_ws_bytes']


def _same_lists(a, b, where):
    assert len(a) == len(b), where
    for k, ((ai, ao), (bi, bo)) in enumerate(zip(a, b)):
        assert ai.dtype == bi.dtype == np.int32 and np.array_equal(ai, bi) and np.array_equal(ao, bo), f'{where}: offset {k}'


def test_brute_force_reference_equals_the_oracle_rulebooks_bit_for_bit():
    for name in G.SCENES:
        _, B, shape, coords = G.scene(name)
        oc, oshape, pairs = G.brute('k2s2p0', name)
        roc, roshape, rpairs = so.build_down_rulebook(coords, shape)
        assert torch.equal(oc, roc) and tuple(oshape) == tuple(int(s) for s in roshape), name
        _same_lists(pairs, rpairs, f'k2s2p0 on {name}')
        oc, oshape, pairs = G.brute(G.SUBM_K3, name)
        assert torch.equal(oc, coords) and tuple(oshape) == tuple(shape), name
        _same_lists(pairs, so.build_subm_rulebook(coords, shape), f'subm k3 on {name}')


def test_every_reference_list_ascends_in_both_columns_without_repeats():
    empty = 0
    for cfg in G.CONFIGS:
        k = G.geom(cfg)[0]
        for name in G.SCENES:
            n = len(G.scene(name)[3])
            oc, oshape, pairs = G.brute(cfg, name)
            assert len(pairs) == k[0] * k[1] * k[2], (cfg, name)
            assert tuple(oshape) == (tuple(G.scene(name)[2]) if G.geom(cfg)[4] else G.out_shape(G.scene(name)[2], cfg))
            c = oc.long()
            key = ((c[:, 0] * oshape[0] + c[:, 1]) * oshape[1] + c[:, 2]) * oshape[2] + c[:, 3]
            assert bool((key[1:] > key[:-1]).all()), (cfg, name)
            assert len(oc) == 0 or (bool((c[:, 1:] >= 0).all()) and bool((c[:, 1:] < torch.tensor(oshape)[None]).all())), (cfg, name)
            empty += len(oc) == 0
            for t, (pi, po) in enumerate(pairs):
                assert len(pi) == len(po) <= min(n, len(oc)), (cfg, name, t)
                assert np.all(np.diff(pi) > 0) and np.all(np.diff(po) > 0), (cfg, name, t)
                assert len(pi) == 0 or (pi.min() >= 0 and pi.max() < n and po.min() >= 0 and po.max() < len(oc)), (cfg, name, t)
    # the configurations do what they are in the list for
    assert len(G.brute('k3s1p1', 'block4')[0]) == 6 ** 3 > 64                       # a regular convolution grows the set
    assert len(G.brute('k3s3p1', 'line_x_33')[0]) == 11 and sum(len(i) for i, _ in G.brute('k3s3p1', 'line_x_33')[2]) == 33
    assert len(G.brute('k1s2p0', 'block4')[0]) == 8 and len(G.brute('k1s2p0', 'block4')[2]) == 1    # K = 1: odd cells have no output
    assert [len(G.brute(c, 'block5')[2]) for c in ('k331s221p110', 'k122s2p0', 'k321s121p100', 'subm_k133')] == [9, 4, 6, 9]
    n_in = len(G.scene('block5')[3])
    assert len(G.brute('k3s2p1', 'block5')[0]) != n_in and len(G.brute('k3s2p1', 'block5')[2]) == 27     # n_in != n_out at K = 27
    d2 = [len(i) for i, _ in G.brute('subm_k3d2', 'block5')[2]]
    assert d2[13] == 125 and d2[0] == 27 and d2 != [len(i) for i, _ in G.brute(G.SUBM_K3, 'block5')[2]]  # neighbours two cells away
    assert len(G.brute('k3s2p0', 'block_in_far_corner')[0]) < len(G.brute('k3s2p1', 'block_in_far_corner')[0])      # p = 0 drops the far edge
    # empty output levels are among the cases: a line at odd y, z under stride 2 without padding and a 1-tap kernel
    assert empty > 0 and len(G.brute('k1s2p0', 'line_x_33')[0]) == 0 and len(G.brute('k1s2p0', 'single_voxel')[0]) == 0


SMALL = [('fwd', 16, 32), ('inv', 32, 16)]


@pytest.mark.parametrize('mode,cin,cout', SMALL)
def test_dense_reference_equals_the_pair_list_sum(mode, cin, cout):
    for ci, cfg in enumerate(G.CONFIGS):
        for name in G.SCENES[ci % 3::3]:               # every scene under a third of the configurations, every configuration on 7 scenes
            inp = G.make_inputs(mode, cfg, name, cin, cout, seed=7 + ci)
            ref, got = G.reference(mode, inp, cfg, name), G.pair_sum(mode, inp, cfg, name)
            for q in ('y', 'dx', 'dw', 'dadd'):
                assert ref[q].shape == got[q].shape, (cfg, name, q)
                if ref[q].numel():                     # (an empty output level: nothing to compare on that side)
                    scale = float(ref[q].abs().max()) + 1e-300
                    assert float((ref[q] - got[q]).abs().max()) <= 1e-12 * scale, (cfg, name, q)
            cnt = G.product_counts(mode, cfg, name)
            assert np.array_equal(cnt['dw'].numpy(), np.array([len(i) for i, _ in G.brute(cfg, name)[2]], np.float64)), (cfg, name)


@pytest.mark.parametrize('mode,cin,cout', SMALL)
def test_fp32_pair_sum_is_inside_the_bound_and_a_sabotaged_one_outside(mode, cin, cout):
    caught = 0
    for cfg in ('k3s2p1', 'k3s2p2d2', 'k321s121p100', 'subm_k3d2', 'k1s2p0'):
        for name in ('line_x_33', 'block5', 'empty_middle_scene', 'block5_odd_extent'):
            c = G.case(mode, cfg, name, cin, cout)
            pairs = G.brute(cfg, name)[2]
            o32 = G.pair_sum(mode, c['inp'], cfg, name, torch.float32)
            for q in ('y', 'dx', 'dw', 'dadd'):
                for operands in ('fp32', 'bf16'):
                    assert cg.excess(o32[q], c['ref'][q], c['bound'][operands][q]) <= 1.0, (cfg, name, q, operands)
            if not any(len(i) for i, _ in pairs):
                # an empty output level (the line lies at odd y and z): nothing to sabotage
                assert len(G.brute(cfg, name)[0]) == 0 and name == 'line_x_33' and cfg in ('k1s2p0', 'k3s2p2d2'), (cfg, name)
                continue
            # one pair dropped: the heaviest source row of the last offset that has pairs
            t = max(j for j in range(len(pairs)) if len(pairs[j][0]))
            src = pairs[t][0] if mode == 'fwd' else pairs[t][1]
            p = int(c['inp']['x'].abs().sum(1)[torch.as_tensor(src, dtype=torch.long)].argmax())
            bad = [(np.delete(i, p), np.delete(o, p)) if j == t else (i, o) for j, (i, o) in enumerate(pairs)]
            y = G.pair_sum(mode, c['inp'], cfg, name, torch.float32, pairs=bad)['y']
            for operands in ('fp32', 'bf16'):
                assert cg.excess(y, c['ref']['y'], c['bound'][operands]['y']) > 1.0, (cfg, name, operands)
            # offsets mirrored (where the kernel has more than one offset), the last row left at zero, an unwritten element
            if len(pairs) > 1:
                w = c['inp']['w']
                flipped = w.reshape(w.shape[0], len(pairs), -1).flip(1).reshape(w.shape)
                y = G.pair_sum(mode, dict(c['inp'], w=flipped), cfg, name, torch.float32)['y']
                assert cg.excess(y, c['ref']['y'], c['bound']['fp32']['y']) > 1.0, (cfg, name)
            y = o32['y'].clone()
            y[-1] = 0.0
            assert cg.excess(y, c['ref']['y'], c['bound']['bf16']['y']) > 1.0, (cfg, name)
            y = o32['y'].clone()
            y[0, 0] = float('nan')
            assert cg.excess(y, c['ref']['y'], c['bound']['bf16']['y']) == float('inf'), (cfg, name)
            caught += 1
    assert caught == 18


# ---------------------------------------------------------------------------------------------------------------- constructor contract
def test_constructors_accept_ints_and_triples():
    from unidet3d_amd import sparse as S
    m = S.SparseConv3d(32, 64, 3, stride=2, padding=1)
    assert tuple(m.weight.shape) == (64, 3, 3, 3, 32) and m.K == 27 and m.kernel_size == 3 and m.general
    assert m.stride == (2, 2, 2) and m.padding == (1, 1, 1) and m.dilation == (1, 1, 1)
    m = S.SparseConv3d(16, 32, (3, 2, 1), stride=[1, 2, 1], padding=(1, 0, 0), dilation=1, indice_key='a')
    assert tuple(m.weight.shape) == (32, 3, 2, 1, 16) and m.K == 6 and m.kernel_size == (3, 2, 1) and m.stride == (1, 2, 1)
    m = S.SparseConv3d(32, 64, kernel_size=2, stride=2, bias=False, indice_key='spconv1')              # the U-Net's own layer: the carve-out
    assert not m.general and m.K == 8 and m.kernel_size == 2 and tuple(m.weight.shape) == (64, 2, 2, 2, 32)
    assert not S.SparseConv3d(32, 64, (2, 2, 2), (2, 2, 2), (0, 0, 0), (1, 1, 1)).general
    assert S.SparseConv3d(32, 64, 2, stride=2, padding=1).general and S.SparseConv3d(32, 64, 2, stride=1).general
    m = S.SubMConv3d(32, 32, kernel_size=3, padding=1, bias=False, indice_key='subm1')
    assert not m.general and m.K == 27 and m.kernel_size == 3
    m = S.SubMConv3d(32, 32, 3, dilation=2)
    assert m.general and m._subm_geom == (3, 3, 3, 1, 1, 1, 2, 2, 2, 2, 2, 2)
    m = S.SubMConv3d(32, 32, (1, 3, 3), stride=2, padding=5)               # stride / padding of a submanifold layer: without effect
    assert m.general and m.K == 9 and m._subm_geom == (1, 3, 3, 1, 1, 1, 0, 1, 1, 1, 1, 1) and tuple(m.weight.shape) == (32, 1, 3, 3, 32)
    assert S.SubMConv3d(32, 64, 1).K == 1 and S.SubMConv3d(32, 64, (1, 1, 1)).kernel_size == 1          # the dense-GEMM route
    m = S.SparseInverseConv3d(64, 32, 3, indice_key='a')
    assert tuple(m.weight.shape) == (32, 3, 3, 3, 64) and m.K == 27
    # the weight packer sees every layer's own offset count
    packs = S.WeightPacks(torch.nn.Sequential(S.SparseConv3d(32, 64, (3, 3, 1), 2, 1), S.SubMConv3d(32, 32, 1)))
    assert [c.K for c in packs.convs] == [9]


@pytest.mark.parametrize('kw,text', [
    (dict(kernel_size=4), '1 <= extent <= 3'), (dict(kernel_size=(3, 0, 3)), '1 <= extent <= 3'), (dict(kernel_size=(3, 3)), 'three ints'),
    (dict(kernel_size=3.0), 'three ints'), (dict(kernel_size=3, stride=0), 'stride must be >= 1'), (dict(kernel_size=3, stride=(2, -1, 2)), 'stride must be >= 1'),
    (dict(kernel_size=3, padding=-1), 'padding must be >= 0'), (dict(kernel_size=3, dilation=0), 'dilation must be >= 1'),
    (dict(kernel_size=3, dilation=(1, 1)), 'three ints'), (dict(kernel_size=3, bias=True), 'bias=True')])
def test_constructors_refuse_with_the_constraint_in_the_text(kw, text):
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    with pytest.raises(L.U3DError, match=re.escape(text)):
        S.SparseConv3d(32, 64, **kw)
    if 'stride' not in kw and 'padding' not in kw:
        with pytest.raises(L.U3DError, match=re.escape(text)):
            S.SubMConv3d(32, 64, **kw)


def test_constructors_accept_numpy_integers():
    from unidet3d_amd import sparse as S
    m = S.SparseConv3d(32, 64, np.int64(3), stride=np.array([2, 2, 1]), padding=np.int32(1), dilation=[np.int64(1)] * 3)
    assert m.geom == (3, 3, 3, 2, 2, 1, 1, 1, 1, 1, 1, 1) and all(type(a) is int for a in m.geom) and m.kernel_size == 3
    assert not S.SparseConv3d(32, 64, np.int64(2), np.int64(2)).general                        # still the carve-out
    assert S.SubMConv3d(32, 32, np.array([1, 3, 3])).K == 9


def test_pair_count_cache_tells_geometries_of_one_level_apart():
    """two rulebooks with the same K and row counts (SubM k=3, dilation 1 and 2) must not book each other's pair count"""
    from unidet3d_amd import sparse as S
    a, b = S.SubMConv3d(32, 32, 3, indice_key='a'), S.SubMConv3d(32, 32, 3, dilation=2, indice_key='b')
    n = 123457                                        # a row count no other test uses: the cache is module state
    ra, rb = [S.Rulebook(torch.zeros(27, 1, dtype=torch.int32), torch.zeros(27, 1, dtype=torch.int32), torch.full((27,), c, dtype=torch.int32), 27, n, n)
              for c in (5, 2)]
    ra.geom, rb.geom = a._rb_geom, b._rb_geom
    assert ra.total_pairs == 27 * 5 and rb.total_pairs == 27 * 2
    again = S.Rulebook(ra.pair_in, ra.pair_out, torch.zeros(27, dtype=torch.int32), 27, n, n)       # same geometry: served from the cache
    again.geom = a._rb_geom
    assert again.total_pairs == 27 * 5


def test_unet_that_holds_a_general_layer_gets_the_empty_fusion_plan():
    from torch import nn
    from unidet3d_amd import sparse as S
    from unidet3d_amd.spconv_unet import SpConvUNet, fusion_plan
    front = S.SparseSequential(S.SubMConv3d(6, 32, 3, padding=1, indice_key='subm1'))
    back = S.SparseSequential(S.SparseBatchNorm(32), nn.ReLU())
    unet = SpConvUNet([32, 64], block_reps=2)
    plan = fusion_plan(unet, front, back)
    assert plan.convs and plan.norms and plan.cats               # the U-Net as it is built: planned
    unet.conv._modules['2'] = S.SparseConv3d(32, 64, 3, stride=2, padding=1, indice_key='spconv1')
    unet.deconv._modules['2'] = S.SparseInverseConv3d(64, 32, 3, indice_key='spconv1')
    plan = fusion_plan(unet, front, back)
    assert not plan.convs and not plan.norms and not plan.cats
    # a dilated submanifold layer inside a block does the same; so does a general first producer
    unet = SpConvUNet([32, 64], block_reps=2)
    unet.blocks[0].conv_branch._modules['2'] = S.SubMConv3d(32, 32, 3, dilation=2, indice_key='dil')
    plan = fusion_plan(unet, front, back)
    assert not plan.convs and not plan.norms and not plan.cats
    unet = SpConvUNet([32, 64], block_reps=2)
    plan = fusion_plan(unet, S.SparseSequential(S.SubMConv3d(6, 32, 3, dilation=2, indice_key='subm1')), back)
    assert not plan.convs and not plan.norms and not plan.cats


def test_submanifold_extents_are_odd():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    for k in (2, (3, 2, 3)):
        with pytest.raises(L.U3DError, match='must be 1 or 3'):
            S.SubMConv3d(32, 32, k)


class _FakeTensor:
    """what ``geometry`` reads of a sparse tensor when the rulebook is already cached"""

    def __init__(self, indice_dict):
        self.indice_dict = indice_dict


def test_shared_indice_key_with_another_geometry_raises():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    z = torch.zeros(1, 1, dtype=torch.int32)

    def rulebook(layer):
        rb = S.Rulebook(z, z, z[0], layer.K, 1, 1)
        rb.geom = layer._rb_geom
        return rb
    a, same, other = S.SparseConv3d(32, 64, 3, 2, 1, indice_key='d'), S.SparseConv3d(32, 64, 3, 2, 1, indice_key='d'), S.SparseConv3d(32, 64, 3, 2, 0, indice_key='d')
    x = _FakeTensor({('__down__', 'd'): (None, None, None, rulebook(a))})
    assert same.geometry(x)[3] is x.indice_dict[('__down__', 'd')][3]
    with pytest.raises(L.U3DError, match='share an indice_key'):
        other.geometry(x)
    with pytest.raises(L.U3DError, match='share an indice_key'):
        S.SparseConv3d(32, 64, 2, 2, indice_key='d').geometry(x)           # the U-Net's layer against a general rulebook
    s1, s2, s3 = S.SubMConv3d(32, 32, 3, indice_key='s'), S.SubMConv3d(32, 32, 3, indice_key='s'), S.SubMConv3d(32, 32, 3, dilation=2, indice_key='s')
    x = _FakeTensor({'s': rulebook(s1)})
    assert s2.geometry(x) is x.indice_dict['s']
    with pytest.raises(L.U3DError, match='share an indice_key'):
        s3.geometry(x)
    with pytest.raises(L.U3DError, match='share an indice_key'):
        S.SubMConv3d(32, 32, (1, 3, 3), indice_key='s').geometry(x)
    # the inverse layer: its kernel must be the strided layer's
    x.indice_dict['d'] = (rulebook(a), None, None, None)
    x.features = torch.zeros(1, 64)
    with pytest.raises(L.U3DError, match='kernel_size'):
        S.SparseInverseConv3d(64, 32, 2, indice_key='d')(x)
    with pytest.raises(L.U3DError, match='no rulebook saved'):
        S.SparseInverseConv3d(64, 32, 3, indice_key='nope')(x)


# ---------------------------------------------------------------------------------------------------------------- C boundary
def test_new_entry_points_are_declared_under_the_unchanged_abi_version():
    from unidet3d_amd import _lib as L
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'u3d.h')).read(), flags=re.S)
    assert L.ABI_VERSION == 117 and int(re.search(r'#define\s+U3D_ABI_VERSION\s+(\d+)', src).group(1)) == 117
    lib = L.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r'\b' + name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert m, f'{name} is not declared in include/u3d.h'
        assert name in L.PROTOTYPES and len(L.PROTOTYPES[name][1]) == len([p for p in m.group(1).split(',') if p.strip()]), name
        assert hasattr(lib, name), name


def test_geometry_entry_points_validate_on_the_host():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    lib = L.lib()
    out = (ctypes.c_int * 3)()

    def shape(k, s, p, d, ext):
        rc = lib.u3d_conv_out_shape(S._geom_array(S.conv_geometry(k, s, p, d)), *ext, out)
        return rc, list(out)
    for cfg in G.CONFIGS:
        k, s, p, d, subm = G.geom(cfg)
        for ext in ((8, 8, 8), (5, 6, 7), (136, 3, 3), (3, 3, 72)):
            assert shape(k, s, p, d, ext) == (0, list(ext) if subm else list(G.out_shape(ext, cfg))), (cfg, ext)
    assert shape(3, 2, 0, 1, (2, 8, 8)) == (0, [0, 3, 3])                       # smaller than the kernel: reported as empty
    bad = (ctypes.c_int * 12)(4, 3, 3, 1, 1, 1, 0, 0, 0, 1, 1, 1)
    assert lib.u3d_conv_out_shape(bad, 8, 8, 8, out) == -3 and b'outside 1..3' in lib.u3d_last_error()
    bad = (ctypes.c_int * 12)(3, 3, 3, 1, 0, 1, 0, 0, 0, 1, 1, 1)
    assert lib.u3d_conv_out_shape(bad, 8, 8, 8, out) == -1 and b'stride' in lib.u3d_last_error()
    big = (ctypes.c_int * 12)(3, 3, 3, 1, 1, 1, 1 << 30, 0, 0, 1, 1, 1)
    assert lib.u3d_conv_out_shape(big, 8, 8, 8, out) == -3 and b'32-bit coordinates' in lib.u3d_last_error()
    assert lib.u3d_conv_out_shape(big, 0, 8, 8, out) == -1
    assert lib.u3d_conv_rulebook_ws_bytes(1000, 27) >= 2 * 27 * 4 * 4 and lib.u3d_conv_rulebook_ws_bytes(0, 27) == 0
    # refused before any launch: null pointers, both / neither output form, a cap below min(n_in, n_out)
    g = S._geom_array(S.conv_geometry(3, 2, 1, 1))
    assert lib.u3d_conv_mark(None, 10, g, 1, 8, 8, 8, None, None, None) == -1
    assert lib.u3d_conv_mark(8, 10, g, 1, 8, 8, 8, None, None, None) == -1 and b'exactly one' in lib.u3d_last_error()
    assert lib.u3d_conv_mark(8, 10, g, 1, 8, 8, 8, 8, 8, None) == -1
    assert lib.u3d_conv_mark(8, 10, S._geom_array(S.conv_geometry(3, 2, 0, 1)), 1, 2, 8, 8, 8, None, None) == -1 and b'empty' in lib.u3d_last_error()
    assert lib.u3d_conv_rulebook(8, 10, 20, 8, 8, 0, 1, 8, 8, 8, g, 9, 8, 8, 8, 8, None) == -1 and b'below min' in lib.u3d_last_error()
    assert lib.u3d_conv_rulebook(8, 0, 20, 8, 8, 0, 1, 8, 8, 8, g, 9, 8, 8, 8, 8, None) == -1


# ---------------------------------------------------------------------------------------------------------------- module boundaries
_MOVED_PUBLIC = ['OccupancyIndex', 'Rulebook', 'UpLevel', 'build_subm_rulebook', 'build_down_rulebook', 'build_conv_rulebook',
                 'build_convt_rulebook', 'conv_geometry', 'conv_out_shape', 'output_padding_of', 'convt_out_shape', 'strided_geometry',
                 'cached_level']
_MOVED_PRIVATE = ['_PAIR_CACHE', '_TILE_HISTORY', '_TILE_PRECOMPUTE', '_INDEX_MODE', '_HASH_ABOVE_BYTES', '_DOWN_K2S2', '_triple', '_geom_array',
                  '_agree']
_BOUNDARY_CHILD = '''
import sys, types
pkg = types.ModuleType('unidet3d_amd')          # the package without its __init__, which registers every model and so imports every module
pkg.__path__ = [sys.argv[1]]
sys.modules['unidet3d_amd'] = pkg
import unidet3d_amd.geometry as geometry
assert sorted(m for m in sys.modules if m.startswith('unidet3d_amd.')) == ['unidet3d_amd._lib', 'unidet3d_amd.geometry'], sorted(sys.modules)
import unidet3d_amd.ops
assert 'unidet3d_amd.sparse' not in sys.modules and 'unidet3d_amd.dense' not in sys.modules
assert unidet3d_amd.ops.OccupancyIndex is geometry.OccupancyIndex
import unidet3d_amd.sparse as sparse
public, private = sys.argv[2].split(','), sys.argv[3].split(',')
for name in public + ['_TILE_HISTORY']:
    assert getattr(sparse, name) is getattr(geometry, name), name
for name in private:
    assert hasattr(geometry, name), name
    assert not hasattr(sparse, name) or getattr(sparse, name) is getattr(geometry, name), name
for name in ('_INDEX_MODE', '_HASH_ABOVE_BYTES', '_TILE_PRECOMPUTE'):          # read where they are owned: a copy here would be a dead switch
    assert not hasattr(sparse, name), name
print('boundaries ok')
'''


def test_geometry_module_stands_below_the_layers_and_the_voxeliser():
    """In a fresh interpreter: ``geometry`` imports nothing of the package but ``_lib``; ``ops`` (the voxeliser) imports neither ``sparse``
    nor ``dense``; and every moved name that ``sparse`` still shows is the object ``geometry`` owns, the three environment switches not
    among them."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, '-c', _BOUNDARY_CHILD, os.path.join(ROOT, 'unidet3d_amd'), ','.join(_MOVED_PUBLIC), ','.join(_MOVED_PRIVATE)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and 'boundaries ok' in r.stdout, r.stderr[-3000:]
