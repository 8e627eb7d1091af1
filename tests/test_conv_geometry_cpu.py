"""Check the checker of tests/test_gpu_conv_geometry.py on the CPU: on every geometry of tests/_conv_geometry.py the float64 dense
references equal the oracle's gather-GEMM-scatter convolution on the oracle's rulebooks (1e-12), the oracle's own fp32 result lies
inside the rounding bound, and three sabotaged results -- one pair dropped, mirrored offsets swapped, the last row left at zero --
lie outside it wherever the sabotage changes anything."""
import numpy as np
import pytest
import torch

import _conv_geometry as cg
from oracle import sparse_ops as so

# (op, source channels, destination channels): small channel counts -- the checker does not depend on them
OPS = [('subm', 16, 32), ('down', 32, 64), ('inv', 64, 32)]


def _cases(op):
    return cg.geometries('subm' if op == 'subm' else 'down')


def _pairs(op, coords, shape):
    """oracle rulebook of ``op``: (pairs, destination rows, inverse flag)"""
    if op == 'subm':
        return so.build_subm_rulebook(coords, shape), len(coords), False
    oc, oshape, pairs = so.build_down_rulebook(coords, shape)
    oc2, oshape2 = cg.down_coords(coords, shape)
    assert torch.equal(oc, oc2) and tuple(int(s) for s in oshape) == oshape2
    return pairs, (len(oc) if op == 'down' else len(coords)), op == 'inv'


def _oracle(inp, pairs, n_dst, inverse, dtype):
    x, w, add = [inp[k].to(dtype).clone().requires_grad_() for k in ('x', 'w', 'add')]
    y = so.sparse_conv(x, w, pairs, n_dst, inverse=inverse) + add
    y.backward(inp['go'].to(dtype))
    return dict(y=y.detach(), dx=x.grad if x.grad is not None else torch.zeros_like(x), dw=w.grad, dadd=add.grad)


def test_geometry_list_is_what_the_kernel_tests_rely_on():
    for kind in ('subm', 'down'):
        for name, B, shape, coords in cg.geometries(kind):
            c = coords.long()
            key = ((c[:, 0] * shape[0] + c[:, 1]) * shape[1] + c[:, 2]) * shape[2] + c[:, 3]
            assert coords.dtype == torch.int32 and bool((key[1:] > key[:-1]).all()), name
            assert 1 <= len(coords) <= 520, name
    rows = {name: len(c) for name, _, _, c in cg.geometries('subm')}
    for L in cg.LINE_LENGTHS:
        assert rows[f'line_x_{L}'] == rows[f'line_z_{L}'] == L
    assert rows['block4'] == 64 and rows['block4_plus_detached'] == 65 and rows['block5'] == 125
    cnt = lambda name: [len(i) for i, _ in so.build_subm_rulebook(*cg.geometry('subm', name)[3:1:-1])]
    assert cnt('two_voxels_apart') == [0] * 13 + [2] + [0] * 13
    faces = [4, 10, 12, 14, 16, 22]
    for name in ('checkerboard8', 'checkerboard8_mod3'):
        c = cnt(name)
        assert all(c[k] == 0 for k in faces) and sum(1 for v in c if v) > 1, (name, c)
    assert cnt('checkerboard8_mod3')[0] > 0 and cnt('checkerboard8')[0] == 0              # corner offsets only in the second
    assert max(cnt('block5')) == 125 and min(cnt('block5')) == 64
    # the far corner: shape - 1 is occupied on every axis, in both scenes
    _, B, shape, coords = cg.geometry('subm', 'block_in_far_corner')
    assert [int(v) for v in coords[:, 1:].max(0)[0]] == [s - 1 for s in shape]
    # the batch with an empty middle scene; the odd extent really drops rows
    assert sorted(set(cg.geometry('subm', 'empty_middle_scene')[3][:, 0].tolist())) == [0, 2]
    _, B, shape, coords = cg.geometry('down', 'block5_odd_extent')
    assert sum(len(i) for i, _ in so.build_down_rulebook(coords, shape)[2]) == 2 * 64 < len(coords)
    for k in range(8):
        _, B, shape, coords = cg.geometry('down', f'child_{k}')
        assert [len(i) for i, _ in so.build_down_rulebook(coords, shape)[2]] == [int(j == k) for j in range(8)]


@pytest.mark.parametrize('op,cin,cout', OPS)
def test_dense_reference_equals_oracle_and_fp32_oracle_is_inside_the_bound(op, cin, cout):
    for gi, (name, B, shape, coords) in enumerate(_cases(op)):
        pairs, n_dst, inverse = _pairs(op, coords, shape)
        inp = cg.make_inputs(op, coords, shape, cin, cout, seed=100 + gi)
        ref = cg.reference(op, inp, coords, B, shape)
        o64 = _oracle(inp, pairs, n_dst, inverse, torch.float64)
        for k in ('y', 'dx', 'dw', 'dadd'):
            scale = float(ref[k].abs().max()) + 1e-300
            assert float((ref[k] - o64[k]).abs().max()) <= 1e-12 * scale, (name, k)
        bnd = cg.bounds(op, inp, coords, B, shape, 'fp32')
        # the counts the bound uses are the rulebook's
        assert np.array_equal(bnd['counts']['dw'].numpy(), np.array([len(i) for i, _ in pairs], np.float64)), name
        o32 = _oracle(inp, pairs, n_dst, inverse, torch.float32)
        for k in ('y', 'dx', 'dw', 'dadd'):
            assert cg.excess(o32[k], ref[k], bnd[k]) <= 1.0, (name, k, cg.excess(o32[k], ref[k], bnd[k]))
            assert cg.excess(o32[k], ref[k], cg.bounds(op, inp, coords, B, shape, 'bf16')[k]) <= 1.0, (name, k)
        # where S == 0 only an exact zero passes
        zero = bnd['dw'] == 0
        if bool(zero.any()):
            bad = ref['dw'].clone()
            bad[zero] = 1e-30
            assert cg.excess(bad, ref['dw'], bnd['dw']) == float('inf'), name
        nanned = ref['y'].clone()
        nanned[-1, -1] = float('nan')
        assert cg.excess(nanned, ref['y'], bnd['y']) == float('inf'), name


def _sabotaged(kind, op, inp, pairs, n_dst, inverse, heaviest=False):
    """the oracle's fp32 forward with one defect; None where the defect changes nothing on this geometry.  ``heaviest``: the dropped pair
    is the one of its offset whose source row has the largest sum |x| instead of the last one"""
    K = len(pairs)
    clean = _oracle(inp, pairs, n_dst, inverse, torch.float32)['y']
    if kind == 'pair_dropped':                 # one pair of the last offset that has any
        k = max(j for j in range(K) if len(pairs[j][0]))
        src = pairs[k][1] if inverse else pairs[k][0]
        p = int(inp['x'].abs().sum(1)[torch.as_tensor(src, dtype=torch.long)].argmax()) if heaviest else len(src) - 1
        bad_pairs = [(np.delete(i, p), np.delete(o, p)) if j == k else (i, o) for j, (i, o) in enumerate(pairs)]
        y = _oracle(inp, bad_pairs, n_dst, inverse, torch.float32)['y']
    elif kind == 'offsets_mirrored':           # offset k computed with the weights of offset K - 1 - k
        k3 = inp['w'].shape[1]
        w = inp['w'].reshape(inp['w'].shape[0], K, -1).flip(1).reshape(inp['w'].shape)
        assert k3 ** 3 == K
        y = _oracle(dict(inp, w=w), pairs, n_dst, inverse, torch.float32)['y']
    else:                                      # the last row of the last tile left at zero
        y = clean.clone()
        y[-1] = 0.0
    return None if torch.equal(y, clean) else y


@pytest.mark.parametrize('kind', ['pair_dropped', 'offsets_mirrored', 'last_row_zero'])
@pytest.mark.parametrize('op,cin,cout', OPS)
def test_sabotaged_results_are_outside_the_bound(op, cin, cout, kind):
    """Under the fp32 bound every defect is caught whichever pair is dropped.  The bf16 bound is 2**-7 of S by construction: one product
    row among the up to 27 of an output whose |x| is small next to its heavy-tailed neighbours moves no element by that much and is
    invisible to ANY bound that admits bf16 rounding -- there the dropped pair is its offset's heaviest row."""
    caught = unchanged = 0
    for gi, (name, B, shape, coords) in enumerate(_cases(op)):
        pairs, n_dst, inverse = _pairs(op, coords, shape)
        inp = cg.make_inputs(op, coords, shape, cin, cout, seed=100 + gi)
        y = _sabotaged(kind, op, inp, pairs, n_dst, inverse)
        if y is None:
            # only mirrored offsets can change nothing: SubM rulebooks whose only pairs are the centre tap's
            assert kind == 'offsets_mirrored' and op == 'subm' and name in ('single_voxel', 'two_voxels_apart'), (name, kind)
            unchanged += 1
            continue
        ref = cg.reference(op, inp, coords, B, shape)['y']
        for operands in ('fp32', 'bf16'):
            if operands == 'bf16' and kind == 'pair_dropped':
                y = _sabotaged(kind, op, inp, pairs, n_dst, inverse, heaviest=True)
            bnd = cg.bounds(op, inp, coords, B, shape, operands)['y']
            assert cg.excess(y, ref, bnd) > 1.0, (name, kind, operands, cg.excess(y, ref, bnd))
        caught += 1
    assert caught >= len(_cases(op)) - 2 and unchanged <= 2
