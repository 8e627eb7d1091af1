"""Sparse convolutions (csrc/spconv*.hip through sparse.sparse_conv) on the degenerate level geometries of tests/_conv_geometry.py:
a handful of rows, offsets without pairs, row counts one off a 32- / 64-row tile, scenes that touch in coordinates but not in batch
id, voxels on the faces of the grid.  Every y, dx, dW and addend gradient is compared ELEMENTWISE with the float64 dense
convolution (F.conv3d / F.conv_transpose3d sampled at the active sites) under the derived rounding bound of _conv_geometry.bound
-- an error confined to small elements (the last row of a ragged tile, a row whose only pair is the centre tap, the dW slice of an
offset with few pairs) does not hide behind the tensor's maximum.  Freed NaN-filled blocks of the sizes of dst, dW and the offset-group
workspace are handed to the caching allocator in front of every forward and backward, so an element a kernel fails to write is not finite.
The largest err / bound per kernel selection goes to the parity log (_parity.log_errors, test 'conv_geometry')."""
import contextlib

import numpy as np
import pytest
import torch

import _conv_geometry as cg
import _parity
from oracle import sparse_ops as so
from test_gpu_kernels import CONV_SHAPES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DOWN_SHAPES = [(32, 64), (64, 96), (96, 128), (128, 160)]            # the list of test_strided_and_inverse_conv_fwd_bwd
# the four settings of test_gpu_kernels.math_mode, bf16 operands gathered from fp32 rows, bf16 operands gathered from bf16 rows
SELECTIONS = ['bf16x3', 'bf16x3-ts', 'bf16x3-wavetile', 'mfma', 'bf16', 'bf16-rows']


@contextlib.contextmanager
def _selection(sel):
    from unidet3d_amd import precision as P
    from unidet3d_amd import sparse
    with contextlib.ExitStack() as st:
        if sel in ('bf16', 'bf16-rows'):
            st.enter_context(P.operands('bf16'))
            st.enter_context(P.bf16_rows_mode(sel == 'bf16-rows'))
        else:
            st.enter_context(P.fp32_math(sel.split('-')[0]))
            st.enter_context(P.conv_kernel('wave' if sel.endswith('wavetile') else 'workgroup'))
            st.enter_context(sparse.conv_ts(sel.endswith('-ts')))
        yield


def _operands(sel):
    return 'bf16' if sel.startswith('bf16') and not sel.startswith('bf16x3') else 'fp32'


def _check_pairs(gpu_lists, oracle_lists, name):
    assert len(gpu_lists) == len(oracle_lists), name
    for k, ((gi, go), (oi, oo)) in enumerate(zip(gpu_lists, oracle_lists)):
        assert np.array_equal(gi, oi) and np.array_equal(go, oo), f'{name}: offset {k} differs'


_LEVELS = {}


def _level(kind, name):
    """index, canonical rows and rulebook(s) of a geometry, built once; every rulebook bit for bit the oracle's"""
    from unidet3d_amd import sparse
    if (kind, name) not in _LEVELS:
        _, B, shape, coords = cg.geometry(kind, name)
        ix = sparse.OccupancyIndex.from_coords(coords.to(DEV), B, shape)
        n = ix.count()
        rows = ix.coords(n)
        assert n == len(coords) and torch.equal(rows.cpu(), coords), f'{name}: canonical rows'
        lvl = dict(B=B, shape=shape, coords=coords, n=n)
        if kind == 'subm':
            lvl['rb'] = sparse.build_subm_rulebook(rows, ix)
            lvl['pairs'] = so.build_subm_rulebook(coords, shape)
            _check_pairs(lvl['rb'].lists(), lvl['pairs'], name)
        else:
            oc2, oshape2, lvl['pairs'] = so.build_down_rulebook(coords, shape)
            c2, shape2, ix2, lvl['rb'] = sparse.build_down_rulebook(rows, B, shape)
            assert torch.equal(c2.cpu(), oc2) and list(shape2) == [int(s) for s in oshape2], f'{name}: coarse rows'
            _check_pairs(lvl['rb'].lists(), lvl['pairs'], name)
            lvl['coords2'] = oc2
        assert lvl['rb'].counts.cpu().tolist() == [len(i) for i, _ in lvl['pairs']], name
        _LEVELS[(kind, name)] = lvl
    return _LEVELS[(kind, name)]


@pytest.mark.parametrize('kind', ['subm', 'down'])
def test_rulebooks_equal_the_oracle_bit_for_bit(kind):
    for name, _, _, _ in cg.geometries(kind):
        _level(kind, name)


def _poison(sizes):
    """allocate and free NaN-filled blocks of these element counts: the caching allocator hands them to the next torch.empty"""
    blocks = [torch.full((int(s),), float('nan'), dtype=torch.float32, device=DEV) for s in sizes if s > 0]
    del blocks


def _groups(cs, cd, K, n_dst, rows):
    from unidet3d_amd import sparse
    return sparse._plan(cs, cd, K, n_dst, rows)[1] if cd % 32 == 0 and n_dst > 0 else 1


def _run(op, lvl, inp, sel, x=None, go=None):
    """forward (+ addend) and backward of ``op`` under the current selection -> dict(y, dx, dw, dadd) on the device"""
    from unidet3d_amd import sparse
    rb = lvl['rb']
    x = inp['x'] if x is None else x
    go = inp['go'] if go is None else go
    cout, cin = inp['w'].shape[0], inp['w'].shape[-1]
    rows = sel == 'bf16-rows'
    xg = x.to(DEV).clone().requires_grad_(cin != 16)         # 16 channels: the padded network input, whose gradient is not built
    wg, ag, gg = inp['w'].to(DEV).clone().requires_grad_(), inp['add'].to(DEV).clone().requires_grad_(), go.to(DEV).clone()
    if rows and cin % 32 == 0:
        sparse.attach_shadow(xg, sparse.to_shadow(xg))
    if rows and cout % 32 == 0:
        sparse.attach_shadow(gg, sparse.to_shadow(gg))
    ns, nd = xg.shape[0], gg.shape[0]
    K = rb.K
    _poison([nd * cout, _groups(cin, cout, K, nd, rows and cin % 32 == 0) * nd * cout])
    y = sparse.sparse_conv(xg, wg, rb, 'inv' if op == 'inv' else 'fwd', ag)
    _poison([ns * cin, wg.numel(), (_groups(cout, cin, K, ns, rows) if cin != 16 else 1) * ns * cin, nd * cout])
    y.backward(gg)
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xg.grad, dw=wg.grad, dadd=ag.grad)


def _check_case(op, name, cin, cout, sel, ratios, bad, tag=''):
    """one geometry, one channel pair, the current selection: elementwise against the float64 dense reference"""
    kind = 'subm' if op == 'subm' else 'down'
    lvl, case = _level(kind, name), cg.case(op, name, cin, cout)
    got = _run(op, lvl, case['inp'], sel)
    bnd = case['bound'][_operands(sel)]
    where = f'{tag}{op} {cin}->{cout} {sel} on {name}'
    for k in ('y', 'dx', 'dw', 'dadd'):
        if k == 'dx' and cin == 16:
            assert got['dx'] is None, where
            continue
        r = cg.excess(got[k], case['ref'][k], bnd[k])
        if r >= ratios[k][0]:
            ratios[k] = (r, name)
        if not r <= 1.0:
            bad.append(f'{where}: {k} err / bound = {r:.3g}')
    # nothing left unwritten: an offset without pairs has an exactly zero dW slice, a row without pairs is exactly its addend
    K = lvl['rb'].K
    dw = got['dw'].reshape(cout, K, cin)
    for k in np.nonzero(case['counts']['dw'].numpy() == 0)[0]:
        if not bool((dw[:, int(k), :] == 0).all()):
            bad.append(f'{where}: dW of the empty offset {int(k)} is not 0')
    lonely = (case['counts']['y'] == 0).nonzero().flatten().to(DEV)
    if len(lonely) and not torch.equal(got['y'][lonely], case['inp']['add'].to(DEV)[lonely]):
        bad.append(f'{where}: rows without pairs differ from the addend')
    return got


def _log(sel, op, cin, cout, ratios, extra=None):
    rec = dict(selection=sel, op=op, cin=cin, cout=cout, **{f'{k}_ratio': v[0] for k, v in ratios.items()},
               **{f'{k}_worst': v[1] for k, v in ratios.items()}, **(extra or {}))
    _parity.log_errors('conv_geometry', rec)
    print('conv_geometry', rec)


def _fresh():
    return {k: (0.0, None) for k in ('y', 'dx', 'dw', 'dadd')}


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('cin,cout', CONV_SHAPES)
def test_subm_conv_on_every_geometry(cin, cout, sel):
    ratios, bad = _fresh(), []
    with _selection(sel):
        for name, _, _, _ in cg.geometries('subm'):
            _check_case('subm', name, cin, cout, sel, ratios, bad)
    _log(sel, 'subm', cin, cout, ratios)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('cin,cout', DOWN_SHAPES)
def test_strided_and_inverse_conv_on_every_geometry(cin, cout, sel):
    """strided cin -> cout and, on the same pairs, inverse cout -> cin; the rows an odd extent leaves without a parent take no part
    in the strided convolution (dx exactly 0) and receive the bare addend from the inverse one"""
    bad = []
    with _selection(sel):
        for op, a, b in (('down', cin, cout), ('inv', cout, cin)):
            ratios = _fresh()
            for name, _, _, _ in cg.geometries('down'):
                _check_case(op, name, a, b, sel, ratios, bad)
            _log(sel, op, a, b, ratios)
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------------------- plans at tile edges
# kernel forms of the pair-list kernels: operand format x gathered rows x tile form.  The bf16-row kernel (u3d_spconv_gmm_bf16a) exists
# in the workgroup-tile form only.
PLAN_SELECTIONS = {'x3-wave': ('bf16x3', 'wave'), 'x3-workgroup': ('bf16x3', 'workgroup-all'), 'bf16-wave': ('bf16', 'wave'),
                   'bf16-workgroup': ('bf16', 'workgroup-all'), 'bf16rows-workgroup': ('bf16-rows', 'workgroup-all')}
# 16 source channels have no bf16 / three-plane and no workgroup-tile instantiation (gmm_wg_supported: cs16 = 1): that layer runs the fp32
# wave-tile kernel under every selection -- and under every plan, which is why it is in the list
PLAN_SUBM_SHAPES = [(16, 32), (32, 32), (64, 32), (96, 96)]
PLAN_DOWN_SHAPES = [(32, 64)]


def _plan_refused(cs, cd, K, n_dst, rows, R, G):
    """plan_gmm honours U3D_GMM_R always and U3D_GMM_G only for 27-offset rulebooks: the combinations it refuses are exactly
    (8 offsets, G in {3, 9}), where it keeps one group -- the launch is then the G = 1 launch that is checked anyway"""
    from unidet3d_amd import sparse
    got = sparse._plan(cs, cd, K, n_dst, rows)
    if got == (R, G):
        return False
    assert K < 27 and G > 1 and got == (R, 1), (cs, cd, K, n_dst, rows, R, G, got)
    return True


@pytest.mark.parametrize('R', [32, 64])
@pytest.mark.parametrize('form', list(PLAN_SELECTIONS))
def test_every_plan_at_every_tile_edge(form, R, monkeypatch):
    """U3D_GMM_R x U3D_GMM_G (read by plan_gmm on every call) on the lines of 31 .. 129 rows and the blocks: every plan against the
    same reference under the same bound, and the results of 1, 3 and 9 offset groups within 2 * bound of each other.
    Refused, by name: strided / inverse rulebooks (8 offsets) with G = 3 and G = 9 -- plan_gmm keeps one group there."""
    from unidet3d_amd import precision as P
    sel, kernel = PLAN_SELECTIONS[form]
    monkeypatch.setenv('U3D_GMM_R', str(R))
    bad, refused = [], set()
    cases = [('subm', s) for s in PLAN_SUBM_SHAPES] + [('down', s) for s in PLAN_DOWN_SHAPES] + [('inv', s[::-1]) for s in PLAN_DOWN_SHAPES]
    ratios = {G: _fresh() for G in (1, 3, 9)}
    with _selection(sel), P.conv_kernel(kernel):
        for op, (cin, cout) in cases:
            kind = 'subm' if op == 'subm' else 'down'
            for name in [g[0] for g in cg.geometries(kind) if cg.is_line_or_block(g[0])]:
                lvl, by_g = _level(kind, name), {}
                ns, nd = cg.n_rows(op, lvl['coords'], lvl['shape'])
                rows = sel == 'bf16-rows'
                for G in (1, 3, 9):
                    monkeypatch.setenv('U3D_GMM_G', str(G))
                    fwd_refused = _plan_refused(cin, cout, lvl['rb'].K, nd, rows and cin % 32 == 0, R, G)
                    if cin != 16:
                        assert _plan_refused(cout, cin, lvl['rb'].K, ns, rows, R, G) == fwd_refused
                    if fwd_refused:
                        refused.add((lvl['rb'].K, G))
                        continue
                    by_g[G] = _check_case(op, name, cin, cout, sel, ratios[G], bad, tag=f'R={R} G={G} {kernel} ')
                bnd = cg.case(op, name, cin, cout)['bound'][_operands(sel)]
                for G in (3, 9):
                    if G not in by_g:
                        continue
                    for k in ('y', 'dx'):
                        if by_g[G][k] is None:
                            continue
                        d = (by_g[G][k].double().cpu() - by_g[1][k].double().cpu()).abs()
                        if not bool((d <= 2 * bnd[k]).all()):
                            bad.append(f'R={R} {form} {op} {cin}->{cout} on {name}: {k} of G={G} and G=1 differ by more than 2 * bound')
    for G in (1, 3, 9):
        _log(sel, 'plans', 0, 0, ratios[G], dict(form=form, R=R, G=G))
    assert refused == {(8, 3), (8, 9)}, refused
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------------------- row isolation
@pytest.mark.parametrize('sel', SELECTIONS)
def test_rows_of_one_scene_do_not_see_the_other_scene(sel):
    """two scenes at identical coordinates: with one scene's features (forward) and incoming gradients (input gradient) replaced by
    NaN, the other scene's y and dx rows stay finite and bit-identical to the clean run -- same geometry, same launch, no shared
    product.  (dW sums over both scenes and is not looked at.)  Both ways round."""
    cases = [('subm', n, c) for n in ('two_scenes_same_coords', 'block_in_far_corner') for c in ((32, 32), (64, 32), (96, 96))]
    cases += [(op, 'block5_odd_extent', c) for op, c in (('down', (32, 64)), ('inv', (64, 32)))]
    with _selection(sel):
        for op, name, (cin, cout) in cases:
            kind = 'subm' if op == 'subm' else 'down'
            lvl, case = _level(kind, name), cg.case(op, name, cin, cout)
            fine, coarse = lvl['coords'][:, 0], (lvl['coords2'][:, 0] if kind == 'down' else None)
            b_src, b_dst = dict(subm=(fine, fine), down=(fine, coarse), inv=(coarse, fine))[op]
            clean = _run(op, lvl, case['inp'], sel)
            for dead in (1, 0):
                x, go = case['inp']['x'].clone(), case['inp']['go'].clone()
                x[b_src == dead] = float('nan')
                go[b_dst == dead] = float('nan')
                got = _run(op, lvl, case['inp'], sel, x=x, go=go)
                for k, b in (('y', b_dst), ('dx', b_src)):
                    live = (b != dead).to(DEV)
                    where = f'{op} {cin}->{cout} {sel} on {name}, scene {dead} NaN: {k}'
                    assert bool(live.any()) and bool(torch.isfinite(got[k][live]).all()), where
                    assert torch.equal(got[k][live], clean[k][live]), where
                    assert bool(torch.isnan(got[k][~live]).any()), where          # the NaN did go through the launch
