"""Segment reductions between the backbone and the decoder (csrc/pool.hip, the scan of csrc/misc.hip underneath) at every
instantiated width, both decompositions, the grid edges and the chunk edges: superpoint pooling through the C ABI and through
autograd, mask boxes across LDS chunks, the CSR builder around the scan's and the radix key's switches, the id gather and the
superpoint centres at block edges.

Inputs, float64 references and acceptance bounds come from tests/_segments.py (checked on the host by tests/test_segments_cpu.py):
rounding bounds of the operation for random values, 3 u for the integer-valued cases whose sums are exact, equality for everything
that is integer or min / max.  No id outside its range is passed anywhere: that is a precondition of these entry points."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _segments as SG
from _parity import log_errors
from oracle import sparse_ops as so

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = -12345.0
N_GUARD = 8


def _d(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ============================================================================================================ 1. pooling, C ABI
def _gather_sum(case):
    """-> (out [S, C], guard rows [N_GUARD, C]) on the CPU; source rows no segment names are NaN"""
    from unidet3d_amd import _lib as L
    src = case.src.clone()
    src[case.unreferenced] = float('nan')
    src_d, rows_d, off_d, sso_d = _d(src), _d(case.rows), _d(case.offsets), _d(case.src_seg_offsets)
    out = torch.full((case.S + N_GUARD, case.C), GUARD, device=DEV)
    L.call('u3d_segment_gather_sum', L.ptr(src_d), L.ptr(rows_d), L.ptr(off_d), case.S, case.C, case.mean_mode, L.ptr(sso_d),
           L.ptr(out), L.stream())
    out = out.cpu()
    return out[:case.S], out[case.S:]


@pytest.mark.parametrize('mode', list(SG.MODES))
@pytest.mark.parametrize('C', SG.WIDTHS)
def test_segment_gather_sum_every_width_mode_and_grid_edge(C, mode):
    worst = {v: 0.0 for v in SG.VALUES}
    exact_u = 0.0
    for values in SG.VALUES:
        for S in SG.pool_sizes(C, mode):
            case = SG.pool_case(C, mode, values, S)
            ref, abs_ref = SG.pool_ref(case)
            bound = SG.pool_bound(case, ref, abs_ref)
            got, guard = _gather_sum(case)
            what = (C, mode, values, S)
            assert bool((guard == GUARD).all()), what                    # nothing written past row S
            assert bool(torch.isfinite(got).all()), what                 # lanes past `hi` read nothing
            m = SG.margin(got, ref, bound)
            worst[values] = max(worst[values], m)
            if values == 'exact':
                nz = ref != 0
                exact_u = max(exact_u, float(((got.double() - ref).abs()[nz] / (SG.U * ref.abs()[nz])).max()))
            print('segment_gather_sum', what, 'worst error / bound', m)
            assert m <= 1.0, (what, m, torch.nonzero(SG.rows_outside(got, ref, bound)).flatten().tolist(), case.lengths.tolist())
            assert SG.empty_rows_are_plus_zero(case, got), what
            again, _ = _gather_sum(case)
            assert torch.equal(_bits(again), _bits(got)), what           # one summation order, run after run
    log_errors('segments_gather_sum', dict(C=C, mode=mode, worst_error_over_bound=worst, exact_error_in_u=exact_u))


# ============================================================================================================ 2. refused arguments
@pytest.mark.parametrize('C', [8, 48, 512])
def test_segment_gather_sum_refuses_widths_it_has_no_kernel_for(C):
    from unidet3d_amd import _lib as L
    src = torch.ones(4, C, device=DEV)
    rows = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=DEV)
    off = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    for mean_mode in (0, 1):
        out = torch.full((2 + N_GUARD, C), GUARD, device=DEV)
        with pytest.raises(L.U3DError, match=f'C={C} unsupported'):
            L.call('u3d_segment_gather_sum', L.ptr(src), L.ptr(rows), L.ptr(off), 2, C, mean_mode, None, L.ptr(out), L.stream())
        assert bool((out == GUARD).all())


def test_segment_gather_sum_refuses_zero_segments():
    from unidet3d_amd import _lib as L
    src = torch.ones(4, 32, device=DEV)
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    off = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.full((N_GUARD, 32), GUARD, device=DEV)
    for mean_mode in (0, 1):
        rc = L.lib().u3d_segment_gather_sum(L.ptr(src), L.ptr(rows), L.ptr(off), 0, 32, mean_mode, None, L.ptr(out), L.stream())
        assert rc == -1                                                  # U3D_EINVAL
    assert bool((out == GUARD).all())


# ============================================================================================================ 3. pooling, autograd
_SCENE = {}


def _pool_scene():
    """Three scenes (the middle one empty) voxelised at 0.05, superpoint ids with gaps, a superpoint of one point and one that covers
    a third of its scene; the PoolPlan and the host copies the references need."""
    if _SCENE:
        return _SCENE
    from unidet3d_amd import ops
    rng = np.random.default_rng(77)
    pts, sps, per_scene = [], [], 90
    for b, n in enumerate((1500, 0, 1400)):
        p = np.concatenate([rng.uniform(0, 0.5, (n, 3)) + 3.0 * b, rng.uniform(0, 1, (n, 3))], 1).astype(np.float32)
        sp = 2 * rng.integers(1, 40, n)                                  # even ids 2 .. 78: every odd id is an empty superpoint
        if n:
            sp[:n // 3] = 0                                              # a third of the scene
            sp[n // 2] = 81                                              # a single point
        pts.append(torch.from_numpy(p))
        sps.append(torch.from_numpy(sp.astype(np.int64)) + per_scene * b)
    sp = torch.cat(sps)
    S = per_scene * 3
    vb = ops.voxelize([p.to(DEV) for p in pts], 0.05, 16)
    plan = ops.PoolPlan(vb, sp.to(DEV), S)
    inv = vb.inverse.cpu()
    n_vox = int(vb.coords.shape[0])
    cnt_sp, cnt_vox = torch.bincount(sp, minlength=S), torch.bincount(inv, minlength=n_vox)
    assert int(cnt_sp[81]) == 1 and int(cnt_sp[0]) == 500 and int((cnt_sp == 0).sum()) > S // 2 and int(cnt_sp[per_scene:2 * per_scene].sum()) == 0
    assert int(cnt_vox.min()) >= 1 and int(cnt_vox.max()) >= 4 and n_vox < len(sp)       # several points of one voxel
    _SCENE.update(plan=plan, sp=sp, S=S, inv=inv, n_vox=n_vox, cnt_sp=cnt_sp, cnt_vox=cnt_vox)
    return _SCENE


@pytest.mark.parametrize('C', [16, 64, 128, 256])
def test_superpoint_pool_forward_and_gradient_at_every_other_width(C):
    from unidet3d_amd import ops
    sc = _pool_scene()
    sp, S, inv, n_vox = sc['sp'], sc['S'], sc['inv'], sc['n_vox']
    g = torch.Generator().manual_seed(C)
    f = torch.randn(n_vox, C, generator=g) * 2 + 0.5
    go = torch.randn(S, C, generator=g) * 2 + 0.5
    f64 = f.double().requires_grad_()
    ref = so.scatter_mean(f64[inv], sp, S)
    ref.backward(go.double())
    abs_ref = so.scatter_mean(f.double().abs()[inv], sp, S)
    w = (go.double().abs() / sc['cnt_sp'].clamp(min=1).double()[:, None])[sp]             # |gradient| each point hands to its voxel
    abs_grad = torch.zeros(n_vox, C, dtype=torch.float64).index_add_(0, inv, w)
    runs = []
    for _ in range(2):
        fg = f.to(DEV).requires_grad_()
        pg = ops.superpoint_pool(fg, sc['plan'])
        pg.backward(go.to(DEV))
        runs.append((pg.detach().cpu(), fg.grad.cpu()))
    got, grad = runs[0]
    m_f = SG.margin(got, ref.detach(), SG.randn_bound(sc['cnt_sp'].numpy(), abs_ref))
    m_b = SG.margin(grad, f64.grad, SG.randn_bound(sc['cnt_vox'].numpy(), abs_grad))     # n_s = points of the voxel
    print('superpoint_pool', C, 'worst error / bound: forward', m_f, 'gradient', m_b)
    log_errors('segments_superpoint_pool', dict(C=C, forward_error_over_bound=m_f, gradient_error_over_bound=m_b))
    assert m_f <= 1.0 and m_b <= 1.0, (C, m_f, m_b)
    assert bool((got[sc['cnt_sp'] == 0] == 0).all())
    assert torch.equal(_bits(runs[1][0]), _bits(got)) and torch.equal(_bits(runs[1][1]), _bits(grad))


# ============================================================================================================ 4. dtype guard
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float64])
def test_superpoint_pool_refuses_tensors_that_are_not_fp32(dtype):
    from unidet3d_amd import _lib as L, ops
    sc = _pool_scene()
    name = str(dtype).replace('torch.', '')
    f = torch.ones(sc['n_vox'], 32, device=DEV, dtype=dtype)
    with pytest.raises(L.U3DError, match=name):
        ops.superpoint_pool(f, sc['plan'])
    dout = torch.ones(sc['S'], 32, device=DEV, dtype=dtype)
    with pytest.raises(L.U3DError, match=name):
        ops._PoolFn.backward(SimpleNamespace(plan=sc['plan']), dout)


# ============================================================================================================ 5. mask boxes
def _minmax_gpu(case, with_sub):
    from unidet3d_amd import _lib as L
    pts, ids = _d(case.points), _d(case.ids)
    n_seg = case.n_seg
    out = torch.full((n_seg + N_GUARD, 6), GUARD, device=DEV)
    ws = torch.empty(n_seg * 24 + 64, dtype=torch.uint8, device=DEV)
    st, po = (_d(case.stats), _d(case.pt_offsets)) if with_sub else (None, None)
    L.call('u3d_segment_minmax_xyz', L.ptr(pts), 3, L.ptr(ids), pts.shape[0], n_seg, L.ptr(st), 12, L.ptr(po), 3 if with_sub else 0,
           L.ptr(out), L.ptr(ws), L.stream())
    out = out.cpu()
    assert bool((out[n_seg:] == GUARD).all())
    return out[:n_seg]


def _check_absent(case, got):
    absent = torch.zeros(case.n_seg, dtype=torch.bool)
    absent[case.absent] = True
    assert torch.equal(torch.isnan(got).any(1), absent)                  # NaN on exactly the instances without points ...
    assert bool(torch.isnan(got[absent]).all())                          # ... in all six components
    if case.absent:
        b = _bits(got[absent])
        assert bool((b == b[0]).all())                                   # the same thing whichever chunk holds them
    return absent


@pytest.mark.parametrize('n_seg', SG.MINMAX_SIZES)
def test_instance_minmax_and_boxes_across_segment_chunks(n_seg):
    from unidet3d_amd import ops
    case = SG.minmax_case(n_seg)
    for with_sub in (True, False):
        ref = SG.minmax_ref(case, with_sub)
        got = _minmax_gpu(case, with_sub)
        absent = _check_absent(case, got)
        assert bool(torch.isfinite(ref[~absent]).all()) and not bool(torch.isfinite(ref[absent]).any())
        assert np.array_equal(got[~absent].double().numpy(), ref[~absent].numpy()), (n_seg, with_sub)   # exact; signed zeros by value
    vb = ops.VoxelBatch(coords=None, feats=None, inverse=None, spatial_shape=[], index=None, vox_offsets=None, vox_points=None,
                        pt_offsets=_d(case.pt_offsets), stats=_d(case.stats), points=_d(case.points))
    boxes = ops.instance_boxes(vb, _d(case.ids), n_seg).cpu()
    absent = _check_absent(case, boxes)
    r32 = SG.minmax_ref(case, True).float()
    lo, hi = r32[:, :3], r32[:, 3:]
    want = torch.cat(((hi + lo) / 2, hi - lo), 1)
    assert np.array_equal(boxes[~absent].numpy(), want[~absent].numpy())


# ============================================================================================================ 6. CSR builder
@pytest.mark.parametrize('S', SG.CSR_S)
def test_csr_build_around_scan_and_key_width_switches(S):
    from unidet3d_amd import ops
    for L_ in SG.CSR_L:
        for shape in SG.CSR_SHAPES:
            ids = SG.csr_case(L_, S, shape)
            want_off, want_lst = SG.csr_ref(ids, S)
            ids_d = ids.to(DEV)
            off, lst = ops.csr_build(ids_d, S)
            what = (L_, S, shape)
            assert off.dtype == lst.dtype == torch.int32 and off.shape == (S + 1,) and lst.shape == (L_,), what
            assert torch.equal(off.cpu(), want_off), what
            assert torch.equal(lst.cpu(), want_lst), what                # ascending inside every segment: the stable order
            off2, lst2 = ops.csr_build(ids_d, S)
            assert torch.equal(off2, off) and torch.equal(lst2, lst), what
            assert torch.equal(ids_d.cpu(), ids), what                   # the input is left as it was


# ============================================================================================================ 7. gather, centres
@pytest.mark.parametrize('L_', SG.BLOCK_EDGES)
def test_gather_i64_to_i32_at_block_edges(L_):
    from unidet3d_amd import _lib as L
    rng = np.random.default_rng(L_)
    M = 300
    mp = torch.from_numpy(rng.integers(-1, 2 ** 31 - 1, M).astype(np.int64))
    mp[0], mp[1] = -1, 2 ** 31 - 1
    lst = torch.from_numpy(rng.integers(0, M, L_).astype(np.int32))
    lst[0] = 1
    lst[-1] = 0
    out = torch.full((L_ + N_GUARD,), -7, dtype=torch.int32, device=DEV)
    mp_d, lst_d = mp.to(DEV), lst.to(DEV)
    L.call('u3d_gather_i64_to_i32', L.ptr(mp_d), L.ptr(lst_d), L_, L.ptr(out), L.stream())
    out = out.cpu()
    assert torch.equal(out[:L_].long(), mp[lst.long()]) and bool((out[L_:] == -7).all())
    assert torch.equal(mp_d.cpu(), mp) and torch.equal(lst_d.cpu(), lst)


@pytest.mark.parametrize('pt_ld', [3, 6])
@pytest.mark.parametrize('S', SG.BLOCK_EDGES)
def test_segment_mean_xyz_at_block_edges(S, pt_ld):
    """The kernel takes the fp32 difference xyz - sub[scene] and accumulates it in fp64: against the fp64 mean of the same fp32
    differences only the final rounding to fp32 remains -- one ulp."""
    from unidet3d_amd import _lib as L
    case = SG.centers_case(S, pt_ld)
    pts, lst, off, sub, po = _d(case.points), _d(case.lst), _d(case.offsets), _d(case.sub), _d(case.pt_offsets)
    empty = torch.diff(case.offsets.long()) == 0
    for with_sub in (False, True):
        out = torch.full((S + N_GUARD, 3), GUARD, device=DEV)
        L.call('u3d_segment_mean_xyz', L.ptr(pts), pt_ld, L.ptr(lst), L.ptr(off), S, L.ptr(sub) if with_sub else None, 12,
               L.ptr(po) if with_sub else None, 3 if with_sub else 0, L.ptr(out), L.stream())
        out = out.cpu()
        got = out[:S]
        assert bool((out[S:] == GUARD).all()), (S, pt_ld, with_sub)
        assert bool(torch.isfinite(got).all()) and bool((got[empty] == 0).all()), (S, pt_ld, with_sub)
        ref = SG.centers_ref(case, with_sub)
        worst = float(SG.ulps(got, ref).max())
        print('segment_mean_xyz', S, pt_ld, with_sub, 'ulps', worst)
        assert worst <= 1.0, (S, pt_ld, with_sub, worst)
