"""The conditions the segment-reduction tests (tests/test_gpu_segments.py) rely on, checked on the host: the references of
tests/_segments.py equal the oracle's scatter_mean and its autograd, an fp32 emulation of the kernel's summation orders sits inside
the derived bounds, the bounds reject a dropped row, a row of the neighbouring segment and a wrong divisor, and the case builders
keep the lengths, repeats and grid edges they promise."""
import numpy as np
import pytest
import torch

import _segments as SG
from oracle import sparse_ops as so

POOL_KEYS = [(C, mode, values, S) for C in SG.WIDTHS for mode in SG.MODES for values in SG.VALUES for S in SG.pool_sizes(C, mode)]
_POOL = {}


def pool(key):
    """(case, ref, abs_ref), built once"""
    if key not in _POOL:
        case = SG.pool_case(*key)
        _POOL[key] = (case,) + SG.pool_ref(case)
    return _POOL[key]


def _by_width(C):
    return [k for k in POOL_KEYS if k[0] == C]


# ============================================================================================================ the builders
@pytest.mark.parametrize('C', SG.WIDTHS)
def test_pool_cases_keep_their_properties(C):
    SL = SG.slots(C)
    assert SL * C == 256
    for mode in SG.MODES:
        K = 1 if mode.startswith('wave') else SL
        assert SG.pool_sizes(C, mode) == sorted({1, 4 * K - 1, 4 * K, 4 * K + 1, SG.FULL_S})
    for key in _by_width(C):
        case, _, _ = pool(key)
        _, mode, values, S = key
        lens = case.lengths
        off, rows = case.offsets.numpy(), case.rows.numpy()
        n_src = case.src.shape[0]
        assert case.S == S == len(lens) and off[0] == 0 and off[-1] == len(rows) and (lens >= 0).all(), key
        assert case.src.dtype == torch.float32 and case.rows.dtype == case.offsets.dtype == torch.int32, key
        assert case.mean_mode == (1 if mode.startswith('wave') else 0), key
        assert (case.src_seg_offsets is not None) == (mode in ('group', 'wave_scaled')), key
        if S >= 13:                                                      # room for every mandatory length
            have = sorted(lens.tolist())
            for want in set(SG.mandatory_lengths(C)):
                assert have.count(want) >= SG.mandatory_lengths(C).count(want), (key, want)
            assert (lens == 0).sum() >= 2 and (lens == 3001).sum() == 1, key
            assert not (lens[:-1] == np.sort(lens[:-1])).all(), key     # shuffled
        if S >= 2:
            assert lens[-1] == 0, key                                    # the last segment is empty
        assert rows.min() >= 0 and rows.max() < n_src, key
        assert bool(case.unreferenced.any()), key                        # some source rows are never read
        segs = [rows[off[s]:off[s + 1]] for s in range(S)]
        assert any(len(np.unique(r)) < len(r) for r in segs), key        # a row repeats inside a segment
        assert any(len(r) >= 2 and (np.diff(r) < 0).any() for r in segs), key        # rows are not sorted
        if values == 'exact':
            assert torch.equal(case.src, case.src.round()) and float(case.src.abs().max()) <= 8, key
        if case.src_seg_offsets is not None:
            sso = case.src_seg_offsets.numpy()
            cnt = np.diff(sso)
            assert len(sso) == n_src + 1 and sso[0] == 0 and (cnt >= 0).all(), key
            if values == 'exact':
                assert all(c == 0 or c & (c - 1) == 0 for c in cnt.tolist()), key     # every scale count a power of two
            if case.counts_match_rows:
                assert np.array_equal(cnt, np.bincount(rows, minlength=n_src)), key
            if mode == 'wave_scaled':
                assert (cnt[rows] == 0).any(), key                       # the clamp of src_scale is exercised


def test_minmax_cases_keep_their_properties():
    for n_seg in SG.MINMAX_SIZES:
        case = SG.minmax_case(n_seg)
        ids = case.ids.numpy()
        assert [len(s) for s in case.scenes][1] == 0 and len(case.scenes) == 3 and len(case.scenes[0]) and len(case.scenes[2])
        assert len(ids) == len(case.points) and ids.min() == -1 and ids.max() < n_seg
        present = np.unique(ids[ids >= 0])
        assert sorted(set(range(n_seg)) - set(present.tolist())) == case.absent
        n0 = len(case.scenes[0])
        if n_seg > 1:
            assert len(case.absent) == 3 and case.absent[0] < SG.SEG_CHUNK and case.absent[-1] == n_seg - 1
            lo_last = SG.SEG_CHUNK * ((n_seg - 1) // SG.SEG_CHUNK)
            assert any(a >= lo_last for a in case.absent)
            assert 2.5 < (ids >= 0).sum() / len(present) < 3.5           # about three points per instance
            assert ids[:n0].max() < ids[n0:][ids[n0:] >= 0].min()        # batch-global: the second scene continues the numbering
        pts = case.points.numpy()
        assert np.abs(pts).max() <= 5 and len(np.unique(pts, axis=0)) < len(pts)     # exact duplicates
        inter = (ids[:-1] >= 0) != (ids[1:] >= 0)
        assert inter.sum() >= min(4, len(ids) // 4)                      # -1 interleaved with the instances
        st = case.stats
        assert torch.isnan(st[1]).all() and torch.equal(st[0, :3], case.scenes[0].min(0)[0]) and torch.equal(st[2, :3], case.scenes[2].min(0)[0])
        assert case.pt_offsets.tolist() == [0, n0, n0, len(pts)]
    assert [len(SG.minmax_absent(n)) for n in SG.MINMAX_SIZES] == [0, 3, 3, 3, 3]
    assert SG.minmax_absent(2049) == [7, 2047, 2048] and SG.minmax_absent(2047) == [7, 1023, 2046]


def test_minmax_ref_on_a_hand_made_scene():
    case = SG.MinMaxCase(3, [torch.tensor([[1.0, 2.0, 3.0], [0.0, 5.0, -1.0], [4.0, 4.0, 4.0]]), torch.zeros(0, 3),
                             torch.tensor([[10.0, 10.0, 10.0], [11.0, 9.0, 10.0]])], torch.tensor([0, 0, -1, 2, 2]), [1])
    raw = SG.minmax_ref(case, False)
    assert raw[0].tolist() == [0, 2, -1, 1, 5, 3] and raw[2].tolist() == [10, 9, 10, 11, 10, 10]
    assert raw[1].tolist() == [float('inf')] * 3 + [float('-inf')] * 3
    sh = SG.minmax_ref(case, True)                                       # scene minima (0, 2, -1) and (10, 9, 10)
    assert sh[0].tolist() == [0, 0, 0, 1, 3, 4] and sh[2].tolist() == [0, 0, 0, 1, 1, 0]


@pytest.mark.parametrize('shape', SG.CSR_SHAPES)
def test_csr_cases_and_reference(shape):
    for S in SG.CSR_S:
        for L in SG.CSR_L:
            ids = SG.csr_case(L, S, shape)
            assert ids.dtype == torch.int64 and ids.shape == (L,) and int(ids.min()) >= 0 and int(ids.max()) < S
            if shape == 'all_in_first':
                assert int(ids.max()) == 0
            elif shape == 'all_in_last':
                assert int(ids.min()) == S - 1
            elif shape == 'every_other_empty':
                assert bool((ids % 2 == 0).all())
            off, lst = SG.csr_ref(ids, S)
            assert off.dtype == lst.dtype == torch.int32 and off.shape == (S + 1,) and int(off[0]) == 0 and int(off[-1]) == L
            o, l, s = off.tolist(), lst.tolist(), ids.tolist()
            assert sorted(l) == list(range(L))
            for k in {0, S // 2, S - 1}:                                 # a plain restatement on a few segments
                assert l[o[k]:o[k + 1]] == [i for i in range(L) if s[i] == k]
    assert 1 + max(SG.CSR_S) > SG.SCAN_B and SG.SCAN_B - 1 in SG.CSR_S and SG.SCAN_B in SG.CSR_S      # both sides of the scan's switch
    assert {1024, 1025, 2048, 2049} <= set(SG.CSR_S)                                                 # both sides of two key widths


@pytest.mark.parametrize('pt_ld', [3, 6])
def test_centers_cases_keep_their_properties(pt_ld):
    for S in SG.BLOCK_EDGES:
        case = SG.centers_case(S, pt_ld)
        lens = torch.diff(case.offsets.long())
        assert case.points.shape[1] == pt_ld and int((lens == 3001).sum()) == 1 and len(lens) == S
        assert S == 1 or int((lens == 0).sum()) >= 2
        assert not torch.isnan(case.points[:, :3]).any() and (pt_ld == 3 or torch.isnan(case.points[:, 3:]).all())
        po = case.pt_offsets.tolist()
        assert po[0] == po[1] == 0 and po[3] == len(case.points) and torch.isnan(case.sub[0]).all()      # the first scene is empty
        lst = case.lst.long()
        assert len(torch.unique(lst)) == len(lst) == int(lens.sum()) < len(case.points)
        seg = torch.repeat_interleave(torch.arange(S), lens)
        scene = (lst >= po[2]).long()
        for s in range(S):                                               # the points of a segment share a scene
            assert len(torch.unique(scene[seg == s])) <= 1
        assert S == 1 or len(torch.unique(scene)) == 2
        ref = SG.centers_ref(case, True)
        assert bool((ref[lens == 0] == 0).all()) and bool((ref >= 0).all()) and float(ref.max()) <= 10
        raw = SG.centers_ref(case, False)
        assert bool((raw[lens == 0] == 0).all()) and float(raw.abs().max()) > 1000


# ============================================================================================================ the references
@pytest.mark.parametrize('C', SG.WIDTHS)
def test_pool_ref_is_scatter_mean_forward_and_its_gradient_backward(C):
    for key in _by_width(C):
        case, ref, abs_ref = pool(key)
        if case.mode == 'wave':
            want = so.scatter_mean(case.src.double()[case.rows.long()], case.seg_of_row, case.S)
            assert torch.equal(ref, want), key
            assert torch.equal(abs_ref, so.scatter_mean(case.src.double().abs()[case.rows.long()], case.seg_of_row, case.S)), key
        elif case.mode == 'group':
            # segments are voxels, `rows` names the superpoint of each of their points, src is the gradient of the pooled tensor
            f = torch.zeros(case.S, C, dtype=torch.float64, requires_grad=True)
            pooled = so.scatter_mean(f[case.seg_of_row], case.rows.long(), case.src.shape[0])
            pooled.backward(case.src.double())
            assert float((f.grad - ref).abs().max()) <= 1e-13 * float(abs_ref.max()), key
        assert bool((abs_ref >= ref.abs()).all()), key
        assert bool((ref[torch.from_numpy(case.lengths == 0)] == 0).all()), key


# ============================================================================================================ the bounds
@pytest.mark.parametrize('C', SG.WIDTHS)
def test_fp32_emulation_of_the_kernel_orders_is_inside_the_bounds(C):
    worst = {}
    for key in _by_width(C):
        case, ref, abs_ref = pool(key)
        got = SG.pool_emulate(case)
        m = SG.margin(got, ref, SG.pool_bound(case, ref, abs_ref))
        assert m <= 1.0, (key, m)
        assert SG.empty_rows_are_plus_zero(case, got), key
        worst[key[1], key[2]] = max(worst.get((key[1], key[2]), 0.0), m)
    print(C, worst)


@pytest.mark.parametrize('C', SG.WIDTHS)
def test_every_mutant_is_rejected(C):
    for key in _by_width(C):
        case, ref, abs_ref = pool(key)
        bound = SG.pool_bound(case, ref, abs_ref)
        lens = torch.from_numpy(case.lengths)
        for name, wrong, altered in SG.mutants(case, ref):
            if not bool(altered.any()):
                continue
            assert not torch.equal(wrong, ref), (key, name)
            caught = SG.rows_outside(wrong, ref, bound)
            must = altered if case.values == 'exact' else altered & (lens <= 200)       # the 3001-row segment: the exact cases
            assert bool(caught[must].all()), (key, name, torch.nonzero(must & ~caught).flatten().tolist())
            assert not bool(caught[~altered].any()), (key, name)


def test_gamma_and_ulps():
    assert SG.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and SG.gamma(3004) == pytest.approx(3004 * 2.0 ** -24, rel=1e-3)
    one = torch.tensor([1.0])
    assert float(SG.ulps(one, torch.tensor([1.0 + 2.0 ** -23], dtype=torch.float64))[0]) == 1.0
    assert float(SG.ulps(torch.zeros(1), torch.zeros(1, dtype=torch.float64))[0]) == 0.0
