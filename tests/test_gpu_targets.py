"""Batched distance targets (csrc/targets.hip, ops.targets_by_distance) on the MI355X against the CPU oracle
(oracle.criterion.get_targets), the vectors recorded from the reference (tests/golden/ref_detector.npz T0..T2) and a numpy
expectation on inputs whose arithmetic is exact.  Nothing here is compared with the code under test."""
import numpy as np
import pytest
import torch

import test_ref_golden_cpu as R
from oracle import criterion as oc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
D, T = R.D, R.T
F32 = np.float32


def _run(pts_list, ctr_list, topk, ld=3):
    """one launch chain for the scenes -> per-scene [G_b, S_b] bool arrays, the packed bytes and the offsets"""
    from unidet3d_amd import ops
    sp_off = np.concatenate(([0], np.cumsum([len(p) for p in pts_list]))).tolist()
    box_off = np.concatenate(([0], np.cumsum([len(c) for c in ctr_list]))).tolist()
    centers = torch.from_numpy(np.concatenate(pts_list).astype(F32).reshape(-1, 3)).to(DEV)
    rows = np.zeros((box_off[-1], ld), F32)
    rows[:, :3] = np.concatenate(ctr_list).reshape(-1, 3)
    rows[:, 3:] = 77.0                                                     # wider rows (cached gt_rows): the rest must not be read as centres
    boxes = torch.from_numpy(rows).to(DEV)
    packed, mask_off = ops.targets_by_distance(centers, sp_off, boxes[:, :3] if ld > 3 else boxes, box_off, topk)
    assert packed.dtype == torch.bool and packed.shape == (mask_off[-1],) and len(mask_off) == len(pts_list) + 1
    host = packed.cpu().numpy()
    out = [host[mask_off[b]:mask_off[b + 1]].reshape(len(ctr_list[b]), len(pts_list[b])) for b in range(len(pts_list))]
    return out, host, mask_off


def _numpy_targets(pts, ctr, topk):
    """strict `<` against the k-th smallest distance, stable argmin over the boxes; float32 in the kernel's order"""
    p, c = pts.astype(F32), ctr.astype(F32)
    if len(c) == 0:
        return np.zeros((0, len(p)), bool)
    dx, dy, dz = (c[None, :, k] - p[:, None, k] for k in range(3))
    d = (dx * dx + dy * dy) + dz * dz                                      # [S, G] float32
    assert d.dtype == F32
    kth = np.sort(d, axis=0)[min(topk + 1, len(p)) - 1]
    cand = d < kth[None]
    best = np.argmin(np.where(cand, d, np.inf), axis=1)                     # first minimum: the lowest box index
    out = np.zeros((len(c), len(p)), bool)
    has = cand.any(1)
    out[best[has], np.nonzero(has)[0]] = True
    return out


@pytest.fixture(scope='module')
def golden():
    """the reference fixtures with the oracle's answer on the CPU, computed once"""
    cases = []
    for tag in ('T0', 'T1', 'T2'):
        pts, ctr, topk = D[f'{tag}.pts'], D[f'{tag}.centers'], int(D[f'{tag}.topk'])
        want = oc.get_targets(T(pts), T(ctr), topk).numpy()
        assert np.array_equal(want, D[f'{tag}.targets'])
        cases.append((pts, ctr, topk, want))
    assert len({c[2] for c in cases}) == 1
    return cases


@pytest.mark.parametrize('which', [0, 1, 2])
def test_reference_fixture_alone(golden, which):
    pts, ctr, topk, want = golden[which]
    got, _, _ = _run([pts], [ctr], topk)
    assert got[0].shape == want.shape and np.array_equal(got[0], want)


def test_reference_fixtures_as_one_batch(golden):
    got, _, mask_off = _run([c[0] for c in golden], [c[1] for c in golden], golden[0][2], ld=7)
    assert mask_off == np.concatenate(([0], np.cumsum([c[3].size for c in golden]))).tolist()
    for g, c in zip(got, golden):
        assert np.array_equal(g, c[3])


def _lattice(rng, n):
    return (rng.randint(0, 512, (n, 3)) / 64.0).astype(F32)               # multiples of 2^-6 in [0, 8): squares and sums are exact


@pytest.fixture(scope='module')
def synthetic():
    """Six scenes: fewer superpoints than topk + 1, exactly topk + 1 (topk 6), one more, a wave boundary, many waves; a box count
    above one LDS tile of 64; a scene without boxes.  Exact arithmetic makes the planted ties real ties."""
    rng = np.random.RandomState(2024)
    S, G = [1, 5, 7, 8, 65, 1500], [2, 1, 3, 65, 0, 12]
    pts = [_lattice(rng, s) for s in S]
    ctr = [_lattice(rng, g) for g in G]
    # scene 3 (8 superpoints, 65 boxes): box 0 sees distances 0, 1, 1, 4, 4, 9, 12.25, 12.25 -- the 7th and 8th smallest are equal
    # (topk 6), so are the 4th and 5th (topk 3), and equal values sit in different lanes
    pts[3] = np.array([[1, 1, 1], [2, 1, 1], [3, 1, 1], [4, 1, 1], [5, 1, 1], [6, 1, 1], [0.5, 1, 1], [7.5, 1, 1]], F32)
    ctr[3][0] = [4, 1, 1]
    ctr[3][64] = ctr[3][0]                                                 # a duplicate across the tile boundary
    # scene 5: duplicated centres; boxes 2 / 3 with superpoints on their bisecting plane
    ctr[5][1] = ctr[5][0]
    ctr[5][2], ctr[5][3] = [2, 2, 2], [2.25, 2, 2]
    pts[5][:8] = [[2.125, 2 + a / 64, 2 + b / 64] for a, b in ((0, 0), (1, 0), (0, -1), (2, 1), (-2, 2), (3, 3), (-3, 0), (1, -4))]
    pts[5][8:12] = ctr[5][4]                                               # four superpoints ON a centre: distance 0 four times
    # scene 2 (exactly topk + 1 = 7 superpoints): two boxes share a centre
    ctr[2][2] = ctr[2][0]
    want = {k: [_numpy_targets(p, c, k) for p, c in zip(pts, ctr)] for k in (6, 3)}
    for k in (6, 3):                                                        # the oracle agrees with the numpy expectation on the CPU
        for p, c, w in zip(pts, ctr, want[k]):
            if len(c):
                assert np.array_equal(oc.get_targets(T(p), T(c), k).numpy(), w)
    d = ((ctr[3][0][None] - pts[3]) ** 2).sum(1)
    assert np.sort(d)[6] == np.sort(d)[7] and np.sort(d)[3] == np.sort(d)[4]
    d2, d3 = ((ctr[5][2][None] - pts[5][:8]) ** 2).sum(1), ((ctr[5][3][None] - pts[5][:8]) ** 2).sum(1)
    assert np.array_equal(d2, d3)                                           # equidistant from two boxes
    assert want[6][5][2, :8].any() and not want[6][5][3, :8].any()          # ... and the lower index takes them
    assert not want[6][5][1].any() and want[6][5][0].any()                  # the duplicate never wins
    assert want[6][0].sum() == 0 and want[6][1].sum() == 4                  # 1 superpoint: nothing is strictly below the k-th; 5: all but the farthest
    return pts, ctr, want


@pytest.mark.parametrize('topk', [6, 3])
def test_synthetic_batch_in_one_launch(synthetic, topk):
    pts, ctr, want = synthetic
    got, raw, mask_off = _run(pts, ctr, topk)
    assert mask_off[5] == mask_off[4]                                       # the scene without boxes owns an empty block
    for b, (g, w) in enumerate(zip(got, want[topk])):
        assert g.shape == w.shape and np.array_equal(g, w), (b, int((g != w).sum()))
        assert (g.sum(0) <= 1).all()                                        # a superpoint belongs to at most one box
    _, again, _ = _run(pts, ctr, topk)
    assert raw.tobytes() == again.tobytes()                                 # same inputs, same bytes


def test_wave_boundary_with_boxes_and_wide_rows():
    """65 and 64 superpoints WITH boxes (the six-scene batch above pairs 65 with the scene without boxes), centres read in place from 7-float rows"""
    rng = np.random.RandomState(5)
    pts = [_lattice(rng, 65), _lattice(rng, 64), _lattice(rng, 257)]
    ctr = [_lattice(rng, 3), _lattice(rng, 2), _lattice(rng, 64)]
    got, _, _ = _run(pts, ctr, 6, ld=7)
    for p, c, g in zip(pts, ctr, got):
        assert np.array_equal(g, _numpy_targets(p, c, 6)) and np.array_equal(g, oc.get_targets(T(p), T(c), 6).numpy())


def test_topk_beyond_the_register_list_is_refused():
    from unidet3d_amd import _lib, ops
    c = torch.zeros(20, 3, device=DEV)
    with pytest.raises(_lib.U3DError, match='topk'):
        ops.targets_by_distance(c, [0, 20], torch.zeros(2, 3, device=DEV), [0, 2], 16)
    packed, off = ops.targets_by_distance(c, [0, 20], torch.zeros(0, 3, device=DEV), [0, 0], 6)      # no boxes at all: nothing to launch
    assert packed.numel() == 0 and off == [0, 0]
