"""Shared inputs of the segment-reduction tests (tests/test_segments_cpu.py, tests/test_gpu_segments.py): superpoint pooling
(``u3d_segment_gather_sum``, csrc/pool.hip seg_gather_sum_k), superpoint centres, mask boxes, the CSR builder and the id gather.

Pooling cases are built around the edges of the kernel, not around a scene: ``SLOTS = 256 / C`` segments share a wave in the
one-group-per-segment decomposition and ``SLOTS`` rows of a segment are in flight in the one-wave-per-segment decomposition, a block
holds ``4 * K`` segments (K = 1 / SLOTS), and the segment lengths sit on both sides of SLOTS, of a wave (64) and of nothing at all
(0, 1).  References are float64 restatements of include/u3d.h; the acceptance bounds are the textbook rounding bounds of the
operation -- none of them comes from a measurement.  Nothing here touches a GPU."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24                                   # unit roundoff of fp32
WIDTHS = (16, 32, 64, 128, 256)                  # the instantiated C of u3d_segment_gather_sum
# mode -> (mean_mode, src_seg_offsets given).  'wave' is the forward call of ops._PoolFn, 'group' its backward call; the two others
# are the combinations the ABI also allows (mean_mode alone picks the decomposition).
MODES = {'wave': (1, False), 'group': (0, True), 'wave_scaled': (1, True), 'group_plain': (0, False)}
VALUES = ('randn', 'exact')
FULL_S = 21                                      # a case that holds every mandatory length whatever the grid edges are
SEG_CHUNK = 2048                                 # csrc/pool.hip u3d_segment_minmax_xyz: segments per LDS pass
SCAN_B = 2048                                    # csrc/misc.hip: items of one scan block


def gamma(k):
    """k u / (1 - k u): the bound of k accumulated fp32 roundings (Higham, Accuracy and Stability of Numerical Algorithms, 3.1)"""
    ku = np.asarray(k, np.float64) * U
    return ku / (1.0 - ku)


def slots(C: int) -> int:
    return 256 // C


def grid_k(C: int, mode: str) -> int:
    """segments per wave: a block of 256 threads serves 4 * grid_k segments"""
    return 1 if MODES[mode][0] else slots(C)


def pool_sizes(C: int, mode: str) -> List[int]:
    """S at the grid edges (one segment, one short of a block, a full block, one over) and FULL_S"""
    K = grid_k(C, mode)
    return sorted({1, 4 * K - 1, 4 * K, 4 * K + 1, FULL_S})


def mandatory_lengths(C: int) -> List[int]:
    SL = slots(C)
    return [0, 0, 1, 2, SL - 1, SL, SL + 1, 2 * SL + 1, 63, 64, 65, 200, 3001]


def _lengths(C: int, S: int, rng) -> np.ndarray:
    """Every mandatory length when S has room for them (shuffled, padded with short random lengths, the last segment empty);
    the first S of them in the order below otherwise."""
    SL = slots(C)
    must = mandatory_lengths(C)
    if S >= len(must):
        body = must[1:] + [int(v) for v in rng.integers(0, 6, S - len(must))]
        rng.shuffle(body)
        return np.asarray(body + [0], np.int64)
    if S == 1:
        return np.asarray([65], np.int64)
    first = [65, 2 * SL + 1, 0, 200, 1, SL + 1, 64, 3001, 2, SL, 63, SL - 1][:S - 1]
    rng.shuffle(first)
    return np.asarray(first + [0], np.int64)


@dataclass
class PoolCase:
    C: int
    mode: str
    values: str
    S: int
    mean_mode: int
    src: torch.Tensor                            # float32 [n_src, C]
    rows: torch.Tensor                           # int32 [sum of lengths]
    offsets: torch.Tensor                        # int32 [S + 1]
    src_seg_offsets: Optional[torch.Tensor]      # int32 [n_src + 1] or None
    counts_match_rows: bool                      # src_seg_offsets counts how often `rows` names each source row ('group')

    @property
    def lengths(self) -> np.ndarray:
        return np.diff(self.offsets.numpy().astype(np.int64))

    @property
    def seg_of_row(self) -> torch.Tensor:
        return torch.repeat_interleave(torch.arange(self.S), torch.from_numpy(self.lengths))

    @property
    def unreferenced(self) -> torch.Tensor:
        m = torch.ones(self.src.shape[0], dtype=torch.bool)
        m[self.rows.long()] = False
        return m


def pool_case(C: int, mode: str, values: str, S: int = FULL_S) -> PoolCase:
    mean_mode, scaled = MODES[mode]
    rng = np.random.default_rng(100_000 * C + 10_000 * list(MODES).index(mode) + 5_000 * VALUES.index(values) + S)
    lens = _lengths(C, S, rng)
    T = int(lens.sum())
    # how often each referenced source row is named: a power of two for 'exact' (its 1 / count scale is then exact)
    mult, rem = [], T
    while rem > 0:
        m = int(rng.choice((1, 2, 4, 8))) if values == 'exact' else int(rng.integers(1, 7))
        while m > rem:
            m = m // 2 if values == 'exact' else rem
        mult.append(m)
        rem -= m
    n_ref = len(mult)
    n_src = n_ref + max(3, n_ref // 5)                                  # the others are never referenced
    ref_ids = np.sort(rng.permutation(n_src)[:n_ref])
    rows = np.repeat(ref_ids, mult)
    rng.shuffle(rows)
    cnt = np.zeros(n_src, np.int64)
    cnt[ref_ids] = mult
    if mode == 'wave_scaled':
        cnt[ref_ids[::4]] = 0                                           # the max(count, 1) clamp of src_scale on rows that are read
    if values == 'exact':
        src = rng.integers(-8, 9, (n_src, C)).astype(F32)
    else:
        src = (rng.standard_normal((n_src, C)) * 2 + 0.5).astype(F32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    sso = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)) if scaled else None
    return PoolCase(C, mode, values, S, mean_mode, torch.from_numpy(src), torch.from_numpy(rows.astype(np.int32)),
                    torch.from_numpy(offsets), sso, mode == 'group')


def _scaled_rows(case: PoolCase) -> torch.Tensor:
    """float64 [len(rows), C]: src_scale(rows[j]) * src[rows[j]]"""
    v = case.src.double()[case.rows.long()]
    if case.src_seg_offsets is not None:
        cnt = torch.diff(case.src_seg_offsets.long()).clamp(min=1).double()
        v = v / cnt[case.rows.long()][:, None]
    return v


def pool_ref(case: PoolCase):
    """(ref, abs_ref) float64 [S, C]: out_scale(s) * sum_j src_scale(rows[j]) * src[rows[j]] as include/u3d.h states it, and the
    same expression over absolute values"""
    v = _scaled_rows(case)
    seg = case.seg_of_row
    ref = torch.zeros(case.S, case.C, dtype=torch.float64).index_add_(0, seg, v)
    abs_ref = torch.zeros(case.S, case.C, dtype=torch.float64).index_add_(0, seg, v.abs())
    if case.mean_mode:
        n = torch.from_numpy(case.lengths).clamp(min=1).double()[:, None]
        ref, abs_ref = ref / n, abs_ref / n
    return ref, abs_ref


def randn_bound(n, abs_ref: torch.Tensor) -> torch.Tensor:
    """gamma(n + 3) * abs_ref: n fp32 additions in any order, the reciprocal, the product of a row with its scale and the product
    with the segment's scale.  n int [S] (rows of the segment)."""
    return torch.from_numpy(gamma(np.asarray(n, np.float64) + 3))[:, None] * abs_ref


def pool_bound(case: PoolCase, ref: torch.Tensor, abs_ref: torch.Tensor) -> torch.Tensor:
    if case.values == 'exact':
        return 3 * U * ref.abs()                  # every sum is exact: only 1.0f / n and the product with it round
    return randn_bound(case.lengths, abs_ref)


def margin(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """worst error / bound over the elements with a non-zero bound; inf when an element with bound 0 is not met exactly"""
    err = (got.double() - ref).abs()
    if bool((err > bound).logical_and(bound == 0).any()) or not bool(torch.isfinite(got).all()):
        return float('inf')
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def rows_outside(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """bool [S]: the segment misses the bound in at least one column"""
    return ((got.double() - ref).abs() > bound).any(1) | ~torch.isfinite(got.double()).all(1)


def empty_rows_are_plus_zero(case: PoolCase, got: torch.Tensor) -> bool:
    e = got[torch.from_numpy(case.lengths == 0)]
    return bool((e == 0).all()) and not bool(torch.signbit(e).any())


def pool_emulate(case: PoolCase) -> torch.Tensor:
    """The kernel's arithmetic in numpy fp32.  One wave per segment (mean_mode 1): SLOTS slot-strided sequential sums, the xor
    butterfly over the slots, the product with 1.0f / n.  One group per segment (mean_mode 0): one sequential sum."""
    src, rows = case.src.numpy(), case.rows.numpy()
    v = src[rows]
    if case.src_seg_offsets is not None:
        cnt = np.maximum(np.diff(case.src_seg_offsets.numpy()), 1).astype(F32)
        v = v * (F32(1) / cnt)[rows][:, None]
    SL = slots(case.C)
    off = case.offsets.numpy()
    out = np.zeros((case.S, case.C), F32)
    for s in range(case.S):
        lo, hi = int(off[s]), int(off[s + 1])
        n = hi - lo
        if n == 0:
            continue
        if case.mean_mode:
            steps = -(-n // SL)
            blk = np.zeros((steps * SL, case.C), F32)
            blk[:n] = v[lo:hi]
            acc = np.cumsum(blk.reshape(steps, SL, case.C), axis=0, dtype=F32)[-1]          # sequential inside every slot
            m = 1
            while m < SL:
                acc = acc + acc[np.arange(SL) ^ m]
                m <<= 1
            out[s] = acc[0] * (F32(1) / F32(n))
        else:
            out[s] = np.cumsum(v[lo:hi], axis=0, dtype=F32)[-1]
    return torch.from_numpy(out)


def mutants(case: PoolCase, ref: torch.Tensor):
    """Three wrong results a kernel could plausibly produce, in float64: (name, wrong [S, C], bool [S] segments it alters)."""
    v = _scaled_rows(case)
    lens = case.lengths
    off = case.offsets.numpy().astype(np.int64)
    scale = torch.ones(case.S, dtype=torch.float64)
    if case.mean_mode:
        scale = 1.0 / torch.from_numpy(lens).clamp(min=1).double()
    # 1. the last row of every segment of two or more rows is dropped
    alt = lens >= 2
    w = ref.clone()
    idx = torch.from_numpy(np.nonzero(alt)[0])
    w[idx] -= scale[idx, None] * v[torch.from_numpy(off[1:][alt] - 1)]
    yield 'last_row_dropped', w, torch.from_numpy(alt)
    # 2. the first row of the next non-empty segment is added in
    nxt = np.full(case.S, -1, np.int64)
    seen = -1
    for s in range(case.S - 1, -1, -1):
        nxt[s] = seen
        if lens[s] > 0:
            seen = s
    alt = nxt >= 0
    w = ref.clone()
    idx = torch.from_numpy(np.nonzero(alt)[0])
    w[idx] += scale[idx, None] * v[torch.from_numpy(off[nxt[alt]])]
    yield 'next_row_added', w, torch.from_numpy(alt)
    # 3. a division by n + 1 where the division by n (or none) belongs
    alt = lens >= 1
    f = torch.from_numpy(np.maximum(lens, 1) / (lens + 1.0))
    yield 'divided_by_n_plus_1', ref * f[:, None], torch.from_numpy(alt)


# ============================================================================================================ mask boxes
MINMAX_SIZES = (1, 2047, 2048, 2049, 4097)


@dataclass
class MinMaxCase:
    n_seg: int
    scenes: List[torch.Tensor]                   # float32 [n_b, 3]: scene 1 of the three is empty
    ids: torch.Tensor                            # int64 [n]: batch-global instance ids, -1 = no instance
    absent: List[int]                            # instances without points

    @property
    def points(self) -> torch.Tensor:
        return torch.cat(self.scenes)

    @property
    def pt_offsets(self) -> torch.Tensor:
        return torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in self.scenes])]), dtype=torch.int64)

    @property
    def stats(self) -> torch.Tensor:
        """float32 [B, 12] like VoxelBatch.stats: the scene's min xyz first; the empty scene's row is NaN (never to be read)"""
        st = torch.full((len(self.scenes), 12), float('nan'))
        for b, s in enumerate(self.scenes):
            if len(s):
                st[b, :3], st[b, 3:6], st[b, 6:] = s.min(0)[0], s.max(0)[0], 0.0
        return st


def minmax_absent(n_seg: int) -> List[int]:
    """one instance without points in the first chunk, one in the last chunk and the last id -- as many as n_seg allows"""
    if n_seg < 16:
        return []
    lo_last = SEG_CHUNK * ((n_seg - 1) // SEG_CHUNK)
    out = {7, lo_last + (n_seg - 1 - lo_last) // 2, n_seg - 1}
    if len(out) < 3:
        out.add(SEG_CHUNK - 1)                   # a last chunk of one id: the last id of the first chunk instead
    return sorted(out)


def _minmax_scene(rng, inst: np.ndarray):
    k = rng.integers(1, 6, len(inst))                                   # about three points per instance
    lab = np.repeat(inst, k)
    lab = np.concatenate([lab, np.full(max(5, len(lab) // 3), -1, np.int64)])       # unlabelled points between them
    rng.shuffle(lab)
    xyz = rng.uniform(-5, 5, (len(lab), 3)).astype(F32)
    n_dup = max(2, len(lab) // 20)
    xyz[rng.integers(0, len(lab), n_dup)] = xyz[rng.integers(0, len(lab), n_dup)]   # a few exact duplicates
    return torch.from_numpy(xyz), lab


def minmax_case(n_seg: int) -> MinMaxCase:
    rng = np.random.default_rng(7000 + n_seg)
    absent = minmax_absent(n_seg)
    h = (n_seg + 1) // 2                                                # scene 0 holds ids [0, h), scene 2 the others
    present = np.setdiff1d(np.arange(n_seg), np.asarray(absent, np.int64))
    p0, l0 = _minmax_scene(rng, present[present < h])
    p2, l2 = _minmax_scene(rng, present[present >= h])
    return MinMaxCase(n_seg, [p0, torch.zeros(0, 3), p2], torch.from_numpy(np.concatenate([l0, l2])), absent)


def minmax_ref(case: MinMaxCase, shifted: bool) -> torch.Tensor:
    """float64 [n_seg, 6] scatter amin / amax of the fp32 (coord - scene min), or of the raw coordinates; instances without points
    keep +inf / -inf here"""
    src = torch.cat([(s - s.min(0)[0]) if (shifted and len(s)) else s for s in case.scenes]).double()
    keep = case.ids >= 0
    sh, ix = src[keep], case.ids[keep][:, None].expand(-1, 3)
    lo = torch.full((case.n_seg, 3), float('inf'), dtype=torch.float64).scatter_reduce(0, ix, sh, 'amin', include_self=False)
    hi = torch.full((case.n_seg, 3), float('-inf'), dtype=torch.float64).scatter_reduce(0, ix, sh, 'amax', include_self=False)
    return torch.cat((lo, hi), 1)


# ============================================================================================================ CSR builder
CSR_S = (1, 2, 3, 1024, 1025, 2047, 2048, 2049)          # around the radix key widths (2^10, 2^11) and S + 1 == SCAN_B
CSR_L = (1, 257, 5000)
CSR_SHAPES = ('uniform', 'all_in_first', 'all_in_last', 'every_other_empty')


def csr_case(L: int, S: int, shape: str) -> torch.Tensor:
    """int64 [L] segment ids in [0, S)"""
    rng = np.random.default_rng(100 * S + 10 * L + CSR_SHAPES.index(shape))
    if shape == 'uniform':
        ids = rng.integers(0, S, L)
    elif shape == 'all_in_first':
        ids = np.zeros(L, np.int64)
    elif shape == 'all_in_last':
        ids = np.full(L, S - 1, np.int64)
    else:
        ids = 2 * rng.integers(0, (S + 1) // 2, L)
    return torch.from_numpy(ids.astype(np.int64))


def csr_ref(seg_ids: torch.Tensor, S: int):
    """offsets int32 [S + 1], list int32 [L]: element ids ascending inside every segment"""
    order = torch.sort(seg_ids, stable=True)[1]
    cnt = torch.bincount(seg_ids, minlength=S)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cnt, 0)])
    return off.to(torch.int32), order.to(torch.int32)


# ============================================================================================================ centres
BLOCK_EDGES = (1, 255, 256, 257)                 # the kernels of this section run 256 threads, one per element / segment


@dataclass
class CentersCase:
    S: int
    points: torch.Tensor                         # float32 [n, pt_ld]; columns past xyz are NaN (never to be read)
    lst: torch.Tensor                            # int32: point ids, grouped by segment
    offsets: torch.Tensor                        # int32 [S + 1]
    sub: torch.Tensor                            # float32 [3, 12]: per-scene shift, the empty first scene's row is NaN
    pt_offsets: torch.Tensor                     # int64 [4]


def centers_case(S: int, pt_ld: int) -> CentersCase:
    rng = np.random.default_rng(9000 + 10 * S + pt_ld)
    lens = [3001] if S == 1 else [3001, 0, 0] + [int(v) for v in rng.integers(1, 7, S - 3)]
    lens = np.asarray(lens, np.int64)
    rng.shuffle(lens)
    scene = rng.integers(1, 3, S)                                       # scene 0 is empty; a segment's points share a scene
    scene[lens == 3001] = 2                                             # the long one in the scene 1000 m out
    need = [0, int(lens[scene == 1].sum()), int(lens[scene == 2].sum())]
    size = [0, need[1] + 10, need[2] + 10]                              # ten points of each scene belong to no segment
    base = np.concatenate([[0], np.cumsum(size)])
    pool = {b: list(base[b] + rng.permutation(size[b])) for b in (1, 2)}
    lst = []
    for s in range(S):
        b = int(scene[s])
        lst += [pool[b].pop() for _ in range(int(lens[s]))]
    n = int(base[-1])
    pts = np.full((n, pt_ld), np.nan, F32)
    pts[:size[1], :3] = rng.uniform(-5, 5, (size[1], 3))
    pts[size[1]:, :3] = rng.uniform(1000, 1004, (size[2], 3))
    sub = np.full((3, 12), np.nan, F32)
    sub[1, :3], sub[2, :3] = pts[:size[1], :3].min(0), pts[size[1]:, :3].min(0)
    sub[1:, 3:] = 0
    return CentersCase(S, torch.from_numpy(pts), torch.tensor(lst, dtype=torch.int32),
                       torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)), torch.from_numpy(sub),
                       torch.from_numpy(base.astype(np.int64)))


def centers_ref(case: CentersCase, with_sub: bool) -> torch.Tensor:
    """float64 [S, 3]: mean of the fp32 differences xyz - sub[scene] (of xyz without sub); 0 for a segment without points"""
    xyz = case.points[:, :3]
    if with_sub:
        scene = torch.bucketize(torch.arange(len(xyz)), case.pt_offsets[1:], right=True)
        xyz = xyz - case.sub[scene, :3]                                 # fp32 subtraction, as the kernel does it
    lens = torch.diff(case.offsets.long())
    seg = torch.repeat_interleave(torch.arange(case.S), lens)
    tot = torch.zeros(case.S, 3, dtype=torch.float64).index_add_(0, seg, xyz.double()[case.lst.long()])
    return tot / lens.clamp(min=1).double()[:, None]


def ulps(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """|got - ref| in units of the fp32 spacing at the larger of the two"""
    g = got.numpy()
    sp = np.maximum(np.spacing(np.abs(g)), np.spacing(np.abs(ref.float().numpy()))).astype(np.float64)
    return (got.double() - ref).abs() / torch.from_numpy(sp)
