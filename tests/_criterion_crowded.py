"""Crowded scenes for the fused criterion (unidet3d_amd/csrc/criterion.hip): more than 64 ground-truth boxes in a scene, so the
matched set of a (layer, query) spans several 64-bit words and the cost matrix is computed by the pair-parallel kernel.  Case
builders only (plain CPU tensors, no test functions, no device use), in the format and under the rules of tests/_criterion_edges.py,
whose helpers are reused: a case is admitted only if ``E.margin_violations`` is empty at ``E.MARGIN`` against the fp64 oracle and
``E.all_finite`` holds -- the builders assert both.

  crowded_single    ScanNet, 6-dof; scenes of (queries, GTs) = (40, 65) one GT past the word, (70, 129) three words with one bit in
                    the last, (30, 0), (33, 64) the old boundary in the same batch.  Non-overlapping axis-aligned pairs all cost
                    2 (1 + rc0(q)) - 0.5 prob, so with 258 GT columns per layer a few second costs land within 1e-4 of the kth
                    whatever the seed: the builder repairs them deterministically (new logits and a +-0.01 centre jitter for the
                    last close query of every violation, drawn from the case's generator), at most 40 rounds.
  crowded_mixed     joint config, scattered class columns in a 30-column row, 7 box columns: ARKitScenes (24, 70) rotated,
                    S3DIS (50, 200), ScanNet (20, 3).  Seeds are tried in a fixed order as in ``E.build``.
  crowded_last_bit  ScanNet, a scene of 128 GTs modelled on ``class_bookkeeping``: query 5 is matched to GT 0, 63, 64 and 127 only
                    (labels 4, 13, 2, 9 -> target 9, bits 0 and 63 of both words), query 9 to GT 64 only (target 2).
"""
import torch

import _criterion_edges as E
import test_criterion_edges_cpu as EC

CASES = ['crowded_single', 'crowded_mixed', 'crowded_last_bit']
ROTATED = ('crowded_mixed',)
# Blocks whose bound is 4 x the fp32-oracle-vs-fp64-oracle error (the rule of test_criterion_edges_cpu.MEASURED): none is needed --
# test_criterion_crowded_cpu.py asserts that the fp32 oracle is within 1e-4 of the fp64 oracle on every block of every case.
MEASURED = set()
REPAIR_ROUNDS = 40


def _repair(case, g):
    """-> (fp64 oracle, rounds used).  Every violation (l, b, j, close): the last close query gets new logits in its scene's columns
    and its box centre moves by +-0.01 per axis; both draws come from the case's generator, so the result is deterministic."""
    starts = [0]
    for n in case['sizes']:
        starts.append(starts[-1] + n)
    for rnd in range(REPAIR_ROUNDS + 1):
        ora = E.run_oracle(case, torch.float64)
        bad = E.margin_violations(case, ora)
        if not bad or rnd == REPAIR_ROUNDS:
            return ora, rnd
        for l, b, j, close in bad:
            assert not isinstance(close, str), (case['name'], l, b, j, close)        # a sentinel column cannot be repaired by a redraw
            row = starts[b] + close[-1]
            case['cls'][l][row] = torch.randn(case['CU'], generator=g) * 1.5
            sign = (torch.rand(3, generator=g) < 0.5).float() * 2 - 1
            case['box'][l][row, :3] += 0.01 * sign


def crowded_single():
    g = E._gen(7000)
    scenes = [E._random_scene(g, 'scannet', n, k) for n, k in ((40, 65), (70, 129), (30, 0), (33, 64))]
    case = E._pack('crowded_single', 'scannet', scenes, g)
    ora, rounds = _repair(case, g)
    case['repair_rounds'] = rounds
    return case, ora


def mixed_columns():
    """the interleaved, non-monotonic class-column lists of ``E.scattered_columns``: 30 columns, "no object" last"""
    CU, cols = 30, {}
    for k, name in enumerate(E.DATASETS):
        perm = torch.randperm(CU - 1, generator=E._gen(77 + k))[:E.N_CLS[name]].tolist()
        cols[name] = perm + [CU - 1]
    return CU, cols


def crowded_mixed():
    CU, cols = mixed_columns()
    names = ['arkitscenes', 's3dis', 'scannet']
    for seed in range(7000, 7050):
        g = E._gen(seed)
        scenes = [E._random_scene(g, nm, n, k) for nm, n, k in zip(names, (24, 50, 20), (70, 200, 3))]
        case = E._pack('crowded_mixed', 'joint', scenes, g, cidx=[cols[nm] for nm in names], CU=CU)
        ora = E.run_oracle(case, torch.float64)
        if not E.margin_violations(case, ora):
            break
    case['seed'] = seed
    return case, ora


def crowded_last_bit():
    for seed in range(7100, 7150):
        g = E._gen(seed)
        s = E._random_scene(g, 'scannet', 30, 128, p_mask=0.08)
        own = [0, 63, 64, 127]
        s['labels'][own] = torch.tensor([4, 13, 2, 9])
        s['qmask'][own] = False
        s['qmask'][0, [5, 6]] = True; s['qmask'][63, [5, 7]] = True; s['qmask'][64, [5, 9]] = True; s['qmask'][127, [5, 8]] = True
        others = [j for j in range(128) if j not in own]
        s['qmask'][others, 5] = False                                      # nothing else on query 5 ...
        s['qmask'][others, 9] = False                                      # ... and GT 64 alone on query 9
        case = E._pack('crowded_last_bit', 'scannet', [s, E._random_scene(g, 'scannet', 20, 3)], g)
        ora = E.run_oracle(case, torch.float64)
        if not E.margin_violations(case, ora):
            break
    case['seed'] = seed
    return case, ora


BUILDERS = dict(crowded_single=crowded_single, crowded_mixed=crowded_mixed, crowded_last_bit=crowded_last_bit)
_ORACLE, _O32 = {}, {}


def build(name):
    """-> (case, fp64 oracle), computed once per process and left unchanged; admissibility is asserted, never skipped"""
    if name not in _ORACLE:
        case, ora = BUILDERS[name]()
        assert not E.margin_violations(case, ora), (name, E.margin_violations(case, ora))
        assert E.all_finite(case, ora), name
        _ORACLE[name] = (case, ora)
    return _ORACLE[name]


def oracle32(name):
    if name not in _O32:
        _O32[name] = E.run_oracle(build(name)[0], torch.float32)
    return _O32[name]


def check_errors(case, loss, dcls, dbox, o64, o32, tag, tol_loss=2e-6):
    """``EC.check_errors`` for these cases (that function picks the rotated bounds by the names of its own cases): loss 2e-6; per
    (layer, scene) block of the packed gradients (``EC.scene_errors``) 2e-5 for an axis-aligned batch, 1e-4 (class) / 1e-3 (box) for
    a batch with rotated boxes; a block named in ``MEASURED`` has 4 x the fp32 oracle's own error as its box bound."""
    tol_c, tol_b = (1e-4, 1e-3) if case['name'] in ROTATED else (2e-5, 2e-5)
    e_l = abs(float(loss) - float(o64['loss'])) / abs(float(o64['loss']))
    errs, e32 = EC.scene_errors(case, dcls, dbox, o64), EC.scene_errors(case, o32['dcls'], o32['dbox'], o64)
    rec = dict(loss_rel=e_l, dcls=max(e[0] for e in errs.values()), dbox=max(e[1] for e in errs.values()),
               dbox_fp32_oracle=max(e[1] for e in e32.values()))
    print(tag, rec)
    assert e_l < tol_loss, rec
    for (l, b), (e_c, e_b) in errs.items():
        bound = 4 * e32[l, b][1] if (case['name'], b) in MEASURED else tol_b
        assert e_c < tol_c and e_b < bound, (tag, l, b, e_c, e_b, bound)
    return rec


def flat_gt(case, device):
    """``UniDet3DCriterion._flat_gt`` on the case, as ``_loss_fused`` calls it -> (criterion, instances, the flat-GT dict or None)"""
    from unidet3d_amd.registry import MODELS
    crit = MODELS.build(EC.CFG[case['crit']])
    insts = EC.product_insts(case, device)
    B, bd, cidx = len(insts), case['BD'], case['cidx']
    idxs = [crit.datasets.index(n) for n in case['names']]
    c1s = [len(c) for c in cidx] if cidx is not None else [case['CU']] * B
    yaw = case['yaw'] or [bd == 7] * B
    g = crit._flat_gt(insts, case['sizes'], device, [crit.topk[i] for i in idxs], [crit.datasets_weights[i] for i in idxs], c1s, yaw, cidx, bd)
    return crit, insts, g


def match_words(matched, W):
    """bool [n, g] matched set -> int64 [n, W]: GT j = bit j & 63 of word j >> 6 (bit 63 is the int64 sign bit)"""
    n, g = matched.shape
    out = torch.zeros(n, W, dtype=torch.int64)
    for j in range(g):
        bit = torch.tensor(1 << (j & 63) if (j & 63) < 63 else -(1 << 63), dtype=torch.int64)
        out[:, j >> 6] |= torch.where(matched[:, j], bit, torch.zeros((), dtype=torch.int64))
    return out

