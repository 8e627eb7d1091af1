"""Device-side training augmentation (unidet3d_amd/augment.py, csrc/augment.hip) on the MI355X against the host pipeline
(unidet3d_amd/transforms.py) and the vectors recorded from the reference (tests/golden/ref_transforms.npz).  Nothing here is
compared with the code under test."""
import os
import warnings

import numpy as np
import pytest
import torch

from _detw import fill_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
ELASTIC = dict(gran=[6, 20], mag=[40, 160])


def _G():
    return np.load(os.path.join(GOLD, 'ref_transforms.npz'))


def _fixture_scene(G, inst='X.sn.inst', sem='X.sn.sem'):
    return dict(points=G['X.points'].copy(), sp_pts_mask=G['X.sn.sp'].astype(np.int64), pts_instance_mask=G[inst].astype(np.int64),
                pts_semantic_mask=G[sem].astype(np.int64), lidar_path='data/scannet/points/fixture.bin')


def _synthetic(idx, n):
    """A ScanNet-like raw scene: rgb 0..255, instance ids with gaps, semantic ids 0 / 1 (stuff) and 2.. (things)."""
    from unidet3d_amd.synthetic import make_scene
    sc = make_scene(idx, n_points=n)
    inst = np.where(sc.instance_mask >= 0, sc.instance_mask * 3 + 2, -1).astype(np.int64)
    sem = np.where(sc.instance_mask >= 0, sc.labels[np.maximum(sc.instance_mask, 0)] + 2, np.arange(n) % 2).astype(np.int64)
    pts = sc.points.copy()
    pts[:, 3:] = np.round((pts[:, 3:] + 1) * 127.5)
    return dict(points=pts.astype(F32), sp_pts_mask=sc.superpoints.astype(np.int64), pts_instance_mask=inst, pts_semantic_mask=sem,
                lidar_path=f'data/scannet/points/syn{idx}.bin')


def _draws(B, seed=0, gate=None, identity=False):
    from unidet3d_amd import AugmentDraws
    r = np.random.RandomState(seed)
    d = AugmentDraws(flip_h=r.rand(B) < 0.5, flip_v=r.rand(B) < 0.5, angle=r.uniform(-3.14, 3.14, B), scale=r.uniform(0.8, 1.2, B),
                     trans=r.randn(B, 3) * 0.1, elastic_gate=np.zeros(B, bool) if gate is None else np.asarray(gate, bool))
    if identity:
        d.flip_h[:] = False; d.flip_v[:] = False; d.angle[:] = 0; d.scale[:] = 1; d.trans[:] = 0
    return d


class _SceneNoise:
    """noise(scene, pass, dims) drawing from numpy in the host's order: scene b owns the stream of ``np.random.seed(seeds[b])``, whose
    first draw is the gate's ``rand()`` (transforms.ElasticTransfrom.transform), then three ``randn`` grids per pass."""

    def __init__(self, seeds):
        self.rs = [np.random.RandomState(s) for s in seeds]
        for r in self.rs:
            r.rand()

    def __call__(self, b, p, dims):
        return np.stack([self.rs[b].randn(*dims).astype('float32') for _ in range(3)])


def _affine_np(A, xyz):
    """the numpy float32 expression the point map is defined by"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([((A[r, 0] * x + A[r, 1] * y) + A[r, 2] * z) + A[r, 3] for r in range(3)], 1).astype(F32)


def _host_pipeline(dicts, draws, seeds, mapping='scannet', elastic=True):
    """transforms.py on every scene with the same draws -> to_batch_inputs on the CPU."""
    from unidet3d_amd import transforms as X
    from unidet3d_amd.augment import compose_affine
    A = compose_affine(draws.flip_h, draws.flip_v, draws.angle, draws.scale, draws.trans)
    out = []
    for b, d in enumerate(dicts):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        d['points'] = np.concatenate([_affine_np(A[b], d['points'][:, :3]), d['points'][:, 3:]], 1)
        d = X.NormalizePointsColor_([127.5] * 3)(d)
        d = X.PointDetClassMappingScanNet(20, [0, 1])(d) if mapping == 'scannet' else X.PointDetClassMappingS3DIS([7, 8, 9, 10, 11])(d)
        if elastic:
            np.random.seed(seeds[b])
            d = X.ElasticTransfrom(ELASTIC['gran'], ELASTIC['mag'], 0.02, 1.0 if draws.elastic_gate[b] else 0.0)(d)
        out.append(d)
    return X.to_batch_inputs(out, 'cpu'), out


def _aug(elastic=True, mapping=('scannet', 20, [0, 1]), num_points=None, color=True):
    from unidet3d_amd import DeviceAugment
    return DeviceAugment(0.02, num_points=num_points, color_mean=[127.5] * 3 if color else None, color_std=127.5 if color else None,
                         mapping=mapping, elastic=dict(p=0.5, **ELASTIC) if elastic else None)


def _same_samples(got, want, sem=None):
    for g, w in zip(got, want):
        assert torch.equal(g.gt_pts_seg.pts_instance_mask.cpu(), w.gt_pts_seg.pts_instance_mask) and g.gt_pts_seg.pts_instance_mask.dtype == torch.int64
        assert torch.equal(g.gt_pts_seg.sp_pts_mask.cpu(), w.gt_pts_seg.sp_pts_mask)
        assert torch.equal(g.gt_instances_3d.labels_3d.cpu(), w.gt_instances_3d.labels_3d) and g.gt_instances_3d.labels_3d.dtype == torch.int64
        assert g.gt_instances_3d.sp_masks.dtype == torch.bool and g.gt_instances_3d.sp_masks.shape == w.gt_instances_3d.sp_masks.shape
        assert torch.equal(g.gt_instances_3d.sp_masks.cpu(), w.gt_instances_3d.sp_masks)
        assert g.n_superpoints == w.n_superpoints and g.lidar_path == w.lidar_path


def _ulp_ok(dev32, host64):
    ref = host64.astype(F32)
    return np.abs(dev32.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- kernels
def test_blurred_grids_bit_equal():
    """gran 6 and 20 on the fixture's extent, a ragged batch with an empty slot and a grid axis of length 3."""
    from unidet3d_amd import transforms as X
    from unidet3d_amd.augment import blur_noise_grids
    G = _G()
    ext = np.abs(G['X.points'][:, :3] / 0.02).max(0)
    cases = []
    for seed, (e, gran) in enumerate([(ext, 6), (ext, 20), (np.array([2.0, 50.0, 7.0]), 6), (np.array([0.5, 0.5, 0.5]), 20)]):
        np.random.seed(100 + seed)
        want, dim = X.elastic_noise_grids(e, gran)
        np.random.seed(100 + seed)
        noise = np.stack([np.random.randn(*dim).astype('float32') for _ in range(3)])
        cases.append((noise, np.asarray(dim), np.stack(want)))
    assert 3 in cases[2][1].tolist() and cases[3][1].tolist() == [3, 3, 3]
    dims = np.stack([cases[0][1], cases[2][1], np.zeros(3, np.int64), cases[1][1], cases[3][1]])       # slot 2: a scene without a pass
    order = [0, 2, None, 1, 3]
    flat = torch.from_numpy(np.concatenate([cases[i][0].reshape(-1) for i in order if i is not None])).to(DEV)
    grids, _, goff = blur_noise_grids(flat, dims, DEV)
    goff = goff.cpu().numpy()
    g = grids.cpu().numpy()
    for slot, i in enumerate(order):
        if i is None:
            assert goff[slot] == goff[slot + 1]
            continue
        got = g[goff[slot]:goff[slot + 1], :3].reshape(*dims[slot], 3).transpose(3, 0, 1, 2)
        assert got.dtype == np.float32 and np.array_equal(got, cases[i][2]), (slot, dims[slot])


def test_elastic_kernel_range_and_gate():
    """Called directly with undersized dims: points outside the node range get 0 (x comes back), inside ones the host's trilinear
    value; a scene whose gate is off passes through, and the float64 -> float32 pass rounds once."""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import transforms as X
    from unidet3d_amd.augment import blur_noise_grids
    rng = np.random.RandomState(3)
    x = (rng.rand(4000, 3) * 100 - 50).astype(F32)                      # nodes of a [3, 4, 3] grid at gran 6 span +-12 / +-18 / +-12
    x[:6] = [[12, 18, 12], [-12, -18, -12], [12.000001, 0, 0], [0, 0, 0], [5.5, -17.25, 11.75], [0, 18.5, 0]]
    dims = np.array([[3, 4, 3], [3, 4, 3]])
    noise = rng.randn(2, 3, 3, 4, 3).astype(F32)
    grids, d_dims, d_goff = blur_noise_grids(torch.from_numpy(noise.reshape(-1)).to(DEV), dims, DEV)
    host_grids = [noise[0]]
    for axis in (0, 1, 2, 0, 1, 2):
        host_grids = [np.stack([X._box_blur3(n, axis) for n in host_grids[0]])]
    off = torch.tensor([0, 2500, 4000], dtype=torch.int64, device=DEV)
    gate = torch.tensor([1, 0], dtype=torch.uint8, device=DEV)
    xin = torch.from_numpy(x).to(DEV)
    out64 = torch.empty((4000, 3), dtype=torch.float64, device=DEV)
    L.call('u3d_aug_elastic', L.ptr(xin), 0, L.ptr(out64), 1, L.ptr(off), 2, 4000, L.ptr(grids), L.ptr(d_goff), L.ptr(d_dims), L.ptr(gate), 6.0, 40.0,
           L.stream())
    got = out64.cpu().numpy()
    v = X.trilinear_lookup(list(host_grids[0]), dims[0], 6, x[:2500])
    t = (x[:2500].astype(np.float64) + (dims[0] - 1) * 6) / 12.0
    inside = ((t >= 0) & (t <= dims[0] - 1)).all(1)
    assert inside[:2].all() and not inside[2] and inside[3] and inside[4] and not inside[5] and 10 < inside.sum() < 2000
    assert np.array_equal(got[:2500][~inside], x[:2500][~inside].astype(np.float64))         # 0 outside the node range
    want = x[:2500].astype(np.float64) + v * 40.0
    assert np.abs(got[:2500] - want).max() <= 1e-11 and np.abs(v[inside]).max() > 1e-3          # two float64 evaluations of one formula
    assert np.array_equal(got[2500:], x[2500:].astype(np.float64))                              # gate off
    out32 = torch.empty((4000, 3), dtype=torch.float32, device=DEV)
    L.call('u3d_aug_elastic', L.ptr(out64), 1, L.ptr(out32), 0, L.ptr(off), 2, 4000, L.ptr(grids), L.ptr(d_goff), L.ptr(d_dims), L.ptr(gate), 6.0, 0.0,
           L.stream())
    assert np.array_equal(out32.cpu().numpy()[2500:], x[2500:])                                 # float32 -> float64 -> float32: bit for bit


def test_extent_is_exact_for_ragged_batches():
    from unidet3d_amd import _lib as L
    rng = np.random.RandomState(5)
    sizes = [5000, 0, 1, 70001]
    x = (rng.randn(sum(sizes), 3) * 300).astype(F32)
    off = np.concatenate(([0], np.cumsum(sizes)))
    d_off = torch.from_numpy(off).to(DEV)
    for dt, name in ((torch.float32, 'u3d_aug_extent_f32'), (torch.float64, 'u3d_aug_extent_f64')):
        xd = torch.from_numpy(x).to(DEV).to(dt)
        ext = torch.full((4, 3), -1.0, dtype=dt, device=DEV)
        L.call(name, L.ptr(xd), L.ptr(d_off), 4, max(sizes), L.ptr(ext), L.stream())
        want = np.stack([np.abs(x[off[b]:off[b + 1]]).max(0) if sizes[b] else np.zeros(3, F32) for b in range(4)])
        assert np.array_equal(ext.cpu().numpy(), want.astype(ext.cpu().numpy().dtype))


# ---------------------------------------------------------------------------------------------------------------- against the reference fixture
def test_elastic_matches_reference_fixture_and_host_port():
    from unidet3d_amd import DeviceSceneCache
    from unidet3d_amd import transforms as X
    G = _G()
    cache = DeviceSceneCache.from_scene_dicts([_fixture_scene(G)], DEV)
    aug = _aug(color=False, mapping=None)
    d = _draws(1, gate=[True], identity=True)
    np.random.seed(1234)
    np.random.rand()                                                                 # the gate's draw, as in the host's order
    d.noise = lambda b, p, dims: np.stack([np.random.randn(*dims).astype('float32') for _ in range(3)])
    inputs, _ = aug(cache, [0], d)
    e = inputs['elastic_coords'][0].cpu().numpy()
    assert e.dtype == np.float32                                                     # to_batch_inputs' dtype (the fixture keeps the pipeline's float64)
    err = np.abs(e - G['X.elastic']).max()
    print('elastic vs reference fixture: max |diff| =', err, 'voxel')
    assert err < 1e-4                                                                # the bound test_transforms_match_reference holds the host port to
    assert np.array_equal(inputs['points'][0].cpu().numpy(), G['X.points'])          # identity affine, no colour step: bit for bit
    np.random.seed(1234)
    host = X.ElasticTransfrom(ELASTIC['gran'], ELASTIC['mag'], 0.02, 1.0)(dict(points=G['X.points'].copy()))['elastic_coords']
    assert host.dtype == np.float64
    ok = _ulp_ok(e, host)
    print('elastic vs host port: elements off by one float32 ulp:', int((e != host.astype(F32)).sum()), 'of', e.size)
    assert ok.all()
    d0 = _draws(1, gate=[False], identity=True)
    e0 = aug(cache, [0], d0)[0]['elastic_coords'][0].cpu().numpy()
    assert e0.dtype == np.float32 and np.array_equal(e0, G['X.elastic_off'])       # gate off: bit for bit
    assert aug.last_host_reads == 0


def test_point_sample_matches_reference_fixture():
    from unidet3d_amd import DeviceSceneCache
    G = _G()
    d = _fixture_scene(G, inst='X.ps.in_inst')
    cache = DeviceSceneCache.from_scene_dicts([d], DEV)
    aug = _aug(elastic=False, mapping=None, num_points=1500, color=False)
    dr = _draws(1, identity=True)
    np.random.seed(99)
    dr.indices = [np.random.choice(range(len(d['points'])), 1500)]
    inputs, samples = aug(cache, [0], dr)
    seg = samples[0].gt_pts_seg
    assert np.array_equal(inputs['points'][0].cpu().numpy(), G['X.ps.points'])
    assert np.array_equal(seg.pts_instance_mask.cpu().numpy(), G['X.ps.inst'])
    assert np.array_equal(seg.pts_semantic_mask.cpu().numpy(), G['X.ps.sem'])
    assert np.array_equal(seg.sp_pts_mask.cpu().numpy(), G['X.ps.sp'])
    assert samples[0].n_superpoints == int(G['X.ps.sp'].max()) + 1 and 'elastic_coords' not in inputs


def _crafted():
    """no instances at all | a superpoint split exactly in half between an instance and stuff | instance ids with gaps"""
    def scene(sp, inst, sem, name):
        n = len(sp)
        rng = np.random.RandomState(n)
        return dict(points=np.concatenate([rng.randn(n, 3), rng.rand(n, 3) * 255], 1).astype(F32), sp_pts_mask=np.asarray(sp, np.int64),
                    pts_instance_mask=np.asarray(inst, np.int64), pts_semantic_mask=np.asarray(sem, np.int64), lidar_path=f'data/scannet/points/{name}.bin')
    none = scene([0, 1, 1, 2, 0], [-1, -1, -1, -1, -1], [0, 1, 0, 20, 1], 'none')
    half = scene([0, 0, 0, 0, 1, 1, 1, 2], [4, 4, -1, -1, 4, 4, -1, 9], [5, 5, 0, 1, 5, 5, 1, 7], 'half')
    gaps = scene([3, 3, 0, 1, 2, 2, 3, 1, 0, 0], [17, 17, 2, -1, 40, 40, 5, 2, 3, 3], [9, 9, 4, 0, 3, 3, 19, 4, 1, 20], 'gaps')   # ids 3: stuff class
    return [none, half, gaps]


def test_class_mappings_match_reference_fixture_and_host():
    from unidet3d_amd import DeviceSceneCache
    from unidet3d_amd import transforms as X
    G = _G()
    dicts = [_fixture_scene(G)] + _crafted()
    cache = DeviceSceneCache.from_scene_dicts(dicts, DEV)
    aug = _aug(elastic=False, color=False)
    _, samples = aug(cache, [0, 1, 2, 3], _draws(4, identity=True))
    s = samples[0]
    assert np.array_equal(s.gt_pts_seg.pts_instance_mask.cpu().numpy(), G['X.sn.out_inst'])
    assert np.array_equal(s.gt_instances_3d.labels_3d.cpu().numpy(), G['X.sn.out_labels'])
    assert np.array_equal(s.gt_instances_3d.sp_masks.cpu().numpy(), G['X.sn.out_sp_masks'])
    host = [X.PointDetClassMappingScanNet(20, [0, 1])({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}) for d in dicts]
    (_, want) = X.to_batch_inputs(host, 'cpu')
    _same_samples(samples, want)
    assert samples[1].gt_instances_3d.sp_masks.shape == (0, 3) and len(samples[1].gt_instances_3d.labels_3d) == 0
    m = samples[2].gt_instances_3d.sp_masks.cpu().numpy()
    assert m.shape == (2, 3) and not m[0, 0] and m[0, 1] and m[1, 2]               # 2 hits of 4: exactly half is not "more than half"
    assert samples[3].gt_pts_seg.pts_instance_mask.cpu().numpy().tolist() == [2, 2, 0, -1, 3, 3, 1, 0, -1, -1]
    # S3DIS: ids from the fixture, class filter and remap
    d3 = _fixture_scene(G, inst='X.s3.inst', sem='X.s3.sem')
    d3['lidar_path'] = 'data/s3dis/points/fixture.bin'
    c3 = DeviceSceneCache.from_scene_dicts([d3, d3], DEV)
    a3 = _aug(elastic=False, color=False, mapping=('s3dis', [7, 8, 9, 10, 11]))
    _, s3 = a3(c3, [1, 0], _draws(2, identity=True))
    for s in s3:
        assert np.array_equal(s.gt_pts_seg.pts_instance_mask.cpu().numpy(), G['X.s3.out_inst'])
        assert np.array_equal(s.gt_instances_3d.labels_3d.cpu().numpy(), G['X.s3.out_labels'])
        assert np.array_equal(s.gt_instances_3d.sp_masks.cpu().numpy(), G['X.s3.out_sp_masks'])


def _s3dis_like(seed, n, n_sp=300, per_inst=10):
    """every point belongs to an instance (ids from 0, contiguous), superpoints mostly inside one instance, 13 semantic classes"""
    rng = np.random.RandomState(seed)
    sp = rng.randint(0, n_sp, n)
    inst = sp // per_inst
    stray = rng.rand(n) < 0.2                                        # superpoints that straddle instances: masks near the 1/2 threshold
    inst[stray] = rng.randint(0, n_sp // per_inst, stray.sum())
    sem = rng.randint(0, 13, n_sp // per_inst)[inst]
    pts = np.concatenate([rng.randn(n, 3) * 2, np.round(rng.rand(n, 3) * 255)], 1).astype(F32)
    return dict(points=pts, sp_pts_mask=sp.astype(np.int64), pts_instance_mask=inst.astype(np.int64), pts_semantic_mask=sem.astype(np.int64),
                lidar_path=f'data/s3dis/points/area{seed}.bin')


def test_sampled_s3dis_pipeline_equals_host_pipeline():
    """PointSample_ -> flip / rotation / scale / translation -> PointDetClassMappingS3DIS -> NormalizePointsColor_ -> ElasticTransfrom(p=-1),
    the reference's S3DIS train order, with injected sample indices: relabelled superpoints in batch order feed the GT masks, the
    class filter remaps the instance ids and scatters the labels.  One scene is smaller than num_points."""
    from unidet3d_amd import DeviceSceneCache
    from unidet3d_amd import transforms as X
    from unidet3d_amd.augment import compose_affine
    dicts = [_s3dis_like(1, 6000), _s3dis_like(2, 1800), _s3dis_like(3, 9000, n_sp=500, per_inst=25)]
    cache = DeviceSceneCache.from_scene_dicts(dicts, DEV)
    aug = _aug(mapping=('s3dis', [7, 8, 9, 10, 11]), num_points=2500)
    aug.elastic['p'] = -1
    d = _draws(3, seed=51)
    seeds = [61, 62, 63]
    d.indices = []
    host = []
    A = compose_affine(d.flip_h, d.flip_v, d.angle, d.scale, d.trans)
    for b, sc in enumerate(dicts):
        np.random.seed(seeds[b])
        d.indices.append(np.random.choice(range(len(sc['points'])), min(2500, len(sc['points']))))
        np.random.seed(seeds[b])
        h = X.PointSample_(2500)({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()})
        h['points'] = np.concatenate([_affine_np(A[b], h['points'][:, :3]), h['points'][:, 3:]], 1)
        for t in (X.PointDetClassMappingS3DIS([7, 8, 9, 10, 11]), X.NormalizePointsColor_([127.5] * 3),
                  X.ElasticTransfrom(ELASTIC['gran'], ELASTIC['mag'], 0.02, -1)):
            h = t(h)
        host.append(h)
    inputs, samples = aug(cache, [0, 1, 2], d)
    winputs, wsamples = X.to_batch_inputs(host, 'cpu')
    assert [len(p) for p in inputs['points']] == [2500, 1800, 2500] and aug.last_host_reads == 1
    for k in ('points', 'elastic_coords'):
        for g, w in zip(inputs[k], winputs[k]):
            assert g.dtype == w.dtype and torch.equal(g.cpu(), w), k
    _same_samples(samples, wsamples)
    for s, h in zip(samples, host):
        assert np.array_equal(s.gt_pts_seg.pts_semantic_mask.cpu().numpy(), h['pts_semantic_mask'])
        assert 0 < len(s.gt_instances_3d.labels_3d) < int(h['pts_instance_mask'].max()) + 1 + 30       # the class filter dropped some
        assert s.gt_instances_3d.sp_masks.any() and s.n_superpoints < 500


def test_affine_and_colour_bit_equal():
    from unidet3d_amd import DeviceSceneCache
    from unidet3d_amd.augment import compose_affine
    dicts = [_synthetic(300, 20000), _synthetic(301, 777)]
    cache = DeviceSceneCache.from_scene_dicts(dicts, DEV)
    aug = _aug(elastic=True, mapping=None)
    d = _draws(2, seed=11)
    d.flip_h[:] = [True, False]; d.flip_v[:] = [False, True]
    inputs, _ = aug(cache, [0, 1], d)
    A = compose_affine(d.flip_h, d.flip_v, d.angle, d.scale, d.trans)
    for b, sc in enumerate(dicts):
        got = inputs['points'][b].cpu().numpy()
        xyz = _affine_np(A[b], sc['points'][:, :3])
        assert np.array_equal(got[:, :3], xyz)
        assert np.array_equal(got[:, 3:], (sc['points'][:, 3:] - np.asarray([127.5] * 3, F32)) / np.asarray(127.5, F32))
        assert np.array_equal(inputs['elastic_coords'][b].cpu().numpy(), xyz / 0.02)          # gate off: x' / float32(voxel_size)


# ---------------------------------------------------------------------------------------------------------------- whole pipeline
def _model():
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd.config import build_model, scannet_model_cfg
    cfg = scannet_model_cfg(voxel_size=0.02)
    cfg['decoder']['num_layers'] = 2
    return fill_state_dict(build_model(cfg), tag0=3400, scale=0.06).to(DEV).train()


def test_whole_pipeline_elastic_off_equals_host_pipeline_and_loss_bits():
    from unidet3d_amd import DeviceSceneCache
    one = _synthetic(312, 4000)
    one = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in one.items()}                       # a 1-point scene
    one['pts_instance_mask'] = np.array([-1]); one['pts_semantic_mask'] = np.array([0]); one['sp_pts_mask'] = np.array([0])
    dicts = [_synthetic(310, 9000), one, _synthetic(311, 14000)]
    cache = DeviceSceneCache.from_scene_dicts(dicts, DEV)
    aug = _aug()
    d = _draws(3, seed=21)
    inputs, samples = aug(cache, [0, 1, 2], d)
    (winputs, wsamples), _ = _host_pipeline(dicts, d, [0, 0, 0])
    for k in ('points', 'elastic_coords'):
        for g, w in zip(inputs[k], winputs[k]):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), k
    _same_samples(samples, wsamples)
    model = _model()
    torch.manual_seed(0)
    a = model.loss(inputs, samples)['det_loss']
    winputs = {k: [t.to(DEV) for t in v] for k, v in winputs.items()}
    for s in wsamples:
        for obj in (s.gt_pts_seg, s.gt_instances_3d):
            for k, v in list(vars(obj).items()):
                if torch.is_tensor(v):
                    setattr(obj, k, v.to(DEV))
    torch.manual_seed(0)
    b = model.loss(winputs, wsamples)['det_loss']
    print('loss on the device-built batch', float(a), 'on the host-built batch', float(b))
    assert torch.isfinite(a) and torch.equal(a, b)


def test_whole_pipeline_elastic_on_and_training_through_prefetch_step():
    from unidet3d_amd import DeviceSceneCache
    dicts = [_synthetic(320, 12000), _synthetic(321, 5000), _synthetic(322, 8000)]
    cache = DeviceSceneCache.from_scene_dicts(dicts, DEV)
    aug = _aug()
    seeds = [41, 42, 43]
    d = _draws(3, seed=31, gate=[True, False, True])
    d.noise = _SceneNoise(seeds)
    inputs, samples = aug(cache, [0, 1, 2], d)
    assert aug.last_host_reads == 2
    (winputs, wsamples), hdicts = _host_pipeline(dicts, d, seeds)
    _same_samples(samples, wsamples)
    for b in range(3):
        assert torch.equal(inputs['points'][b].cpu(), winputs['points'][b])
        e = inputs['elastic_coords'][b].cpu().numpy()
        h = np.asarray(hdicts[b]['elastic_coords'])
        assert e.dtype == np.float32 and _ulp_ok(e, h.astype(np.float64)).all(), b
        if not d.elastic_gate[b]:
            assert np.array_equal(e, h)
        else:
            assert np.abs(e - inputs['points'][b].cpu().numpy()[:, :3] / F32(0.02)).max() > 10        # a real distortion

    class OptimWrapper:
        def __init__(self, params):
            self.opt = torch.optim.AdamW(params, lr=1e-3)

        def update_params(self, loss):
            loss.backward(); self.opt.step(); self.opt.zero_grad()
    model = _model()
    ow = OptimWrapper(model.parameters())
    d.noise = _SceneNoise(seeds)
    batch = dict(zip(('inputs', 'data_samples'), aug(cache, [0, 1, 2], d)))
    model.prefetch_step(batch)
    losses = []
    for it in range(3):
        log = model.train_step(batch, ow)
        if it < 2:
            d.noise = _SceneNoise(seeds)                       # the same augmented batch again: three steps on it lower the loss
            batch = dict(zip(('inputs', 'data_samples'), aug(cache, [0, 1, 2], d)))
            model.prefetch_step(batch)
            assert model._staged is not None and model._prefetched is not None
        losses.append(float(log['loss'].detach()))
    torch.cuda.synchronize()
    print('train_step losses fed by DeviceAugment through prefetch_step:', losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_host_reads_and_determinism():
    from unidet3d_amd import DeviceAugment, DeviceSceneCache
    from test_augment_cpu import S3DIS_TRAIN, SCANNET_TRAIN
    dicts = [_synthetic(330 + i, 6000 + 1500 * i) for i in range(4)]
    cache = DeviceSceneCache.from_scene_dicts(dicts, DEV)
    sn = DeviceAugment.from_pipeline(SCANNET_TRAIN, 0.02)
    sn.elastic['p'] = 1.0                                               # every scene takes both passes: the most reads a batch can need
    s3 = DeviceAugment.from_pipeline([dict(s, num_points=5000) if s['type'] == 'PointSample_' else s for s in S3DIS_TRAIN], 0.02)
    s3.mapping = ('s3dis', [2, 3, 4, 5, 6, 7])

    def flat(res):
        inputs, samples = res
        ts = [t for k in ('points', 'elastic_coords') for t in inputs[k]]
        for s in samples:
            ts += [s.gt_pts_seg.pts_instance_mask, s.gt_pts_seg.sp_pts_mask, s.gt_instances_3d.labels_3d, s.gt_instances_3d.sp_masks]
        return ts
    for aug, max_reads in ((sn, 3), (s3, 3)):
        g = torch.Generator(DEV)
        g.manual_seed(7)
        first = flat(aug(cache, [3, 0, 2, 1], generator=g))                 # warm: library, allocator, pinned staging
        torch.cuda.synchronize()
        g.manual_seed(7)
        prev = torch.cuda.get_sync_debug_mode()
        try:
            torch.cuda.set_sync_debug_mode('warn')
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter('always')
                again = flat(aug(cache, [3, 0, 2, 1], generator=g))
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        syncs = [str(w.message) for w in rec if 'synchroniz' in str(w.message).lower()]
        print('host reads:', len(syncs), 'reported', aug.last_host_reads, 'launches', aug.last_launches)
        assert len(syncs) <= max_reads and len(syncs) == aug.last_host_reads, syncs
        assert len(first) == len(again) and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(first, again))   # same state, same bits
        other = flat(aug(cache, [3, 0, 2, 1], generator=g))                 # the state has moved on
        assert not torch.equal(other[0], first[0])
    assert sn.last_host_reads == 2 and s3.last_host_reads == 1
