"""Fused inference on the device, bit for bit: the output epilogue of the pair-list convolutions (u3d_spconv_gmm_ep)
against today's entry point followed by u3d_bn_apply; the U-Net in eval mode under no_grad with the toggle on against the toggle off;
UniDet3D.predict with the toggle on against off.  Every comparison is torch.equal on int32 views: -0.0 and +0.0 differ."""
import copy
import ctypes
import functools
import os

import pytest
import torch
from torch import nn

import _conv_geometry as cg

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
PATTERN = 0x7FC0BEEF                  # a NaN: what an output buffer holds wherever the launch must not write
SHAPES = [(16, 32), (32, 32), (64, 96), (192, 96), (224, 64)]        # (224, 64): the chunk loop of the wave-tile kernel
N_DST = (1, 127, 128, 129, 255, 256, 257)                            # around the 4R-row workgroup tile, R = 32 and 64
GUARD = 4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _level(n):
    """SubM rulebook (27 offsets) of a strip of n voxels, two wide: neighbours along two axes, nine offsets with pairs"""
    from unidet3d_amd import sparse
    _, B, shape, coords = cg._case(f'strip_{n}', 1, (n // 2 + 5, 4, 3), [(0, 2 + i // 2, 1 + i % 2, 1) for i in range(n)])
    ix = sparse.OccupancyIndex.from_coords(coords.to(DEV), B, shape)
    assert ix.count() == n
    rows = ix.coords(n)
    assert torch.equal(rows.cpu(), coords)
    return sparse.build_subm_rulebook(rows, ix)


@functools.lru_cache(maxsize=None)
def _inputs(cs, cd, n):
    g = torch.Generator().manual_seed(cs * 1000 + cd + n)
    x = torch.randn(n, cs, generator=g).to(DEV)
    w = (torch.randn(cd, 27, cs, generator=g) * 0.1).to(DEV)
    add = torch.randn(n, cd, generator=g).to(DEV)
    return x, w, add


@functools.lru_cache(maxsize=None)
def _affine(cd, j):
    """scale / shift over cd + 32 columns (the wide layout's own columns; the plain layout takes columns 32 ..): negative scales, exact
    zeros, and -- scale 0 with shift -0.0 / +0.0 -- results that are exactly -0.0 and +0.0 in front of the ReLU"""
    g = torch.Generator().manual_seed(77 + j)
    scale, shift = torch.randn(cd + 32, generator=g), torch.randn(cd + 32, generator=g)
    scale[33::8] = 0.0
    shift[33::16] = -0.0
    shift[41::16] = 0.0
    scale[34::8] = -1.0
    shift[34::16] = 0.0
    scale[36::8] = -scale[36::8].abs()
    return scale.to(DEV), shift.to(DEV)


class _Pins:
    """U3D_GMM_R / U3D_GMM_G: the plan of today's entry points (read on every call)"""

    def __init__(self, R, G):
        self.want = {'U3D_GMM_R': str(R), 'U3D_GMM_G': str(G)}

    def __enter__(self):
        self.prev = {k: os.environ.get(k) for k in self.want}
        os.environ.update(self.want)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _out_buffer(n, ld):
    return torch.full((n + GUARD, ld), PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)


def _check_buffer(buf, n, col, want, what):
    b = buf.view(torch.int32)
    cd = want.shape[1]
    block = (b[:n, col:col + cd] == _bits(want)).all()
    beside = (b[:n, :col] == PATTERN).all() & (b[:n, col + cd:] == PATTERN).all()
    guard = (b[n:] == PATTERN).all()
    ok = torch.stack((block, beside, guard)).tolist()              # one read-back per buffer
    assert ok[0], f'{what}: differs from the reference'
    assert ok[1], f'{what}: wrote outside its column block'
    assert ok[2], f'{what}: wrote past the last row'


@pytest.mark.parametrize('cs,cd', SHAPES)
@pytest.mark.parametrize('form', [2, 0])
@pytest.mark.parametrize('fmt', [0, 1, 2])
def test_epilogue_equals_todays_entry_then_bn_apply(fmt, form, cs, cd):
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse
    lib = L.lib()
    pack, entry = sparse._GMM_ENTRY[fmt]
    prev_form = lib.u3d_conv_kernel(form)
    try:
        for n in N_DST:
            rb = _level(n)
            x, w, add = _inputs(cs, cd, n)
            if fmt and cs % 32:          # the bf16 / three-plane kernels take multiples of 32 source channels: both entries refuse alike
                p = L.ptr(x)
                old = getattr(lib, entry)(p, n, p, p, p, p, 27, rb.cap, cs, cd, n, 64, 1, None, p, None, None, 0.0, None)
                ep = L.ConvEpilogue()
                ep.raw, ep.raw_ld = p, cd
                new = lib.u3d_spconv_gmm_ep(fmt, p, n, p, p, p, p, 27, rb.cap, cs, cd, n, 64, 1, None, None, None, ctypes.byref(ep), 0.0, None)
                assert old == new == -3
                continue
            wp = torch.empty(sparse._pack_floats(w.numel(), fmt), dtype=torch.float32, device=DEV)
            L.call(pack, L.ptr(w), L.ptr(wp), cd, 27, cs, 0, L.stream())
            for R in (32, 64):
                tiles = rb.tile_starts('out', R)
                for G in (1, 9):
                    ws = torch.empty(G * n * cd, dtype=torch.float32, device=DEV) if G > 1 else None
                    head = (L.ptr(x), n, L.ptr(wp), L.ptr(rb.pair_in), L.ptr(rb.pair_out), L.ptr(tiles), 27, rb.cap, cs, cd, n, R, G)
                    for addend in (None, add):
                        # ---- the reference: today's entry point, then u3d_bn_apply for each (norm, relu)
                        dst = torch.empty(n, cd, dtype=torch.float32, device=DEV)
                        with _Pins(R, G):
                            L.call(entry, *head, L.ptr(addend), L.ptr(dst), L.ptr(ws), None, 0.0, L.stream())
                        want = {}
                        for j in (0, 1):
                            sc, sf = (t[32:].contiguous() for t in _affine(cd, j))
                            for relu in (0, 1):
                                y = torch.empty_like(dst)
                                L.call('u3d_bn_apply', L.ptr(dst), L.ptr(sc), L.ptr(sf), relu, n, cd, L.ptr(y), None, L.stream())
                                want[j, relu] = y
                        # ---- the epilogue, every output set and layout
                        for relu in (0, 1):
                            for n_act in (1, 2):
                                for with_raw in (True, False):
                                    for wide in (False, True):
                                        what = f'fmt {fmt} form {form} {cs}->{cd} n {n} R {R} G {G} addend {addend is not None} relu {relu} ' \
                                               f'acts {n_act} raw {with_raw} wide {wide}'
                                        ld, col = (cd + 32, 32) if wide else (cd, 0)
                                        ep = L.ConvEpilogue()
                                        raw = _out_buffer(n, ld) if with_raw else None
                                        if with_raw:
                                            ep.raw, ep.raw_ld, ep.raw_col = raw.data_ptr(), ld, col
                                        ep.n_act = n_act
                                        acts, keep = [], []
                                        for j in range(n_act):
                                            sc, sf = _affine(cd, j) if wide else (t[32:].contiguous() for t in _affine(cd, j))
                                            keep += [sc, sf]
                                            acts.append(_out_buffer(n, ld))
                                            rj = relu if j == 0 else 1 - relu
                                            ep.act[j], ep.act_ld[j], ep.act_col[j] = acts[j].data_ptr(), ld, col
                                            ep.scale[j], ep.shift[j], ep.relu[j] = sc.data_ptr(), sf.data_ptr(), rj
                                        L.call('u3d_spconv_gmm_ep', fmt, *head, L.ptr(addend), L.ptr(ws), None, ctypes.byref(ep), 0.0, L.stream())
                                        if with_raw:
                                            _check_buffer(raw, n, col, dst, what + ': raw')
                                        for j in range(n_act):
                                            _check_buffer(acts[j], n, col, want[j, relu if j == 0 else 1 - relu], what + f': activated {j}')
                        z = want[0, 0]
                        if n >= 127:      # the value domain the comparison is about: both zeros in front of the ReLU
                            zb = _bits(z)
                            assert bool((zb == 0).any()) and bool((zb == -2 ** 31).any()), 'no +0.0 / -0.0 among the results'
    finally:
        lib.u3d_conv_kernel(prev_form)


def test_bf16_rows_form_through_the_epilogue():
    """fmt 3 (bf16 source rows, the shadow a batch norm wrote): raw and activated outputs against u3d_spconv_gmm_bf16a + u3d_bn_apply"""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse
    for cs, cd in ((32, 32), (64, 96), (192, 96)):
        for n in (129, 257):
            rb = _level(n)
            x, w, add = _inputs(cs, cd, n)
            xb = sparse.to_shadow(x)
            wp = torch.empty(sparse._pack_floats(w.numel(), 1), dtype=torch.float32, device=DEV)
            L.call('u3d_weight_pack_bf16', L.ptr(w), L.ptr(wp), cd, 27, cs, 0, L.stream())
            for R, G in ((32, 1), (64, 1), (32, 9), (32, 3)):
                tiles = rb.tile_starts('out', R)
                ws = torch.empty(G * n * cd, dtype=torch.float32, device=DEV) if G > 1 else None
                head = (L.ptr(xb), n, L.ptr(wp), L.ptr(rb.pair_in), L.ptr(rb.pair_out), L.ptr(tiles), 27, rb.cap, cs, cd, n, R, G)
                dst = torch.empty(n, cd, dtype=torch.float32, device=DEV)
                with _Pins(R, G):
                    L.call('u3d_spconv_gmm_bf16a', *head, L.ptr(add), L.ptr(dst), L.ptr(ws), 0.0, L.stream())
                sc, sf = _affine(cd, 0)
                y = torch.empty_like(dst)
                L.call('u3d_bn_apply', L.ptr(dst), L.ptr(sc[32:].contiguous()), L.ptr(sf[32:].contiguous()), 1, n, cd, L.ptr(y), None, L.stream())
                raw, act = _out_buffer(n, cd + 32), _out_buffer(n, cd + 32)
                ep = L.ConvEpilogue()
                ep.raw, ep.raw_ld, ep.raw_col, ep.n_act = raw.data_ptr(), cd + 32, 32, 1
                ep.act[0], ep.act_ld[0], ep.act_col[0], ep.scale[0], ep.shift[0], ep.relu[0] = act.data_ptr(), cd + 32, 32, sc.data_ptr(), sf.data_ptr(), 1
                L.call('u3d_spconv_gmm_ep', 3, *head, L.ptr(add), L.ptr(ws), None, ctypes.byref(ep), 0.0, L.stream())
                _check_buffer(raw, n, 32, dst, f'{cs}->{cd} n {n} R {R} G {G}: raw')
                _check_buffer(act, n, 32, y, f'{cs}->{cd} n {n} R {R} G {G}: activated')


def test_refusals_leave_every_output_untouched():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse
    lib = L.lib()
    n, cs, cd = 129, 32, 32
    rb = _level(n)
    x, w, _ = _inputs(cs, cd, n)
    wp = torch.empty(sparse._pack_floats(w.numel(), 2), dtype=torch.float32, device=DEV)
    L.call('u3d_weight_pack_x3', L.ptr(w), L.ptr(wp), cd, 27, cs, 0, L.stream())
    tiles = rb.tile_starts('out', 64)
    head = (2, L.ptr(x), n, L.ptr(wp), L.ptr(rb.pair_in), L.ptr(rb.pair_out), L.ptr(tiles), 27, rb.cap, cs, cd, n, 64, 1, None, None)
    sc, sf = _affine(cd, 0)
    raw, act, part = _out_buffer(n, cd + 32), _out_buffer(n, cd + 32), _out_buffer(3, 2 * cd)

    def call(bn_partial=None, raw_ptr=raw.data_ptr(), ld=cd + 32, col=32, n_act=1, act_ld=cd + 32, act_col=32):
        ep = L.ConvEpilogue()
        ep.raw, ep.raw_ld, ep.raw_col, ep.n_act = raw_ptr, ld, col, n_act
        for j in range(min(n_act, 2)):
            ep.act[j], ep.act_ld[j], ep.act_col[j], ep.scale[j], ep.shift[j] = act.data_ptr(), act_ld, act_col, sc.data_ptr(), sf.data_ptr()
        return lib.u3d_spconv_gmm_ep(*head, bn_partial, ctypes.byref(ep), 0.0, L.stream())
    assert call(ld=cd - 4, col=0) == -1
    assert call(act_ld=cd - 4, act_col=0) == -1
    assert call(ld=cd + 34) == -1 and call(col=30) == -1 and call(act_ld=cd + 34) == -1 and call(act_col=34) == -1
    assert call(ld=cd + 16) == -1                      # column block past the row
    assert call(n_act=3) == -3 and b'at most two' in lib.u3d_last_error()
    assert call(raw_ptr=None, n_act=0) == -1 and b'no output' in lib.u3d_last_error()
    assert call(bn_partial=part.data_ptr()) == -3 and b'exclude each other' in lib.u3d_last_error()
    torch.cuda.synchronize()
    for t in (raw, act, part):
        assert bool((t.view(torch.int32) == PATTERN).all())
    assert call() == 0                                 # the same arguments, valid: launches and writes
    torch.cuda.synchronize()
    assert not bool((raw.view(torch.int32)[:n, 32:] == PATTERN).any())


# ------------------------------------------------------------------------------------------------------------------ module level
def _model(seed=5):
    from unidet3d_amd.sparse import SparseBatchNorm, SparseSequential, SubMConv3d
    from unidet3d_amd.spconv_unet import SpConvUNet
    front = SparseSequential(SubMConv3d(6, 32, 3, padding=1, indice_key='subm1'))
    unet = SpConvUNet([32, 64, 96], block_reps=2, return_blocks=True)
    back = SparseSequential(SparseBatchNorm(32), nn.ReLU())
    g = torch.Generator().manual_seed(seed)
    net = nn.ModuleList([front, unet, back])
    for m in net.modules():
        if isinstance(m, SparseBatchNorm):
            m.weight.data = torch.randn(m.weight.shape, generator=g) * 0.5 + 1.0
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.2
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.5 + 0.5)
        elif getattr(m, 'weight', None) is not None:
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (2.0 / (27 * m.weight.shape[-1])) ** 0.5
    return net.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _scenes():
    """(two synthetic scenes of about 3 000 voxels each, the single-voxel scene) as (features, coordinates, shape, batch size)"""
    from unidet3d_amd import ops
    from unidet3d_amd.synthetic import make_scene
    vb = ops.voxelize([torch.from_numpy(make_scene(51 + i, n_points=4_000).points).to(DEV) for i in range(2)], 0.05, 128)
    print('voxels of the two scenes:', vb.coords.shape[0])
    one = (torch.randn(1, 6, generator=torch.Generator().manual_seed(1)).to(DEV), torch.tensor([[0, 3, 4, 5]], dtype=torch.int32, device=DEV), (8, 8, 8), 1)
    return (vb.feats, vb.coords, tuple(vb.spatial_shape), 2), one


def _forward(net, scene, announce=True):
    from unidet3d_amd.sparse import SparseConvTensor
    from unidet3d_amd.spconv_unet import begin_fusion
    front, unet, back = net
    feats, coords, shape, B = scene
    x = SparseConvTensor(feats, coords, shape, B)
    if announce:
        begin_fusion(x, unet, front, back)
    y, blocks = unet(front(x))
    return [back(y).features] + [b.features for b in blocks]


def _record(monkeypatch):
    from unidet3d_amd import _lib as L
    log, real = [], L.call

    def call(name, *args):
        log.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, 'call', call)
    return log


class _TorchProxy:
    """``torch`` as spconv_unet sees it, counting its torch.cat calls"""

    def __init__(self):
        self.cats = 0

    def __getattr__(self, k):
        return getattr(torch, k)

    def cat(self, *a, **k):
        self.cats += 1
        return torch.cat(*a, **k)


MODES = ['bf16x3', 'mfma', 'bf16', 'bf16+rows']


def _mode(stack, name):
    from unidet3d_amd import precision as P
    if name in ('bf16x3', 'mfma'):
        stack.enter_context(P.operands('fp32'))
        stack.enter_context(P.fp32_math(name))
    else:
        stack.enter_context(P.operands('bf16'))
        stack.enter_context(P.bf16_rows_mode(name == 'bf16+rows'))


@pytest.mark.parametrize('mode', MODES)
def test_unet_fused_equals_unfused_bit_for_bit(mode, monkeypatch):
    import contextlib
    from unidet3d_amd import sparse, spconv_unet
    net = _model()
    plan = spconv_unet.fusion_plan(net[1], net[0], net[2])
    unfused_norms = sum(not e.fused for e in plan.norms.values())
    assert unfused_norms == 0 and len(plan.norms) == 25
    proxy = _TorchProxy()
    monkeypatch.setattr(spconv_unet, 'torch', proxy)
    log = _record(monkeypatch)
    with contextlib.ExitStack() as stack, torch.no_grad():
        _mode(stack, mode)
        for scene in _scenes():
            with sparse.fused_inference(False):
                del log[:]
                proxy.cats = 0
                want = _forward(net, scene)
                assert log.count('u3d_bn_apply') == 25 and 'u3d_spconv_gmm_ep' not in log and proxy.cats == 2
            with sparse.fused_inference(True):
                del log[:]
                proxy.cats = 0
                got = _forward(net, scene)
                assert log.count('u3d_bn_apply') == unfused_norms, log.count('u3d_bn_apply')
                assert log.count('u3d_spconv_gmm_ep') == len(plan.convs) == 25
                assert proxy.cats == 0
            assert len(got) == len(want) == 4
            for i, (a, b) in enumerate(zip(got, want)):
                assert torch.isfinite(b).all() and _same(a, b), f'{mode}: output {i} differs, max |diff| {float((a - b).abs().max())}'
            # a U-Net whose neighbours nobody announced: its first norm and the output layer's norm launch, everything else is fused
            with sparse.fused_inference(True):
                del log[:]
                got = _forward(net, scene, announce=False)
                assert log.count('u3d_bn_apply') == 2 and proxy.cats == 0
            for i, (a, b) in enumerate(zip(got, want)):
                assert _same(a, b), f'{mode}: unannounced, output {i} differs'


def test_grad_mode_and_training_mode_keep_todays_launch_sequence(monkeypatch):
    from unidet3d_amd import sparse
    base = _model()
    scene = _scenes()[0]
    log = _record(monkeypatch)

    def names(net, on, grad):
        with sparse.fused_inference(on), (torch.enable_grad() if grad else torch.no_grad()):
            del log[:]
            _forward(net, scene)
            return list(log)
    for train, grad in ((False, True), (True, True), (True, False)):
        seqs = []
        for on in (False, True):
            net = copy.deepcopy(base)
            net.train(train)
            seqs.append(names(net, on, grad))
        assert seqs[0] == seqs[1] and 'u3d_spconv_gmm_ep' not in seqs[1], (train, grad)
    assert 'u3d_spconv_gmm_ep' in names(copy.deepcopy(base), True, False)


def test_running_statistics_updated_in_place_reach_the_next_fused_forward():
    from unidet3d_amd import sparse
    net = _model()
    scene = _scenes()[0]
    norms = [m for m in net.modules() if isinstance(m, sparse.SparseBatchNorm)]
    with torch.no_grad():
        with sparse.fused_inference(True):
            before = _forward(net, scene)
        for m in (norms[1], norms[7], norms[-1]):
            m.running_mean.add_(0.25)                         # in place: ``_version`` moves, the cached (scale, shift) is stale
        with sparse.fused_inference(True):
            after = _forward(net, scene)
        for m in norms:
            m.invalidate_affine()                             # the reference does not rely on the cache's key
        with sparse.fused_inference(False):
            want = _forward(net, scene)
    assert not _same(before[0], after[0])
    for i, (a, b) in enumerate(zip(after, want)):
        assert _same(a, b), f'output {i}'


def test_a_training_forward_between_two_inference_forwards_is_seen():
    """the statistics kernels update running_mean / running_var in place WITHOUT a ``_version`` bump: the training-mode forward itself
    drops the cached (scale, shift), so the inference forward after it normalises with the new statistics"""
    from unidet3d_amd import sparse
    net = _model()
    scene = _scenes()[0]
    norms = [m for m in net.modules() if isinstance(m, sparse.SparseBatchNorm)]
    with sparse.fused_inference(True):
        with torch.no_grad():
            before = _forward(net, scene)
        rm = norms[3].running_mean.clone()
        net.train()
        _forward(net, scene)
        net.eval()
        assert not torch.equal(rm, norms[3].running_mean)
        with torch.no_grad():
            after = _forward(net, scene)
    for m in norms:
        m.invalidate_affine()
    with torch.no_grad(), sparse.fused_inference(False):
        want = _forward(net, scene)
    assert not _same(before[0], after[0])
    for i, (a, b) in enumerate(zip(after, want)):
        assert _same(a, b), f'output {i}'


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_predict_is_identical_with_the_toggle_on_and_off(monkeypatch):
    import unidet3d_amd  # noqa: F401
    from _detw import fill_state_dict
    from unidet3d_amd import sparse
    from unidet3d_amd.config import build_model, scannet_model_cfg
    from unidet3d_amd.data import make_batch_inputs
    from unidet3d_amd.synthetic import make_scene
    cfg = scannet_model_cfg()
    cfg['decoder']['num_layers'] = 2
    model = fill_state_dict(build_model(cfg), tag0=3000, scale=0.06).to(DEV).eval()
    model.voxel_size = 0.05
    scenes = [make_scene(s, n_points=20_000) for s in (11, 12)]
    log = _record(monkeypatch)
    res = {}
    for on in (False, True):
        inputs, samples = make_batch_inputs(scenes, DEV)
        del log[:]
        with torch.no_grad(), sparse.fused_inference(on):
            out = model.predict(inputs, samples)
        res[on] = [(o.pred_instances_3d.bboxes_3d.tensor, o.pred_instances_3d.scores_3d, o.pred_instances_3d.labels_3d) for o in out]
        if on:
            assert log.count('u3d_bn_apply') == 0 and log.count('u3d_spconv_gmm_ep') > 0
        else:
            assert log.count('u3d_bn_apply') > 0 and log.count('u3d_spconv_gmm_ep') == 0
    assert len(res[True]) == len(res[False]) == 2
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        assert len(b[1]) > 0
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and torch.equal(a[2], b[2]), f'scene {i}'
