"""bf16-row outputs of the convolution epilogue on the device, bit for bit: an activated output of u3d_spconv_gmm_ep
flagged U3D_EP_BF16_ROWS against ``to_shadow`` of the fp32 output of the same launch; the rounding domain; the U-Net's concat as two bf16
column blocks read back by u3d_spconv_gmm_bf16a; refusals; the U-Net and UniDet3D.predict under bf16 operands + bf16 rows with the fused
path on against off.  Every comparison is torch.equal on integer views; no tolerance anywhere."""
import contextlib

import pytest
import torch

import _fused_rows as fr
from _fused_rows import DEV

pytestmark = pytest.mark.gpu
RELU, ROWS = 1, 2                     # U3D_EP_RELU, U3D_EP_BF16_ROWS
SHAPES = {0: [(16, 32)], 1: [(32, 32), (64, 96), (192, 96)], 2: [(32, 32), (64, 96), (192, 96)], 3: [(32, 32), (64, 96), (192, 96)]}


@contextlib.contextmanager
def _kernel_form(form):
    from unidet3d_amd import _lib as L
    prev = L.lib().u3d_conv_kernel(form)
    try:
        yield
    finally:
        L.lib().u3d_conv_kernel(prev)


def test_flag_constants_match_the_library():
    from unidet3d_amd import _lib as L
    assert (L.EP_RELU, L.EP_BF16_ROWS) == (RELU, ROWS) and L.lib().u3d_spconv_gmm_ep_formats() == 3


# ---------------------------------------------------------------------------------------------------------------- 1. the epilogue
@pytest.mark.parametrize('form', [2, 0])
@pytest.mark.parametrize('fmt', [0, 1, 2, 3])
def test_bf16_rows_equal_the_shadow_of_the_fp32_output(fmt, form):
    """slot 0 = fp32, slot 1 = bf16 rows of the same norm, in buffers wider (ld = Cd + 32, first column 32) and longer than written"""
    from unidet3d_amd import sparse
    with _kernel_form(form):
        for cs, cd in SHAPES[fmt]:
            sc, sf = fr.affine(cd + 32)
            for n in fr.NS:
                add = fr.inputs(cs, cd, n)[2]
                for R, G in fr.PLANS:
                    args, ws, keep = fr.head(fmt, cs, cd, n, R, G)
                    for relu in (0, 1):
                        what = f'fmt {fmt} form {form} {cs}->{cd} n {n} R {R} G {G} relu {relu}'
                        # the launch without the bf16 slot: today's outputs
                        raw0, act0 = fr.out_f32(n, cd + 32), fr.out_f32(n, cd + 32)
                        fr.launch(args, ws, fr.descriptor((raw0, 32), [(act0, 32, sc, sf, relu)]), add)
                        raw, act, rows = fr.out_f32(n, cd + 32), fr.out_f32(n, cd + 32), fr.out_b16(n, cd + 32)
                        fr.launch(args, ws, fr.descriptor((raw, 32), [(act, 32, sc, sf, relu), (rows, 32, sc, sf, relu | ROWS)]), add)
                        assert fr.same(raw, raw0), what + ': raw moved'
                        assert fr.same(act, act0), what + ': fp32 output moved'
                        y = act[:n, 32:].contiguous()
                        assert bool(torch.isfinite(y).all())
                        fr.check_block(act, n, 32, y, what + ': fp32')
                        fr.check_block(rows, n, 32, sparse.to_shadow(y), what + ': bf16 rows')


# ---------------------------------------------------------------------------------------------------------------- 2. rows only
@pytest.mark.parametrize('fmt', [1, 3])
def test_rows_only_launch_is_valid_and_writes_the_same_bytes(fmt):
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse
    cs, cd = 64, 96
    sc, sf = fr.affine(cd + 32)
    for n in fr.NS:
        for R, G in fr.PLANS:
            args, ws, keep = fr.head(fmt, cs, cd, n, R, G)
            act = fr.out_f32(n, cd + 32)
            fr.launch(args, ws, fr.descriptor(None, [(act, 32, sc, sf, RELU)]))
            rows = fr.out_b16(n, cd + 32)
            fr.launch(args, ws, fr.descriptor(None, [(rows, 32, sc, sf, RELU | ROWS)]))          # raw = NULL, one bf16-row output
            fr.check_block(rows, n, 32, sparse.to_shadow(act[:n, 32:].contiguous()), f'fmt {fmt} n {n} R {R} G {G}')
            assert fr.launch(args, ws, fr.descriptor(None, []), check=False) == -1 and b'no output' in L.lib().u3d_last_error()


# ---------------------------------------------------------------------------------------------------------------- 3. rounding
def _crafted(cd):
    f = lambda bits: torch.tensor([bits], dtype=torch.int32).view(torch.float32).item()
    one = 0x3F800000
    vals = [
        1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,                      # ties: to even downwards (1.0) and upwards (1 + 2^-6)
        f(one + 0x8000 - 1), f(one + 0x8000 + 1),                  # one fp32 ulp either side of the first tie
        f(one + 0x18000 - 1), f(one + 0x18000 + 1),                # ... and of the second
        f(0x3FFFFFFF), f(0x3FFF8000),                              # round up into the next exponent (2.0): just below 2, and a tie
        f(0x00000001), f(0x007FFFFF), f(0x00008000), f(0x00018000), f(0x00012345),      # fp32 subnormals, two ties among them
        f(0x00800000),                                             # the smallest normal
        f(0x7F7F7FFF), f(0x7F7F8000), f(0x7F7FFFFF),               # the largest value that stays finite in bf16; the first that rounds to inf; FLT_MAX
        0.1, 3.14159274, 65504.0, 1e-30, 0.0,
    ]
    vals = vals + [-v for v in vals]
    t = torch.tensor(vals, dtype=torch.float32)
    return torch.cat((t, t * 0.75, t * 0.375))[:cd]


def test_rounding_is_torchs_round_to_nearest_even_over_the_value_domain():
    cs, cd, n, fmt = 32, 96, 129, 1
    shift = _crafted(cd)
    shift_d, scale_d = shift.to(DEV), torch.zeros(cd, device=DEV)              # scale 0: the activated value is shift[c] itself
    for R, G in ((32, 1), (32, 3)):                                            # the kernel tail and the reduce kernel
        args, ws, keep = fr.head(fmt, cs, cd, n, R, G)
        for relu in (0, 1):
            act, rows = fr.out_f32(n, cd), fr.out_b16(n, cd)
            fr.launch(args, ws, fr.descriptor(None, [(act, 0, scale_d, shift_d, relu), (rows, 0, scale_d, shift_d, relu | ROWS)]))
            y = act[:n].cpu()
            want = torch.clamp_min(shift, 0.0) if relu else shift
            assert torch.equal(y, want.expand(n, cd)), 'the activated fp32 values are not the crafted ones'
            # the crafted set is not vacuous: ties (low half exactly 0x8000), and values whose rounding changes the exponent
            yb = y[0].view(torch.int32)
            ties = (yb & 0xFFFF) == 0x8000
            rounded = y[0].to(torch.bfloat16)
            grows = (rounded.float().view(torch.int32) >> 23) != (yb >> 23)
            assert int(ties.sum()) >= (3 if relu else 6) and int(grows.sum()) >= (3 if relu else 6)
            assert bool(torch.isinf(rounded).any()) and bool(torch.isfinite(y).all())      # finite in fp32, inf once rounded
            if not relu:
                assert bool((y[0] < 0).any())
            # expected: torch's conversion of the fp32 activated values, in fragment order
            got = rows[:n].cpu()
            frag = y.reshape(n, cd // 32, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(n, cd).to(torch.bfloat16)
            assert fr.same(got, frag), f'R {R} G {G} relu {relu}'
            assert fr.untouched(rows[n:]) and fr.untouched(act[n:])


# ---------------------------------------------------------------------------------------------------------------- 4. concat
@pytest.mark.parametrize('c', [32, 96])
def test_two_bf16_column_blocks_feed_the_bf16_row_kernel_like_the_fp32_concat(c):
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse
    sc, sf = fr.affine(2 * c, 1)
    for n in (129, 257):
        rb = fr.level(n)
        cat16, cat32 = fr.out_b16(n, 2 * c), fr.out_f32(n, 2 * c)
        for blk in (0, 1):                                            # the two producers: c -> c convolutions with their own inputs and weights
            args, ws, keep = fr.head(1, c, c, n, 64, 1, seed=blk)
            fr.launch(args, ws, fr.descriptor(None, [(cat32, blk * c, sc, sf, RELU)]))               # today's epilogue
            fr.launch(args, ws, fr.descriptor(None, [(cat16, blk * c, sc, sf, RELU | ROWS)]))
        want16 = sparse.to_shadow(cat32[:n].contiguous())
        fr.check_block(cat16, n, 0, want16, f'c {c} n {n}: the bf16 concat')
        # the reader: u3d_spconv_gmm_bf16a (2c -> c) on either buffer
        wp = fr.packed(1, 2 * c, c, n, seed=3)
        R, G = sparse._plan(2 * c, c, 27, n, True)
        tiles = rb.tile_starts('out', R)
        ws = torch.empty(G * n * c, dtype=torch.float32, device=DEV) if G > 1 else None
        outs = []
        for src in (cat16[:n].contiguous(), want16):
            dst = fr.out_f32(n, c)
            L.call('u3d_spconv_gmm_bf16a', L.ptr(src), n, L.ptr(wp), L.ptr(rb.pair_in), L.ptr(rb.pair_out), L.ptr(tiles), 27, rb.cap, 2 * c, c,
                   n, R, G, None, L.ptr(dst), L.ptr(ws), 0.0, L.stream())
            outs.append(dst)
        assert bool(torch.isfinite(outs[1][:n]).all()) and fr.same(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_every_buffer_untouched():
    from unidet3d_amd import _lib as L
    n, cs, cd = 129, 32, 32
    args, ws, keep = fr.head(1, cs, cd, n, 64, 1)
    sc, sf = fr.affine(cd + 64)
    raw, act, rows = fr.out_f32(n, cd + 32), fr.out_f32(n, cd + 32), fr.out_b16(n, cd + 64)

    def call(ld=cd + 64, col=32, flags=RELU | ROWS):
        ep = fr.descriptor((raw, 32), [(act, 32, sc, sf, RELU), (rows, col, sc, sf, flags)])
        ep.act_ld[1] = ld
        return fr.launch(args, ws, ep, check=False)
    err = L.lib().u3d_last_error
    assert call(ld=cd + 48) == -1 and b'bf16 rows' in err()         # leading dimension: a multiple of 4, not of 32
    assert call(col=16) == -1 and call(col=48) == -1               # first column likewise
    assert call(ld=cd + 32, col=64) == -1                          # the block runs past the row
    assert call(ld=cd, col=32) == -1
    assert call(flags=RELU | ROWS | 4) == -3 and b'flag word' in err()
    assert call(flags=8) == -3
    torch.cuda.synchronize()
    assert fr.untouched(raw) and fr.untouched(act) and fr.untouched(rows)
    assert call() == 0                                             # the same arguments, valid: launches and writes
    torch.cuda.synchronize()
    assert not bool((fr.bits(rows)[:n, 32:32 + cd] == fr.PATTERN16).any()) and not bool((fr.bits(raw)[:n, 32:] == fr.PATTERN).any())
    assert fr.untouched(rows[:, :32]) and fr.untouched(rows[:, 32 + cd:]) and fr.untouched(rows[n:])


# ---------------------------------------------------------------------------------------------------------------- 6. module level
def test_unet_under_bf16_rows_fused_equals_unfused_and_reads_rows_only(monkeypatch):
    from unidet3d_amd import sparse, spconv_unet
    net = fr.model()
    plan = spconv_unet.fusion_plan(net[1], net[0], net[2])
    capable = {n for n in plan.norms if plan.rows_capable(n)}
    assert len(plan.norms) == 25 and len(capable) == 24 and net[2][0] not in capable
    rec = fr.Recorder(monkeypatch)
    with contextlib.ExitStack() as stack, torch.no_grad():
        fr.enter_mode(stack, 'bf16+rows')
        for scene in fr.scenes():
            with sparse.fused_inference(False):
                rec.clear()
                want = fr.forward(net, scene)
                assert rec.names.count('u3d_bn_apply') == 25 and not rec.eps
            with sparse.fused_inference(True):
                rec.clear()
                sparse.SHADOW_STATS.update(hit=0, miss=0)
                got = fr.forward(net, scene)
                stats = dict(sparse.SHADOW_STATS)
            assert rec.names.count('u3d_bn_apply') == 0 and rec.names.count('u3d_spconv_gmm_ep') == len(rec.eps) == len(plan.convs) == 25
            assert len(got) == len(want) == 4
            for i, (a, b) in enumerate(zip(got, want)):
                assert bool(torch.isfinite(b).all()) and fr.same(a, b), f'output {i} differs'
            wide = [e for e in rec.eps if e[2] % 32 == 0]
            assert len(wide) == 24 and all(e[1] == 3 for e in wide), [e[1] for e in rec.eps]          # every 32-multiple source: bf16 rows
            assert [e[1] for e in rec.eps if e[2] % 32] == [0]                                        # the 6 (16) -> 32 input convolution: fp32
            assert stats == {'hit': len(wide), 'miss': 0}
            # descriptors: each rows-capable norm is written as bf16 rows and has no fp32 buffer anywhere; the sink is fp32
            written = {}
            for layer, _, _, cout, d in rec.eps:
                cp = plan.convs[layer]
                assert d['n_act'] == len(cp.acts)
                for j, (norm, relu, where) in enumerate(cp.acts):
                    assert bool(d['flags'][j] & RELU) == relu
                    written.setdefault(norm, []).append((bool(d['flags'][j] & ROWS), d['act'][j], d['ld'][j], d['col'][j]))
            assert set(written) == set(plan.norms)
            for norm, outs in written.items():
                assert all(o[0] for o in outs) if norm in capable else not any(o[0] for o in outs), plan.name(norm)
                assert len(outs) == len(plan.norms[norm].producers)
                assert len({o[1] for o in outs}) == 1 and all(o[2] == norm.num_features for o in outs)      # one buffer per norm
                assert sorted(o[3] for o in outs) == sorted(lo for _, lo, _ in plan.norms[norm].producers)


@pytest.mark.parametrize('mode', ['bf16x3', 'mfma', 'bf16'])
def test_no_flag_is_set_in_any_other_mode(mode, monkeypatch):
    from unidet3d_amd import sparse
    net = fr.model()
    rec = fr.Recorder(monkeypatch)
    with contextlib.ExitStack() as stack, torch.no_grad(), sparse.fused_inference(True):
        fr.enter_mode(stack, mode)
        fr.forward(net, fr.scenes()[0])
    assert len(rec.eps) == 25
    assert all(not (f & ROWS) for e in rec.eps for f in e[4]['flags'][:e[4]['n_act']])
    assert all(e[1] != 3 for e in rec.eps)


# ---------------------------------------------------------------------------------------------------------------- 7. other readers
def test_reading_a_rows_only_tensor_as_values_raises():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import dense, sparse
    n = 129
    rb = fr.level(n)
    t = sparse.rows_only(sparse.to_shadow(fr.inputs(32, 32, n)[0]))
    w = fr.inputs(32, 32, n)[1]
    with torch.no_grad():
        with pytest.raises(L.U3DError, match='bf16 rows only'):
            sparse.SparseBatchNorm(32).to(DEV).eval()(t, relu=True)
        with pytest.raises(L.U3DError, match='bf16 rows only'):
            sparse.sparse_conv(t, w, rb)
        with pytest.raises(L.U3DError, match='bf16 rows only'):
            dense.linear(t, torch.zeros(32, 32, device=DEV))
        # ... and the fused launch itself, where it would not gather bf16 rows (fp32 operands)
        from unidet3d_amd import precision as P
        y = torch.empty(n, 32, device=DEV)
        with P.operands('fp32'), pytest.raises(L.U3DError, match='bf16 rows only'):
            sparse.sparse_conv_fused(t, w.reshape(32, 3, 3, 3, 32), rb, 'fwd', None, (y, 0), [])


# ---------------------------------------------------------------------------------------------------------------- 8. end to end
def test_predict_under_bf16_rows_is_identical_for_every_toggle_state(monkeypatch):
    import unidet3d_amd  # noqa: F401
    from _detw import fill_state_dict
    from unidet3d_amd import precision as P
    from unidet3d_amd import sparse
    from unidet3d_amd.config import build_model, scannet_model_cfg
    from unidet3d_amd.data import make_batch_inputs
    from unidet3d_amd.synthetic import make_scene
    cfg = scannet_model_cfg()
    cfg['decoder']['num_layers'] = 2
    model = fill_state_dict(build_model(cfg), tag0=3000, scale=0.06).to(DEV).eval()
    model.voxel_size = 0.05
    scenes = [make_scene(s, n_points=20_000) for s in (11, 12)]
    rec = fr.Recorder(monkeypatch)
    res = {}
    with P.operands('bf16'), P.bf16_rows_mode(True):
        for on in (False, True, None):
            inputs, samples = make_batch_inputs(scenes, DEV)
            rec.clear()
            with torch.no_grad(), sparse.fused_inference(on):
                if on is None:       # the default DESIGN.md 4.28 decided: under bf16 rows the unfused sequence; the fused one is opt-in
                    assert not sparse.fused_inference_on()
                out = model.predict(inputs, samples)
            res[on] = [(o.pred_instances_3d.bboxes_3d.tensor, o.pred_instances_3d.scores_3d, o.pred_instances_3d.labels_3d) for o in out]
            if on:
                assert rec.names.count('u3d_bn_apply') == 0 and len(rec.eps) > 0
                assert all(e[1] == 3 for e in rec.eps if e[2] % 32 == 0)
                assert sum(bool(f & ROWS) for e in rec.eps for f in e[4]['flags'][:e[4]['n_act']]) > 0
            else:
                assert rec.names.count('u3d_bn_apply') > 0 and not rec.eps
    for on in (True, None):
        assert len(res[on]) == len(res[False]) == 2
        for i, (a, b) in enumerate(zip(res[on], res[False])):
            assert len(b[1]) > 0
            assert fr.same(a[0], b[0]) and fr.same(a[1], b[1]) and torch.equal(a[2], b[2]), f'toggle {on}: scene {i}'
