"""Helpers of tests/test_gpu_fused_rows.py: small SubM levels, pattern-filled output buffers of both element types, the descriptor of
u3d_spconv_gmm_ep, the [32, 64, 96] net and its scenes, and a recorder of the C-ABI calls that keeps a copy of every epilogue descriptor."""
import ctypes
import functools

import torch
from torch import nn

import _conv_geometry as cg

DEV = torch.device('cuda:0')
PATTERN = 0x7FC0BEEF                  # fp32 buffers: a NaN wherever the launch must not write
PATTERN16 = 0x7FC5                    # bf16 buffers likewise (never a rounded finite value of the tests: a NaN)
GUARD = 4                             # rows behind the last one
NS = (1, 129, 257)                    # one row, 2 * 64 + 1, 4 * 64 + 1
PLANS = ((32, 1), (64, 1), (32, 3), (32, 9))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def level(n):
    """SubM rulebook (27 offsets) of a strip of n voxels, two wide: neighbours along two axes, nine offsets with pairs"""
    from unidet3d_amd import sparse
    _, B, shape, coords = cg._case(f'rows_strip_{n}', 1, (n // 2 + 5, 4, 3), [(0, 2 + i // 2, 1 + i % 2, 1) for i in range(n)])
    ix = sparse.OccupancyIndex.from_coords(coords.to(DEV), B, shape)
    assert ix.count() == n
    rows = ix.coords(n)
    assert torch.equal(rows.cpu(), coords)
    return sparse.build_subm_rulebook(rows, ix)


@functools.lru_cache(maxsize=None)
def inputs(cs, cd, n, seed=0):
    g = torch.Generator().manual_seed(cs * 1000 + cd + n + 7919 * seed)
    x = torch.randn(n, cs, generator=g).to(DEV)
    w = (torch.randn(cd, 27, cs, generator=g) * 0.1).to(DEV)
    add = torch.randn(n, cd, generator=g).to(DEV)
    return x, w, add


@functools.lru_cache(maxsize=None)
def affine(width, j=0):
    """scale / shift over ``width`` columns: negative scales, exact zeros, and -0.0 / +0.0 in front of the ReLU"""
    g = torch.Generator().manual_seed(177 + j + width)
    scale, shift = torch.randn(width, generator=g), torch.randn(width, generator=g)
    scale[1::8] = 0.0
    shift[1::16] = -0.0
    shift[9::16] = 0.0
    scale[2::8] = -1.0
    scale[4::8] = -scale[4::8].abs()
    return scale.to(DEV), shift.to(DEV)


@functools.lru_cache(maxsize=None)
def packed(fmt, cs, cd, n, seed=0):
    """the weights of ``inputs`` packed for operand format ``fmt`` (fmt 3 gathers bf16 rows against the bf16 pack)"""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse
    w = inputs(cs, cd, n, seed)[1]
    pf = 1 if fmt == 3 else fmt
    wp = torch.empty(sparse._pack_floats(w.numel(), pf), dtype=torch.float32, device=DEV)
    L.call(sparse._GMM_ENTRY[pf][0], L.ptr(w), L.ptr(wp), cd, 27, cs, 0, L.stream())
    return wp


def out_f32(n, ld):
    return torch.full((n + GUARD, ld), PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)


def out_b16(n, ld):
    return torch.full((n + GUARD, ld), PATTERN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def untouched(buf):
    return bool((bits(buf) == (PATTERN16 if buf.dtype == torch.bfloat16 else PATTERN)).all())


def check_block(buf, n, col, want, what):
    """rows [0, n), columns [col, col + width of want) of ``buf`` hold ``want`` bit for bit; everything else still holds the pattern"""
    b, w = bits(buf), bits(want)
    pat = PATTERN16 if buf.dtype == torch.bfloat16 else PATTERN
    cd = want.shape[1]
    assert buf.dtype == want.dtype
    block = (b[:n, col:col + cd] == w).all()
    beside = (b[:n, :col] == pat).all() & (b[:n, col + cd:] == pat).all()
    guard = (b[n:] == pat).all()
    ok = torch.stack((block, beside, guard)).tolist()              # one read-back per buffer
    assert ok[0], f'{what}: differs from the reference'
    assert ok[1], f'{what}: wrote outside its column block'
    assert ok[2], f'{what}: wrote past the last row'


def descriptor(raw=None, acts=()):
    """u3d_conv_epilogue: ``raw`` = (buffer, first column) or None; ``acts`` = up to two (buffer, first column, scale, shift, flags) --
    the leading dimension is the buffer's, in its own elements"""
    from unidet3d_amd import _lib as L
    ep = L.ConvEpilogue()
    if raw is not None:
        ep.raw, ep.raw_ld, ep.raw_col = raw[0].data_ptr(), raw[0].shape[1], raw[1]
    ep.n_act = len(acts)
    for j, (buf, col, sc, sf, flags) in enumerate(acts):
        ep.act[j], ep.act_ld[j], ep.act_col[j] = buf.data_ptr(), buf.shape[1], col
        ep.scale[j], ep.shift[j], ep.relu[j] = sc.data_ptr(), sf.data_ptr(), flags
    return ep


def head(fmt, cs, cd, n, R, G, seed=0):
    """(arguments of u3d_spconv_gmm_ep up to k_groups, tensors to keep alive): fmt 3 gathers ``to_shadow`` of the fp32 source"""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse
    rb = level(n)
    x = inputs(cs, cd, n, seed)[0]
    src = sparse.to_shadow(x) if fmt == 3 else x
    wp = packed(fmt, cs, cd, n, seed)
    tiles = rb.tile_starts('out', R)
    ws = torch.empty(G * n * cd, dtype=torch.float32, device=DEV) if G > 1 else None
    args = (fmt, L.ptr(src), n, L.ptr(wp), L.ptr(rb.pair_in), L.ptr(rb.pair_out), L.ptr(tiles), 27, rb.cap, cs, cd, n, R, G)
    return args, ws, (src, wp, tiles, rb)


def launch(args, ws, ep, addend=None, check=True):
    """u3d_spconv_gmm_ep; returns the status code (``check``: raise on any but 0)"""
    from unidet3d_amd import _lib as L
    rc = L.lib().u3d_spconv_gmm_ep(*args, L.ptr(addend), L.ptr(ws), None, ctypes.byref(ep), 0.0, L.stream())
    if check and rc != 0:
        raise L.U3DError(f'u3d_spconv_gmm_ep failed with code {rc}: {L.lib().u3d_last_error().decode()}')
    return rc


# ------------------------------------------------------------------------------------------------------------------ module level
def model(seed=5):
    """front convolution 6 -> 32, SpConvUNet([32, 64, 96]) with two blocks per stage, output norm + ReLU; random norms and weights"""
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
def scenes():
    """(two synthetic scenes of about 3 000 voxels together with a batch index each, the single-voxel scene)"""
    from unidet3d_amd import ops
    from unidet3d_amd.synthetic import make_scene
    vb = ops.voxelize([torch.from_numpy(make_scene(61 + i, n_points=4_000).points).to(DEV) for i in range(2)], 0.05, 128)
    print('voxels of the two scenes:', vb.coords.shape[0])
    one = (torch.randn(1, 6, generator=torch.Generator().manual_seed(2)).to(DEV), torch.tensor([[0, 3, 4, 5]], dtype=torch.int32, device=DEV), (8, 8, 8), 1)
    return (vb.feats, vb.coords, tuple(vb.spatial_shape), 2), one


def forward(net, scene):
    from unidet3d_amd.sparse import SparseConvTensor
    from unidet3d_amd.spconv_unet import begin_fusion
    front, unet, back = net
    feats, coords, shape, B = scene
    x = SparseConvTensor(feats, coords, shape, B)
    begin_fusion(x, unet, front, back)
    y, blocks = unet(front(x))
    return [back(y).features] + [b.features for b in blocks]


class Recorder:
    """``_lib.call`` with a log of the entry-point names; of every u3d_spconv_gmm_ep call also (layer, fmt, cin, cout, descriptor as a dict):
    the layer comes from ``FusionRun.conv``, which makes exactly one such call for a level with rows."""

    def __init__(self, monkeypatch):
        from unidet3d_amd import _lib as L
        from unidet3d_amd import sparse
        self.names, self.eps, self._layer = [], [], None
        real_call, real_conv = L.call, sparse.FusionRun.conv

        def call(name, *args):
            self.names.append(name)
            if name == 'u3d_spconv_gmm_ep':
                e = args[17]._obj
                d = dict(raw=e.raw, n_act=e.n_act, act=list(e.act), ld=list(e.act_ld), col=list(e.act_col), flags=list(e.relu))
                self.eps.append((self._layer, args[0], args[9], args[10], d))
            return real_call(name, *args)

        def conv(run, layer, *a, **k):
            self._layer = layer
            try:
                return real_conv(run, layer, *a, **k)
            finally:
                self._layer = None
        monkeypatch.setattr(L, 'call', call)
        monkeypatch.setattr(sparse.FusionRun, 'conv', conv)

    def clear(self):
        del self.names[:], self.eps[:]


MODES = ['bf16x3', 'mfma', 'bf16', 'bf16+rows']


def enter_mode(stack, name):
    from unidet3d_amd import precision as P
    if name in ('bf16x3', 'mfma'):
        stack.enter_context(P.operands('fp32'))
        stack.enter_context(P.fp32_math(name))
    else:
        stack.enter_context(P.operands('bf16'))
        stack.enter_context(P.bf16_rows_mode(name == 'bf16+rows'))
