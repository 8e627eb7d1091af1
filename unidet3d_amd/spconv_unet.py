"""Sparse-voxel residual U-Net backbone over the gfx950 kernels.

Drop-in for the reference's ``SpConvUNet`` (unidet3d/spconv_unet.py:94-240): same registry
name, constructor arguments (:108-115), forward signature / return types (:205-240) and
``state_dict`` keys (blocks.block{i}.conv_branch.{0,2,3,5}, .i_branch.0, conv.{0,2}, u.*,
deconv.{0,2}, blocks_tail.*), so OneFormer3D / UniDet3D checkpoints load unchanged.

Differences are all below the module surface: convolutions, rulebooks and batch-norm run as
HIP kernels through include/u3d.h, BN+ReLU is one fused kernel, and the residual add of
``ResidualBlock.forward`` (:88-89) is folded into the accumulator init of the block's last
convolution.  A norm that does not sit in a ``SparseSequential`` of its own (the two of a block, the one the U-Net's skip
connection leaves next to) runs through ``SparseBatchNorm.on``, which also says that a convolution reads the result; what a
convolution leaves for the norm behind it travels on the feature tensor (``sparse.stats_of``), not through these classes.
In inference (``eval()`` under ``torch.no_grad()``) the convolutions write the norms behind them and the concat buffers themselves:
``fusion_plan`` says which convolution writes which norm, ``begin_fusion`` starts such a pass.
"""
from __future__ import annotations

import functools
from collections import OrderedDict
from types import SimpleNamespace

import torch
from torch import nn

from . import sparse as S
from ._lib import U3DError
from .registry import MODELS
from .sparse import (SparseBatchNorm, SparseConv3d, SparseConvTensor, SparseInverseConv3d, SparseModule,
                     SparseSequential, SubMConv3d)


def _norm_factory(sync: bool):
    return functools.partial(SparseBatchNorm, eps=1e-4, momentum=0.1, sync=sync)


class ResidualBlock(SparseModule):
    """(BN, ReLU, SubM3) x 2 + identity / SubM1 skip  (spconv_unet.py:13-91)."""

    def __init__(self, in_channels, out_channels, norm_fn=None, indice_key=None, normalize_before=True):
        super().__init__()
        norm_fn = norm_fn or _norm_factory(False)
        self.normalize_before = normalize_before
        if in_channels == out_channels:
            self.i_branch = SparseSequential(nn.Identity())
        else:
            self.i_branch = SparseSequential(SubMConv3d(in_channels, out_channels, kernel_size=1, bias=False))
        conv1 = SubMConv3d(in_channels, out_channels, kernel_size=3, padding=1, bias=False, indice_key=indice_key)
        conv2 = SubMConv3d(out_channels, out_channels, kernel_size=3, padding=1, bias=False, indice_key=indice_key)
        if normalize_before:
            self.conv_branch = SparseSequential(norm_fn(in_channels), nn.ReLU(), conv1,
                                                norm_fn(out_channels), nn.ReLU(), conv2)
        else:
            self.conv_branch = SparseSequential(conv1, norm_fn(out_channels), nn.ReLU(),
                                                conv2, norm_fn(out_channels), nn.ReLU())

    def forward(self, input: SparseConvTensor) -> SparseConvTensor:
        if not self.normalize_before:
            skip = self.i_branch(input).features
            out = self.conv_branch(input)
            return out.replace_feature(out.features + skip)
        mods = list(self.conv_branch._modules.values())
        # the block input feeds the first norm AND the skip branch: the norm hands the input back as a second output so that
        # both gradients meet inside its backward kernel (no accumulation kernel)
        # (each norm finds the statistics of its input on that tensor, when a convolution's epilogue wrote them: sparse.stats_of)
        x, identity = mods[0].on(input, relu=True, skip=True, feeds_conv=True)
        skip = self.i_branch(identity).features
        x = mods[3].on(mods[2](x), relu=True, feeds_conv=True)
        return mods[5](x, addend=skip)          # conv + residual in one kernel


# ----------------------------------------------------------------------------------------
# fused inference: which convolution writes which norm
# ----------------------------------------------------------------------------------------
class FusionPlan:
    """Successor plan of a pre-activation U-Net for the fused inference path.  Pure bookkeeping (no tensors):
      ``norms``  SparseBatchNorm -> (name, relu, producers [(convolution, first column, end column)], fused, reader); no producers =
                 unfused: that norm runs u3d_bn_apply as always; reader = the planned convolution that is the ONLY reader of the norm's
                 result (None: somebody else reads it, or nobody the plan knows) -- ``rows_capable``;
      ``convs``  convolution -> (raw, acts): raw = 'own' (a tensor of its own), None (nobody reads the raw result) or (level, first
                 column) of that U-Net level's concat buffer; acts = up to two (norm, relu, None | (level, first column)): the activated
                 tensor of its own, or a column block of the level's activated concat buffer;
      ``cats``   U-Net level -> (width 2c, the first tail norm, relu): the two [n, 2c] buffers ``sparse.FusionRun`` allocates."""

    def __init__(self, root):
        self.root = root
        self.norms: OrderedDict = OrderedDict()
        self.convs = {}
        self.cats = {}
        self.names = {}

    def conv(self, m):
        if m not in self.convs:
            self.convs[m] = SimpleNamespace(raw='own', acts=[])
        return self.convs[m]

    def norm(self, m, relu, producers):
        assert m not in self.norms
        self.norms[m] = SimpleNamespace(relu=bool(relu), producers=list(producers), fused=bool(producers), reader=None)

    def read_by(self, norm, conv):
        """``conv`` (3x3x3 or strided: a pair-list launch) is the only reader of ``norm``'s result"""
        self.norms[norm].reader = conv

    def rows_capable(self, norm) -> bool:
        """The producers of ``norm`` may write its result as bf16 rows ONLY (``sparse.FusionRun``, precision.bf16_rows): every column of
        it comes from an epilogue, and the one reader is a planned convolution, which gathers rows."""
        e = self.norms.get(norm)
        return e is not None and e.fused and e.reader is not None

    def feed(self, conv, norm, relu, lo, hi, where=None):
        """``conv`` writes columns [lo, hi) of ``norm``'s result"""
        self.conv(conv).acts.append((norm, bool(relu), where))
        if norm in self.norms:
            self.norms[norm].producers.append((conv, lo, hi))
            self.norms[norm].fused = True
        else:
            self.norm(norm, relu, [(conv, lo, hi)])

    @property
    def modules(self):
        return [*self.convs, *self.norms]

    def name(self, m):
        return self.names.get(m, type(m).__name__)

    def describe(self):
        """{norm name: [(producer name, first column, end column)]} ([] = unfused) and {convolution name: (raw, [norm names])}"""
        norms = OrderedDict((self.name(n), [(self.name(c), lo, hi) for c, lo, hi in e.producers]) for n, e in self.norms.items())
        convs = {self.name(c): (e.raw if not isinstance(e.raw, tuple) else (self.name(e.raw[0]), e.raw[1]),
                                [(self.name(a[0]), None if a[2] is None else (self.name(a[2][0]), a[2][1])) for a in e.acts])
                 for c, e in self.convs.items()}
        return norms, convs


def _pre_act_block(b):
    """(norm1, conv1, norm2, conv2) of a pre-activation ResidualBlock, or None for anything else"""
    if type(b) is not ResidualBlock or not b.normalize_before:
        return None
    m = list(b.conv_branch._modules.values())
    ok = len(m) == 6 and all(isinstance(m[i], SparseBatchNorm) and isinstance(m[i + 1], nn.ReLU) and isinstance(m[i + 2], SubMConv3d)
                             and m[i + 2].kernel_size == 3 for i in (0, 3))
    return (m[0], m[2], m[3], m[5]) if ok else None


def _norm_relu_conv(seq, conv_type):
    m = list(seq._modules.values()) if isinstance(seq, SparseSequential) else []
    if len(m) == 3 and isinstance(m[0], SparseBatchNorm) and isinstance(m[1], nn.ReLU) and isinstance(m[2], conv_type):
        return m[0], m[2]
    return None


def _plan_level(plan, u, feed, sink):
    """``feed``: the convolution whose result is this level's input (None: unknown); ``sink``: (norm, relu) that reads this level's
    output (None: none known).  False where the level is not the pre-activation structure."""
    c = u.num_planes[0]

    def chain(blocks, prod, width):
        for b in blocks:
            parts = _pre_act_block(b)
            if parts is None:
                return False, None
            n1, conv1, n2, conv2 = parts
            if n1 in plan.norms:              # the first tail norm: planned with its two producers
                pass
            elif prod is None:
                plan.norm(n1, True, [])       # nobody known to produce its input: unfused
            else:
                plan.feed(prod, n1, True, 0, width)
            plan.read_by(n1, conv1)           # (the identity branch next to n1 reads the norm's INPUT)
            plan.conv(conv1).raw = None       # only norm 2 reads conv 1
            plan.feed(conv1, n2, True, 0, conv1.out_channels)
            plan.read_by(n2, conv2)
            plan.conv(conv2)
            prod, width = conv2, conv2.out_channels
        return True, prod

    blocks = list(u.blocks._modules.values())
    if not blocks:
        return False
    ok, prod = chain(blocks, feed, c)
    if not ok:
        return False
    if len(u.num_planes) > 1:
        down, up = _norm_relu_conv(u.conv, SparseConv3d), _norm_relu_conv(u.deconv, SparseInverseConv3d)
        tail = list(u.blocks_tail._modules.values())
        if down is None or up is None or not tail or _pre_act_block(tail[0]) is None:
            return False
        tnorm = _pre_act_block(tail[0])[0]
        plan.cats[u] = SimpleNamespace(width=2 * c, norm=tnorm, relu=True)
        # the last convolution of ``blocks``: raw -> concat columns [0, c); the norm in front of the down convolution; the first tail
        # norm's columns [0, c)
        plan.conv(prod).raw = (u, 0)
        plan.feed(prod, down[0], True, 0, c)
        plan.read_by(down[0], down[1])
        plan.feed(prod, tnorm, True, 0, c, (u, 0))
        if not _plan_level(plan, u.u, down[1], (up[0], True)):
            return False
        plan.read_by(up[0], up[1])            # the inner level's sink; the outermost one (``last_consumer``) has no planned reader
        # the inverse convolution: raw and the first tail norm, columns [c, 2c)
        plan.conv(up[1]).raw = (u, c)
        plan.feed(up[1], tnorm, True, c, 2 * c, (u, c))
        ok, prod = chain(tail, None, 2 * c)
        if not ok:
            return False
    if sink is not None:
        plan.feed(prod, sink[0], sink[1], 0, c)
    return True


def fusion_plan(unet, first_producer=None, last_consumer=None) -> FusionPlan:
    """Which convolution writes which norm on the fused inference path (pure Python, cached on ``unet``).
    ``first_producer``: the convolution (or a SparseSequential ending in one) whose result is the U-Net's input;
    ``last_consumer``: the norm that reads the U-Net's output -- a SparseSequential starting with it tells whether a ReLU follows, a bare
    SparseBatchNorm is taken without one.  U-Nets with ``normalize_before=False`` or foreign block classes get an EMPTY plan: the
    current path.  A convolution has at most two activated outputs; a norm that would be a third stays unfused (none in this U-Net)."""
    key = (id(first_producer), id(last_consumer), tuple(id(m) for m in unet.modules()))
    hit = unet.__dict__.get('_u3d_fusion_plan')
    if hit is not None and hit[0] == key:
        return hit[1]
    plan = FusionPlan(unet)
    feed = sink = None
    if isinstance(first_producer, SparseSequential) and len(first_producer):
        first_producer = first_producer[len(first_producer) - 1]
    if isinstance(first_producer, S._ConvBase) and first_producer.kernel_size != 1:
        feed = first_producer
        plan.names[feed] = '<first_producer>'
    if isinstance(last_consumer, SparseSequential) and len(last_consumer) and isinstance(last_consumer[0], SparseBatchNorm):
        sink = (last_consumer[0], len(last_consumer) > 1 and isinstance(last_consumer[1], nn.ReLU))
    elif isinstance(last_consumer, SparseBatchNorm):
        sink = (last_consumer, False)
    if sink is not None:
        plan.names[sink[0]] = '<last_consumer>'
    for name, m in unet.named_modules():
        plan.names[m] = name or '<unet>'
    # (a layer of the general geometry -- any kernel / stride / padding / dilation but the U-Net's own -- runs unfused: the whole plan steps aside)
    # (so does a layer with a bias and a transposed layer, planned or anywhere in the U-Net: no fused epilogue knows about either)
    held = [m for m in unet.modules() if isinstance(m, S._ConvBase)] + ([feed] if feed is not None else [])
    aside = any(m.bias is not None or isinstance(m, S.SparseConvTranspose3d) for m in held)
    if aside or not _plan_level(plan, unet, feed, sink) or any(getattr(c, 'general', False) for c in plan.convs):
        plan = FusionPlan(unet)
    for conv, e in plan.convs.items():          # at most two activated outputs per launch
        for norm, _, _ in e.acts[2:]:
            plan.norms[norm].producers, plan.norms[norm].fused = [], False
        del e.acts[2:]
    for cat in plan.cats.values():              # (a concat norm that lost a producer above cannot be assembled)
        assert plan.norms[cat.norm].fused and len(plan.norms[cat.norm].producers) == 2
    unet.__dict__['_u3d_fusion_plan'] = (key, plan)
    return plan


def begin_fusion(x: SparseConvTensor, unet, first_producer=None, last_consumer=None) -> bool:
    """Announce a forward pass over ``first_producer`` -> ``unet`` -> ``last_consumer`` on the sparse tensor ``x`` that enters it: where
    the fused inference path applies (``sparse.fusion_active`` for every planned layer) the pass's ``sparse.FusionRun`` is put into
    ``x.indice_dict``, where the layers find it; otherwise any earlier one is removed and every call is the current one."""
    x.indice_dict.pop(S.FUSE_KEY, None)
    if not S.fused_inference_on() or torch.is_grad_enabled():
        return False
    plan = fusion_plan(unet, first_producer, last_consumer)
    if not plan.convs or not S.fusion_active(*plan.modules, *plan.cats):
        return False
    x.indice_dict[S.FUSE_KEY] = S.FusionRun(plan)
    return True


POOL_WIDTHS = (32, 64, 128, 256)       # channel counts the superpoint pooling that reads the U-Net's output is built for (ops.superpoint_pool)


def check_num_planes(num_planes):
    """The channel contract of the sparse kernels, stated once for a whole U-Net: every plane a multiple of 32 up to 512, a plane above
    the deepest level at most 256 (its tail block reads the 2c-channel concatenation), and the first plane a pooling width."""
    planes = [int(c) for c in num_planes]
    ok = bool(planes) and all(c > 0 and c % 32 == 0 and c <= 512 for c in planes) and all(2 * c <= 512 for c in planes[:-1])
    if not ok or planes[0] not in POOL_WIDTHS:
        raise U3DError(f'SpConvUNet: num_planes={planes} is outside what the gfx950 kernels are built for: every entry must be a multiple '
                       f'of 32 (at most 512; at most 256 above the deepest level, whose tail blocks read 2c channels), and num_planes[0] '
                       f'must be one of {list(POOL_WIDTHS)}, the widths of the superpoint pooling behind the backbone')


@MODELS.register_module()
class SpConvUNet(nn.Module):
    def __init__(self, num_planes, use_sync_bn=True, block_reps=2, block=ResidualBlock, indice_key_id=1,
                 normalize_before=True, return_blocks=False, *, _inner=False):
        super().__init__()
        self._outer = not _inner
        self.return_blocks = return_blocks
        self.num_planes = list(num_planes)
        if not _inner:                     # the outermost U-Net checks the whole list (an inner level's first plane is not pooled)
            check_num_planes(self.num_planes)
        # The reference's recursion passes its norm_fn partial in the ``use_sync_bn`` slot
        # (spconv_unet.py:166-168), which is truthy: every inner level is SyncBatchNorm even when
        # the top level asked for BatchNorm1d.  Reproduced: inner levels always sync.
        norm_fn = _norm_factory(bool(use_sync_bn))
        if isinstance(block, str):
            area = ['residual', 'vgg', 'asym']
            assert block in area, f'block must be in {area}, but got {block}'
            if block != 'residual':
                raise NotImplementedError(f'block {block!r} is not defined by the reference either')
            block = ResidualBlock
        c0 = self.num_planes[0]
        self.blocks = SparseSequential(OrderedDict(
            (f'block{i}', block(c0, c0, norm_fn, normalize_before=normalize_before, indice_key=f'subm{indice_key_id}'))
            for i in range(block_reps)))
        if len(self.num_planes) > 1:
            c1 = self.num_planes[1]
            down = SparseConv3d(c0, c1, kernel_size=2, stride=2, bias=False, indice_key=f'spconv{indice_key_id}')
            up = SparseInverseConv3d(c1, c0, kernel_size=2, bias=False, indice_key=f'spconv{indice_key_id}')
            if normalize_before:
                self.conv = SparseSequential(norm_fn(c0), nn.ReLU(), down)
            else:
                self.conv = SparseSequential(down, norm_fn(c1), nn.ReLU())
            self.u = SpConvUNet(self.num_planes[1:], True, block_reps, block, indice_key_id=indice_key_id + 1,
                                normalize_before=normalize_before, return_blocks=return_blocks, _inner=True)
            if normalize_before:
                self.deconv = SparseSequential(norm_fn(c1), nn.ReLU(), up)
            else:
                self.deconv = SparseSequential(up, norm_fn(c0), nn.ReLU())
            self.blocks_tail = SparseSequential(OrderedDict(
                (f'block{i}', block(c0 * (2 - i), c0, norm_fn, indice_key=f'subm{indice_key_id}',
                                    normalize_before=normalize_before))
                for i in range(block_reps)))

    def prepare_geometry(self, x: SparseConvTensor):
        """Build every level's coordinates and rulebooks before any feature kernel is queued: the voxel
        counts of the coarser levels are host read-backs, and taking them here (integer kernels only in
        flight) keeps them from draining a pipeline full of convolutions later.  The per-tile pair ranges the convolution kernels
        walk (``Rulebook.tile_starts``) are built here too, for the tile heights the previous step used."""
        [m for m in self.blocks[0].conv_branch if isinstance(m, SubMConv3d) and m.kernel_size == 3][0].geometry(x).precompute_tiles()
        if len(self.num_planes) > 1:
            down = [m for m in self.conv if isinstance(m, SparseConv3d)][0]
            oc, oshape, ix2, rb_down = down.geometry(x)
            rb_down.precompute_tiles()
            self.u.prepare_geometry(SparseConvTensor(None, oc, oshape, x.batch_size, x.indice_dict, ix2))

    def forward(self, input: SparseConvTensor, previous_outputs=None):
        run = input.indice_dict.get(S.FUSE_KEY)
        if getattr(self, '_outer', False):
            if run is None or run.plan.root is not self or run.used:      # not announced by the caller (begin_fusion), or an earlier pass's
                begin_fusion(input, self)
                run = input.indice_dict.get(S.FUSE_KEY)
            if run is not None:
                run.used = True
        fused_cat = run is not None and self in run.plan.cats and S.fusion_active(self)
        output = self.blocks(input)
        identity = output
        if len(self.num_planes) > 1:
            cm = list(self.conv._modules.values())
            if isinstance(cm[0], SparseBatchNorm) and len(cm) == 3:       # normalize_before: the skip connection leaves next to a norm
                y, identity = cm[0].on(output, relu=True, skip=True, feeds_conv=True)
                dec = cm[2](y)
            else:
                dec = self.conv(output)
            if self.return_blocks:
                dec, previous_outputs = self.u(dec, previous_outputs)
            else:
                dec = self.u(dec)
            dec = self.deconv(dec)
            if fused_cat:      # both producers wrote their column block of the concatenation, and of the first tail norm of it
                output = output.replace_feature(run.concat(self, output.features.shape[0], output.features.device))
            else:
                output = output.replace_feature(torch.cat((identity.features, dec.features), dim=1))
            output = self.blocks_tail(output)
        if self.return_blocks:
            if previous_outputs is None:
                previous_outputs = []
            previous_outputs.append(output)
            return output, previous_outputs
        return output
