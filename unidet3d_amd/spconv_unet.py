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
"""
from __future__ import annotations

import functools
from collections import OrderedDict

import torch
from torch import nn

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
            output = output.replace_feature(torch.cat((identity.features, dec.features), dim=1))
            output = self.blocks_tail(output)
        if self.return_blocks:
            if previous_outputs is None:
                previous_outputs = []
            previous_outputs.append(output)
            return output, previous_outputs
        return output
