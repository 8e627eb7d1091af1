"""Generate tests/golden/encoder_heads_golden.npz from the REAL reference decoder: configs whose head dim is 64 (d_model / num_heads),
which the reference takes like any other pair nn.MultiheadAttention takes.

Same procedure as tools/gen_golden_encoder.py (its import placeholders and its class lists are reused): the reference's
``unidet3d/encoder.py`` is imported as it is, weights come from tests/_detw.fill_state_dict (regenerable, so the fixture holds arrays
only: inputs, outputs, gradients).

  H4  num_layers 2, d_model 256, num_heads 4, hidden_dim 1024, one dataset, scenes [48, 17]: forward, loss, input gradients and the
      first 8 rows of some parameter gradients
  H2  num_layers 2, d_model 128, num_heads 2, hidden_dim 256, two datasets (one with a rotated head), scenes [9, 70, 0] (the last one
      empty): forward only
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_encoder import CLASSES, CLASSES_B, _load_encoder, fill_state_dict  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), '..', 'tests', 'golden', 'encoder_heads_golden.npz')
CFG_H4 = dict(num_layers=2, datasets_classes=[CLASSES], in_channels=32, d_model=256, num_heads=4, hidden_dim=1024,
              dropout=0.0, activation_fn='gelu', datasets=['scannet'], angles=[False])
CFG_H2 = dict(num_layers=2, datasets_classes=[CLASSES, CLASSES_B], in_channels=32, d_model=128, num_heads=2, hidden_dim=256,
              dropout=0.0, activation_fn='gelu', datasets=['scannet', 's3dis'], angles=[False, True])
GRAD_ROWS = ('input_proj.0.weight', 'self_attn_layers.0.attn.in_proj_weight', 'self_attn_layers.1.attn.out_proj.bias',
             'ffn_layers.1.net.3.weight', 'out_norm.weight', 'outs_cls.2.bias', 'out_bboxes.linear.weight')


def main():
    enc = _load_encoder()
    out = {}
    torch.manual_seed(4321)
    m = fill_state_dict(enc.UniDet3DEncoder(**CFG_H4), tag0=1100)
    ns = [48, 17]
    x = [torch.randn(n, 32, requires_grad=True) for n in ns]
    c = [torch.randn(n, 3) for n in ns]
    res = m(x, c, ['scannet', 'scannet'])
    loss = sum((t ** 2).sum() for t in res['cls_preds']) + sum(t.sum() for t in res['bboxes'])
    for a in res['aux_outputs']:
        loss = loss + sum((t * 0.5).sum() for t in a['cls_preds']) + sum((t ** 2).sum() for t in a['bboxes'])
    loss.backward()
    for i in range(2):
        out[f'H4.x{i}'] = x[i].detach().numpy(); out[f'H4.c{i}'] = c[i].numpy()
        out[f'H4.cls{i}'] = res['cls_preds'][i].detach().numpy()
        out[f'H4.box{i}'] = res['bboxes'][i].detach().numpy()
        out[f'H4.gx{i}'] = x[i].grad.numpy()
        for l, a in enumerate(res['aux_outputs']):
            out[f'H4.aux{l}.cls{i}'] = a['cls_preds'][i].detach().numpy()
            out[f'H4.aux{l}.box{i}'] = a['bboxes'][i].detach().numpy()
    out['H4.loss'] = np.float64(loss.item())
    for k, p in m.named_parameters():
        if k in GRAD_ROWS:
            out['H4.g.' + k] = p.grad.numpy()[:8].copy()      # first 8 rows keep the fixture small
    assert sum(k.startswith('H4.g.') for k in out) == len(GRAD_ROWS)
    m2 = fill_state_dict(enc.UniDet3DEncoder(**CFG_H2), tag0=1700)
    ns2 = [9, 70, 0]
    x2 = [torch.randn(n, 32) for n in ns2]
    c2 = [torch.randn(n, 3) for n in ns2]
    with torch.no_grad():
        r2 = m2(x2, c2, ['s3dis', 'scannet', 's3dis'])
    for i in range(3):
        out[f'H2.x{i}'] = x2[i].numpy(); out[f'H2.c{i}'] = c2[i].numpy()
        out[f'H2.cls{i}'] = r2['cls_preds'][i].numpy(); out[f'H2.box{i}'] = r2['bboxes'][i].numpy()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
