"""Sparse layer stacks on the device, checked layer by layer against float64 on the product's own tensors (tests/_layer_stacks.py has the
stacks, the references and the checker; tests/test_layer_stacks_cpu.py checks the checker).

Recorder: forward hooks (``with_kwargs``) on every ``SparseModule`` leaf and every ``SparseBatchNorm`` snapshot what a layer received and
what it returned, tensor hooks capture the gradient that reaches every feature tensor.  A bare ReLU calls no module: its input is the
previous record's output, its output the next record's input (or the stack's result).  ``prune`` and ``sparse_add`` are called and
recorded by the test.  Every stack runs in training mode under the four operand selections; stack E also in eval mode with autograd on;
stack T also under the hashed occupancy index.  What passes between the layers is what is tested: levels, the shared ``indice_dict``, the
fresh one behind ``sparse_add`` / ``prune``, bf16 shadows and marks on feature tensors, the autograd graph.

Which test fails when a fix of unidet3d_amd/sparse.py is taken back:
  the bare ReLU's backward            every ``test_stack_layer_by_layer`` case ('no gradient: tensor ...'), and the Z cases raise on the empty level;
  ``sparse_conv``'s rulebook check    ``test_a_key_met_again_on_another_level_is_refused`` (and tests/test_layer_stacks_cpu.py's refusals)."""
import json

import pytest
import torch
from torch import nn

import _layer_stacks as LS
import _parity
from test_gpu_conv_geometry import _selection

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SELECTIONS = ['bf16x3', 'mfma', 'bf16', 'bf16-rows']
ATTRS = ('_u3d_shadow', '_u3d_stats', '_u3d_from_conv', '_u3d_act', '_u3d_rows_only')
CASES = [(s, n) for s in ('E', 'P', 'T', 'Z') for n in LS.SCENES[s]]


# ---------------------------------------------------------------------------------------------------------------- the stacks as modules
def _module(o, p):
    """the layer of one operation with the parameters of ``_layer_stacks.params`` (None: the operation has no module)"""
    from unidet3d_amd import sparse as S
    kind = o['kind']
    if kind == 'subm':
        m = S.SubMConv3d(o['cin'], o['cout'], o['k'], dilation=o['d'], indice_key=o['key'])
    elif kind == 'conv':
        m = S.SparseConv3d(o['cin'], o['cout'], o['k'], stride=o['s'], padding=o['p'], dilation=o['d'], indice_key=o['key'])
    elif kind == 'inv':
        m = S.SparseInverseConv3d(o['cin'], o['cout'], o['k'], indice_key=o['key'], bias=o['bias'])
    elif kind == 'convt':
        m = S.SparseConvTranspose3d(o['cin'], o['cout'], o['k'], stride=o['s'], padding=o['p'], output_padding=o['q'], dilation=o['d'],
                                    bias=o['bias'], indice_key=o['key'])
    elif kind in ('maxpool', 'avgpool'):
        m = (S.SparseMaxPool3d if kind == 'maxpool' else S.SparseAvgPool3d)(o['k'], o['s'], o['p'], o['d'], indice_key=o['key'])
    elif kind == 'bn':
        m = S.SparseBatchNorm(o['C'])
    else:
        return None
    with torch.no_grad():
        if 'w' in p:
            m.weight.copy_(p['w'])
        if 'b' in p:
            m.bias.copy_(p['b'])
        if kind == 'bn':
            m.weight.copy_(p['gamma']), m.bias.copy_(p['beta']), m.running_mean.copy_(p['rm0']), m.running_var.copy_(p['rv0'])
    return m


def _sequential(ops, mods, lo, hi):
    """operations lo .. hi - 1 as ONE ``SparseSequential``: a norm's fused ReLU is the nn.ReLU behind it, a bare ReLU behind a norm is kept
    apart from it by an nn.Identity"""
    from unidet3d_amd import sparse as S
    layers = []
    for i in range(lo, hi):
        o = ops[i]
        if o['kind'] == 'relu':
            if layers and isinstance(layers[-1], S.SparseBatchNorm):
                layers.append(nn.Identity())
            layers.append(nn.ReLU())
        else:
            layers.append(mods[i])
            if o['kind'] == 'bn' and o['relu']:
                layers.append(nn.ReLU())
    return S.SparseSequential(*layers)


class _Recorder:
    def __init__(self, mods):
        from unidet3d_amd import sparse as S
        self.S, self.calls, self.grads, self.keep, self.handles = S, [], {}, [], []
        for m in mods:
            if m is None:
                continue
            assert isinstance(m, S.SparseBatchNorm) or (isinstance(m, S.SparseModule) and not list(m.children()))
            self.handles.append(m.register_forward_pre_hook(self._before, with_kwargs=True))
            self.handles.append(m.register_forward_hook(self._after, with_kwargs=True))

    def close(self):
        for h in self.handles:
            h.remove()

    def watch(self, t):
        """the gradient that reaches feature tensor ``t``, once (a tensor outside the graph gets none: the checker reports it)"""
        if t.requires_grad and id(t) not in self.grads:
            self.grads[id(t)] = None
            self.keep.append(t)
            t.register_hook(lambda g, key=id(t): self.grads.__setitem__(key, g.detach().clone()))

    @staticmethod
    def level(x):
        return (x.batch_size, list(x.spatial_shape), x.indices.detach().cpu().clone())

    def _before(self, mod, args, kwargs):
        if isinstance(mod, self.S.SparseBatchNorm):
            mod._seen_before = (mod.running_mean.detach().cpu().clone(), mod.running_var.detach().cpu().clone())

    def _after(self, mod, args, kwargs, out):
        S = self.S
        if isinstance(mod, S.SparseBatchNorm):
            f, y = args[0], out
            assert not kwargs.get('skip', False) and isinstance(out, torch.Tensor)
            rec = dict(module=mod, relu=bool(kwargs.get('relu', False)), training=mod.training, rm0=mod._seen_before[0], rv0=mod._seen_before[1],
                       rm1=mod.running_mean.detach().cpu().clone(), rv1=mod.running_var.detach().cpu().clone(), in_level=None, level=None)
            if not mod.training:
                rec['scale'], rec['shift'] = (t.detach().cpu().clone() for t in mod.eval_affine())
        else:
            f, y = args[0].features, out.features
            rec = dict(module=mod, in_level=self.level(args[0]), level=self.level(out))
        self.add(rec, [f], y)

    def add(self, rec, fs, y):
        """one executed operation: snapshots of what it received and returned, and the gradient hooks"""
        rec.update(x=[f.detach().cpu().clone() for f in fs], y=y.detach().cpu().clone(), x_obj=list(fs), y_obj=y,
                   x_attrs=[[a for a in ATTRS if hasattr(f, a)] for f in fs])
        for t in (*fs, y):
            self.watch(t)
        self.calls.append(rec)


def _run_stack(stack, name, training=True):
    """-> (run as ``_layer_stacks.check`` takes it, the stack's result, the input tensor)"""
    from unidet3d_amd import sparse as S
    ops, prm = LS.STACKS[stack], LS.params(stack)
    _, B, shape, coords = LS.scene(name)
    x0, dy = LS.inputs(stack, name)
    mods = [_module(o, p) for o, p in zip(ops, prm)]
    net = nn.ModuleList([m for m in mods if m is not None]).to(DEV).train(training)
    rec = _Recorder(mods)
    feats = x0.to(DEV).requires_grad_()
    xin = S.SparseConvTensor(feats, coords.to(DEV), shape, B)

    def pruned(t, r):
        keep = LS.prune_mask(t.indices.cpu(), r).to(DEV)
        out = S.prune(t, keep)
        rec.add(dict(module=None, keep=keep.cpu(), in_level=rec.level(t), level=rec.level(out)), [t.features], out.features)
        return out
    try:
        if stack in ('T', 'T0'):
            head = 4
            u = _sequential(ops, mods, 0, head)(xin)
            if stack == 'T':
                u, head = pruned(u, ops[4]['r']), 5
            a = pruned(mods[head](xin), ops[head + 1]['r'])
            w = S.sparse_add(u, a)
            assert w.indice_dict is not xin.indice_dict or stack == 'T0'
            rec.add(dict(module=None, in_level=rec.level(u), level=rec.level(w)), [u.features, a.features], w.features)
            out = _sequential(ops, mods, head + 3, len(ops))(w)
        else:
            out = _sequential(ops, mods, 0, len(ops))(xin)
        out.features.backward(dy.to(DEV))
        S.join_wgrad_stream()
        torch.cuda.synchronize()
    finally:
        rec.close()
    # ---- the calls, in execution order, against the operations; the bare ReLUs in between
    records, it, readers = [], iter(rec.calls), LS.consumers(ops)
    for i, o in enumerate(ops):
        if o['kind'] == 'relu':
            records.append(dict(kind='relu', src=list(o['src']), params={}, pgrads={}))
            continue
        c = next(it)
        assert c['module'] is mods[i], f'operation {i} ({o["kind"]}): another module ran'
        m = mods[i]
        c.update(kind=o['kind'], src=list(o['src']), params={}, pgrads={})
        if o['kind'] in LS.CONV_KINDS:
            c['params'], c['pgrads'] = dict(w=m.weight.detach().cpu()), dict(w=m.weight.grad)
            if m.bias is not None:
                c['params']['b'], c['pgrads']['b'] = m.bias.detach().cpu(), m.bias.grad
        elif o['kind'] == 'bn':
            assert c['relu'] == o['relu']
            c['params'], c['pgrads'] = dict(gamma=m.weight.detach().cpu(), beta=m.bias.detach().cpu()), dict(gamma=m.weight.grad, beta=m.bias.grad)
        c['pgrads'] = {k: None if g is None else g.detach().cpu() for k, g in c['pgrads'].items()}
        records.append(c)
    assert next(it, None) is None, 'more module calls than operations'
    final = dict(x=[out.features.detach().cpu().clone()], x_obj=[out.features], in_level=rec.level(out),
                 x_attrs=[[a for a in ATTRS if hasattr(out.features, a)]])
    for i in reversed(range(len(ops))):
        r, nxt = records[i], [records[j] for j in readers.get(i + 1, [])] or [final]
        if r['kind'] == 'relu':                # input: what the producer returned; output: what the reader received
            t = ops[i]['src'][0]
            j = 0 if nxt[0] is final else nxt[0]['src'].index(i + 1)
            r.update(x=[records[t - 1]['y']], y=nxt[0]['x'][j], y_obj=nxt[0]['x_obj'][j], y_attrs=nxt[0]['x_attrs'][j])
        if r.get('level') is None:             # a norm or a bare ReLU: the level its reader received, or the one its reader is on
            r['level'] = nxt[0]['in_level'] if nxt[0].get('in_level') is not None else nxt[0]['level']
    grads = {0: None if feats.grad is None else feats.grad.detach().cpu()}
    for i, r in enumerate(records):
        g = rec.grads.get(id(r['y_obj']))
        grads[i + 1] = None if g is None else g.cpu()
    return dict(records=records, grads=grads, x0=x0), out, xin


def _checked(stack, name, sel, training=True, tag=''):
    with _selection(sel):
        run, out, xin = _run_stack(stack, name, training)
    ratios, fails = LS.check(stack, name, run, LS.OPERANDS[sel])
    rec = dict(stack=stack, scene=name, selection=sel, mode=('train' if training else 'eval') + tag, worst=max(ratios.values(), default=0.0),
               **{k: round(v, 4) for k, v in sorted(ratios.items())})
    print('layer_stacks', json.dumps(rec))
    _parity.log_errors('layer_stacks', rec)
    assert not fails, f'{stack} on {name} under {sel}:\n' + '\n'.join(fails)
    assert ratios and all(r <= 1.0 for r in ratios.values())
    assert {o['kind'] for o in LS.STACKS[stack]} <= {k.split('.')[0] for k in ratios}
    # a bare ReLU returns a new tensor inside the graph that carries nothing of the layer in front
    for r in run['records']:
        if r['kind'] == 'relu':
            assert r['y_attrs'] == [] and r['y_obj'].requires_grad and r['y_obj'].grad_fn is not None, (stack, name, sel, r['y_attrs'])
            assert r['y_obj'] is not run['records'][r['src'][0] - 1]['y_obj']
    return run, out, xin


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('stack,name', CASES)
def test_stack_layer_by_layer(stack, name, sel):
    run, out, xin = _checked(stack, name, sel)
    if stack == 'Z':
        recs = run['records']
        assert tuple(recs[1]['y'].shape) == (0, 64) and tuple(recs[3]['y'].shape) == (0, 64)
        assert torch.equal(recs[4]['y'], recs[4]['params']['b'].expand(2, -1))                  # every row of the inverse layer: exactly its bias
        assert torch.equal(recs[2]['rm1'], recs[2]['rm0']) and torch.equal(recs[2]['rv1'], recs[2]['rv0'])
        assert tuple(out.features.shape) == (2, 32)
        for i, k in ((0, 'w'), (1, 'w'), (2, 'gamma'), (2, 'beta'), (4, 'w')):                  # zero gradients are exact zeros
            assert bool((recs[i]['pgrads'][k] == 0).all()), (i, k)
    if stack == 'T':                             # the union is a new voxel set: it starts from a fresh indice_dict, where 's0' is built again
        rb = out.indice_dict['s0']
        assert out.indice_dict is not xin.indice_dict and xin.indice_dict['s0'] is not rb
        assert rb.n_in == len(run['records'][7]['level'][2]) != xin.indice_dict['s0'].n_in


@pytest.mark.parametrize('name', LS.SCENES['E'])
def test_stack_e_in_eval_mode_with_autograd(name):
    for sel in SELECTIONS:
        run, _, _ = _checked('E', name, sel, training=False)
        assert all(torch.equal(r['rm1'], r['rm0']) and torch.equal(r['rv1'], r['rv0']) for r in run['records'] if r['kind'] == 'bn')


@pytest.mark.parametrize('name', LS.SCENES['T'])
def test_stack_t_under_the_hashed_index(name, monkeypatch):
    from unidet3d_amd import geometry
    monkeypatch.setattr(geometry, '_INDEX_MODE', 'hash')
    for sel in SELECTIONS:
        _, out, xin = _checked('T', name, sel, tag='-hash')
        assert out.index.hashed and xin.index.hashed


@pytest.mark.parametrize('name', LS.SCENES['T0'])
def test_a_key_met_again_on_another_level_is_refused(name):
    """Stack T without the prune of its up-sampled branch: that branch covers the other operand, ``sparse_add`` returns the union on ITS
    level with ITS ``indice_dict`` -- the one the input level filled -- and the second 's0' layer finds the rulebook of the input level
    there.  The kernels would read rows past the tensor as zeros and return a wrong result without a fault: the layer must refuse."""
    from unidet3d_amd._lib import U3DError
    lv, _ = LS.geometry('T0', name)
    n0, nu = len(lv[0][2]), len(lv[7][2])
    assert n0 != nu
    with pytest.raises(U3DError, match=rf"\({nu}, 32\) features, the rulebook has {n0} source rows in mode 'fwd' \(rulebook \('subm', 's0'\)\)"):
        _run_stack('T0', name)


# ---------------------------------------------------------------------------------------------------------------- the ReLU kernels alone
def _values(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x, dy = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g)
    flat = x.view(-1)
    special = torch.tensor([0.0, -0.0, float('inf'), float('-inf'), float('nan'), 1e-45, -1e-45, 3.4e38])
    flat[:min(len(flat), len(special))] = special[:len(flat)]
    return x, dy


@pytest.mark.parametrize('n,C', [(1, 1), (1, 3), (7, 5), (3, 32), (603, 64), (65, 516), (70001, 64)])
def test_bare_relu_forward_and_backward_are_exact(n, C):
    """every count class: below one 16-byte piece, a scalar tail, whole pieces, more elements than the capped grid holds at once, and a
    buffer that is not 16-byte aligned (the scalar path); signed zeros, infinities, denormals and NaN as the documented rule gives them"""
    from unidet3d_amd import sparse as S
    for offset in (0, 1):
        x, dy = _values(n + offset, C, n * 1000 + C)
        xd = x.to(DEV)[offset:].requires_grad_()
        x, dy = x[offset:], dy[offset:]
        y = S._relu(xd)
        y.backward(dy.to(DEV))
        want = torch.where(x > 0, x, torch.zeros(()))
        assert LS.SS.same(y, want) and LS.SS.same(xd.grad, torch.where(x > 0, dy, torch.zeros(())))
        assert torch.equal(want[torch.isfinite(x)], torch.relu(x)[torch.isfinite(x)])


def test_bare_relu_writes_nothing_outside_its_buffer_and_takes_an_empty_level():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    for count in (1, 5, 1024, 1027):
        x = torch.randn(count, generator=torch.Generator().manual_seed(count)).to(DEV)
        for off in (4, 5):                       # an aligned and a misaligned destination
            buf = torch.full((count + 12,), 12345.0, device=DEV)
            L.call('u3d_relu_fwd', x.data_ptr(), count, buf[off:].data_ptr(), L.stream())
            torch.cuda.synchronize()
            assert bool((buf[:off] == 12345.0).all()) and bool((buf[off + count:] == 12345.0).all())
            assert torch.equal(buf[off:off + count], torch.relu(x))
    for C in (64, 6):
        e = torch.zeros(0, C, device=DEV, requires_grad=True)
        y = S._relu(e)
        y.sum().backward()
        assert tuple(y.shape) == (0, C) and y.grad_fn is not None and tuple(e.grad.shape) == (0, C)
