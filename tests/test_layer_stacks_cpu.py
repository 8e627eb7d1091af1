"""The checker of the layer-stack tests (tests/_layer_stacks.py) checked on the CPU.
  * Every stack a second time as a plain dense float64 torch net (a value grid and an occupancy-mask grid side by side), run end to end:
    its output rows, its levels and every gradient must agree with the chained pair-list references -- two float64 evaluations that
    differ in summation order only; the largest relative difference is logged and must stay below 1e-9.  No ReLU pre-activation and no
    max-pool top-two gap of these seeds lies within 1e-9 of a decision.
  * An fp32 CPU evaluation of each stack, as a run, passes the checker with every ratio <= 1; each planted fault fails it for its reason.
  * ``sparse_conv`` refuses feature rows, channel counts and addends that do not fit the rulebook before anything is launched."""
import json

import pytest
import torch
import torch.nn.functional as F

import _layer_stacks as LS

CASES = [(s, n) for s in sorted(LS.STACKS) if s != 'T0' for n in LS.SCENES[s]]


def test_the_levels_are_the_ones_the_stacks_were_chosen_for():
    for (stack, name), rows in LS.ROWS.items():
        lv, _ = LS.geometry(stack, name)
        seen = [len(lv[0][2])]
        for _, _, c in lv[1:]:
            if len(c) != seen[-1]:
                seen.append(len(c))
        assert tuple(seen[:len(rows)]) == rows, (stack, name, seen)
    for name in LS.SCENES['T']:
        # the union level of T: the extent and batch of tensor 0, other rows, and neither operand's level -- a new voxel set
        lv, geo = LS.geometry('T', name)
        n0, nu, na, nw = (len(lv[t][2]) for t in (0, 5, 7, 8))
        assert lv[8][:2] == lv[0][:2] and nw not in (n0, nu, na) and min(n0, nu, na) > 0, (name, n0, nu, na, nw)
        assert 0 < nu < len(lv[4][2]) and 0 < na < len(lv[6][2])
        # T0, the stack without the first prune: the up-sampled level covers the other operand, the union IS that level
        lv, geo = LS.geometry('T0', name)
        assert torch.equal(lv[7][2], lv[4][2]) and len(lv[7][2]) != len(lv[0][2]) and 0 < len(lv[6][2]) < len(lv[5][2])
    lv, geo = LS.geometry('Z', LS.TWO_VOXELS[0])
    assert len(lv[2][2]) == 0 and all(len(s) == 0 for s, _ in geo[4].pairs)


# ---------------------------------------------------------------------------------------------------------------- the dense float64 net
def _t3(v):
    return (v,) * 3 if isinstance(v, int) else tuple(v)


def _grid(rows, coords, B, shape):
    c = coords.long()
    V = rows.new_zeros(B, *shape, rows.shape[1]).index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), rows).permute(0, 4, 1, 2, 3)
    M = torch.zeros(B, 1, *shape, dtype=rows.dtype)
    M[c[:, 0], 0, c[:, 1], c[:, 2], c[:, 3]] = 1.0
    return V, M


def _rows(V, M):
    c = M[:, 0].nonzero()                                            # row-major: canonical order
    return V[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]], c.int()


def _channels(v):
    return v[None, :, None, None, None]


def dense_net(stack, name, prm, x0, dy):
    """-> (output rows, [coords of every tensor], parameter gradients per operation, gradient of x0)"""
    ops = LS.STACKS[stack]
    _, B, shape, coords = LS.scene(name)
    x0 = x0.double().requires_grad_()
    P = [{k: v.double().requires_grad_() for k, v in p.items() if k in ('w', 'b', 'gamma', 'beta')} for p in prm]
    tens, saved = [_grid(x0, coords, B, shape)], {}
    for i, o in enumerate(ops):
        kind, p = o['kind'], P[i]
        V, M = tens[o['src'][0]]
        if kind in ('subm', 'conv', 'convt', 'maxpool', 'avgpool'):
            k, s, pad, d = _t3(o['k']), _t3(o['s']), _t3(o['p']), _t3(o['d'])
            ones = torch.ones(1, 1, *k, dtype=torch.float64)
        if kind == 'subm':
            pad = tuple(d[a] * (k[a] - 1) // 2 for a in range(3))
            out = F.conv3d(V, p['w'].permute(0, 4, 1, 2, 3), padding=pad, dilation=d) * M, M
        elif kind == 'conv':
            M2 = (F.conv3d(M, ones, stride=s, padding=pad, dilation=d) > 0).double()
            out = F.conv3d(V, p['w'].permute(0, 4, 1, 2, 3), stride=s, padding=pad, dilation=d) * M2, M2
            saved[i] = (tuple(V.shape[2:]), M, (s, pad, d))
        elif kind == 'inv':                      # the vector-Jacobian product of the strided layer's dense convolution, weight axes swapped
            in_shape, M_in, (s, pad, d) = saved[o['of']]
            u = torch.zeros(B, o['cout'], *in_shape, dtype=torch.float64, requires_grad=True)
            f = F.conv3d(u, p['w'].permute(4, 0, 1, 2, 3), stride=s, padding=pad, dilation=d)
            up = torch.autograd.grad(f, u, grad_outputs=V, create_graph=True)[0]
            out = (up + _channels(p['b'])) * M_in, M_in
        elif kind == 'convt':
            q = _t3(o['q'])
            M2 = (F.conv_transpose3d(M, ones, stride=s, padding=pad, output_padding=q, dilation=d) > 0).double()
            up = F.conv_transpose3d(V, p['w'].permute(4, 0, 1, 2, 3), stride=s, padding=pad, output_padding=q, dilation=d)
            out = (up + _channels(p['b'])) * M2, M2
        elif kind == 'bn':
            n = M.sum()
            if float(n) == 0:
                out = V, M
            else:
                m = (V * M).sum((0, 2, 3, 4)) / n
                var = (((V - _channels(m)) * M) ** 2).sum((0, 2, 3, 4)) / n
                y = (V - _channels(m)) / torch.sqrt(_channels(var) + LS.EPS) * _channels(p['gamma']) + _channels(p['beta'])
                out = (torch.relu(y) if o['relu'] else y) * M, M
        elif kind == 'relu':
            out = torch.relu(V), M
        elif kind == 'maxpool':                  # absent cells hold -inf: they never win, and a window without a present cell is no output row
            M2 = (F.max_pool3d(M, k, s, pad, d) > 0)
            y = F.max_pool3d(torch.where(M > 0, V, torch.full((), float('-inf'), dtype=torch.float64)), k, s, pad, d)
            out = torch.where(M2, y, torch.zeros((), dtype=torch.float64)), M2.double()
        elif kind == 'avgpool':                  # sum over count
            cnt = F.avg_pool3d(M, k, s, pad, divisor_override=1)
            out = F.avg_pool3d(V, k, s, pad, divisor_override=1) / cnt.clamp(min=1.0) * (cnt > 0), (cnt > 0).double()
        elif kind == 'prune':
            ax = [torch.arange(n).reshape([-1 if a == b else 1 for b in range(3)]) for a, n in enumerate(V.shape[2:])]
            K = ((ax[0] + ax[1] + ax[2]) % 3 != o['r']).double()[None, None]
            out = V * K, M * K
        else:
            Vb, Mb = tens[o['src'][1]]
            out = V + Vb, torch.maximum(M, Mb)
        tens.append(out)
    y, _ = _rows(*tens[-1])
    leaves = [x0] + [t for p in P for t in p.values()]
    gs = torch.autograd.grad(y, leaves, dy.double(), allow_unused=True)
    gs = [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, gs)]
    it = iter(gs[1:])
    return y.detach(), [_rows(V.detach(), M)[1] for V, M in tens], [{k: next(it) for k in p} for p in P], gs[0]


def _rel(a, b, scale=None):
    """largest difference against the tensor's largest magnitude (``scale`` where the tensor itself cancels to zero)"""
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if not a.numel():
        return 0.0
    scale = float(b.abs().max()) if scale is None else scale
    return float((a - b).abs().max() / scale) if scale > 0 else float((a - b).abs().max())


@pytest.mark.parametrize('stack,name', CASES)
def test_dense_float64_net_agrees_with_the_chained_references(stack, name):
    prm = LS.params(stack)
    x0, dy = LS.inputs(stack, name)
    run = LS.emulate(stack, name, torch.float64)
    lv, geo = LS.geometry(stack, name)
    y, levels, pgrads, dx0 = dense_net(stack, name, prm, x0, dy)
    for t, (c, (_, _, rc)) in enumerate(zip(levels, lv)):
        assert c.dtype == rc.dtype and torch.equal(c, rc), f'{stack} on {name}: level of tensor {t}'
    worst = dict(y=_rel(y, run['records'][-1]['y']), dx0=_rel(dx0, run['grads'][0]))
    for i, (pg, rec) in enumerate(zip(pgrads, run['records'])):
        assert set(pg) == set(rec['pgrads']) == set(rec['params']), (i, rec['kind'])
        for k, g in pg.items():
            # a bias in front of a training-mode norm: its gradient, the column sum of dy, cancels to zero -- taken against the
            # magnitude of that sum's terms
            worst[f"{i}.{rec['kind']}.{k}"] = _rel(g, rec['pgrads'][k], float(run['grads'][i + 1].abs().sum(0).max()) if k == 'b' else None)
    # how far every decision of these seeds is from flipping
    margin = float('inf')
    for o, g, rec in zip(LS.STACKS[stack], geo, run['records']):
        x = rec['x'][0]
        if o['kind'] == 'relu' and x.numel():
            margin = min(margin, float(x.abs().min()))
        elif o['kind'] == 'bn' and o['relu'] and x.numel():
            margin = min(margin, float(LS.bn_expr(x, rec['params']['gamma'], rec['params']['beta'], False)[0].abs().min()))
        elif o['kind'] == 'maxpool' and g.n_dst:
            v, have = LS._window(x, g, float('-inf'))
            top = v.sort(1, descending=True)[0]
            # (a window whose maximum is an exact zero of the ReLU in front holds ties of exact zeros: decided by rule, first wins,
            #  not by rounding, and that ReLU drops their gradient)
            gap = (top[:, 0] - top[:, 1])[(have.sum(1) > 1)[:, None] & (top[:, 0] > 0)]
            if gap.numel():
                margin = min(margin, float(gap.min()))
    rec = dict(stack=stack, scene=name, largest=max(worst.values()), decision_margin=margin, **{k: v for k, v in worst.items() if v > 1e-13})
    print('layer_stacks_dense', json.dumps(rec))
    import _parity
    _parity.log_errors('layer_stacks_dense', rec)
    assert margin > 1e-9, f'{stack} on {name}: a decision within {margin:.3g} of flipping: change the seed'
    assert max(worst.values()) < 1e-9, worst


# ---------------------------------------------------------------------------------------------------------------- fp32 runs and planted faults
_RUNS = {}


def _fp32(stack, name):
    if (stack, name) not in _RUNS:
        _RUNS[stack, name] = LS.emulate(stack, name, torch.float32)
    return _RUNS[stack, name]


def _copy(run):
    return dict(records=[dict(r, x=list(r['x']), pgrads=dict(r['pgrads'])) for r in run['records']], grads=dict(run['grads']), x0=run['x0'])


@pytest.mark.parametrize('stack,name', CASES)
def test_fp32_evaluation_passes_the_checker(stack, name):
    ratios, fails = LS.check(stack, name, _fp32(stack, name), 'fp32')
    print('layer_stacks_fp32', stack, name, json.dumps({k: round(v, 4) for k, v in ratios.items()}))
    assert not fails, '\n'.join(fails)
    assert ratios and all(r <= 1.0 for r in ratios.values())
    kinds = {k.split('.')[0] for k in ratios}
    assert {o['kind'] for o in LS.STACKS[stack]} <= kinds, kinds
    if stack == 'T':
        assert 'shared.dx' in ratios


def test_fp32_evaluation_in_eval_mode_passes_the_checker():
    for name in LS.SCENES['E']:
        ratios, fails = LS.check('E', name, LS.emulate('E', name, torch.float32, training=False), 'fp32')
        assert not fails, '\n'.join(fails)
        assert all(k in ratios for k in ('bn.y', 'bn.dgamma', 'bn.dbeta', 'bn.dx', 'bn.running_mean'))


def _fails(stack, name, run, *needles):
    ratios, fails = LS.check(stack, name, run, 'fp32')
    text = '\n'.join(fails)
    assert fails and all(n in text for n in needles), (needles, text)
    return text


def test_fault_two_output_rows_swapped():
    run = _copy(_fp32('E', 'block5_odd_extent'))
    r = run['records'][2]
    y = r['y'].clone()
    y[[3, 4]] = y[[4, 3]]
    r['y'] = y
    run['records'][3]['x'] = [y]                 # the chain stays whole: the values alone are wrong
    text = _fails('E', 'block5_odd_extent', run, 'record 2 (conv): bound: y')
    assert 'chain' not in text and 'level' not in text


@pytest.mark.parametrize('name', LS.SCENES['T'])
def test_fault_second_s0_layer_over_the_pairs_of_the_first_level(name):
    run = LS.emulate('T', name, torch.float32, fault=('reuse_pairs', 8))
    text = _fails('T', name, run, 'record 8 (subm): bound: y')
    assert 'record 5' not in text and 'record 7' not in text


def test_fault_bare_relu_without_backward():
    run = LS.emulate('E', 'empty_middle_scene', torch.float32, fault=('relu_no_grad', 5))
    text = _fails('E', 'empty_middle_scene', run, 'no gradient: tensor 5 (output of record 4, subm)', 'no gradient: tensor 0 (the stack input)',
                  'record 4 (subm): no gradient: parameter w', 'record 0 (subm): no gradient: parameter w')
    assert 'record 6' not in text and 'record 7' not in text           # behind the ReLU everything is in order
    run = LS.emulate('T', 'empty_middle_scene', torch.float32, fault=('relu_no_grad', 3))      # one branch cut: x0 still gets the other's
    text = _fails('T', 'empty_middle_scene', run, 'no gradient: tensor 3', 'record 0 (conv): no gradient: parameter w')
    assert 'tensor 0' not in text


def test_fault_norm_statistics_with_one_row_left_out():
    for stack, name, op in (('E', 'line_x_65', 1), ('P', 'block_odd_mixed_extent', 5)):
        text = _fails(stack, name, LS.emulate(stack, name, torch.float32, fault=('row_dropped', op)), f'record {op} (bn): bound: y')
        assert 'running_mean' in text


def test_fault_bias_missing_on_rows_without_pairs():
    name = LS.TWO_VOXELS[0]
    text = _fails('Z', name, LS.emulate('Z', name, torch.float32, fault=('bias_lonely', 4)), 'record 4 (inv): bound: y_without_pairs')
    run = LS.emulate('Z', name, torch.float32)
    rec = run['records'][4]
    assert torch.equal(rec['y'], rec['params']['b'].expand(2, -1))       # every output row of the inverse layer: exactly its bias
    assert all(not bool(run['records'][i]['pgrads'][k].any()) for i, k in ((1, 'w'), (2, 'gamma'), (2, 'beta'), (4, 'w')))     # exact zeros


def test_fault_strided_output_rows_in_another_order():
    run = _copy(_fp32('E', 'line_x_65'))
    r = run['records'][2]
    B, shape, coords = r['level']
    r['level'], r['y'] = (B, shape, coords.flip(0).contiguous()), r['y'].flip(0).contiguous()
    run['records'][3]['x'] = [r['y']]
    _fails('E', 'line_x_65', run, 'record 2 (conv): level')
    run = _copy(_fp32('E', 'line_x_65'))
    run['records'][2]['level'] = (B, shape, coords.long())             # the right rows in another integer type
    _fails('E', 'line_x_65', run, 'record 2 (conv): level')


def test_a_broken_chain_is_reported():
    run = _copy(_fp32('P', 'single_voxel'))
    x = run['records'][2]['x'][0].clone()
    x[0, 0] = -x[0, 0]
    run['records'][2]['x'] = [x]
    _fails('P', 'single_voxel', run, 'record 2 (maxpool): chain')


# ---------------------------------------------------------------------------------------------------------------- refusals of sparse_conv
def _rulebook(S, K, n_in, n_out, tag=None):
    z = torch.zeros(K, 1, dtype=torch.int32)
    rb = S.Rulebook(z, z, torch.zeros(K, dtype=torch.int32), K, n_in, n_out)
    rb.tag = tag
    return rb


def test_sparse_conv_refuses_rows_channels_and_addends_that_do_not_fit_the_rulebook():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    w = torch.zeros(64, 3, 3, 3, 32)
    rb = _rulebook(S, 27, 39, 35, ('__down__', 'd'))
    with pytest.raises(L.U3DError, match=r"\(35, 32\) features.*39 source rows in mode 'fwd'.*'d'"):
        S.sparse_conv(torch.zeros(35, 32), w, rb, 'fwd')
    with pytest.raises(L.U3DError, match=r"\(39, 64\) features.*35 source rows in mode 'inv'.*'d'"):
        S.sparse_conv(torch.zeros(39, 64), torch.zeros(32, 3, 3, 3, 64), rb, 'inv')
    with pytest.raises(L.U3DError, match=r'features have 64 channels, the weight takes 32.*__down__'):
        S.sparse_conv(torch.zeros(39, 64), w, rb, 'fwd')
    with pytest.raises(L.U3DError, match=r'addend is \(39, 64\), the result \[35, 64\]'):
        S.sparse_conv(torch.zeros(39, 32), w, rb, 'fwd', torch.zeros(39, 64))
    with pytest.raises(L.U3DError, match=r'addend is \(35, 32\), the result \[35, 64\]'):
        S.sparse_conv(torch.zeros(39, 32), w, rb, 'fwd', torch.zeros(35, 32))
    with pytest.raises(L.U3DError, match=r'addend is \(35, 32\), the result \[39, 32\]'):
        S.sparse_conv(torch.zeros(35, 64), torch.zeros(32, 3, 3, 3, 64), rb, 'inv', torch.zeros(35, 32))
    with pytest.raises(L.U3DError, match='7 source rows') as e:            # no tag: the message names the numbers alone
        S.sparse_conv(torch.zeros(5, 32), w, _rulebook(S, 27, 7, 7), 'fwd')
    assert '(rulebook' not in str(e.value)
    with pytest.raises(L.U3DError, match='mode must be'):
        S.sparse_conv(torch.zeros(39, 32), w, rb, 'bwd')
    # what fits passes the check and is refused only at the first device pointer: nothing was launched
    with pytest.raises(L.U3DError, match='CUDA'):
        S.sparse_conv(torch.zeros(39, 32), w, rb, 'fwd', torch.zeros(35, 64))


class _FakeTensor:
    """what a convolution layer reads of a sparse tensor when its rulebook is already cached"""

    def __init__(self, indice_dict, features):
        self.indice_dict, self.features = indice_dict, features

    def replace_feature(self, features):
        return _FakeTensor(self.indice_dict, features)


def test_a_subm_key_met_again_on_another_level_is_refused_by_the_layer():
    """the cache hit on a rulebook of another row count: the union level of stack T reusing 's0' WITHOUT a fresh indice_dict"""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse as S
    layer = S.SubMConv3d(32, 32, 3, indice_key='s0')
    rb = _rulebook(S, 27, 54, 54, ('subm', 's0'))
    rb.geom = layer._rb_geom
    with pytest.raises(L.U3DError, match=r"\(70, 32\) features.*54 source rows.*'s0'"):
        layer(_FakeTensor({'s0': rb}, torch.zeros(70, 32)))
    inv = S.SparseInverseConv3d(64, 32, 3, indice_key='d')
    down = _rulebook(S, 27, 39, 35, ('__down__', 'd'))
    down.geom = ('conv', 3, 3, 3, 2, 2, 2, 1, 1, 1, 1, 1, 1)
    with pytest.raises(L.U3DError, match=r"\(39, 64\) features.*35 source rows in mode 'inv'"):      # fed from the strided layer's INPUT level
        inv(_FakeTensor({'d': (down, None, None, None)}, torch.zeros(39, 64)))
