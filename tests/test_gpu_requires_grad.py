"""The autograd wrappers under PARTIAL requires_grad: fine-tuning with a frozen backbone, frozen norms, bias-only training.

Every hand-written backward branches on ``ctx.needs_input_grad``; those branches decide which kernels launch, on which stream, and which
of the returned tensors autograd keeps.  One table-driven harness runs each wrapped op over the subsets of its differentiable inputs
(all non-empty subsets up to five inputs; above that every single input, every all-but-one subset and the full set) and checks, per subset:

  * forward      the result equals the all-inputs-trainable result bit for bit (the forward must not depend on requires_grad);
  * frozen       a frozen input ends with ``.grad is None``;
  * trainable    a trainable input ends with a gradient of the input's shape, float32;
  * reference    that gradient against the same operation in float64 with plain torch ops on the CPU, under the bound and the error
                 norm the op's existing full-gradient test asserts (cited at each builder; nothing here is a new tolerance);
  * bitwise      that gradient equals the all-inputs-trainable run's bit for bit -- same kernel, same arguments.  The one place where
                 another path legitimately runs is a bias whose weight is frozen: the column sums then do not ride along with the
                 weight-gradient GEMM (u3d_gemm_tn, fixed-order split reduction) but come from ``dy.sum(0)``; those cases carry
                 ``fallback_<bias>`` in their id and keep the float64 bound only.

Then the same on the whole model (frozen backbone / frozen decoder / frozen biases and norms / biases only), and the state the
wrappers keep between calls: the pre-split weight planes of ``dense.transposed_weights`` after an in-place update, and the per-pass
bookkeeping of the weight-gradient side stream after a backward pass that died of an exception.
"""
import contextlib
import copy
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sparse_ops as so

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ---------------------------------------------------------------------------------------------------------------- error norms
def _rel(a, b):
    """max |a - b| / max |b|: the norm of test_gpu_model.py / test_gpu_kernels.py / test_gpu_bf16.py"""
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12)) if a.numel() else 0.0


def _fro(a, b):
    """Frobenius norm of the difference over that of the reference (test_mlp_bf16_close, ReLU)"""
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _rows(a, b):
    """per row: max |a - b| / max |b| of that row (test_gpu_criterion_edges._check_rows on finite rows)"""
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float(((a - b).abs() / b.abs().amax(1, keepdim=True).clamp(min=1e-30)).max())


# ---------------------------------------------------------------------------------------------------------------- the harness
_CASES = {}         # key -> (names of the differentiable inputs, builder, fallback(name, subset) -> bool)
_BUILT = {}         # key -> (op, float64 reference gradients, all-trainable run): computed once, shared by every subset's test


def _register(key, names, build, fallback=None):
    assert key not in _CASES, key
    _CASES[key] = (tuple(names), build, fallback or (lambda name, sub: False))


def _subsets(names):
    n = len(names)
    if n <= 5:
        return [c for k in range(1, n + 1) for c in itertools.combinations(names, k)]
    return [(x,) for x in names] + [tuple(y for y in names if y != x) for x in names] + [tuple(names)]


def _params(prefix):
    out = []
    for key, (names, _, fb) in _CASES.items():
        if not key.startswith(prefix):
            continue
        for sub in _subsets(names):
            on_fallback = [k for k in sub if fb(k, sub)]
            tag = 'all' if len(sub) == len(names) else 'only_' + '+'.join(sub)
            out.append(pytest.param(key, sub, id=f'{key}-{tag}' + ('-fallback_' + '+'.join(on_fallback) if on_fallback else '')))
    assert out, prefix
    return out


def _tup(o):
    return tuple(o) if isinstance(o, (tuple, list)) else (o,)


def _stack(*factories):
    """a context-manager factory entering ``factories`` in order"""
    @contextlib.contextmanager
    def cm():
        with contextlib.ExitStack() as st:
            for f in factories:
                st.enter_context(f())
            yield
    return cm


@contextlib.contextmanager
def _attr(obj, name, value):
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(obj, name, value)
        yield


def _run(op, sub, ctx=None, pre=None):
    """one forward (+ backward when ``sub`` is not empty) on the device -> (detached outputs, {name: .grad or None})"""
    leaves = {k: v.clone().to(DEV).requires_grad_(k in sub) for k, v in op.inputs.items()}
    if pre is not None:
        pre(leaves)
    with (ctx or op.ctx)():
        outs = _tup(op.fn(leaves))
        if sub:
            used = [i for i in op.used if outs[i].requires_grad]
            assert used, 'no consumed output depends on a trainable input'
            torch.autograd.backward([outs[i] for i in used], [op.gos[i].to(DEV) for i in used])
    # .grad is read as soon as backward() has returned, with no synchronisation in between: a weight gradient that was left on a
    # side stream without a join would be read early
    return [o.detach() for o in outs], {k: t.grad for k, t in leaves.items()}


def _state(key):
    if key not in _BUILT:
        names, build, _ = _CASES[key]
        op = build()
        assert tuple(op.inputs) == names, (key, tuple(op.inputs), names)
        t64 = {k: v.double().clone().requires_grad_() for k, v in op.inputs.items()}
        outs = _tup(op.ref(t64))
        torch.autograd.backward([outs[i] for i in op.used], [op.gos[i].double() for i in op.used])
        ref = {k: t.grad for k, t in t64.items()}
        base = _run(op, names)
        plain, _ = _run(op, ())                                     # nothing requires a gradient: the same forward bits
        for a, b in zip(plain, base[0]):
            assert torch.equal(a, b), f'{key}: the forward differs between no input and every input requiring a gradient'
        _BUILT[key] = (op, ref, base)
    return _BUILT[key]


def _check(key, sub, ctx=None, pre=None, expect=None):
    """the five checks of the module docstring for one subset; ``expect(name, base gradient)``: what a trainable input's gradient must
    equal bit for bit when it is not the base gradient itself (accumulation into an existing .grad)"""
    names, _, fallback = _CASES[key]
    op, ref, base = _state(key)
    outs, grads = _run(op, sub, ctx, pre)
    for i, (a, b) in enumerate(zip(outs, base[0])):
        assert torch.equal(a, b), f'{key} {sub}: output {i} differs from the all-trainable forward'
    for k in names:
        g = grads[k]
        if k not in sub:
            assert g is None, f'{key} {sub}: frozen input {k} has a gradient'
            continue
        assert g is not None, f'{key} {sub}: trainable input {k} has no gradient'
        assert g.shape == op.inputs[k].shape and g.dtype == torch.float32, (key, sub, k, g.shape, g.dtype)
        want = base[1][k] if expect is None else expect(k, base[1][k])
        if expect is None:
            tol, err = op.bounds[k]
            e = err(g, ref[k])
            print(f'{key} {"+".join(sub)}: d{k} {e:.2e} (bound {tol:.0e})')
            assert e < tol, (key, sub, k, e, tol)
        if not fallback(k, sub):
            assert torch.equal(g, want), f'{key} {sub}: d{k} differs from the all-trainable run, max |diff| {float((g - want).abs().max()):.3e}'


# ---------------------------------------------------------------------------------------------------------------- dense ops
def _bias_fallback(pairs):
    """fallback(name, subset) for (bias, its weight) pairs: the bias gradient is ``dy.sum(0)`` when the weight is frozen"""
    return lambda name, sub: any(name == b and w not in sub for b, w in pairs)


def _b16():
    from unidet3d_amd import precision as P
    return _stack(lambda: P.operands('bf16'), lambda: P.bf16_act_mode(True))()


def _b16_on(fn):
    """``fn`` with the bf16-activation data flow asserted on (dense16.py is what runs)"""
    def run(t):
        from unidet3d_amd import precision as P
        assert P.bf16_act()
        return fn(t)
    return run


def _build_linear(M, K, N, bias, b16):
    from unidet3d_amd import dense
    g = torch.Generator().manual_seed(M + N + int(bias))
    x = torch.randn(M, K, generator=g); w = torch.randn(N, K, generator=g) * 0.1; b = torch.randn(N, generator=g)
    inputs = dict(x=x, w=w, **(dict(b=b) if bias else {}))
    fn = lambda t: dense.linear(t['x'], t['w'], t.get('b'))                               # noqa: E731
    # fp32: test_dense_linear_fwd_bwd (dx 1e-5, dw 2e-5, db 1e-5); bf16: test_linear_bf16_self_consistent_and_close (1e-2, db 1e-5)
    bounds = dict(x=(1e-2, _rel), w=(1e-2, _rel), b=(1e-5, _rel)) if b16 else dict(x=(1e-5, _rel), w=(2e-5, _rel), b=(1e-5, _rel))
    return SimpleNamespace(fn=_b16_on(fn) if b16 else fn, inputs=inputs, ref=lambda t: F.linear(t['x'], t['w'], t.get('b')),
                           gos=[torch.randn(M, N, generator=g)], used=(0,), bounds=bounds, ctx=_b16 if b16 else contextlib.nullcontext)


for _M, _K, _N in ((130, 32, 64), (130, 32, 19), (1, 32, 64)):          # (.., 19): the padded-N head path; one row
    for _bias in (True, False):
        _register(f'linear_{_M}x{_K}x{_N}_{"bias" if _bias else "nobias"}', ('x', 'w', 'b') if _bias else ('x', 'w'),
                  lambda a=(_M, _K, _N, _bias): _build_linear(*a, False), _bias_fallback([('b', 'w')]))
for _bias in (True, False):
    _register(f'b16_linear_130x32x64_{"bias" if _bias else "nobias"}', ('x', 'w', 'b') if _bias else ('x', 'w'),
              lambda a=(130, 32, 64, _bias): _build_linear(*a, True), _bias_fallback([('b', 'w')]))


def _build_mlp(M, d_in, hid, d_out, act, fuse, b16):
    from unidet3d_amd import dense
    g = torch.Generator().manual_seed(M + hid + d_out)
    inputs = dict(x=torch.randn(M, d_in, generator=g), w1=torch.randn(hid, d_in, generator=g) * 0.1, b1=torch.randn(hid, generator=g),
                  w2=torch.randn(d_out, hid, generator=g) * 0.05, b2=torch.randn(d_out, generator=g))

    def ref(t):
        h = F.linear(t['x'], t['w1'], t['b1'])
        return F.linear(torch.relu(h) if act == 'relu' else F.gelu(h), t['w2'], t['b2'])
    fn = lambda t: dense.mlp(t['x'], t['w1'], t['b1'], t['w2'], t['b2'], act)             # noqa: E731
    if b16:     # test_mlp_bf16_close: GELU 2e-2 in the maximum norm, ReLU 6e-2 in the Frobenius norm (units next to zero switch sides)
        bound = (2e-2, _rel) if act == 'gelu' else (6e-2, _fro)
        ctx = _b16
    else:       # test_mlp_fused_epilogues_fwd_bwd: 3e-5, GELU as GEMM epilogue and as the stand-alone pass (dense.FUSE_GELU)
        bound = (3e-5, _rel)
        ctx = contextlib.nullcontext if fuse is None else (lambda: _attr(dense, 'FUSE_GELU', fuse))
    return SimpleNamespace(fn=_b16_on(fn) if b16 else fn, inputs=inputs, ref=ref, gos=[torch.randn(M, d_out, generator=g)], used=(0,),
                           bounds={k: bound for k in inputs}, ctx=ctx)


_MLP_IN = ('x', 'w1', 'b1', 'w2', 'b2')
for _shape in ((130, 32, 64, 32), (130, 32, 64, 19)):
    for _act, _fuse in (('relu', None), ('gelu', True), ('gelu', False)):
        _register('mlp_' + 'x'.join(map(str, _shape)) + f'_{_act}' + ({None: '', True: '_fused', False: '_unfused'}[_fuse]), _MLP_IN,
                  lambda a=_shape + (_act, _fuse): _build_mlp(*a, False), _bias_fallback([('b1', 'w1'), ('b2', 'w2')]))
for _act in ('relu', 'gelu'):
    _register(f'b16_mlp_130x32x64x32_{_act}', _MLP_IN, lambda a=(130, 32, 64, 32, _act, None): _build_mlp(*a, True),
              _bias_fallback([('b1', 'w1'), ('b2', 'w2')]))


def _build_layer_norm(M, C, res, n_out, b16):
    from unidet3d_amd import dense
    g = torch.Generator().manual_seed(M + C + n_out)
    x = torch.randn(M, C, generator=g) * 2 + 0.5; r = torch.randn(M, C, generator=g); w = torch.randn(C, generator=g); b = torch.randn(C, generator=g)
    inputs = dict(x=x, **(dict(r=r) if res else {}), w=w, b=b)

    def ref(t):
        y = F.layer_norm(t['x'] + t['r'] if res else t['x'], (C,), t['w'], t['b'], 1e-5)
        return (y,) * n_out
    fn = lambda t: dense.layer_norm(t['x'], t['w'], t['b'], 1e-5, t.get('r'), n_out)       # noqa: E731
    # test_layer_norm_fwd_bwd: dx, dres 1e-5, dgamma, dbeta 2e-5; with the bf16 copies the fp32 results are the same bits
    # (test_layer_norm_b16_copies_are_the_rounded_outputs), so the same bounds
    return SimpleNamespace(fn=_b16_on(fn) if b16 else fn, inputs=inputs, ref=ref, gos=[torch.randn(M, C, generator=g) for _ in range(n_out)],
                           used=tuple(range(n_out)), bounds=dict(x=(1e-5, _rel), r=(1e-5, _rel), w=(2e-5, _rel), b=(2e-5, _rel)),
                           ctx=_b16 if b16 else contextlib.nullcontext)


for _b16flag in (False, True):
    for _tag, _res, _n_out in (('res', True, 1), ('nores', False, 1), ('res_two_outputs', True, 2)):
        _register(('b16_' if _b16flag else '') + f'layer_norm_77x32_{_tag}', ('x', 'r', 'w', 'b') if _res else ('x', 'w', 'b'),
                  lambda a=(77, 32, _res, _n_out, _b16flag): _build_layer_norm(*a))


def _build_ln_linear(M, C, N, used, b16):
    from unidet3d_amd import dense
    g = torch.Generator().manual_seed(M + N)
    inputs = dict(x=torch.randn(M, C, generator=g) * 2 + 0.3, gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.1,
                  w=torch.randn(N, C, generator=g) * 0.1, b=torch.randn(N, generator=g))

    def ref(t):
        nq = F.layer_norm(t['x'], (C,), t['gamma'], t['beta'], 1e-5)
        return nq, F.linear(nq, t['w'], t['b'])
    fn = lambda t: dense.ln_linear(t['x'], t['gamma'], t['beta'], 1e-5, t['w'], t['b'])     # noqa: E731
    if b16:     # the Linear is a bf16 product: test_linear_bf16_self_consistent_and_close (1e-2); its bias gradient, the column sums of
        # the fp32 dy inside u3d_gemm_tn_b16: test_gemm_tn_b16_every_dtype_combination (2e-5)
        bounds = dict(x=(1e-2, _rel), gamma=(1e-2, _rel), beta=(1e-2, _rel), w=(1e-2, _rel), b=(2e-5, _rel))
    else:       # test_ln_linear_fwd_bwd: 3e-5 on every gradient
        bounds = {k: (3e-5, _rel) for k in inputs}
    return SimpleNamespace(fn=_b16_on(fn) if b16 else fn, inputs=inputs, ref=ref, gos=[torch.randn(M, C, generator=g), torch.randn(M, N, generator=g)],
                           used=used, bounds=bounds, ctx=_b16 if b16 else contextlib.nullcontext)


_LNL_IN = ('x', 'gamma', 'beta', 'w', 'b')
_register('ln_linear_130x32x8_both_outputs', _LNL_IN, lambda: _build_ln_linear(130, 32, 8, (0, 1), False))
_register('ln_linear_130x32x8_linear_output_only', _LNL_IN, lambda: _build_ln_linear(130, 32, 8, (1,), False))
_register('b16_ln_linear_130x32x8_both_outputs', _LNL_IN, lambda: _build_ln_linear(130, 32, 8, (0, 1), True))


@pytest.mark.parametrize('key,sub', _params('linear_'))
def test_linear_subsets(key, sub):
    _check(key, sub)


@pytest.mark.parametrize('key,sub', _params('mlp_'))
def test_mlp_subsets(key, sub):
    """includes only b1, only b2 and b1+b2 with both weights frozen: the bias gradients autograd used to get ``None`` for"""
    _check(key, sub)


@pytest.mark.parametrize('key,sub', _params('layer_norm_') + _params('ln_linear_'))
def test_layer_norm_and_ln_linear_subsets(key, sub):
    _check(key, sub)


@pytest.mark.parametrize('key,sub', _params('b16_'))
def test_bf16_activation_data_flow_subsets(key, sub):
    """the four dense ops through dense16.py (precision.bf16_act()), at the bounds of the bf16 tests"""
    _check(key, sub)


# ---------------------------------------------------------------------------------------------------------------- sparse convolution
_GEOM = {}


def _geometry():
    """two scenes of 3,000 synthetic points at 0.05 m (test_batchnorm_statistics_from_the_convolution_epilogue's smallest): SubM and
    strided rulebooks of the product and of the oracle"""
    if not _GEOM:
        from unidet3d_amd import ops, sparse
        from unidet3d_amd.synthetic import make_scene
        scenes = [make_scene(51 + i, n_points=3_000) for i in range(2)]
        vb = ops.voxelize([torch.from_numpy(s.points).to(DEV) for s in scenes], 0.05, 128)
        oc, oshape = vb.coords.cpu(), vb.spatial_shape
        oc2, _, down_pairs = so.build_down_rulebook(oc, oshape)
        _GEOM.update(n=len(oc), n2=len(oc2), subm=sparse.build_subm_rulebook(vb.coords, vb.index),
                     down=sparse.build_down_rulebook(vb.coords, 2, vb.spatial_shape)[3],
                     subm_pairs=so.build_subm_rulebook(oc, oshape), down_pairs=down_pairs, scenes=scenes, vb=vb)
        assert _GEOM['n'] > 256 and _GEOM['n2'] > 64                 # more than one row tile on both levels
    return _GEOM


def _build_conv(kind, cin, cout):
    from unidet3d_amd import sparse
    G = _geometry()
    n_src, n_dst, k, rb, pairs, mode = dict(subm=(G['n'], G['n'], 3, G['subm'], G['subm_pairs'], 'fwd'),
                                            strided=(G['n'], G['n2'], 2, G['down'], G['down_pairs'], 'fwd'),
                                            inverse=(G['n2'], G['n'], 2, G['down'], G['down_pairs'], 'inv'))[kind]
    g = torch.Generator().manual_seed(cin * 1000 + cout + k)
    inputs = dict(src=torch.randn(n_src, cin, generator=g), weight=torch.randn(cout, k, k, k, cin, generator=g) * 0.1,
                  addend=torch.randn(n_dst, cout, generator=g))
    # test_subm_conv_fwd_bwd: dsrc, dweight 1e-4, daddend 1e-6; test_strided_and_inverse_conv_fwd_bwd: 1e-4
    return SimpleNamespace(fn=lambda t: sparse.sparse_conv(t['src'], t['weight'], rb, mode, t['addend']),
                           ref=lambda t: so.sparse_conv(t['src'], t['weight'], pairs, n_dst, inverse=(kind == 'inverse')) + t['addend'],
                           inputs=inputs, gos=[torch.randn(n_dst, cout, generator=g)], used=(0,),
                           bounds=dict(src=(1e-4, _rel), weight=(1e-4, _rel), addend=(1e-6, _rel)), ctx=contextlib.nullcontext)


for _kind, _cin, _cout in (('subm', 32, 32), ('subm', 64, 32), ('strided', 32, 32), ('inverse', 32, 32)):
    _register(f'conv_{_kind}_{_cin}x{_cout}', ('src', 'weight', 'addend'), lambda a=(_kind, _cin, _cout): _build_conv(*a))


@contextlib.contextmanager
def _overlap(mode, log=None):
    """sparse.set_wgrad_overlap(mode) for the block; ``log`` (a list) receives, in order, every kernel launch ('launch', entry point, raw
    stream that was current) and every stream join ('wait', raw waiting stream, raw stream waited for)"""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import sparse
    prev = sparse.set_wgrad_overlap(mode)
    try:
        with pytest.MonkeyPatch.context() as mp:
            if log is not None:
                real_call, real_wait = L.call, torch.cuda.Stream.wait_stream

                def call(name, *args):
                    log.append(('launch', name, L.stream()))
                    return real_call(name, *args)

                def wait_stream(self, other):
                    log.append(('wait', self.cuda_stream, other.cuda_stream))
                    return real_wait(self, other)
                mp.setattr(L, 'call', call)
                mp.setattr(torch.cuda.Stream, 'wait_stream', wait_stream)
            yield
    finally:
        sparse.set_wgrad_overlap(prev)


def _side_launches_are_joined(log, main):
    """-> the side-stream launches of ``log``, after asserting that the main stream waited for each of those streams AFTER the launch"""
    side = [(i, e) for i, e in enumerate(log) if e[0] == 'launch' and e[2] != main]
    for i, (_, name, s) in side:
        assert any(e == ('wait', main, s) for e in log[i + 1:]), f'{name} ran on a side stream that the main stream never waited for'
    return [e for _, e in side]


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('key,sub', _params('conv_'))
def test_sparse_conv_subsets(key, sub, mode):
    """SubM 27-tap, strided and inverse convolution under set_wgrad_overlap 0 / 1 / 2, every gradient against the mode-0 all-trainable
    run bit for bit.  The weight gradient is read as soon as backward() has returned; on top of that the stream joins are observed
    directly (a missing join is a race, and a race does not show on every run): every stream a weight-gradient kernel was launched on
    is waited for by the main stream afterwards."""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import wgrad_stream as WS
    main = L.stream()
    log = []
    _state(key)                                                     # (the mode-0 base is not part of the log)
    _check(key, sub, ctx=lambda: _overlap(mode, log))
    assert L.stream() == main
    side = _side_launches_are_joined(log, main)
    wgrad_on_side = [e for e in side if e[1].startswith('u3d_spconv_wgrad')]
    assert len(wgrad_on_side) == (1 if mode and 'src' in sub and 'weight' in sub else 0), (mode, sub, side)
    assert not WS._ASYNC_DW_SEEN


@pytest.mark.parametrize('sub', [('weight',), ('weight', 'addend'), ('src', 'weight')], ids='+'.join)
def test_sparse_conv_mode_2_accumulates_into_an_existing_grad_in_line(sub):
    """set_wgrad_overlap(2) with a weight that already has a .grad: autograd ADDS dW on the main stream as soon as the layer's backward
    returns, so the kernel must not stay on the side stream unjoined (src frozen: in line; src trainable: joined inside the layer)."""
    from unidet3d_amd import _lib as L
    key, main, log = 'conv_subm_32x32', L.stream(), []
    _state(key)

    def pre(leaves):
        leaves['weight'].grad = torch.full_like(leaves['weight'], 0.25)
    _check(key, sub, ctx=lambda: _overlap(2, log), pre=pre, expect=lambda k, g: g + 0.25 if k == 'weight' else g)
    side = _side_launches_are_joined(log, main)
    assert len(side) == (1 if 'src' in sub else 0), side


# ---------------------------------------------------------------------------------------------------------------- batch norm
def _build_bn(relu, training, variant):
    """variant: 'plain' (no skip output) | 'skip_y' / 'skip_both' / 'skip_only' (skip=True; which outputs carry a gradient)"""
    from unidet3d_amd import sparse
    n, C = 1000, 32
    g = torch.Generator().manual_seed(C + int(relu) + 2 * int(training))
    x = torch.randn(n, C, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rm, rv = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    skip = variant != 'plain'
    used = dict(plain=(0,), skip_y=(0,), skip_both=(0, 1), skip_only=(1,))[variant]
    # only the skip output consumed: gamma and beta are not inputs of anything that is differentiated
    inputs = dict(x=x) if variant == 'skip_only' else dict(x=x, gamma=gamma, beta=beta)

    def fn(t):
        bn = sparse.SparseBatchNorm(C).to(DEV)
        bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
        for attr, name, const in (('weight', 'gamma', gamma), ('bias', 'beta', beta)):
            del bn._parameters[attr]
            setattr(bn, attr, t[name] if name in t else const.to(DEV))
        bn.train(training)
        return bn(t['x'], relu=relu, skip=skip)

    def ref(t):
        ga, be = t.get('gamma', gamma.double()), t.get('beta', beta.double())
        y = F.batch_norm(t['x'], None if training else rm.double(), None if training else rv.double(), ga, be, training, 0.1, 1e-4)
        y = torch.relu(y) if relu else y
        return (y, t['x'] * 1.0) if skip else y
    # test_batchnorm_relu_fwd_bwd: 1e-4 on dx, dgamma, dbeta
    return SimpleNamespace(fn=fn, ref=ref, inputs=inputs, gos=[torch.randn(n, C, generator=g), torch.randn(n, C, generator=g)], used=used,
                           bounds={k: (1e-4, _rel) for k in inputs}, ctx=contextlib.nullcontext)


for _relu in (True, False):
    for _training in (True, False):
        for _variant in ('plain', 'skip_y', 'skip_both', 'skip_only'):
            _register(f'bn_{"relu" if _relu else "norelu"}_{"train" if _training else "eval"}_{_variant}',
                      ('x',) if _variant == 'skip_only' else ('x', 'gamma', 'beta'), lambda a=(_relu, _training, _variant): _build_bn(*a))


@pytest.mark.parametrize('key,sub', _params('bn_'))
def test_batch_norm_subsets(key, sub):
    """sparse.SparseBatchNorm, training and eval() (the eval backward is a branch of its own), with and without the skip output"""
    _check(key, sub)


# ---------------------------------------------------------------------------------------------------------------- single-input ops
def _build_pool():
    from unidet3d_amd import ops
    G = _geometry()
    sps, bias = [], 0
    for s in G['scenes']:
        sp = torch.from_numpy(s.superpoints) + bias
        bias = int(sp.max()) + 1
        sps.append(sp)
    sp_all = torch.cat(sps)
    plan = ops.PoolPlan(G['vb'], sp_all.to(DEV), bias)
    inverse = G['vb'].inverse.cpu().long()
    g = torch.Generator().manual_seed(1)
    # test_superpoint_pool_and_centers: 1e-5
    return SimpleNamespace(fn=lambda t: ops.superpoint_pool(t['feats'], plan), ref=lambda t: so.scatter_mean(t['feats'][inverse], sp_all, dim_size=bias),
                           inputs=dict(feats=torch.randn(G['n'], 32, generator=g)), gos=[torch.randn(bias, 32, generator=g)], used=(0,),
                           bounds=dict(feats=(1e-5, _rel)), ctx=contextlib.nullcontext)


def _build_attention(lens):
    from unidet3d_amd.encoder import attention_varlen
    H, hd = 8, 32
    n = sum(lens)
    g = torch.Generator().manual_seed(n)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)

    def ref(t):
        outs, o = [], 0
        for ln in lens:
            q, k, v = [a.view(ln, H, hd).transpose(0, 1) for a in t['qkv'][o:o + ln].chunk(3, -1)]
            o += ln
            outs.append((torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), -1) @ v).transpose(0, 1).reshape(ln, H * hd))
        return torch.cat(outs)
    # test_attention_varlen_fwd_bwd: dqkv 2e-5
    return SimpleNamespace(fn=lambda t: attention_varlen(t['qkv'], cu, max(lens), H), ref=ref, inputs=dict(qkv=torch.randn(n, 3 * H * hd, generator=g) * 1.5),
                           gos=[torch.randn(n, H * hd, generator=g)], used=(0,), bounds=dict(qkv=(2e-5, _rel)), ctx=contextlib.nullcontext)


def _build_decode(form):
    from test_gpu_criterion_edges import _decode_ref
    from unidet3d_amd.encoder import _BoxDecode7Fn, _BoxDecodeFn
    M = 257
    g = torch.Generator().manual_seed(M)
    cen = torch.rand(M, 3, generator=g) * 4
    dof = 6 if form == 'six' else 7
    yaw = (torch.arange(M) % 2 == 0).to(torch.uint8) if form == 'seven_alternating' else None
    yd = None if yaw is None else yaw.to(DEV)
    fn = (lambda t: _BoxDecodeFn.apply(t['raw'], cen.to(DEV))) if dof == 6 else (lambda t: _BoxDecode7Fn.apply(t['raw'], cen.to(DEV), yd))
    # test_box_decode_kernels_match_fp64_restatement: 1e-6 of each row's largest reference entry
    return SimpleNamespace(fn=fn, ref=lambda t: _decode_ref(t['raw'], cen.double(), yaw, dof), inputs=dict(raw=torch.randn(M, 8, generator=g)),
                           gos=[(torch.rand(M, dof, generator=g) - 0.5) * 0.5], used=(0,), bounds=dict(raw=(1e-6, _rows)), ctx=contextlib.nullcontext)


_register('one_pool', ('feats',), _build_pool)
_register('one_attention_48_17', ('qkv',), lambda: _build_attention([48, 17]))
_register('one_attention_1_64_65', ('qkv',), lambda: _build_attention([1, 64, 65]))
for _form in ('six', 'seven', 'seven_alternating'):
    _register(f'one_box_decode_{_form}', ('raw',), lambda a=_form: _build_decode(a))


@pytest.mark.parametrize('key,sub', _params('one_'))
def test_single_input_ops(key, sub):
    """ops.superpoint_pool, encoder.attention_varlen, both box decodes: one differentiable input each, so what remains is that the
    forward does not depend on requires_grad (checked when the case is built) and that the gradient is there and right"""
    _check(key, sub)


# ---------------------------------------------------------------------------------------------------------------- fused criterion
def _build_criterion():
    import _criterion_edges as E
    import test_criterion_edges_cpu as EC
    from unidet3d_amd.registry import MODELS
    case, o64 = E.build('class_bookkeeping')
    scale = 1.3
    crit = MODELS.build(EC.CFG[case['crit']])
    crit.fused = True

    def fn(t):
        Ln = case['L']
        cls, box = [t['cls'][l] for l in range(Ln)], [t['box'][l] for l in range(Ln)]
        vc, vb = E.scene_views(case, cls, box)
        insts = EC.product_insts(case, DEV)
        pred = dict(cls_preds=vc[0], bboxes=vb[0], aux_outputs=[dict(cls_preds=vc[l], bboxes=vb[l]) for l in range(1, Ln)],
                    _packed=dict(cls=cls, box=box, sizes=list(case['sizes']), cls_stacked=t['cls'], box_stacked=t['box']))
        assert crit._can_fuse(pred, insts, case['names'])                  # the kernel is what runs
        return crit(pred, insts, case['names'])['det_loss']

    class _Ref(torch.autograd.Function):              # the fp64 oracle's loss and gradients (E.run_oracle), as computed for the CPU tests
        @staticmethod
        def forward(ctx, cls, box):
            return o64['loss'].double().clone()

        @staticmethod
        def backward(ctx, go):
            return torch.stack(o64['dcls']) * go, torch.stack(o64['dbox']) * go

    def blocks(got, want):          # EC.scene_errors: max |diff| / max |reference| of every (layer, scene) block
        got, want, worst = got.detach().double().cpu(), want.double(), 0.0
        for l in range(case['L']):
            o = 0
            for n in case['sizes']:
                a, b = got[l, o:o + n], want[l, o:o + n]
                o += n
                if float(b.abs().max()) == 0:
                    assert float(a.abs().max()) == 0
                else:
                    worst = max(worst, _rel(a, b))
        return worst
    # test_fused_criterion_edge_case_matches_fp64_oracle (EC.check_errors): 2e-5 per block on an axis-aligned batch
    return SimpleNamespace(fn=fn, ref=lambda t: _Ref.apply(t['cls'], t['box']), inputs=dict(cls=torch.stack(case['cls']), box=torch.stack(case['box'])),
                           gos=[torch.tensor(scale)], used=(0,), bounds=dict(cls=(2e-5, blocks), box=(2e-5, blocks)), ctx=contextlib.nullcontext)


_register('criterion_class_bookkeeping', ('cls', 'box'), _build_criterion)


@pytest.mark.parametrize('key,sub', _params('criterion_'))
def test_fused_criterion_subsets(key, sub):
    """logits frozen with boxes trainable, the reverse, and both, on a constructed batch of tests/_criterion_edges.py"""
    _check(key, sub)


# ---------------------------------------------------------------------------------------------------------------- the whole model
_E2E = {}


def _e2e():
    """the small end-to-end model of test_end_to_end_features_logits_boxes_loss_grads (one scene of 10,000 points at 0.05 m, weights from
    tests/_detw.py) and its baseline: one loss backward with every parameter trainable"""
    if not _E2E:
        import _parity as PA
        from unidet3d_amd.config import scannet_model_cfg
        from unidet3d_amd.data import make_batch_inputs
        from unidet3d_amd.dense import LayerNorm
        from unidet3d_amd.sparse import SparseBatchNorm
        from unidet3d_amd.synthetic import make_scene
        prod, orac = PA.build_pair(scannet_model_cfg(voxel_size=0.05))
        scenes = [make_scene(40, n_points=10_000)]
        inputs, samples = make_batch_inputs(scenes, DEV)
        names = [k for k, _ in prod.named_parameters()]
        norm = {f'{m}.{p}' for m, mod in prod.named_modules() if isinstance(mod, (SparseBatchNorm, LayerNorm)) for p, _ in mod.named_parameters(recurse=False)}
        assert norm and all(k in names for k in norm)
        S = dict(prod=prod, orac=orac, scenes=scenes, inputs=inputs, samples=samples, names=names, norm=norm)
        S['base'] = _e2e_step(S, {k: True for k in names})
        assert all(g is not None for g in S['base'][1].values())
        _E2E.update(S)
    return _E2E


def _e2e_step(S, trainable, ctx=contextlib.nullcontext):
    prod = S['prod']
    for k, p in prod.named_parameters():
        p.requires_grad_(trainable[k])
        p.grad = None
    try:
        with ctx():
            loss = prod.loss(S['inputs'], copy.deepcopy(S['samples']))['det_loss']
        loss.backward()
        return loss.detach().clone(), {k: (None if p.grad is None else p.grad.clone()) for k, p in prod.named_parameters()}
    finally:
        for p in prod.parameters():
            p.requires_grad_(True)
            p.grad = None


def _e2e_oracle_grads():
    """fp64 oracle gradients on the product's own activation pattern: the reference of the end-to-end test's gradient assertion"""
    if 'g64m' not in _E2E:
        import _parity as PA
        S = _E2E
        run = lambda m: PA.oracle_forward(m, S['scenes'], ['scannet'])                        # noqa: E731
        P = PA.product_forward(S['prod'], S['inputs'], copy.deepcopy(S['samples']), relu_masks=True)
        S['g64m'], _ = PA.oracle_fp64_grads_same_activation_pattern(S['orac'], run, P['relu_masks'])
    return _E2E['g64m']


# The decoder's Linear / MLP biases: with their weight frozen the gradient is ``dy.sum(0)`` instead of the column sums u3d_gemm_tn makes
# next to dW -- not the same bits.  (``out_bboxes.linear.bias`` always rides along in dense.ln_linear; norm biases come from the norm's
# own backward kernel either way.)
_FALLBACK_BIASES = ['decoder.input_proj.0.bias', 'decoder.input_proj.2.bias', 'decoder.outs_cls.0.bias', 'decoder.outs_cls.2.bias'] + \
    [f'decoder.self_attn_layers.{i}.attn.{b}' for i in range(6) for b in ('in_proj_bias', 'out_proj.bias')] + \
    [f'decoder.ffn_layers.{i}.net.{j}.bias' for i in range(6) for j in (0, 3)]


def _freeze_plan(case, names, norm):
    is_bias = lambda k: k.endswith('bias')                                                     # noqa: E731  (in_proj_bias included)
    return {'a_backbone_frozen': {k: k.startswith('decoder.') for k in names},
            'b_decoder_frozen': {k: not k.startswith('decoder.') for k in names},
            'c_biases_and_norms_frozen': {k: not (is_bias(k) or k in norm) for k in names},
            'c_biases_and_norms_frozen_in_transposed_weights': {k: not (is_bias(k) or k in norm) for k in names},
            'd_only_biases_trainable': {k: is_bias(k) for k in names}}[case]


@pytest.mark.parametrize('case', ['a_backbone_frozen', 'b_decoder_frozen', 'c_biases_and_norms_frozen',
                                  'c_biases_and_norms_frozen_in_transposed_weights', 'd_only_biases_trainable'])
def test_model_with_frozen_parameters(case):
    """One training step of the whole model with part of it frozen: the loss equals the all-trainable baseline's bit for bit, frozen
    parameters end with ``.grad is None``, every trainable parameter's gradient equals the baseline's bit for bit -- except, when only
    biases train (d), the Linear / MLP biases of ``_FALLBACK_BIASES`` (their weight is frozen: ``dy.sum(0)``), which are held to the
    end-to-end test's decoder-gradient bound instead: 1e-3 against the fp64 oracle on the product's activation pattern
    (test_end_to_end_features_logits_boxes_loss_grads / _parity.compare).  (c) runs a second time inside an outer
    ``dense.transposed_weights(model)``; that context collects trainable matrices only, so frozen ones take the op's own transpose."""
    from unidet3d_amd import dense
    S = _e2e()
    trainable = _freeze_plan(case, S['names'], S['norm'])
    assert any(trainable.values()) and not all(trainable.values())
    assert {k for k in S['names'] if k.startswith('decoder.')} and {k for k in S['names'] if not k.startswith('decoder.')}
    ctx = (lambda: dense.transposed_weights(S['prod'])) if case.endswith('transposed_weights') else contextlib.nullcontext
    loss, grads = _e2e_step(S, trainable, ctx)
    base_loss, base = S['base']
    assert torch.equal(loss, base_loss), (float(loss), float(base_loss))
    fallback = set(_FALLBACK_BIASES) if case.startswith('d_') else set()
    assert fallback <= set(S['names'])
    has_grad = [k for k in S['names'] if not trainable[k] and grads[k] is not None]
    assert not has_grad, f'frozen parameters with a gradient: {has_grad[:5]}'
    missing = [k for k in S['names'] if trainable[k] and grads[k] is None]
    assert not missing, f'{len(missing)} trainable parameters without a gradient: {missing[:6]}'
    differ = [k for k in S['names'] if trainable[k] and k not in fallback and not torch.equal(grads[k], base[k])]
    assert not differ, f'{len(differ)} gradients differ from the all-trainable step: {differ[:6]}'
    if fallback:
        g64m = _e2e_oracle_grads()
        errs = {k: _rel(grads[k], g64m[k]) for k in sorted(fallback)}
        print('bias gradients on the dy.sum(0) path against the fp64 oracle, worst:', sorted(errs.items(), key=lambda kv: -kv[1])[:3])
        assert max(errs.values()) < 1e-3, errs


# ---------------------------------------------------------------------------------------------------------------- state between calls
@pytest.mark.parametrize('op', ['linear', 'mlp'])
def test_weight_planes_of_an_updated_weight_are_not_reused(op, monkeypatch):
    """dense._planes_of: with the pre-split W planes on, a weight updated in place inside a transposed_weights()
    context (an in-forward optimizer step, an EMA swap that moves ``_version``) must not be multiplied from the planes the context
    made on entry.  The second forward equals a forward outside any context bit for bit (planes on or off is bit-identical), and
    the NEW weight's float64 product within test_dense_linear_fwd_bwd's 1e-5 / test_mlp_fused_epilogues_fwd_bwd's 1e-5."""
    from unidet3d_amd import dense
    from unidet3d_amd import precision as P
    monkeypatch.setattr(dense, '_W_PLANES', True)
    assert not P.bf16() and P.get_fp32_math() == 'bf16x3'
    torch.manual_seed(7)
    net = (torch.nn.Linear(32, 64) if op == 'linear' else torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.ReLU(), torch.nn.Linear(64, 32))).to(DEV)
    lins = [net] if op == 'linear' else [net[0], net[2]]
    x = torch.randn(130, 32, device=DEV)

    def forward(xin):
        if op == 'linear':
            return dense.linear(xin, net.weight, net.bias)
        return dense.mlp(xin, net[0].weight, net[0].bias, net[2].weight, net[2].bias, 'relu')

    def ref():
        h = x.double().cpu()
        for i, l in enumerate(lins):
            h = F.linear(torch.relu(h) if i else h, l.weight.detach().double().cpu(), l.bias.detach().double().cpu())
        return h
    with dense.transposed_weights(net):
        assert all(dense._planes_of(l.weight) is not None and dense._wt_of(l.weight) is not None for l in lins)      # not vacuous
        y_old = forward(x)
        assert _rel(y_old, ref()) < 1e-5
        with torch.no_grad():
            for l in lins:
                l.weight.data.mul_(2)            # (does not move _version on its own)
                l.weight.add_(0.125)             # moves it
        xg = x.clone().requires_grad_()
        y_new = forward(xg)
        y_new.backward(torch.ones_like(y_new))
    xo = x.clone().requires_grad_()
    y_out = forward(xo)                              # outside any context: the kernel splits W itself
    y_out.backward(torch.ones_like(y_out))
    assert not torch.equal(y_new, y_old)
    assert torch.equal(y_new, y_out), f'stale planes: max |diff| {float((y_new - y_out).abs().max()):.3e}'
    assert _rel(y_new, ref()) < 1e-5
    assert torch.equal(xg.grad, xo.grad)             # and the input gradient did not take the stale transposed copy either


def test_side_stream_is_used_again_after_a_backward_pass_that_raised():
    """wgrad_stream: a backward pass that dies of a Python exception (a tensor hook raising) never runs its
    end-of-backward callback.  The next pass over the same parameters must give the mode-0 gradients bit for bit, must launch its
    weight-gradient kernels on a side stream again (observed as in test_weight_gradient_kernels_run_on_the_side_stream_when_asked)
    and must leave no per-pass bookkeeping behind.  The exception is host-side only; no kernel is involved in it."""
    from unidet3d_amd import _lib as L
    from unidet3d_amd import dense, sparse
    from unidet3d_amd import wgrad_stream as WS
    rb, n = _geometry()['subm'], _geometry()['n']
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(n, 32, generator=g)
    shapes = dict(wc1=(32, 3, 3, 3, 32), wc2=(32, 3, 3, 3, 32), wl=(64, 32), bl=(64,))
    p0 = {k: torch.randn(*s, generator=g) * 0.05 for k, s in shapes.items()}

    def leaves():
        return x0.clone().to(DEV).requires_grad_(), {k: v.clone().to(DEV).requires_grad_() for k, v in p0.items()}

    def loss(x, p, hook=None):
        h = sparse.sparse_conv(x, p['wc1'], rb)
        if hook is not None:
            h.register_hook(hook)
        y = dense.linear(sparse.sparse_conv(h, p['wc2'], rb), p['wl'], p['bl'])
        return (y * y).sum()

    def boom(grad):
        raise RuntimeError('raised by a tensor hook')
    main = L.stream()
    x, p = leaves()
    loss(x, p).backward()                                            # mode 0 (asserted): the reference bits
    assert WS.mode() == 0
    want = dict(x=x.grad, **{k: t.grad for k, t in p.items()})
    log = []
    x, p = leaves()
    with _overlap(2, log):
        with pytest.raises(RuntimeError, match='raised by a tensor hook'):
            loss(x, p, boom).backward()
        torch.cuda.synchronize()
        assert p['wc1'].grad is None and x.grad is None              # the pass really stopped half way
        x.grad = None
        for t in p.values():
            t.grad = None                                            # zero_grad(set_to_none=True), as a training loop would
        del log[:]
        loss(x, p).backward()
        got = dict(x=x.grad, **{k: t.grad for k, t in p.items()})
    for k in want:
        assert got[k] is not None and torch.equal(got[k], want[k]), k
    side = _side_launches_are_joined(log, main)
    conv = [e for e in log if e[0] == 'launch' and e[1].startswith('u3d_spconv_wgrad')]
    lin = [e for e in log if e[0] == 'launch' and e[1].startswith('u3d_gemm_tn')]
    assert len(conv) == 2 and len(lin) == 1, [e[1] for e in log if e[0] == 'launch']
    assert all(e in side for e in conv + lin), 'a weight-gradient kernel of the pass after the failed one ran on the main stream'
    assert not WS._ASYNC_DW_SEEN
    assert L.stream() == main
