"""The native optimizer tail (unidet3d_amd/optim.py FlatAdamW, csrc/optim.hip) on the GPU: parity with torch.optim.AdamW +
clip_grad_norm_ in fp64, the gradient norm on values that under- and overflow fp32 sums, bit identity across runs / gradient sources /
alignment, ``None`` gradients, checkpoint exchange with torch.optim.AdamW in both directions, launch count and host waits, and three
steps of the model.

The parameter set: a dozen tensors whose sizes sit on every path of the kernels for chunk size C (``optim.CHUNK``): 1, 3, 4, 5, 18
(dword tails and whole four-element groups), C-1, C, C+1, 2C+3 (the last chunk of a row, more than one block), a 2-D (7, 33), and 16
and 257.  Listed in this order inside a ``FlatGradBucket`` most gradient views are not 16-byte aligned (the dword path); fresh gradient
tensors are aligned (the dwordx4 path).

The error bound of the parity tests is MEASURED against the parent's path in the same test, not fixed: on identical inputs
``FlatGradBucket.clip_grad_norm_`` + ``AdamW(fused=True)`` and ``FlatAdamW`` are both fp32 evaluations of one formula, so FlatAdamW's
max abs error against the fp64 oracle, per tensor, for parameters and both moments, must be <= 2 x the parent path's error on that
tensor (a different, equally valid rounding order) + one fp32 ulp of the largest parameter magnitude (the parent's error can be 0)."""
import copy
import functools

import numpy as np
import pytest
import torch

import _parity as PA
from _detw import fill_state_dict

pytestmark = pytest.mark.gpu
DEV = PA.DEV
STEPS, MAX_NORM, LR0 = 5, 10.0, 1e-2
# ~21 k elements of randn x scale: norm ~ 145 x scale -- clipping at 10 is active at scale 1 and 0.3, inactive at 0.01
SCALES = [1.0, 0.01, 1.0, 0.01, 0.3]


def _shapes():
    from unidet3d_amd import optim
    C = optim.CHUNK
    return [(1,), (3,), (4,), (5,), (18,), (C - 1,), (C,), (C + 1,), (2 * C + 3,), (7, 33), (16,), (257,)]


@functools.lru_cache(maxsize=None)
def _inputs():
    """(initial parameters, gradients per step): fp32 CPU tensors, shared by the tests and never written"""
    g = torch.Generator().manual_seed(11)
    inits = tuple(torch.randn(s, generator=g) for s in _shapes())
    grads = tuple(tuple(torch.randn(s, generator=g) * SCALES[k] for s in _shapes()) for k in range(STEPS))
    return inits, grads


class Rig:
    """One optimizer over the parameter set, two param groups (even positions: weight decay 0.05, odd: 0), lr through PolynomialLR.
    kind: 'oracle' (fp64 CPU torch.optim.AdamW + torch clip_grad_norm_), 'parent' (FlatGradBucket.clip_grad_norm_ + AdamW(fused=True)),
    'parent_fresh' (torch clip_grad_norm_ + AdamW(fused=True) on plain .grad tensors), 'flat' (FlatAdamW on bucket views),
    'flat_fresh' (FlatAdamW on fresh gradient tensors)."""

    def __init__(self, kind, inits):
        from unidet3d_amd import FlatAdamW
        from unidet3d_amd.dist import FlatGradBucket
        self.kind = kind
        dev, dt = ('cpu', torch.float64) if kind == 'oracle' else (DEV, torch.float32)
        self.params = [torch.nn.Parameter(t.detach().to(device=dev, dtype=dt).clone()) for t in inits]
        groups = [dict(params=self.params[0::2], weight_decay=0.05), dict(params=self.params[1::2], weight_decay=0.0)]
        self.bucket = FlatGradBucket(self.params) if kind in ('parent', 'flat') else None
        if kind == 'oracle':
            self.opt = torch.optim.AdamW(groups, lr=LR0)
        elif kind in ('parent', 'parent_fresh'):
            self.opt = torch.optim.AdamW(groups, lr=LR0, fused=True)
        else:
            self.opt = FlatAdamW(groups, lr=LR0, max_norm=MAX_NORM, bucket=self.bucket)
        self.sched = torch.optim.lr_scheduler.PolynomialLR(self.opt, total_iters=STEPS, power=1.0)

    def step(self, grads, none=()):
        """one step on the given fp32 CPU gradients (``none``: positions whose .grad is None); returns the total norm"""
        if self.bucket is not None:
            assert not none
            for v, g in zip(self.bucket.views, grads):
                v.copy_(g)
            self.bucket.attach()
        else:
            for i, (p, g) in enumerate(zip(self.params, grads)):
                p.grad = None if i in none else g.to(device=p.device, dtype=p.dtype)
        if self.kind == 'parent':
            norm = self.bucket.clip_grad_norm_(MAX_NORM)
            self.opt.step()
        elif self.kind in ('oracle', 'parent_fresh'):
            norm = torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
            self.opt.step()
        else:
            norm = self.opt.step()
        self.sched.step()
        return norm

    def result(self):
        out = dict(p=[], exp_avg=[], exp_avg_sq=[])
        for p in self.params:
            st = self.opt.state.get(p, {})
            out['p'].append(p.detach().cpu().clone())
            for k in ('exp_avg', 'exp_avg_sq'):
                out[k].append(st[k].detach().cpu().clone() if k in st else torch.zeros_like(p, device='cpu'))
        return out


def _run(kind, none_at=None):
    inits, grads = _inputs()
    rig = Rig(kind, inits)
    norms = [rig.step(grads[k], none=(none_at or {}).get(k, ())) for k in range(STEPS)]
    return rig, rig.result(), norms


def _check_bound(tag, flat, parent, oracle):
    """the module docstring's bound; prints and logs both errors per tensor"""
    ulp = float(np.spacing(np.float32(max(float(p.abs().max()) for p in oracle['p']))))
    rows, bad = [], []
    for key in ('p', 'exp_avg', 'exp_avg_sq'):
        for i, (f, q, o) in enumerate(zip(flat[key], parent[key], oracle[key])):
            ef = float((f.double() - o.double()).abs().max())
            ep = float((q.double() - o.double()).abs().max())
            rows.append(dict(tensor=f'{key}[{i}]', shape=list(f.shape), flat=ef, parent=ep))
            if not ef <= 2 * ep + ulp:
                bad.append(rows[-1])
    print(f'{tag}: max abs error against the fp64 oracle (FlatAdamW | parent path), ulp floor {ulp:.3e}')
    for r in rows:
        print(f"  {r['tensor']:>15} {str(r['shape']):>10}  {r['flat']:.3e} | {r['parent']:.3e}")
    PA.log_errors(tag, dict(ulp=ulp, rows=rows))
    assert not bad, bad


def _bits_equal(a, b):
    return all(torch.equal(x, y) for k in a for x, y in zip(a[k], b[k]))


def _ulp_close(got, want64):
    want = np.float32(want64)
    return abs(float(got) - float(want)) <= float(np.spacing(want))


@functools.lru_cache(maxsize=None)
def _reference_runs():
    """oracle, parent path and FlatAdamW (bucket views) over the 5 steps: computed once, read by several tests"""
    return {k: _run(k) for k in ('oracle', 'parent', 'flat')}


def test_parity_with_the_fp64_oracle_is_as_good_as_the_parent_path():
    runs = _reference_runs()
    (orig, ores, onorms), (_, pres, _), (frig, fres, fnorms) = runs['oracle'], runs['parent'], runs['flat']
    clipped = [float(n) > MAX_NORM for n in onorms]
    print('oracle norms', [float(n) for n in onorms], 'FlatAdamW', [float(n) for n in fnorms])
    assert any(clipped) and not all(clipped), onorms                     # clipping active on some steps, inactive on others
    lrs = [LR0 * (1 - k / STEPS) for k in range(STEPS + 1)]
    assert frig.opt.param_groups[0]['lr'] == pytest.approx(lrs[-1], abs=1e-12) and orig.opt.param_groups[1]['lr'] == pytest.approx(lrs[-1], abs=1e-12)
    for n, o in zip(fnorms, onorms):
        assert n.is_cuda and n.dim() == 0 and _ulp_close(n, float(o)), (float(n), float(o))
    # the step left the gradients unclipped (clip_grad_norm_ would have scaled them): the documented difference
    _, grads = _inputs()
    assert torch.equal(frig.bucket.views[8].cpu(), grads[-1][8])
    assert all(int(frig.opt.state[p]['step']) == STEPS and not frig.opt.state[p]['step'].is_cuda for p in frig.params)
    _check_bound('optim_parity_5_steps', fres, pres, ores)


@pytest.mark.parametrize('case', ['1e-30 and 1e18', 'all 1e-30'])
def test_norm_is_the_fp64_norm_rounded_once(case):
    """Squares are exact in fp64 and summed in fp64: the returned norm is the fp64 oracle's rounded to fp32, within 1 ulp -- also when
    an fp32 accumulator would overflow (1e18 squared) or flush the squares to zero (1e-30 squared)."""
    inits, grads = _inputs()
    g = [t.clone() for t in grads[0]]
    if case == 'all 1e-30':
        g = [torch.full_like(t, 1e-30) for t in g]
    else:
        g[5] = torch.full_like(g[5], 1e-30)
        g[8] = torch.full_like(g[8], 1e18)
    for kind in ('flat', 'flat_fresh'):
        want = float(Rig('oracle', inits).step(g))
        rig = Rig(kind, inits)
        got = rig.step(g)
        print(case, kind, 'norm', float(got), 'oracle', want)
        assert 0 < want < 3e38 and _ulp_close(got, want), (case, kind, float(got), want)
        assert all(bool(torch.isfinite(p).all()) for p in rig.params)


def test_results_are_bit_identical_across_runs_sources_and_alignment():
    from unidet3d_amd import FlatAdamW, optim
    first = _reference_runs()['flat'][1]
    again = _run('flat')[1]
    assert _bits_equal(first, again)                                       # (a) the same inputs twice
    rig, fresh, _ = _run('flat_fresh')
    assert rig.opt.uploads >= 1
    assert _bits_equal(first, fresh)                                       # (b) bucket views (mostly misaligned) against fresh tensors
    assert rig.bucket is None
    views = _reference_runs()['flat'][0].bucket.views
    assert sum(v.data_ptr() % 16 != 0 for v in views) >= 6                 # the bucket run did take the dword path
    # (c) one tensor, gradient through an aligned and through a misaligned view
    n = 2 * optim.CHUNK + 3
    g = torch.Generator().manual_seed(12)
    w0 = torch.randn(n, generator=g)
    gs = [torch.randn(n, generator=g) * s for s in (1.0, 0.01, 0.3)]
    out = []
    for off in (4, 1):
        p = torch.nn.Parameter(w0.to(DEV).clone())
        opt = FlatAdamW([p], lr=LR0, weight_decay=0.05, max_norm=MAX_NORM)
        buf = torch.zeros(n + 8, device=DEV)
        p.grad = buf[off:off + n]
        assert (p.grad.data_ptr() % 16 == 0) == (off == 4)
        for gk in gs:
            p.grad.copy_(gk)
            opt.step()
        assert opt.uploads == 1
        out.append([p.detach().clone(), opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()])
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert not torch.equal(out[0][0].cpu(), w0)


def test_none_gradients_skip_the_parameter_like_torch():
    """Position 6 (numel C) has no gradient on steps 2 and 3 of 5: no decay and no moment update on those steps, its bias correction
    lags (its own step count ends at 3).  Position 9 never gets one: bit-unchanged, no state."""
    none_at = {k: ((6, 9) if k in (1, 2) else (9,)) for k in range(STEPS)}
    inits, _ = _inputs()
    (orig, ores, _), (_, pres, _), (frig, fres, _) = (_run(k, none_at) for k in ('oracle', 'parent_fresh', 'flat_fresh'))
    assert float(frig.opt.state[frig.params[6]]['step']) == 3 == float(orig.opt.state[orig.params[6]]['step'])
    assert float(frig.opt.state[frig.params[0]]['step']) == STEPS
    assert torch.equal(fres['p'][9], inits[9]) and len(frig.opt.state.get(frig.params[9], {})) == 0
    assert not torch.equal(fres['p'][6], inits[6])
    _check_bound('optim_none_gradients', fres, pres, ores)


def _resume(kind_a, kind_b):
    """3 steps with kind_a, state_dict into kind_b (fresh parameters holding kind_a's values), 2 more steps"""
    inits, grads = _inputs()
    a = Rig(kind_a, inits)
    for k in range(3):
        a.step(grads[k])
    b = Rig(kind_b, [p.detach().cpu() for p in a.params])
    b.opt.load_state_dict(copy.deepcopy(a.opt.state_dict()))
    b.sched.load_state_dict(a.sched.state_dict())
    return a, b, grads


def test_checkpoints_move_between_torch_adamw_and_flat_adamw():
    runs = _reference_runs()
    ores, pres = runs['oracle'][1], runs['parent'][1]
    # torch.optim.AdamW -> FlatAdamW
    a, b, grads = _resume('parent', 'flat')
    flat = b.opt
    lo = flat._exp_avg.data_ptr()
    hi = lo + flat._exp_avg.numel() * 4
    for p in b.params:
        st = flat.state[p]
        assert lo <= st['exp_avg'].data_ptr() < hi and st['exp_avg'].untyped_storage().data_ptr() == flat._exp_avg.untyped_storage().data_ptr()
        assert st['exp_avg_sq'].untyped_storage().data_ptr() == flat._exp_avg_sq.untyped_storage().data_ptr()
        assert float(st['step']) == 3
    for k in (3, 4):
        b.step(grads[k])
    _check_bound('optim_resume_torch_to_flat', b.result(), pres, ores)
    # FlatAdamW -> torch.optim.AdamW
    a, b, grads = _resume('flat', 'parent')
    assert all(float(a.opt.state[p]['step']) == 3 for p in a.params)
    for k in (3, 4):
        b.step(grads[k])
    assert all(float(b.opt.state[p]['step']) == STEPS for p in b.params)
    assert all(float(a.opt.state[p]['step']) == 3 for p in a.params)      # the loaded optimizer does not count into the saved one
    _check_bound('optim_resume_flat_to_torch', b.result(), pres, ores)


def _record_calls(monkeypatch):
    """every ``_lib.call`` (by entry point) and every ``_lib.h2d`` ('h2d') from here on in the returned list"""
    from unidet3d_amd import _lib as L
    log, real, real_h2d = [], L.call, L.h2d

    def call(name, *args):
        log.append(name)
        return real(name, *args)

    def h2d(*args, **kwargs):
        log.append('h2d')
        return real_h2d(*args, **kwargs)
    monkeypatch.setattr(L, 'call', call)
    monkeypatch.setattr(L, 'h2d', h2d)
    return log


def test_steady_state_is_three_launches_no_upload_and_no_host_wait(monkeypatch):
    from unidet3d_amd import optim
    inits, grads = _inputs()
    rig = Rig('flat', inits)
    log = _record_calls(monkeypatch)
    rig.step(grads[0])
    assert log.count('h2d') == 1                                           # the first step uploads the table
    del log[:]
    rig.step(grads[1])                                                     # the scheduler moved the lr: one upload
    assert log.count('h2d') == 1
    rig.opt.step()                                                         # (and once more after the second scheduler step)
    del log[:]
    # steady state: the gradients are the bucket's views, the lr stands still
    rig.opt.step()
    rig.opt.step()
    assert log == ['u3d_optim_grad_sumsq', 'u3d_optim_adamw'] * 2, log     # at most three u3d_optim_* calls per step, no h2d
    rig.opt.max_norm = 0.0                                                 # no clipping: no norm launch, nothing returned
    del log[:]
    assert rig.opt.step() is None and log == ['u3d_optim_adamw']
    rig.opt.max_norm = MAX_NORM
    rig.opt.param_groups[1]['lr'] *= 0.5                                   # one group's lr: exactly one upload
    del log[:]
    rig.opt.step()
    assert log.count('h2d') == 1 and len(log) == 3
    del log[:]
    rig.opt.step()
    assert 'h2d' not in log
    # no host synchronisation: step() returns while a long stretch of work queued in front of it is still running
    x = torch.randn(4096, 4096, device=DEV)
    (x @ x).sum().item()                                                   # warm the GEMM up
    torch.cuda.synchronize()
    for _ in range(40):
        y = x @ x
    ev = torch.cuda.Event()
    ev.record()
    norm = rig.opt.step()
    still_running = not ev.query()
    torch.cuda.synchronize()
    assert still_running, 'the queue in front of step() had drained when it returned: step() waited for the device (or the stretch was too short)'
    assert float(norm) > 0 and y.shape == x.shape
    # through the registry, as a config would
    built = optim.OPTIMIZERS.build(dict(type='FlatAdamW', params=rig.params, lr=2e-4, weight_decay=0.05, max_norm=10))
    assert isinstance(built, optim.FlatAdamW) and float(built.step()) > 0


def test_three_steps_of_the_model_match_torch_adamw_and_eval_sees_the_weights():
    """UniDet3D on one tiny scene, 3 steps of loss.backward() + FlatAdamW.for_model(model, max_norm=10).step() against an identically
    initialised model stepped by clip_grad_norm_ + AdamW(fused=False): the same losses to the run-to-run noise bound of
    test_gpu_gradients.py::test_convolutions_see_the_weights_an_optimizer_step_wrote (2e-6 relative).  Then, in eval mode, a native
    step between two forwards: the second one runs on the stepped weights (FlatAdamW writes through raw pointers, Tensor._version
    does not move; for_model wires invalidate_weight_packs)."""
    import unidet3d_amd  # noqa: F401
    from unidet3d_amd import FlatAdamW
    from unidet3d_amd.config import build_model, scannet_model_cfg
    from unidet3d_amd.data import make_batch_inputs
    from unidet3d_amd.synthetic import make_scene
    cfg = scannet_model_cfg(voxel_size=0.05)
    cfg['decoder']['num_layers'] = 2
    sc = make_scene(44, n_points=9000)
    inputs, samples0 = make_batch_inputs([sc], DEV)
    losses = {}
    for kind in ('flat', 'torch'):
        model = fill_state_dict(build_model(cfg), tag0=3600, scale=0.06).to(DEV).train()
        opt = FlatAdamW.for_model(model, max_norm=10) if kind == 'flat' else torch.optim.AdamW(model.parameters(), fused=False)
        losses[kind] = []
        for _ in range(3):
            for p in model.parameters():
                p.grad = None
            loss = model.loss(inputs, copy.deepcopy(samples0))['det_loss']
            loss.backward()
            if kind == 'torch':
                torch.nn.utils.clip_grad_norm_(model.parameters(), 10)
            opt.step()
            losses[kind].append(float(loss.detach()))
        if kind == 'flat':
            flat_model, flat_opt = model, opt
    print('losses FlatAdamW', losses['flat'], 'AdamW(fused=False)', losses['torch'])
    assert abs(losses['flat'][2] - losses['flat'][0]) > 1e-3 * abs(losses['flat'][0])          # the steps moved the loss
    for a, b in zip(losses['flat'], losses['torch']):
        assert abs(a - b) <= 2e-6 * abs(b), (losses['flat'], losses['torch'])
    # eval mode: forward, native step (the gradients of the last backward are still there), forward
    sp = torch.from_numpy(sc.superpoints).to(DEV)
    S = int(sc.superpoints.max()) + 1

    def run(m):
        with torch.no_grad():
            m.collate(inputs['points'])
            return m.extract_feat(m._sparse_input(1), sp, m._vb.inverse, [0, S])[0].clone()
    flat_model.eval()
    before = run(flat_model)
    assert PA.rel(before, run(flat_model)) < 1e-6
    flat_opt.step()
    after = run(flat_model)
    fresh = build_model(cfg).to(DEV).eval()
    fresh.load_state_dict(flat_model.state_dict(), strict=True)
    assert PA.rel(after, run(fresh)) < 1e-5
    assert PA.rel(before, after) > 1e-5, PA.rel(before, after)
