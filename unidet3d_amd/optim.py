"""Native optimizer tail: gradient-norm clipping and AdamW over every parameter of a model in two launches (csrc/optim.hip).

``FlatAdamW`` is ``torch.nn.utils.clip_grad_norm_(max_norm)`` followed by ``torch.optim.AdamW.step()`` -- the reference's
``optim_wrapper`` (``AdamW lr=2e-4 wd=0.05``, ``clip_grad max_norm=10``; configs/unidet3d_1xb8_scannet.py:710-715) -- with these
properties: bit-reproducible (no atomics, fixed-order sums), no host synchronisation, gradients are read once per launch and never
written.  One difference from ``clip_grad_norm_`` follows from the last: ``p.grad`` is left UNCLIPPED after ``step()``; the clip
coefficient is applied to the values as the update kernel reads them.

Registered as ``FlatAdamW`` in mmengine's ``OPTIMIZERS`` when mmengine imports (a config then selects it with
``optimizer=dict(type='FlatAdamW', lr=2e-4, weight_decay=0.05, max_norm=10)`` and drops ``clip_grad`` from the wrapper), in a local
registry of the same surface otherwise.
"""
from __future__ import annotations

import struct

import torch

from . import _lib as L
from .registry import _Registry
from .wgrad_stream import join_wgrad_stream

try:  # pragma: no cover - mmengine is not installed in the build image
    from mmengine.registry import OPTIMIZERS  # type: ignore
    HAVE_MMENGINE = True
except Exception:  # noqa: BLE001
    OPTIMIZERS = _Registry('optimizer')
    HAVE_MMENGINE = False


def __getattr__(name):
    # optim.CHUNK: elements of one parameter that a block covers (include/u3d.h U3D_OPTIM_CHUNK), asked of the library that is loaded
    # -- lazily, because this module is imported with the package, which must import before the library is built
    if name == 'CHUNK':
        return L.lib().u3d_optim_chunk()
    raise AttributeError(name)


def _f64_bits(x: float) -> int:
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


class FlatAdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay) with optional global-norm gradient clipping, on the HIP kernels of csrc/optim.hip.

    * ``lr`` and ``weight_decay`` are per param group and read from ``param_groups`` at every ``step()`` (LR schedulers work
      unmodified); ``betas`` and ``eps`` must be the same in every group (they are scalar arguments of the launch).
    * ``max_norm > 0``: the global L2 norm of all gradients is computed (fp64 accumulation), ``step()`` returns it as a 0-d device
      tensor and the update uses ``g * min(1, max_norm / (norm + 1e-6))``.  ``max_norm <= 0``: no clipping, no norm launch, ``None``.
      ``p.grad`` itself is never written (unlike ``clip_grad_norm_``).
    * The moments live in two flat fp32 buffers; ``state[p]['exp_avg']`` / ``['exp_avg_sq']`` are views of them, ``state[p]['step']``
      a 0-d CPU tensor as in ``torch.optim.AdamW``.  ``state_dict()`` / ``load_state_dict()`` are interchangeable with torch's.
    * A gradient is whatever ``p.grad`` is at ``step()``: a view of ``FlatGradBucket.flat`` or a fresh tensor from backward (a one-GPU
      loop needs no ``pack()``).  A parameter whose ``.grad`` is ``None`` is skipped as torch skips it: no decay, no moment update, its
      step count does not advance.  The device table is uploaded again only when a pointer, an lr, a weight decay or the set of
      ``None`` gradients changed since the previous step.
    * ``on_step`` (optional callable) runs after the launches; ``for_model`` wires it to ``model.invalidate_weight_packs()``.
    * ``bucket``: a ``dist.FlatGradBucket`` over the same parameters; ``step()`` then checks that every gradient it is given lies in
      the bucket's flat buffer (a forgotten ``pack()`` raises instead of silently skipping the all-reduced values).
    No amsgrad / maximize / capturable / closure, fp32 CUDA parameters only: anything else raises (there is no fallback path).
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 capturable=False, max_norm=0.0, bucket=None, on_step=None):
        if not (isinstance(lr, (int, float)) and lr >= 0.0):
            raise ValueError(f'invalid learning rate: {lr!r}')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f'invalid betas: {betas!r}')
        if eps < 0.0 or weight_decay < 0.0:
            raise ValueError(f'invalid eps / weight_decay: {eps!r} / {weight_decay!r}')
        # the keys of torch.optim.AdamW's groups, so that a state_dict of either class loads into the other
        defaults = dict(lr=float(lr), betas=tuple(betas), eps=float(eps), weight_decay=float(weight_decay), amsgrad=amsgrad,
                        maximize=maximize, foreach=None, capturable=capturable, differentiable=False, fused=None,
                        decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self.max_norm = float(max_norm)
        self.bucket = bucket
        self.on_step = on_step
        self._check_groups()
        self._params = [p for g in self.param_groups for p in g['params']]
        if not self._params:
            raise ValueError('FlatAdamW got no parameters')
        for p in self._params:
            if not p.is_cuda:
                raise L.U3DError('FlatAdamW needs CUDA (HIP) parameters: the product path has no CPU fallback')
            if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                raise L.U3DError(f'FlatAdamW needs dense contiguous fp32 parameters, got {p.dtype} {tuple(p.shape)}')
        self._dev = self._params[0].device
        if any(p.device != self._dev for p in self._params):
            raise L.U3DError('FlatAdamW: all parameters must be on one device')
        chunk = L.lib().u3d_optim_chunk()
        self._moff, self._block0, off, blocks = [], [], 0, 0
        for p in self._params:
            self._moff.append(off)
            self._block0.append(blocks)
            off += (p.numel() + 3) // 4 * 4               # every row's moments start 16-byte aligned
            blocks += (p.numel() + chunk - 1) // chunk
        self._blocks = blocks
        self._exp_avg = torch.zeros(max(off, 4), dtype=torch.float32, device=self._dev)
        self._exp_avg_sq = torch.zeros(max(off, 4), dtype=torch.float32, device=self._dev)
        self._views = [(self._exp_avg[o:o + p.numel()].view_as(p), self._exp_avg_sq[o:o + p.numel()].view_as(p))
                       for p, o in zip(self._params, self._moff)]
        self._steps = torch.zeros(len(self._params), dtype=torch.float32)       # state[p]['step'] are 0-d views of this CPU tensor
        self._t = [0] * len(self._params)                 # the same counts as Python ints
        self._gstep = 0                                   # global step: max over the parameters
        self._ws = L.ws(L.lib().u3d_optim_ws_bytes(), self._dev)
        self._key = None                                  # what the uploaded table was built from
        self._rows = None
        self._index_cache = {}
        self.uploads = 0                                  # table uploads so far (tools/optim_time.py, tests)

    @classmethod
    def for_model(cls, model, **kwargs):
        """``FlatAdamW(model.parameters(), ...)`` whose ``on_step`` invalidates the model's packed convolution weights, so that an
        eval-mode forward can never reuse packs from before a native step (sparse.WeightPacks keys on ``Tensor._version``, which
        a kernel that writes through raw pointers does not bump)."""
        inv = getattr(model, 'invalidate_weight_packs', None)
        if callable(inv):
            kwargs.setdefault('on_step', inv)
        return cls(model.parameters(), **kwargs)

    def _check_groups(self):
        g0 = self.param_groups[0]
        for g in self.param_groups:
            for flag in ('amsgrad', 'maximize', 'capturable', 'differentiable'):
                if g.get(flag):
                    raise L.U3DError(f'FlatAdamW does not implement {flag}=True (no fallback path)')
            if not g.get('decoupled_weight_decay', True):
                raise L.U3DError('FlatAdamW implements decoupled weight decay only (AdamW, not Adam with L2)')
            if isinstance(g['lr'], torch.Tensor):
                raise L.U3DError('FlatAdamW needs a float lr (a tensor lr would have to be read back from the device)')
            if tuple(g['betas']) != tuple(g0['betas']) or g['eps'] != g0['eps']:
                raise L.U3DError('FlatAdamW needs the same betas and eps in every param group')

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def _init_state(self, i):
        m, v = self._views[i]
        self.state[self._params[i]] = {'step': self._steps[i], 'exp_avg': m, 'exp_avg_sq': v}

    def state_dict(self):
        """torch.optim.AdamW's layout.  The step counts are copies (torch's loader keeps the tensor it is given and increments it in
        place); the moments are the views, as torch returns its own state tensors."""
        sd = super().state_dict()
        sd['state'] = {k: {**v, 'step': v['step'].clone()} if 'step' in v else v for k, v in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Accepts a state_dict of ``torch.optim.AdamW`` or of this class.  The base class replaces the state tensors with copies;
        their values are copied into the flat buffers here and ``state[p]`` is pointed back at the views."""
        super().load_state_dict(state_dict)
        self._check_groups()
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            m, v = self._views[i]
            if st and 'exp_avg' in st:
                m.copy_(st['exp_avg'])
                v.copy_(st['exp_avg_sq'])
                self._t[i] = int(round(float(st['step'])))
                self._steps[i] = self._t[i]
                self._init_state(i)
            else:
                m.zero_()
                v.zero_()
                self._t[i] = 0
                self._steps[i] = 0
                self.state.pop(p, None)
        self._gstep = max(self._t)
        self._key = None

    # ---- step -------------------------------------------------------------------------------------------------------------------
    def _upload(self, gptrs, pptrs, hyper):
        rows = []
        it = iter(range(len(self._params)))
        for g, (lr, wd) in zip(self.param_groups, hyper):
            lr_b, wd_b = _f64_bits(lr), _f64_bits(wd)
            for _ in g['params']:
                i = next(it)
                # (a skipped row's lag is not read; it is rebuilt when the parameter gets a gradient again: the set of None changes)
                rows.append([pptrs[i], gptrs[i], self._moff[i], self._params[i].numel(), lr_b, wd_b, self._gstep - self._t[i], self._block0[i]])
        self._rows = L.h2d(rows, torch.int64, self._dev)
        self.uploads += 1

    @torch.no_grad()
    def step(self, closure=None):
        """One clip + AdamW step on the current stream.  Returns the total gradient norm (0-d fp32 device tensor; before clipping)
        when ``max_norm > 0``, else ``None``.  Never waits for the device."""
        if closure is not None:
            raise L.U3DError('FlatAdamW.step() takes no closure (it returns the gradient norm, not a loss)')
        join_wgrad_stream()                        # weight gradients still running on a side stream (wgrad_stream, mode 2)
        gptrs = []
        for p in self._params:
            g = p.grad
            if g is None:
                gptrs.append(0)
                continue
            if g.dtype != torch.float32 or g.device != self._dev or g.is_sparse or not g.is_contiguous():
                raise L.U3DError(f'FlatAdamW needs dense contiguous fp32 gradients on {self._dev}, got {g.dtype} on {g.device}')
            gptrs.append(g.data_ptr())
        live = [i for i, a in enumerate(gptrs) if a]
        if self.bucket is not None:
            lo = self.bucket.flat.data_ptr()
            hi = lo + self.bucket.flat.numel() * 4
            if any(not lo <= gptrs[i] < hi for i in live):
                raise L.U3DError('FlatAdamW(bucket=...): a gradient is not a view of the bucket (call pack() / finish() before step())')
        clip = self.max_norm > 0.0
        if not live:
            return torch.zeros((), dtype=torch.float32, device=self._dev) if clip else None
        pptrs = [p.data_ptr() for p in self._params]
        hyper = [(float(g['lr']), float(g['weight_decay'])) for g in self.param_groups]
        key = (tuple(gptrs), tuple(pptrs), tuple(hyper))
        if len(live) == len(self._params):
            self._steps += 1
        else:
            idx = self._index_cache.get(key[0])
            if idx is None:
                self._index_cache.clear()
                idx = self._index_cache.setdefault(key[0], torch.tensor(live, dtype=torch.int64))
            self._steps[idx] += 1
        for i in live:
            if not self._t[i]:
                self._init_state(i)
            self._t[i] += 1
        # the global step advances with the parameters that moved, so the lag of a row that is in use never changes between uploads
        self._gstep += 1
        if key != self._key:
            self._gstep = max(self._t)             # (a parameter ahead of the global count: only after a load_state_dict)
            self._upload(gptrs, pptrs, hyper)
            self._key = key
        g0 = self.param_groups[0]
        rows, n, s = L.ptr(self._rows), len(self._params), L.stream()
        norm = None
        if clip:
            norm = torch.empty((), dtype=torch.float32, device=self._dev)
            L.call('u3d_optim_grad_sumsq', rows, n, self._blocks, L.ptr(self._ws), s)
        L.call('u3d_optim_adamw', rows, n, self._blocks, L.ptr(self._exp_avg), L.ptr(self._exp_avg_sq), float(g0['betas'][0]),
               float(g0['betas'][1]), float(g0['eps']), self.max_norm if clip else 0.0, self._gstep, L.ptr(self._ws),
               L.ptr(norm), s)
        if self.on_step is not None:
            self.on_step()
        return norm


OPTIMIZERS.register_module(module=FlatAdamW)
