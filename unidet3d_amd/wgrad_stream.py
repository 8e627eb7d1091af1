"""Weight gradients on a side stream: the mode, the stream pool, the one launch protocol and the joins.

Shared by the sparse convolutions (sparse.py) and the decoder's Linear layers (dense.py, dense16.py); ``dist.FlatGradBucket`` joins
before it copies a bucket.  Modes (U3D_WGRAD_SIDE_STREAM / ``set_wgrad_overlap``; ``sparse`` re-exports the public names):
  0  off: every kernel of the backward pass on the one stream;
  1  the weight gradient of a sparse convolution runs next to that layer's input gradient and is joined before the layer's backward
     returns (round 2: +0.9 % step throughput);
  2  decoupled: the weight gradients form their own chain on the side stream -- each waits for the gradient it reads, nothing on the
     main stream waits for them until the backward pass ends (an autograd-engine callback joins the streams; FlatGradBucket joins
     before it copies a bucket).  Nothing downstream of a layer needs its dW, so the dgrad / batch-norm chain never stalls on a
     weight-gradient kernel, and the small-level kernels of both chains (a few dozen workgroups each) share the chip.
Overlapped kernels stretch each other, so the bench's per-family HIP-event timings are taken with the overlap off.
"""
from __future__ import annotations

import os
from typing import Dict

import torch

_MODE = int(os.environ.get('U3D_WGRAD_SIDE_STREAM', '0') or 0)       # the ONE binding: read it through mode()
_N_SIDE = max(1, int(os.environ.get('U3D_SIDE_STREAMS', '1') or 1))      # weight-gradient chains (round-robin); A/B: tools, DESIGN.md 4.14
_SIDE: Dict = {}
_SIDE_RR: Dict = {}
_JOIN_PENDING: Dict = {}
_ASYNC_DW_SEEN: Dict = {}       # id(parameter) -> pass (``_pass_id``) whose dW of that parameter went to the side stream


def set_wgrad_overlap(mode: int) -> int:
    global _MODE
    prev, _MODE = _MODE, int(mode)
    return prev


def mode() -> int:
    return _MODE


def _side_stream(device):
    """next weight-gradient stream of ``device`` (round-robin over U3D_SIDE_STREAMS streams)"""
    if device not in _SIDE:
        _SIDE[device] = [torch.cuda.Stream(device=device) for _ in range(_N_SIDE)]
        _SIDE_RR[device] = 0
    i = _SIDE_RR[device]
    _SIDE_RR[device] = (i + 1) % len(_SIDE[device])
    return _SIDE[device][i]


def run_on_side_stream(device, launch, reads):
    """The launch protocol, once: the next side stream waits for everything queued on the current stream (the gradient the kernel
    reads is complete), ``launch()`` runs with the side stream current (``_lib.scratch`` then hands it that stream's own workspace),
    the tensors in ``reads`` -- everything the side kernel reads or writes that was allocated on the main stream -- are kept from
    being recycled under it, and the tensors ``launch`` returns (allocated from the side stream's pool, consumed on the main stream
    after the join; None entries allowed) are kept for their consumer.  Returns (side stream, what ``launch`` returned).  Joining is
    the caller's: ``queue_join(device)`` (mode 2), or a ``wait_stream`` of its own once it has queued the work that is to overlap."""
    main = torch.cuda.current_stream(device)
    side = _side_stream(device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        made = launch()
    for t in reads:
        t.record_stream(side)
    for t in made or ():
        if t is not None:
            t.record_stream(main)
    return side, made


def _pass_id() -> int:
    """The running backward pass: the autograd engine's graph-task id (-1 outside a backward pass).  Ids grow for the life of the process,
    and a nested pass (a backward call made inside a backward pass) has its own, larger than the pass around it."""
    return torch._C._current_graph_task_id()


def async_dw_ok(*params) -> bool:
    """May the weight gradients of ``params`` (a layer's weight and bias) stay on the side stream until the backward pass ends (mode 2)?
    Only when the ONLY consumer of each of them is autograd's AccumulateGrad storing the tensor: a leaf without an existing
    ``.grad``, without tensor hooks or post-accumulate-grad hooks (an optimizer-in-backward would read dW on the main stream at once),
    outside ``create_graph`` -- and used for the FIRST time in this backward pass: a parameter shared by two layers gets its two
    gradients summed by autograd on the main stream as soon as the second arrives.  In that case (and in every other refused one) the
    caller computes in line AND the main stream first waits for everything already queued on the side stream, so that the first
    gradient is complete before autograd adds to it.
    Uses are counted PER PASS: an entry another pass left behind -- one that died of an exception before its end-of-backward callback
    ran -- does not count, so the next pass gets the side stream again.  An entry of the pass AROUND a nested one is
    not this pass's either; it is kept (the outer pass goes on counting with it) and still makes a refused caller join."""
    ok = not torch.is_grad_enabled()
    task = _pass_id()
    for w in params:
        if w is None:
            continue
        ok = ok and w.is_leaf and w.grad is None and not getattr(w, '_backward_hooks', None) and \
            not getattr(w, '_post_accumulate_grad_hooks', None) and _ASYNC_DW_SEEN.get(id(w)) != task
    if ok:
        for w in params:
            if w is not None:
                _ASYNC_DW_SEEN[id(w)] = task
    elif any(w is not None and id(w) in _ASYNC_DW_SEEN for w in params):
        join_wgrad_stream()
    return ok


def join_wgrad_stream(device=None):
    """Make the current stream wait for the weight-gradient kernels queued on the side stream(s) (mode 2).  Called by the autograd
    callback at the end of a backward pass and by anything that reads ``.grad`` of a convolution weight earlier than that
    (``dist.FlatGradBucket`` before it copies a bucket).  A no-op when nothing is pending."""
    for dev in ([device] if device is not None else list(_JOIN_PENDING)):
        if _JOIN_PENDING.pop(dev, None) and dev in _SIDE:
            cur = torch.cuda.current_stream(dev)
            for st in _SIDE[dev]:
                cur.wait_stream(st)


def queue_join(device):
    """Ask the autograd engine to join the side stream(s) when the running backward pass ends.  A callback is queued for EVERY side-stream
    launch (the first one to run joins and clears the pending flag, the rest are no-ops): a flag-guarded single callback would be lost
    for good if a backward pass died between queueing and running it."""
    _JOIN_PENDING[device] = True
    task = _pass_id()
    torch.autograd.Variable._execution_engine.queue_callback(lambda: end_of_backward(device, task))


def end_of_backward(device=None, task=None):
    """The autograd engine's callback when backward pass ``task`` ends: join the side stream(s) and forget which parameters sent their
    gradient there in that pass (``async_dw_ok`` counts uses per pass; a join in the middle of a pass must NOT reset that) -- and in
    the passes nested in it, all over by now (larger ids).  The entries of a pass AROUND it stay: the callback of a nested pass must
    not reset the count of the pass it runs in.  ``task`` None (a direct call): forget everything."""
    join_wgrad_stream(device)
    if task is None:
        _ASYNC_DW_SEEN.clear()
    else:
        for k in [k for k, t in _ASYNC_DW_SEEN.items() if t >= task]:
            del _ASYNC_DW_SEEN[k]
