"""Host-side helpers added in round 5, on CPU tensors (no kernel involved): the no-copy concatenation of row views, batched id offsets,
the packed host->device copy, the per-batch ground-truth rows, the GPU test order."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_cat_views_returns_the_base_only_for_a_full_consecutive_cover():
    from unidet3d_amd.ops import cat_views
    base = torch.arange(40.).reshape(10, 4).requires_grad_()
    y = base * 2                                                    # a non-leaf the views hang off (autograd must flow through it)
    parts = [y[0:3], y[3:3], y[3:7], y[7:10]]                       # incl. an empty slice
    out = cat_views(parts)
    assert out is y
    assert cat_views([y[0:3]]) is not y and torch.equal(cat_views([y[0:3]]), y[0:3])          # single element: returned as is
    for bad in ([y[0:3], y[4:10]], [y[3:7], y[0:3], y[7:10]], [y[0:5], y[5:9]], [y[:, :2][0:5], y[:, :2][5:10]], [y[0:5], (base * 3)[5:10]]):
        got = cat_views(bad)
        assert got is not y and torch.equal(got, torch.cat(bad))
    out.sum().backward()
    assert torch.equal(base.grad, torch.full_like(base, 2.0))
    assert torch.equal(cat_views([torch.ones(2, 3), torch.zeros(1, 3)]), torch.tensor([[1., 1, 1], [1, 1, 1], [0, 0, 0]]))   # plain tensors: cat


def test_cat_views_keeps_the_autograd_state_of_the_slices():
    """slices taken under no_grad of a differentiable base are detached -- torch.cat of them is too, so the (differentiable)
    base must not be returned in their place."""
    from unidet3d_amd.ops import cat_views
    y = torch.arange(24.).reshape(6, 4).requires_grad_() * 2
    with torch.no_grad():
        parts = [y[0:2], y[2:6]]
    out = cat_views(parts)
    ref = torch.cat(parts)
    assert out.requires_grad == ref.requires_grad and out.dtype == ref.dtype and torch.equal(out.detach(), ref.detach())


def test_async_weight_gradient_guard():
    """sparse.async_dw_ok: a weight gradient may stay on the side stream only for a leaf without .grad / hooks, outside
    create_graph, used for the first time in the running backward pass."""
    from unidet3d_amd import sparse
    w, b = torch.zeros(3, requires_grad=True), torch.zeros(3, requires_grad=True)
    nonleaf = w * 1.0
    sparse._ASYNC_DW_SEEN.clear()
    with torch.no_grad():                      # what a backward pass without create_graph looks like
        assert sparse.async_dw_ok(w, b)
        assert not sparse.async_dw_ok(w)       # second use in the same pass: autograd will sum the two gradients
        assert not sparse.async_dw_ok(b, None)
        sparse.join_wgrad_stream()             # a join in the middle of the pass does not forget the uses
        assert not sparse.async_dw_ok(w)
        sparse.end_of_backward()               # end of the pass: forgotten
        assert sparse.async_dw_ok(w, None)
        sparse.end_of_backward()
        w.grad = torch.zeros(3)
        assert not sparse.async_dw_ok(w)       # accumulation into an existing .grad
        w.grad = None
        h = w.register_hook(lambda g: g)
        assert not sparse.async_dw_ok(w)       # a hook reads the gradient at once
        h.remove()
        assert not sparse.async_dw_ok(nonleaf)      # not a leaf
    assert not sparse.async_dw_ok(b)           # grad mode on inside backward = create_graph
    sparse._ASYNC_DW_SEEN.clear()


def test_async_weight_gradient_guard_forgets_an_aborted_pass_and_survives_a_nested_one():
    """wgrad_stream counts the uses of a parameter per backward pass, here with real autograd passes on CPU leaves:
    a pass that dies of an exception never runs its end-of-backward callback, and what it left behind must not make the next pass
    refuse the same parameters; the callback of a pass NESTED in another one must not reset the count of the pass around it."""
    from unidet3d_amd import wgrad_stream as WS
    cpu = torch.device('cpu')
    w, v = torch.zeros(3, requires_grad=True), torch.zeros(3, requires_grad=True)
    answers = []

    class Use(torch.autograd.Function):            # stands for a layer whose backward asks for the side stream, as dense._LinearFn does
        @staticmethod
        def forward(ctx, x, p, tag, inner=None):
            ctx.p, ctx.tag, ctx.inner = p, tag, inner
            return x * 1.0

        @staticmethod
        def backward(ctx, g):
            if ctx.inner is not None:
                ctx.inner()
            ok = WS.async_dw_ok(ctx.p)
            answers.append((ctx.tag, ok))
            if ok:
                WS.queue_join(cpu)
            return g, None, None, None

    def boom(g):
        raise RuntimeError('hook')

    WS._ASYNC_DW_SEEN.clear()
    try:
        # (1) an aborted pass: the layer nearest the loss has asked (and queued its callback) when the hook below it raises
        x = torch.ones(3, requires_grad=True)
        h = Use.apply(x, v, 'below')
        h.register_hook(boom)
        y = Use.apply(h, w, 'above')
        try:
            y.sum().backward()
            raise AssertionError('the hook did not raise')
        except RuntimeError as e:
            assert 'hook' in str(e)
        assert answers == [('above', True)] and id(w) in WS._ASYNC_DW_SEEN          # left behind: no callback ran
        # (2) the next pass over the same parameters gets the side stream again, counts its own uses, and cleans up after itself
        del answers[:]
        x = torch.ones(3, requires_grad=True)
        Use.apply(Use.apply(Use.apply(x, w, 'first'), v, 'other'), w, 'second').sum().backward()
        assert answers == [('second', True), ('other', True), ('first', False)]     # the second use of w in ONE pass is still refused
        assert not WS._ASYNC_DW_SEEN
        # (3) a nested pass between two uses of w in the outer pass: its callback leaves the outer pass's count alone
        del answers[:]

        def inner():
            with torch.enable_grad():
                z = torch.ones(3, requires_grad=True)
                Use.apply(z, v, 'nested').sum().backward()
            assert id(w) in WS._ASYNC_DW_SEEN and id(v) not in WS._ASYNC_DW_SEEN     # the nested callback forgot its own entry only
        x = torch.ones(3, requires_grad=True)
        Use.apply(Use.apply(x, w, 'outer 2', inner), w, 'outer 1').sum().backward()
        assert answers == [('outer 1', True), ('nested', True), ('outer 2', False)]
        assert not WS._ASYNC_DW_SEEN
    finally:
        WS._ASYNC_DW_SEEN.clear()
        WS._JOIN_PENDING.pop(cpu, None)


def test_offset_ids_matches_the_per_scene_loop():
    from unidet3d_amd.ops import offset_ids
    g = torch.Generator().manual_seed(3)
    ids = [torch.randint(-1, 5, (n,), generator=g) for n in (7, 1, 12)]
    biases = [0, 5, 9]
    ref_keep = torch.cat([torch.where(t >= 0, t + b, t) for t, b in zip(ids, biases)])
    ref_plain = torch.cat([t + b for t, b in zip(ids, biases)])
    assert torch.equal(offset_ids(ids, biases, keep_negative=True), ref_keep)
    assert torch.equal(offset_ids(ids, biases), ref_plain)
    assert torch.equal(offset_ids([ids[0]], [4], keep_negative=True), torch.where(ids[0] >= 0, ids[0] + 4, ids[0]))
    assert all(torch.equal(a, b) for a, b in zip(ids, [t.clone() for t in ids]))              # inputs untouched


def test_h2d_pack_round_trips_mixed_dtypes_and_empty_lists():
    from unidet3d_amd._lib import h2d_pack
    specs = [([0, 3, 7], torch.int32), ([1, 2, 3, 4, 5], torch.int64), ([[1, 2, 3, 4], [5, 6, 7, 8]], torch.int32), ([0.5, 1.5], torch.float32),
             ([], torch.int32), ([9], torch.int64)]
    out = h2d_pack(specs, 'cpu')
    assert [o.dtype for o in out] == [d for _, d in specs]
    for o, (v, d) in zip(out, specs):
        assert torch.equal(o, torch.tensor(v, dtype=d).reshape(-1))
        assert o.numel() == 0 or o.data_ptr() % 16 == 0


def test_batch_box_object_hands_row_views_of_its_cached_rows():
    from unidet3d_amd.criterion import _gt_boxes
    from unidet3d_amd.structures import DepthInstance3DBoxes
    g = torch.Generator().manual_seed(5)
    raw = torch.rand(9, 6, generator=g) + 0.5
    whole = DepthInstance3DBoxes(raw, with_yaw=False, box_dim=6, origin=(0.5, 0.5, 0.5))
    whole.cache_gt_rows()
    per_scene = [DepthInstance3DBoxes(raw[a:b], with_yaw=False, box_dim=6, origin=(0.5, 0.5, 0.5)) for a, b in ((0, 4), (4, 4), (4, 9))]
    for (a, b), ref in zip(((0, 4), (4, 4), (4, 9)), per_scene):
        part = whole[a:b]
        assert torch.equal(part.tensor, ref.tensor)                                          # element-wise round trip: same bits batched or not
        assert part.gt_rows is not None and part.gt_rows.data_ptr() == whole.gt_rows[a:b].data_ptr()
        assert torch.equal(_gt_boxes(part), _gt_boxes(ref))
    assert whole[torch.tensor([1, 3])].gt_rows is None                                       # fancy indexing: no stale cache
    assert whole.to('cpu').gt_rows is None


def test_gpu_files_are_collected_parity_first_infrastructure_last():
    import conftest
    class It:                                                    # noqa: E306
        def __init__(self, f): self.fspath = f
    files = ['tests/test_gpu_dist.py', 'tests/test_gpu_bf16.py', 'tests/test_cabi.py', 'tests/test_gpu_eval.py', 'tests/test_gpu_kernels.py',
             'tests/test_gpu_model.py', 'tests/test_gpu_postproc.py', 'tests/test_gpu_ref_golden.py', 'tests/test_gpu_full_size.py',
             'tests/test_gpu_gradients.py']
    order = [os.path.basename(i.fspath) for i in sorted((It(f) for f in files), key=conftest._file_rank)]
    assert order == ['test_gpu_kernels.py', 'test_gpu_model.py', 'test_gpu_ref_golden.py', 'test_gpu_full_size.py', 'test_gpu_gradients.py',
                     'test_gpu_postproc.py', 'test_gpu_eval.py', 'test_cabi.py', 'test_gpu_bf16.py', 'test_gpu_dist.py']


def test_lazy_columns_compute_each_entry_once_and_slices_share_the_cache():
    """encoder._LazyColumns (the per-scene class-column selection of a mixed batch): nothing is computed until an entry is read, every
    entry is computed once, slices / negative indices / iteration / zip behave like a list's."""
    from unidet3d_amd.encoder import _LazyColumns
    calls = []
    cols = _LazyColumns([(lambda i=i: (calls.append(i), torch.tensor([i]))[1]) for i in range(6)])
    part = cols[2:4]
    assert len(cols) == 6 and len(part) == 2 and calls == []
    assert int(part[0]) == 2 and calls == [2]
    assert [int(t) for t in part] == [2, 3] and calls == [2, 3]
    assert int(cols[2]) == 2 and calls == [2, 3]                      # the slice filled the parent's cache
    assert [int(t) for t in cols] == list(range(6)) and calls == [2, 3, 0, 1, 4, 5]
    assert int(cols[-1]) == 5 and [int(t) for t in cols[4:][::-1]] == [5, 4]
    assert [(a, int(t)) for a, t in zip('ab', part)] == [('a', 2), ('b', 3)]


def test_gravity_center_forms_agree_bit_for_bit():
    """DepthInstance3DBoxes.gravity_center: the three-launch form, the cached GT rows and the reference's z + h / 2 give the same bits;
    row slices carry the matching cached rows."""
    from unidet3d_amd.structures import DepthInstance3DBoxes
    g = torch.Generator().manual_seed(0)
    t = torch.randn(13, 7, generator=g)
    t[:, 3:6] = t[:, 3:6].abs() + 0.1
    b = DepthInstance3DBoxes(t, with_yaw=True, box_dim=7, origin=(0.5, 0.5, 0.5))
    want = b.tensor[:, :3].clone()
    want[:, 2] = b.tensor[:, 2] + b.tensor[:, 5] * 0.5
    assert torch.equal(b.gravity_center, want)
    rows = b.cache_gt_rows()
    assert rows.shape == (13, 7) and torch.equal(rows[:, :3], want) and torch.equal(rows[:, 3:], b.tensor[:, 3:])
    assert torch.equal(b.gravity_center, want)                         # now served from the cache
    part = b[3:9]
    assert torch.equal(part.gravity_center, want[3:9]) and torch.equal(part.gt_rows, rows[3:9])
    assert b[torch.tensor([1, 5])].gt_rows is None and torch.equal(b[torch.tensor([1, 5])].gravity_center, want[[1, 5]])


def test_dense_padding_helpers_pad_with_exact_zeros_and_copy_nothing_that_is_aligned():
    """dense._transposed / dense._pad_cols, shared by both data flows of the decoder's dense ops: the [K, N] weight copy and the
    columns of dy are zero-padded to the kernel's granule for the tiny heads (N = 19, 8); aligned operands are returned as they are."""
    import pytest
    from unidet3d_amd import dense
    g = torch.Generator().manual_seed(0)
    K = 32
    for N in (8, 19, 20):
        weight = torch.randn(N, K, generator=g)
        for q in (4, 8, 16, 32):
            Np = (N + q - 1) // q * q
            given = weight.t().contiguous()                # stands for the copy transposed_weights() made
            planes = object()
            if N % q == 0:
                wt, pl = dense._transposed(weight, q, given, planes)
                assert wt is given and pl is planes
            else:
                for have in (None, given):
                    wt, pl = dense._transposed(weight, q, have, planes if have is not None else None)
                    assert pl is None and wt.shape == (K, Np) and wt.dtype == torch.float32 and wt.is_contiguous()
                    assert torch.equal(wt[:, :N], weight.t()) and not wt[:, N:].any()
            for M in (0, 1, 5):
                for dtype in (torch.float32, torch.bfloat16):
                    dy = torch.randn(M, N, generator=g).to(dtype)
                    dyp = dense._pad_cols(dy, q)
                    if N % q == 0:
                        assert dyp is dy
                    else:
                        assert dyp.shape == (M, Np) and dyp.dtype == dtype and torch.equal(dyp[:, :N], dy) and not dyp[:, N:].any()
    with pytest.raises(Exception):                        # aligned and no copy at hand: a u3d_transpose launch, not a torch fallback
        dense._transposed(torch.randn(32, K), 32)


def test_one_command_line_per_source_for_the_build_and_for_variants(tmp_path, monkeypatch):
    """csrc/build.py command() is the one place that says how a source is compiled: the build, variant libraries
    (tools/build_variant.sh -> build_variant) and ISA comparisons all get a file's own options from it."""
    from unidet3d_amd.csrc import build as B
    fp_off = {'postproc.hip', 'augment.hip', 'targets.hip', 'optim.hip', 'evalmap.hip'}          # bit-exact against their references
    vgpr_form = {'spconv.hip', 'spconv_wg.hip', 'attn_x3.hip'}
    assert fp_off | vgpr_form <= set(B.SOURCES)
    for s in B.SOURCES:
        cmd = B.command(s)
        assert ('-ffp-contract=off' in cmd) == (s in fp_off), s
        assert ('-amdgpu-mfma-vgpr-form' in cmd) == (s in vgpr_form), s
        assert '--offload-arch=gfx950' in cmd and '-c' in cmd and cmd[-3] == os.path.join(B.HERE, s) and cmd[-2] == '-o'
        assert all(f in cmd for f in B.FLAGS) and all(f in cmd for f in B.EXTRA.get(s, []))
        # a variant: the same flags, then the caller's, another output; nothing of the file's own options is lost
        var = B.command(s, ['-DU3D_SPLIT_ABL'], str(tmp_path / 'x.o'))
        assert var[:-4] == cmd[:-4] + ['-DU3D_SPLIT_ABL'] and var[-4:] == ['-c', cmd[-3], '-o', str(tmp_path / 'x.o')]
        asm = B.command(s, kind=['--offload-device-only', '-S'])
        assert asm[:-5] == cmd[:-4] and asm[-5:-3] == ['--offload-device-only', '-S']
    # the variant path compiles through command(): record what it would run
    ran = []
    monkeypatch.setattr(B, 'build', lambda **kw: B.LIB)
    monkeypatch.setattr(B, '_compile', lambda jobs, verbose=True: ran.extend(jobs))
    monkeypatch.setattr(B, '_link', lambda lib, objs: ran.append(('link', lib, objs)))
    B.build_variant(str(tmp_path / 'v.so'), ['augment.hip', 'spconv_wg.hip'], ['-DX=1'], str(tmp_path))
    assert ran[0] == B.command('augment.hip', ['-DX=1'], str(tmp_path / 'augment.o')) and '-ffp-contract=off' in ran[0]
    assert ran[1] == B.command('spconv_wg.hip', ['-DX=1'], str(tmp_path / 'spconv_wg.o')) and '-amdgpu-mfma-vgpr-form' in ran[1]
    objs = ran[2][2]
    assert len(objs) == len(B.SOURCES) and str(tmp_path / 'augment.o') in objs and os.path.join(B.HERE, 'gemm.o') in objs
    script = [l for l in open(os.path.join(ROOT, 'tools', 'build_variant.sh')) if not l.startswith('#')]
    assert any('unidet3d_amd.csrc.build --variant' in l for l in script) and not any('hipcc' in l or '-mllvm' in l or 'contract' in l for l in script)


def test_an_object_is_stale_after_any_header_changes(tmp_path, monkeypatch):
    """_stale depends on every *.h next to the sources and on include/u3d.h, not on a hand-kept list of two."""
    from unidet3d_amd.csrc import build as B
    here = tmp_path / 'csrc'
    (tmp_path / 'include').mkdir()
    here.mkdir()
    monkeypatch.setattr(B, 'HERE', str(here))
    monkeypatch.setattr(B, 'ROOT', str(tmp_path))
    old, new = 1_000_000_000, 1_000_000_100
    paths = {n: here / n for n in ('a.hip', 'a.o', 'u3d_common.h', 'spconv_gmm.h', 'attn_common.h')}
    paths['u3d.h'] = tmp_path / 'include' / 'u3d.h'
    for n, p in paths.items():
        p.write_text('')
        os.utime(p, (old, old))
    os.utime(paths['a.o'], (new, new))
    monkeypatch.setattr(B, '__file__', str(paths['a.hip']))               # build.py's own mtime is a dependency as well
    assert not B._stale(str(paths['a.hip']), str(paths['a.o']))
    for n in ('attn_common.h', 'u3d.h', 'a.hip'):                         # a header that is none of the two once named | the ABI header | the source
        os.utime(paths[n], (new + 1, new + 1))
        assert B._stale(str(paths['a.hip']), str(paths['a.o'])), n
        os.utime(paths[n], (old, old))
    assert not B._stale(str(paths['a.hip']), str(paths['a.o']))
    assert B._stale(str(paths['a.hip']), str(here / 'missing.o'))


def test_weight_planes_are_an_argument_of_the_nt_entry_points():
    """The pre-split W planes reach an NT launch as its own `w_planes` argument (placed last before flops_hint; u3d_ffn_fwd takes
    two): no hand-over entry point is left in the header or in the ctypes table, and both agree on the six argument lists."""
    import re
    from unidet3d_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'u3d.h')).read(), flags=re.S)
    assert 'u3d_gemm_w_planes' not in _lib.PROTOTYPES and 'u3d_gemm_w_planes' not in hdr
    for name, n_planes in (('u3d_gemm_nt', 1), ('u3d_linear_act', 1), ('u3d_linear_dact', 1), ('u3d_gemm_nt_add', 1), ('u3d_ln_linear', 1),
                           ('u3d_ffn_fwd', 2)):
        params = [p.strip() for p in re.search(r'\b' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',')]
        args = _lib.PROTOTYPES[name][1]
        assert len(params) == len(args), name
        tail = params[-2 - n_planes:]
        assert all(re.fullmatch(r'const void\* w\d?_planes', p) for p in tail[:n_planes]), (name, tail)
        assert tail[n_planes:] == ['double flops_hint', 'u3d_stream_t stream'], (name, tail)
        assert args[-2 - n_planes:] == [_lib.C.c_void_p] * n_planes + [_lib.C.c_double, _lib.C.c_void_p], name
