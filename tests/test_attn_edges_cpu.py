"""The references, bounds and case lists of the varlen-attention edge tests (tests/_attn_edges.py) checked without a GPU: the float64
formulas against torch.autograd and the `group` closed form against the float64 softmax; the fp32 restatement of the device arithmetic
inside every bound and inside the `group` acceptance; every planted fault outside them; the case lists reach what they name."""
import math

import numpy as np
import pytest
import torch

import _attn_edges as AE

H = 2
CATCH = 4.0           # a planted fault has to leave a bound by this factor


def _autograd(c):
    """float64 softmax attention per scene through torch.autograd: (out, lse, dqkv)"""
    x = c.qkv.double().requires_grad_()
    outs, lses, o = [], [], 0
    for ln in c.lens:
        q, k, v = [t.view(ln, c.H, c.hd).transpose(0, 1) for t in x[o:o + ln].chunk(3, -1)]
        s = q @ k.transpose(1, 2) * AE.scale_of(c.hd)
        outs.append((torch.softmax(s, -1) @ v).transpose(0, 1).reshape(ln, c.D))
        lses.append(torch.logsumexp(s, -1))
        o += ln
    out = torch.cat(outs)
    out.backward(c.dout.double())
    return out.detach(), torch.cat(lses, 1).detach(), x.grad


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize('kind', ['randn', 'voffset', 'group'])
def test_float64_formulas_equal_autograd(kind):
    for lens in ((63, 64, 65), (0, 5, 0, 130)):
        c = AE.make_case(kind, lens, H, 32)
        r = AE.reference(c, 'native')
        out, lse, dqkv = _autograd(c)
        dq, dk, dv = AE.split_dqkv(dqkv, c.D)
        for nm, a, b in (('out', r.out, out), ('lse', r.lse, lse), ('dq', r.dq, dq), ('dk', r.dk, dk), ('dv', r.dv, dv)):
            if kind == 'group' and nm in ('dq', 'dk'):          # dq is zero in exact arithmetic: both sides hold rounding residue
                assert float((a - b).abs().max()) < 1e-9, (kind, lens, nm)
            else:
                assert _rel(a, b) < 1e-12, (kind, lens, nm, _rel(a, b))


@pytest.mark.parametrize('hd', [32, 64])
def test_group_closed_form_equals_float64_softmax(hd):
    for lens in AE.LAYOUTS + tuple(l for _, l, only in AE.DECODE_CASES if only in (None, hd)):
        c = AE.make_case('group', lens, H, hd)
        r = AE.reference(c, 'native')
        out, lse, size = AE.group_closed(c)
        assert _rel(out, r.out) < 1e-12 and _rel(lse, r.lse) < 1e-12, lens
        assert float(size.min()) >= 1, lens          # every query's group has a key


@pytest.mark.parametrize('flow, hd', [('native', 32), ('native', 64)] + [(f, hd) for f in AE.FLOWS[2:] for hd in (32, 64)])
def test_restated_arithmetic_is_inside_every_bound(flow, hd):
    """'native' stands for both fp32 flows: the restatement is plain fp32 and the native bounds are the sharper ones (no 2^-22 term);
    its bounds are formed at head_dim 64 too, where only the three-plane kernels run."""
    for kind in AE.KINDS:
        worst = {}
        for lens in AE.LAYOUTS:
            c = AE.flow_case(kind, lens, H, hd, flow)
            r = AE.cached_reference(kind, lens, H, hd, flow)
            e = AE.emulate(c, flow)
            m = AE.margins(r, e)
            if kind == 'group':
                m['out (group)'] = AE.group_forward_margin(c, flow, e.out)
                bad, mb = AE.group_backward_margins(c, r, e.dq, e.dk, e.dv)
                assert bad == 0, (lens, bad)
                m.update({k + ' (group)': v for k, v in mb.items()})
                if flow != 'bf16_tensors':
                    _, _, size = AE.group_closed(c)
                    pow2 = (size == 2 ** torch.round(torch.log2(size))).t().repeat_interleave(hd, 1)
                    assert torch.equal(e.out[pow2], AE.group_closed(c)[0].float().double()[pow2]), lens      # bit-exact
            for k, v in m.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert all(v <= 1.0 for v in m.values()), (kind, lens, m)
        print(f'attention restated {flow} hd = {hd} {kind}: error / bound', {k: round(v, 4) for k, v in worst.items()})


def _caught(kind, flow, hd, fault, lens):
    """largest factor by which the restated arithmetic with `fault` leaves a bound or the `group` acceptance"""
    c = AE.flow_case(kind, lens, H, hd, flow)
    r = AE.cached_reference(kind, lens, H, hd, flow)
    e = AE.emulate(c, flow, fault)
    m = AE.margins(r, e)
    if kind == 'group':
        m['out (group)'] = AE.group_forward_margin(c, flow, e.out)
        bad, mb = AE.group_backward_margins(c, r, e.dq, e.dk, e.dv)
        m.update(mb)
        if bad:
            m['zeros'] = math.inf
    worst = max(m.values())
    print(f'planted {fault} on {kind} / {flow} hd = {hd} lens = {lens}: leaves a bound by', f'{worst:.3g}', max(m, key=m.get))
    return worst


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('kind', ['randn', 'group'])
@pytest.mark.parametrize('fault', ['mask_last_key', 'dq_skip_last_key', 'dkv_skip_last_query', 'lse_log2'])
def test_mask_and_skip_faults_are_caught(fault, kind, hd):
    for lens in ((63, 64, 65), (0, 5, 0, 700)):
        assert _caught(kind, 'native', hd, fault, lens) >= CATCH


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('kind', ['rising', 'group'])
@pytest.mark.parametrize('fault', ['no_o_rescale', 'no_l_rescale'])
def test_rescale_faults_are_caught(fault, kind, hd):
    for lens in ((63, 64, 65), (0, 5, 0, 700)):
        assert _caught(kind, 'native', hd, fault, lens) >= CATCH


@pytest.mark.parametrize('hd', [32, 64])
def test_truncated_bf16_store_is_caught(hd):
    """Truncation moves a stored element by less than ONE bf16 ulp and the acceptance allows half of one: no element can leave it by a
    factor of 2, let alone 4.  What is asserted: the `group` forward acceptance fails, in more than a tenth of the elements whose
    closed form is not a bf16 number, and the dv bound of `group` fails too."""
    for lens in ((63, 64, 65), (0, 5, 0, 700)):
        assert _caught('group', 'bf16_tensors', hd, 'bf16_trunc', lens) > 1.0
        c = AE.flow_case('group', lens, H, hd, 'bf16_tensors')
        e = AE.emulate(c, 'bf16_tensors', 'bf16_trunc')
        ref = AE.group_closed(c)[0]
        tol = 2 * AE.ulp32(ref)
        tol = tol + AE.half_ulp_bf16(ref.abs() + tol)
        inexact = AE.rne(ref.float()).double() != ref
        wrong = ((e.out - ref).abs() > tol) & inexact
        assert int(wrong.sum()) > 0.1 * int(inexact.sum()) > 0, lens
        assert AE.group_forward_margin(c, 'bf16_tensors', AE.emulate(c, 'bf16_tensors').out) <= 1.0


def test_decode_cases_visit_every_scene_head_and_tile_once():
    """csrc/attn_common.h attn_decode / attn_grid restated: every (scene, head, tile) of every decode case is visited exactly once in
    both tile heights; the other workgroups are padding (scene >= B).  If the restatement drifts from the header the list only loses
    sharpness."""
    seen_padding = seen_full = False
    for Hh, lens, _ in AE.DECODE_CASES + ((2, AE.MAXLEN_LENS, None),):
        B = len(lens)
        for rows in (64, 128):
            for max_len in (max(lens),) + (AE.MAXLEN_OVER if lens == AE.MAXLEN_LENS else ()):
                nt = AE.attn_tiles(max_len, rows)
                grid = AE.attn_grid(Hh, B, nt)
                work = [AE.attn_decode(b, Hh, B, nt) for b in range(grid)]
                real = [w for w in work if w[0] < B]
                assert sorted(real) == [(b, h, t) for b in range(B) for h in range(Hh) for t in range(nt)], (Hh, lens, rows)
                pad = [w for w in work if w[0] >= B]
                assert len(pad) == grid - Hh * B * nt and len(pad) == (-(Hh * B) % 8) * nt
                seen_padding |= bool(pad)
                seen_full |= not pad
    assert seen_padding and seen_full
    assert sorted({Hh for Hh, _, _ in AE.DECODE_CASES}) == [1, 2, 3, 5, 16]
    many = AE.DECODE_CASES[3][1]
    assert len(many) == 17 and set(many) == {0, 1, 3, 64, 65}
    sparse = AE.DECODE_CASES[4][1]
    assert len(sparse) == 33 and sum(1 for v in sparse if v == 0) == 28


@pytest.mark.parametrize('hd', [32, 64])
def test_group_scenes_hold_what_the_docstring_says(hd):
    sizes, uniform, late, single, pow2 = [], 0, 0, 0, 0
    for lens in AE.LAYOUTS:
        assert max(lens) <= 700
        c = AE.make_case('group', lens, H, hd)
        for ln, per_head in zip(c.lens, c.groups):
            for gk, gq, G, dim in per_head:
                if ln == 0:
                    continue
                assert G <= hd and len(set(dim.tolist())) == G
                assert np.isin(gq, gk).all()                         # every query's group has a key
                cnt = np.bincount(gk, minlength=G)
                assert cnt.min() >= 1
                uniform += G == 1 and ln > 1
                single += int((cnt == 1).any() and G > 1)
                pow2 += int(((cnt & (cnt - 1)) == 0).any())
                if ln > 16 and G > 1:
                    sizes.append(ln / G)
        for b, h, first_key, last_tile, queries in AE.late_groups(c):
            assert first_key >= last_tile and last_tile >= 64 and len(queries) >= 2, (lens, b, h)
            late += 1
        # values exact in bf16
        assert torch.equal(AE.rne(c.qkv), c.qkv) and torch.equal(AE.rne(c.dout), c.dout) and bool((c.qkv[:, 2 * c.D:] != 0).all())
    assert uniform and late >= 8 and single and pow2
    assert 12 <= float(np.mean(sizes)) <= 24, np.mean(sizes)
    c = AE.make_case('group', (0, 5, 0, 700), H, hd)
    assert AE.late_groups(c)[0][3] == 640 and 700 - 640 == 60          # eleven key tiles, the last one holds 60 keys


def test_rising_rows_rise_in_every_tile():
    c = AE.make_case('rising', (193,), H, 32)
    for o, ln, h, q, k, v, do in AE._heads(c):
        s = q.double() @ k.double().t()
        tile_max = torch.stack([s[:, 64 * t:64 * t + 64].max(1).values for t in range(4)], 1)
        assert bool((tile_max[:, 1:] > tile_max[:, :-1]).all())
