"""Batch norm kernels (csrc/bn.hip) through the C ABI at every width class, grid edge and value kind against float64: u3d_bn_forward /
u3d_bn_backward, the split entry points of the SyncBatchNorm path (u3d_bn_stats -> u3d_bn_finalize -> u3d_bn_apply, u3d_bn_bwd_stats ->
u3d_bn_bwd_apply), statistics from synthetic convolution-epilogue partials, the eval backward, the agreement of the recomputed ReLU
mask with the forward's decision, the bf16 shadows' fragment order, and SparseBatchNorm with one row and with none.

Cases, float64 / longdouble references and acceptance bounds come from tests/_bn_edges.py (derived there, checked on the host by
tests/test_bn_edges_cpu.py); comparisons are elementwise error / bound <= 1.  Reference gradients take the device's own ReLU decisions
(y > 0), so no element is left out.  Every output buffer carries guard rows that must come back untouched; x and dy are followed by
NaN rows, so a row read past n poisons the sums."""
import numpy as np
import pytest
import torch

import _bn_edges as BE
from _parity import log_errors

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = -12288.0          # exact in bf16 too
N_GUARD = 8
NBT0 = 5


def _L():
    from unidet3d_amd import _lib as L
    return L


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(a):
    """[n, C] input followed by N_GUARD rows of NaN"""
    a = torch.from_numpy(np.ascontiguousarray(a))
    return torch.cat([a, torch.full((N_GUARD, a.shape[1]), float('nan'), dtype=a.dtype)]).to(DEV)


def _out(n, dtype=torch.float32):
    """flat output buffer of n elements followed by N_GUARD guards"""
    return torch.full((n + N_GUARD,), GUARD, dtype=dtype, device=DEV)


def _out2(n, C, dtype=torch.float32):
    return torch.full((n + N_GUARD, C), GUARD, dtype=dtype, device=DEV)


def _init(values):
    t = _out(len(values))
    t[:len(values)] = _d(values)
    return t


def _intact(t, n):
    return bool((t[n:] == GUARD).all())


def _ws(C):
    L = _L()
    return torch.empty(int(L.lib().u3d_bn_ws_bytes(C)), dtype=torch.uint8, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64 if t.element_size() == 8 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Fwd:
    """device buffers of one forward call"""

    def __init__(self, c, shadow=False):
        n, C = c.n, c.C
        self.c, self.n, self.C = c, n, C
        self.x, self.gamma, self.beta = _rows(c.x), _d(c.gamma), _d(c.beta)
        self.rm, self.rv = _init(c.rm0), _init(c.rv0)
        self.nbt = torch.tensor([NBT0] + [int(GUARD)] * N_GUARD, dtype=torch.int64, device=DEV)
        self.y = _out2(n, C)
        self.yb = _out2(n, C, torch.bfloat16) if shadow else None
        self.st = _out(4 * C)
        self.sums = _out(2 * C + 1, torch.float64)
        self.ws = _ws(C)

    def rows(self, k):
        return self.st[k * self.C:(k + 1) * self.C]

    def check_guards(self, what):
        n, C = self.n, self.C
        assert _intact(self.y, n) and _intact(self.st, 4 * C) and _intact(self.sums, 2 * C + 1) and _intact(self.rm, C) and _intact(self.rv, C), what
        assert bool((self.nbt[1:] == int(GUARD)).all()), what
        assert self.yb is None or _intact(self.yb, n), what

    def host(self):
        C = self.C
        st = self.st[:4 * C].cpu().numpy().reshape(4, C)
        from types import SimpleNamespace
        return SimpleNamespace(mean=st[0], istd=st[1], scale=st[2], shift=st[3], y=self.y[:self.n].cpu().numpy(), rm=self.rm[:C].cpu().numpy(),
                               rv=self.rv[:C].cpu().numpy(), sums=self.sums[:2 * C].cpu().numpy(), count=float(self.sums[2 * C]), nbt=int(self.nbt[0]))


def _forward(c, relu, shadow=False):
    L = _L()
    f = Fwd(c, shadow)
    L.call('u3d_bn_forward', L.ptr(f.x), c.n, c.C, None, 0, L.ptr(f.gamma), L.ptr(f.beta), BE.EPS, BE.MOM, L.ptr(f.rm), L.ptr(f.rv), L.ptr(f.nbt),
           relu, L.ptr(f.y), L.ptr(f.yb), L.ptr(f.st), L.ptr(f.sums), L.ptr(f.ws), L.stream())
    f.check_guards((c.kind, c.n, c.C, relu))
    return f


class Bwd:
    def __init__(self, f, with_addend, shadow=False):
        c, n, C = f.c, f.n, f.C
        self.n, self.C = n, C
        self.dy = _rows(c.dy)
        self.addend = _rows(c.addend) if with_addend else None
        self.dx = _out2(n, C)
        self.dxb = _out2(n, C, torch.bfloat16) if shadow else None
        self.dgamma, self.dbeta = _out(C), _out(C)
        self.sums = _out(2 * C + 1, torch.float64)

    def check_guards(self, what, count_written=False):
        n, C = self.n, self.C
        assert _intact(self.dx, n) and _intact(self.dgamma, C) and _intact(self.dbeta, C) and _intact(self.sums, 2 * C + 1), what
        assert count_written or float(self.sums[2 * C]) == GUARD, what        # the backward statistics leave the count slot alone
        assert self.dxb is None or _intact(self.dxb, n), what

    def host(self):
        from types import SimpleNamespace
        C = self.C
        return SimpleNamespace(dx=self.dx[:self.n].cpu().numpy(), dgamma=self.dgamma[:C].cpu().numpy(), dbeta=self.dbeta[:C].cpu().numpy(),
                               sums=self.sums[:2 * C].cpu().numpy())


def _backward(f, relu, with_addend, shadow=False):
    L = _L()
    b = Bwd(f, with_addend, shadow)
    L.call('u3d_bn_backward', L.ptr(f.x), L.ptr(b.dy), L.ptr(f.st), relu, L.ptr(f.sums), L.ptr(b.sums), f.n, f.C, L.ptr(b.dx), L.ptr(b.dxb),
           L.ptr(b.dgamma), L.ptr(b.dbeta), L.ptr(b.addend), L.ptr(f.ws), L.stream())
    b.check_guards((f.c.kind, f.n, f.C, relu, with_addend))
    return b


def _worst(acc, ms, prefix=''):
    for k, v in ms.items():
        acc[prefix + k] = max(acc.get(prefix + k, 0.0), v)


def _check_case(c, worst, relus=(0, 1), addends=(False, True), twice=True):
    """forward and backward of one case against the references; `worst`: kind -> {output: worst error / bound}"""
    r = BE.stats_ref(c)
    acc = worst.setdefault(c.kind, {})
    for relu in relus:
        what = (c.kind, c.n, c.C, relu)
        f = _forward(c, relu)
        h = f.host()
        assert np.isfinite(h.y).all() and np.isfinite(h.sums).all(), what            # no row past n was read
        assert h.count == c.n and h.nbt == NBT0 + 1, what
        ms = BE.forward_margins(c, r, h, relu)
        _worst(acc, ms)
        assert max(ms.values()) <= 1.0, (what, ms)
        if c.kind == 'ints':
            assert np.array_equal(h.sums, np.concatenate([r.s1, r.s2])), what         # bit for bit: no row lost, none doubled
        if c.kind == 'const':
            ref, tol = BE.const_invstd(c)
            assert bool((np.abs(h.istd.astype(np.float64) - ref) <= tol).all()), what   # the variance clamped at 0
        if twice:
            f2 = _forward(c, relu)
            assert _same(f2.y, f.y) and _same(f2.st, f.st) and _same(f2.sums, f.sums) and _same(f2.rm, f.rm) and _same(f2.rv, f.rv), what
        mask = (h.y > 0) if relu else None                                            # the device's own decisions
        for with_addend in addends:
            b = _backward(f, relu, with_addend)
            hb = b.host()
            assert np.isfinite(hb.dx).all() and np.isfinite(hb.sums).all(), what
            ref = BE.bwd_ref(c, r, mask, with_addend)
            mb = BE.backward_margins(ref, hb)
            _worst(acc, {('dx_addend' if with_addend and k == 'dx' else 'bwd_sums' if k == 'sums' else k): v for k, v in mb.items()})
            assert max(mb.values()) <= 1.0, (what, with_addend, mb)
            if c.kind == 'ints':
                assert np.array_equal(hb.sums[:c.C], ref.sums[:c.C]) and np.array_equal(hb.dbeta.astype(np.float64), ref.dbeta), what
            if twice and with_addend:
                b2 = _backward(f, relu, with_addend)
                assert _same(b2.dx, b.dx) and _same(b2.dgamma, b.dgamma) and _same(b2.dbeta, b.dbeta) and _same(b2.sums[:2 * c.C], b.sums[:2 * c.C]), what


def _report(name, worst, **rec):
    for kind, acc in worst.items():
        print(name, rec, kind, 'worst error / bound', {k: round(v, 4) for k, v in acc.items()})
    log_errors(name, dict(worst_error_over_bound=worst, **rec))


# ============================================================================================================ 1. forward / backward
@pytest.mark.parametrize('C', BE.WIDTHS)
def test_forward_backward_every_width_row_edge_and_kind(C):
    worst = {}
    for n in BE.row_edges(C):
        for kind in BE.KINDS:
            _check_case(BE.make_case(kind, n, C), worst)
    _report('bn_edges_forward_backward', worst, C=C, rows=BE.row_edges(C))


@pytest.mark.parametrize('C', BE.EVERY_N_WIDTHS)
def test_every_row_count_up_to_70_is_exact_on_integers(C):
    worst = {}
    for n in range(1, 71):
        _check_case(BE.make_case('ints', n, C), worst, relus=(1,), addends=(True,), twice=False)
    _report('bn_edges_every_row_count', worst, C=C)


@pytest.mark.parametrize('kind', BE.KINDS)
@pytest.mark.parametrize('C', sorted(BE.LARGE_ROWS))
def test_first_row_count_past_the_statistics_grid_cap(C, kind):
    """256 * 16 * rpb + 1 rows: the statistics grid is capped and a workgroup's lanes take a 17th row; at C = 512 the same 8193 rows
    are past the 4096-workgroup cap of the apply kernels."""
    n = BE.LARGE_ROWS[C]
    worst = {}
    _check_case(BE.make_case(kind, n, C), worst, relus=(1,), addends=(True,), twice=kind == 'ints')
    _check_case(BE.make_case(kind, n - 1, C), worst, relus=(0,), addends=(False,), twice=False)
    _report('bn_edges_large_rows', worst, C=C, rows=n)


def test_scale_shift_form_at_large_mean_over_std():
    """y = x scale + shift carries ~u |mean| |scale| of ABSOLUTE error where |mean| >> std (`offset`: |mean| / std up to 1e4; `const`:
    the -1e3 columns, std 0): inside the bound, which allows for it; the measured worst case is logged."""
    rec = {}
    for kind in ('offset', 'const'):
        for n, C in ((4097, 32), (513, 512)):
            c = BE.make_case(kind, n, C)
            r = BE.stats_ref(c)
            h = _forward(c, 0).host()
            yr, yb = BE.y_ref(c, r, 0)
            big = (np.abs(r.m) > 500) & (c.gamma != 0)
            assert bool(big.any())
            err = np.abs(h.y.astype(np.float64) - yr)
            k = f'{kind}_n{n}_C{C}'
            rec[k] = dict(abs_error_mean_1000=float(err[:, big].max()), abs_error_other=float(err[:, ~big].max()),
                          scale_max=float(np.abs(r.s[big]).max()), error_over_bound=BE.margin(h.y, yr, yb))
            print('bn_edges scale / shift form', k, rec[k])
            assert rec[k]['error_over_bound'] <= 1.0, rec[k]
    log_errors('bn_edges_scale_shift_form', rec)


# ============================================================================================================ 2. refused arguments
def _refused_calls(n, C, shadow):
    """every entry point with (n, C) and, with `shadow`, a bf16 pointer: -> [(name, rc)], and the buffers that must stay untouched"""
    L = _L()
    lib = L.lib()
    Cb, nb = max(C, 8), max(n, 2)
    x, dy = torch.ones(nb + N_GUARD, Cb, device=DEV), torch.ones(nb + N_GUARD, Cb, device=DEV)
    gamma, beta = torch.ones(Cb, device=DEV), torch.zeros(Cb, device=DEV)
    st_in = torch.ones(4 * Cb, device=DEV)
    fs = torch.ones(2 * Cb + 1, dtype=torch.float64, device=DEV)
    outs = dict(rm=_out(Cb), rv=_out(Cb), y=_out2(nb, Cb), st=_out(4 * Cb), sums=_out(2 * Cb + 1, torch.float64), dx=_out2(nb, Cb), dgamma=_out(Cb),
                dbeta=_out(Cb), sh=_out2(nb, Cb, torch.bfloat16))
    nbt = torch.tensor([NBT0], dtype=torch.int64, device=DEV)
    ws = _ws(512)
    sh = L.ptr(outs['sh']) if shadow else None
    p, s = L.ptr, L.stream()
    o = outs
    rcs = [('u3d_bn_forward', lib.u3d_bn_forward(p(x), n, C, None, 0, p(gamma), p(beta), BE.EPS, BE.MOM, p(o['rm']), p(o['rv']), p(nbt), 1, p(o['y']), sh,
                                                 p(o['st']), p(o['sums']), p(ws), s)),
           ('u3d_bn_apply', lib.u3d_bn_apply(p(x), p(gamma), p(beta), 1, n, C, p(o['y']), sh, s)),
           ('u3d_bn_backward', lib.u3d_bn_backward(p(x), p(dy), p(st_in), 1, p(fs), p(o['sums']), n, C, p(o['dx']), sh, p(o['dgamma']), p(o['dbeta']), None,
                                                   p(ws), s)),
           ('u3d_bn_bwd_apply', lib.u3d_bn_bwd_apply(p(x), p(dy), p(gamma), p(gamma), p(gamma), p(beta), 1, p(fs), 1.0, n, C, p(o['dx']), sh, p(o['dgamma']),
                                                     p(o['dbeta']), None, s))]
    if not shadow:
        rcs += [('u3d_bn_stats', lib.u3d_bn_stats(p(x), n, C, None, 0, p(o['sums']), p(ws), s)),
                ('u3d_bn_bwd_stats', lib.u3d_bn_bwd_stats(p(x), p(dy), p(gamma), p(gamma), p(gamma), p(beta), 1, n, C, p(o['sums']), p(ws), s))]
    torch.cuda.synchronize()
    return rcs, outs, nbt


@pytest.mark.parametrize('n,C,shadow', [(5, 0, False), (5, 2, False), (5, 6, False), (5, 516, False), (0, 32, False), (5, 36, True), (5, 100, True)])
def test_refused_arguments_launch_nothing(n, C, shadow):
    rcs, outs, nbt = _refused_calls(n, C, shadow)
    assert all(rc == BE.EINVAL for _, rc in rcs), rcs
    for k, t in outs.items():
        assert bool((t == GUARD).all()), (k, n, C)             # nothing ran: not the statistics pass of a call whose apply pass is refused either
    assert int(nbt[0]) == NBT0


def test_epilogue_statistics_refuse_a_tile_count_of_zero():
    L = _L()
    lib = L.lib()
    part = torch.ones(4, 2, 32, device=DEV)
    sums = _out(65, torch.float64)
    ws = _ws(32)
    assert lib.u3d_bn_stats(None, 100, 32, L.ptr(part), 0, L.ptr(sums), L.ptr(ws), L.stream()) == BE.EINVAL
    f = Fwd(BE.make_case('randn', 100, 32))
    rc = lib.u3d_bn_forward(L.ptr(f.x), 100, 32, L.ptr(part), 0, L.ptr(f.gamma), L.ptr(f.beta), BE.EPS, BE.MOM, L.ptr(f.rm), L.ptr(f.rv), L.ptr(f.nbt), 1,
                            L.ptr(f.y), None, L.ptr(f.st), L.ptr(f.sums), L.ptr(f.ws), L.stream())
    assert rc == BE.EINVAL
    torch.cuda.synchronize()
    assert bool((sums == GUARD).all()) and bool((f.y == GUARD).all()) and bool((f.st == GUARD).all()) and int(f.nbt[0]) == NBT0


# ============================================================================================================ 3. split path
def _split_forward(c, relu, count=-1.0):
    """u3d_bn_stats -> u3d_bn_finalize -> u3d_bn_apply into a fresh set of buffers"""
    L = _L()
    f = Fwd(c)
    L.call('u3d_bn_stats', L.ptr(f.x), c.n, c.C, None, 0, L.ptr(f.sums), L.ptr(f.ws), L.stream())
    L.call('u3d_bn_finalize', L.ptr(f.sums), count, L.ptr(f.gamma), L.ptr(f.beta), BE.EPS, BE.MOM, L.ptr(f.rm), L.ptr(f.rv), c.C, L.ptr(f.rows(0)),
           L.ptr(f.rows(1)), L.ptr(f.rows(2)), L.ptr(f.rows(3)), L.ptr(f.nbt), L.stream())
    L.call('u3d_bn_apply', L.ptr(f.x), L.ptr(f.rows(2)), L.ptr(f.rows(3)), relu, c.n, c.C, L.ptr(f.y), None, L.stream())
    f.check_guards(('split', c.kind, c.n, c.C))
    return f


def _split_backward(f, relu, with_addend, explicit_count):
    L = _L()
    b = Bwd(f, with_addend)
    xdy = (L.ptr(f.x), L.ptr(b.dy), L.ptr(f.rows(0)), L.ptr(f.rows(1)), L.ptr(f.rows(2)), L.ptr(f.rows(3)), relu)
    L.call('u3d_bn_bwd_stats', *xdy, f.n, f.C, L.ptr(b.sums), L.ptr(f.ws), L.stream())
    b.check_guards(('split bwd stats', f.n, f.C))
    if not explicit_count:
        b.sums[2 * f.C] = f.sums[2 * f.C]
    L.call('u3d_bn_bwd_apply', *xdy, L.ptr(b.sums), float(f.n) if explicit_count else -1.0, f.n, f.C, L.ptr(b.dx), None, L.ptr(b.dgamma), L.ptr(b.dbeta),
           L.ptr(b.addend), L.stream())
    b.check_guards(('split bwd', f.n, f.C), count_written=not explicit_count)
    return b


@pytest.mark.parametrize('C', [4, 36, 96, 160, 508, 512])
def test_split_entry_points_return_the_bits_of_the_fused_calls(C):
    r_ = BE.rpb(C)
    for n in (1, r_ + 1, 16 * r_ + 1, 64 * r_ + 1):
        for kind in ('randn', 'offset', 'const'):
            c = BE.make_case(kind, n, C)
            for relu in (0, 1):
                what = (kind, n, C, relu)
                f, g = _forward(c, relu), _split_forward(c, relu)
                assert _same(g.y, f.y) and _same(g.st, f.st) and _same(g.sums, f.sums), what
                assert _same(g.rm, f.rm) and _same(g.rv, f.rv) and int(g.nbt[0]) == int(f.nbt[0]) == NBT0 + 1, what
                g2 = _split_forward(c, relu, count=float(n))                          # the count given instead of read from sums[2C]
                assert _same(g2.y, f.y) and _same(g2.st, f.st) and _same(g2.rv, f.rv), what
                for with_addend in (False, True):
                    b = _backward(f, relu, with_addend)
                    for explicit in (True, False):
                        s = _split_backward(f, relu, with_addend, explicit)
                        assert _same(s.dx, b.dx) and _same(s.dgamma, b.dgamma) and _same(s.dbeta, b.dbeta), (what, with_addend, explicit)
                        assert _same(s.sums[:2 * C], b.sums[:2 * C]), (what, with_addend, explicit)


@pytest.mark.parametrize('C', [36, 96, 288])
@pytest.mark.parametrize('kind', BE.KINDS)
def test_two_ranks_simulated_on_one_device(C, kind):
    """statistics of two unequal row halves, the fp64 sums vectors added on the device (what the all-reduce does), one finalize, apply
    per half: within the bounds of the float64 batch norm over ALL rows; the same in backward.  No process group."""
    L = _L()
    n, n1 = 257, 37
    c = BE.make_case(kind, n, C)
    r = BE.stats_ref(c)
    parts = [(0, n1), (n1, n)]
    xs = [_rows(c.x[a:b]) for a, b in parts]
    dys = [_rows(c.dy[a:b]) for a, b in parts]
    ads = [_rows(c.addend[a:b]) for a, b in parts]
    worst = {}
    for relu in (0, 1):
        f = Fwd(c)
        tot = torch.zeros(2 * C + 1, dtype=torch.float64, device=DEV)
        for (a, b), x in zip(parts, xs):
            L.call('u3d_bn_stats', L.ptr(x), b - a, C, None, 0, L.ptr(f.sums), L.ptr(f.ws), L.stream())
            assert _intact(f.sums, 2 * C + 1)
            tot += f.sums[:2 * C + 1]
        f.sums[:2 * C + 1] = tot
        L.call('u3d_bn_finalize', L.ptr(f.sums), -1.0, L.ptr(f.gamma), L.ptr(f.beta), BE.EPS, BE.MOM, L.ptr(f.rm), L.ptr(f.rv), C, L.ptr(f.rows(0)),
               L.ptr(f.rows(1)), L.ptr(f.rows(2)), L.ptr(f.rows(3)), L.ptr(f.nbt), L.stream())
        for (a, b), x in zip(parts, xs):
            y = _out2(b - a, C)
            L.call('u3d_bn_apply', L.ptr(x), L.ptr(f.rows(2)), L.ptr(f.rows(3)), relu, b - a, C, L.ptr(y), None, L.stream())
            assert _intact(y, b - a)
            f.y[a:b] = y[:b - a]
        f.check_guards(('two ranks', kind, C, relu))
        h = f.host()
        assert h.count == n and h.nbt == NBT0 + 1
        ms = BE.forward_margins(c, r, h, relu)
        if kind == 'ints':
            assert np.array_equal(h.sums, np.concatenate([r.s1, r.s2]))
        mask = (h.y > 0) if relu else None
        bw = Bwd(f, True)
        tot = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
        args = []
        for (a, b), x, dy in zip(parts, xs, dys):
            xdy = (L.ptr(x), L.ptr(dy), L.ptr(f.rows(0)), L.ptr(f.rows(1)), L.ptr(f.rows(2)), L.ptr(f.rows(3)), relu)
            L.call('u3d_bn_bwd_stats', *xdy, b - a, C, L.ptr(bw.sums), L.ptr(f.ws), L.stream())
            bw.check_guards(('two ranks bwd stats', kind, C))
            tot += bw.sums[:2 * C]
            args.append(xdy)
        bw.sums[:2 * C] = tot
        bw.sums[2 * C] = f.sums[2 * C]                                                # the global row count of the forward pass
        bw.dbeta[:C] = tot[:C].float()
        bw.dgamma[:C] = tot[C:].float()
        for (a, b), xdy, ad in zip(parts, args, ads):
            dx = _out2(b - a, C)
            L.call('u3d_bn_bwd_apply', *xdy, L.ptr(bw.sums), -1.0, b - a, C, L.ptr(dx), None, None, None, L.ptr(ad), L.stream())
            assert _intact(dx, b - a)
            bw.dx[a:b] = dx[:b - a]
        bw.check_guards(('two ranks bwd', kind, C), count_written=True)
        ref = BE.bwd_ref(c, r, mask, True)
        ms.update({'bwd_' + k: v for k, v in BE.backward_margins(ref, bw.host()).items()})
        _worst(worst.setdefault(kind, {}), ms)
        assert max(ms.values()) <= 1.0, (kind, C, relu, ms)
    _report('bn_edges_two_ranks', worst, C=C)


# ============================================================================================================ 4. epilogue statistics
@pytest.mark.parametrize('C', BE.PARTIAL_WIDTHS)
def test_statistics_from_epilogue_partials_at_tile_count_edges(C):
    L = _L()
    worst = 0.0
    ws = _ws(C)
    for t in BE.tile_edges(C):
        for kind in ('ints', 'randn'):
            p = BE.partials_case(kind, t, C)
            ref, bound = BE.partials_ref(p)
            pd = torch.cat([torch.from_numpy(p), torch.full((N_GUARD, 2, C), float('nan'))]).to(DEV)
            runs = []
            for _ in range(2):
                sums = _out(2 * C + 1, torch.float64)
                L.call('u3d_bn_stats', None, 7 * t, C, L.ptr(pd), t, L.ptr(sums), L.ptr(ws), L.stream())
                assert _intact(sums, 2 * C + 1) and float(sums[2 * C]) == 7 * t, (C, t)
                runs.append(sums)
            assert _same(runs[0], runs[1]), (C, t, kind)
            got = runs[0][:2 * C].cpu().numpy()
            if kind == 'ints':
                assert np.array_equal(got, ref), (C, t)
            else:
                m = BE.margin(got, ref, bound)
                worst = max(worst, m)
                assert m <= 1.0, (C, t, m)
    # through u3d_bn_forward: integer rows, so the fp32 per-tile sums are exact and the whole call must return the bits of the call
    # that makes its own pass over x
    c = BE.make_case('ints', 130, C)
    p = np.zeros((3, 2, C), np.float32)
    for i, (a, b) in enumerate(((0, 64), (64, 128), (128, 130))):
        p[i, 0], p[i, 1] = c.x[a:b].astype(np.float64).sum(0), (c.x[a:b].astype(np.float64) ** 2).sum(0)
    f, own = Fwd(c), _forward(c, 1)
    pd = _d(p)
    L.call('u3d_bn_forward', L.ptr(f.x), c.n, C, L.ptr(pd), 3, L.ptr(f.gamma), L.ptr(f.beta), BE.EPS, BE.MOM, L.ptr(f.rm), L.ptr(f.rv), L.ptr(f.nbt), 1,
           L.ptr(f.y), None, L.ptr(f.st), L.ptr(f.sums), L.ptr(f.ws), L.stream())
    f.check_guards(('partials forward', C))
    assert _same(f.sums, own.sums) and _same(f.st, own.st) and _same(f.y, own.y) and _same(f.rv, own.rv) and int(f.nbt[0]) == NBT0 + 1, C
    print('bn_edges partials', C, 'worst error / bound', worst)
    log_errors('bn_edges_partials', dict(C=C, tiles=BE.tile_edges(C), worst_error_over_bound=worst))


# ============================================================================================================ 5. eval backward
@pytest.mark.parametrize('C', [36, 128, 512])
def test_eval_backward_is_scale_times_masked_dy(C):
    L = _L()
    worst = 0.0
    for n in (1, BE.rpb(C) + 1, 257):
        c = BE.make_case('randn', n, C)
        rng = np.random.default_rng(C + n)
        st = np.stack([c.rm0, 1 / np.sqrt(c.rv0 + np.float32(BE.EPS)), c.gamma * (1 / np.sqrt(c.rv0 + np.float32(BE.EPS))), c.beta]).astype(np.float32)
        st[3] = c.beta - st[0] * st[2]
        x, dy, ad, std = _rows(c.x), _rows(c.dy), _rows(c.addend), _d(st.reshape(-1))
        rows = [std[k * C:(k + 1) * C] for k in range(4)]
        for relu in (0, 1):
            y = _out2(n, C)
            L.call('u3d_bn_apply', L.ptr(x), L.ptr(rows[2]), L.ptr(rows[3]), relu, n, C, L.ptr(y), None, L.stream())
            mask = (y[:n].cpu().numpy() > 0) if relu else None
            for with_addend in (False, True):
                for count in (1.0, -1.0):
                    sums = torch.zeros(2 * C + 1, dtype=torch.float64, device=DEV)
                    sums[2 * C] = 1.0 if count < 0 else float(rng.integers(2, 99))     # ignored when the count is given
                    dx = _out2(n, C)
                    L.call('u3d_bn_bwd_apply', L.ptr(x), L.ptr(dy), L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(rows[2]), L.ptr(rows[3]), relu, L.ptr(sums),
                           count, n, C, L.ptr(dx), None, None, None, L.ptr(ad) if with_addend else None, L.stream())
                    assert _intact(dx, n)
                    ref, bound = BE.eval_bwd_ref(st[2], c.dy, mask, c.addend if with_addend else None)
                    m = BE.margin(dx[:n].cpu().numpy(), ref, bound)
                    worst = max(worst, m)
                    assert m <= 1.0, (C, n, relu, with_addend, count, m)
    print('bn_edges eval backward', C, 'worst error / bound', worst)
    log_errors('bn_edges_eval_backward', dict(C=C, worst_error_over_bound=worst))


# ============================================================================================================ 6. ReLU mask agreement
def _step_ulps(x, k):
    x = x.copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


@pytest.mark.parametrize('C', [36, 512])
def test_recomputed_relu_mask_equals_the_forward_decision_at_the_threshold(C):
    """x at the fp32 value nearest -shift / scale and up to 4 ulps either side, scale over six decades and both signs: the backward
    kernels' recomputed `x scale + shift > 0` must decide as the forward's output did (y > 0) on EVERY element -- if one expression
    were contracted to a fused multiply-add and the other not, units at the threshold would flip."""
    L = _L()
    rng = np.random.default_rng(C)
    reps = 9 if C == 36 else 2
    ks = np.tile(np.arange(-4, 5), reps)
    n = len(ks)
    scale = (10.0 ** rng.uniform(-3, 3, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    shift = (10.0 ** rng.uniform(-2, 2, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    x0 = (-shift.astype(np.float64) / scale.astype(np.float64)).astype(np.float32)
    x = np.stack([_step_ulps(x0, int(k)) for k in ks])
    assert x.shape == (n, C) and n * C >= 2900
    xd, sc, sf = _rows(x), _d(scale), _d(shift)
    zero, one = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    dy = _rows(np.ones((n, C), np.float32))
    y = _out2(n, C)
    L.call('u3d_bn_apply', L.ptr(xd), L.ptr(sc), L.ptr(sf), 1, n, C, L.ptr(y), None, L.stream())
    sums = torch.zeros(2 * C + 1, dtype=torch.float64, device=DEV)
    sums[2 * C] = 1.0
    dx = _out2(n, C)
    L.call('u3d_bn_bwd_apply', L.ptr(xd), L.ptr(dy), L.ptr(zero), L.ptr(one), L.ptr(sc), L.ptr(sf), 1, L.ptr(sums), -1.0, n, C, L.ptr(dx), None, None, None,
           None, L.stream())
    st = _out(2 * C + 1, torch.float64)
    L.call('u3d_bn_bwd_stats', L.ptr(xd), L.ptr(dy), L.ptr(zero), L.ptr(one), L.ptr(sc), L.ptr(sf), 1, n, C, L.ptr(st), L.ptr(_ws(C)), L.stream())
    assert _intact(y, n) and _intact(dx, n) and _intact(st, 2 * C + 1)
    on = y[:n] > 0
    assert bool(on.any(0).all()) and bool((~on).any(0).all())                 # every column crosses its threshold inside +-4 ulps
    flips = int(((dx[:n] != 0) != on).sum())
    print('bn_edges relu mask', C, 'elements', n * C, 'positive', int(on.sum()), 'disagreements in bwd_apply', flips)
    assert flips == 0
    assert torch.equal(st[:C], on.sum(0).double())                          # bn_reduce_k<1>: the count of y > 0 in each column, exactly
    log_errors('bn_edges_relu_mask', dict(C=C, elements=n * C, disagreements=flips))


# ============================================================================================================ 7. bf16 shadows
@pytest.mark.parametrize('C', BE.SHADOW_WIDTHS)
def test_bf16_shadows_are_the_rounded_output_in_fragment_order(C):
    """y_bf16 / dx_bf16 = the fp32 output rounded to nearest even, inside each 32-channel group in the order documented at store_shadow
    (restated in _bn_edges.fragment_order from that comment); rows 1, 3 and the first count past the 4096 x 256 grid-stride edge."""
    idx = torch.from_numpy(BE.fragment_order(C)).to(DEV)
    past = 4096 * 256 // (C // 4) + 1
    for n in (1, 3, past):
        assert n * (C // 4) > 4096 * 256 or n < 4
        c = BE.make_case('randn', n, C)
        f = _forward(c, 1, shadow=True)
        assert torch.equal(_bits(f.yb[:n]), _bits(f.y[:n].to(torch.bfloat16)[:, idx])), (C, n)
        b = _backward(f, 1, True, shadow=True)
        assert torch.equal(_bits(b.dxb[:n]), _bits(b.dx[:n].to(torch.bfloat16)[:, idx])), (C, n)
        ya = _out2(n, C)
        yb = _out2(n, C, torch.bfloat16)
        L = _L()
        L.call('u3d_bn_apply', L.ptr(f.x), L.ptr(f.rows(2)), L.ptr(f.rows(3)), 1, n, C, L.ptr(ya), L.ptr(yb), L.stream())
        assert _same(ya, f.y) and _same(yb, f.yb), (C, n)


# ============================================================================================================ 8. module level
def test_sparse_batchnorm_training_with_one_row_and_with_none():
    from unidet3d_amd import sparse
    C = 64
    c = BE.make_case('randn', 1, C)
    r = BE.stats_ref(c)
    bn = sparse.SparseBatchNorm(C, eps=BE.EPS, momentum=BE.MOM, sync=False).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(_d(c.gamma)); bn.bias.copy_(_d(c.beta)); bn.running_mean.copy_(_d(c.rm0)); bn.running_var.copy_(_d(c.rv0))
    x = _d(c.x).requires_grad_()
    y = bn(x, relu=True)
    y.backward(_d(c.dy))
    yr, yb = BE.y_ref(c, r, 1)
    ref = BE.bwd_ref(c, r, y.detach().cpu().numpy() > 0, False)
    ms = dict(y=BE.margin(y.detach().cpu().numpy(), yr, yb), running_mean=BE.margin(bn.running_mean.cpu().numpy(), r.rm, r.b_rm),
              running_var=BE.margin(bn.running_var.cpu().numpy(), r.rv, r.b_rv), dx=BE.margin(x.grad.cpu().numpy(), ref.dx, ref.b_dx),
              dgamma=BE.margin(bn.weight.grad.cpu().numpy(), ref.dgamma, ref.b_dgamma), dbeta=BE.margin(bn.bias.grad.cpu().numpy(), ref.dbeta, ref.b_dbeta))
    print('bn_edges module n = 1: worst error / bound', ms)
    log_errors('bn_edges_module_one_row', dict(worst_error_over_bound=ms))
    assert max(ms.values()) <= 1.0, ms
    assert int(bn.num_batches_tracked) == 1
    assert np.allclose(bn.running_var.cpu().numpy(), (1 - BE.MOM) * c.rv0, rtol=1e-6)                   # the biased variance, 0, went in
    # ---- no rows: empty result, nothing moves
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    bn.zero_grad()
    xe = torch.empty(0, C, device=DEV, requires_grad=True)
    ye = bn(xe, relu=True)
    assert ye.shape == (0, C)
    ye.backward(torch.empty(0, C, device=DEV))
    assert xe.grad is not None and xe.grad.shape == (0, C)
    for k, v in bn.state_dict().items():
        assert _same(v, before[k]) if v.is_floating_point() else torch.equal(v, before[k]), k
    assert int(bn.num_batches_tracked) == 1
    assert bn.weight.grad is None or float(bn.weight.grad.abs().max()) == 0.0
