"""Sparse geometry (host side): the occupancy index of a level, the rulebooks over it, the per-forward level cache.  Integer kernels only:
no features, no autograd, nothing of the package but the C ABI (``_lib``); ``unidet3d_amd.sparse`` re-exports the public names.
Decided here and nowhere else: how an index is made (``OccupancyIndex.from_marks``), how a general layer's new level gets its pair lists
(``_level_pairs``), what lives where in a ``SparseConvTensor.indice_dict`` (``cached_level``; readers ``saved_under`` / ``tensor_index``),
how a level is made from other levels (``build_union_level``, ``compact_mask``) or from a dense grid (``active_cells``, ``cells_coords``)."""
from __future__ import annotations

import ctypes
import operator
import os
from typing import Dict

import torch

from . import _lib as L


# ----------------------------------------------------------------------------------------
# occupancy index
# ----------------------------------------------------------------------------------------
# A grid whose direct-address table would exceed this many bytes (or that u3d_index_words refuses) gets the hashed index
# (csrc/hashidx.hip: memory follows occupancy).  The six indoor configs stay far below (cfg2: 100 MB); U3D_INDEX=hash forces the
# hashed form everywhere (tests), U3D_INDEX=bitmap forbids it.
_INDEX_MODE = os.environ.get('U3D_INDEX', 'auto')
_HASH_ABOVE_BYTES = int(float(os.environ.get('U3D_INDEX_HASH_ABOVE_MB', '4096')) * (1 << 20))


class OccupancyIndex:
    """Cell -> canonical row of one level: bitmap + popcount rank over the grid extent, or -- large extents -- a hash table over the
    occupied cells.  ``table()`` gives the (pointer, pointer, hash_slots) triple every C entry point takes."""

    def __init__(self, bitmap, rank, B, shape, slots=0, ukeys=None, n_dev=None):
        self.bitmap, self.rank, self.B = bitmap, rank, B          # hashed form: table keys (int64 view of uint64) / table values
        self.shape = [int(s) for s in shape]
        self.slots, self.ukeys, self.n_dev = int(slots), ukeys, n_dev

    @property
    def hashed(self) -> bool:
        return self.slots > 0

    def table(self):
        return L.ptr(self.bitmap), L.ptr(self.rank), self.slots

    @staticmethod
    def wants_hash(B, shape) -> bool:
        if _INDEX_MODE == 'hash':
            return True
        nw = L.lib().u3d_index_words(B, *[int(s) for s in shape])
        if _INDEX_MODE == 'bitmap':
            return False
        return nw < 0 or nw * 12 > _HASH_ABOVE_BYTES

    @staticmethod
    def alloc(B, shape, device):
        nw = L.lib().u3d_index_words(B, *[int(s) for s in shape])
        if nw < 0:
            raise L.U3DError(f'occupancy index refused (code {nw}): {L.lib().u3d_last_error().decode()}')
        bitmap = torch.zeros(nw, dtype=torch.int64, device=device)
        rank = torch.empty(nw + 1, dtype=torch.int32, device=device)
        return OccupancyIndex(bitmap, rank, B, shape)

    @staticmethod
    def from_cells(cells: torch.Tensor, B: int, shape) -> 'OccupancyIndex':
        """Hashed index of the cells in ``cells`` (int64 cell ids, duplicates allowed, INT64_MAX = none)."""
        n, dev = cells.shape[0], cells.device
        slots = L.lib().u3d_hash_index_slots(n)
        ukeys = torch.empty(n, dtype=torch.int64, device=dev)
        n_dev = torch.empty(1, dtype=torch.int32, device=dev)
        vals = torch.empty(slots, dtype=torch.int32, device=dev)
        if n == 0:                 # an empty level / point set: a table of free slots, zero rows (the C entry points take n > 0 only)
            keys = torch.full((slots,), -1, dtype=torch.int64, device=dev)
            return OccupancyIndex(keys, vals, B, shape, slots, ukeys, n_dev.zero_())
        keys = torch.empty(slots, dtype=torch.int64, device=dev)
        w = L.ws(L.lib().u3d_hash_index_ws_bytes(n), dev)
        n_cells = int(B) * int(shape[0]) * int(shape[1]) * ((int(shape[2]) + 63) // 64) * 64       # cell ids are < n_cells: bounds the sort's passes
        L.call('u3d_hash_index_build', L.ptr(cells), n, n_cells if n_cells < (1 << 62) else 0, L.ptr(ukeys), L.ptr(n_dev), L.ptr(keys), L.ptr(vals),
               slots, L.ptr(w), L.stream())
        return OccupancyIndex(keys, vals, B, shape, slots, ukeys, n_dev)

    @staticmethod
    def from_marks(B, shape, device, mark) -> 'OccupancyIndex':
        """The index of the cells a caller's mark kernel marks: THE place that chooses between the two forms and orders the steps.
        ``mark(bitmap)`` launches that kernel (or nothing, for an empty level).  Hashed form: ``bitmap`` is None, ``mark`` returns the int64
        cell ids and no bitmap exists.  Bitmap form: ``mark`` fills the zeroed ``bitmap`` (return value ignored), the rank pass follows."""
        shape = [int(s) for s in shape]
        if OccupancyIndex.wants_hash(B, shape):
            return OccupancyIndex.from_cells(mark(None), B, shape)
        ix = OccupancyIndex.alloc(B, shape, device)
        mark(ix.bitmap)
        ix.build_rank()
        return ix

    def build_rank(self):
        nw = self.bitmap.numel()
        w = L.ws(L.lib().u3d_index_rank_ws_bytes(nw), self.bitmap.device)
        L.call('u3d_index_rank', L.ptr(self.bitmap), nw, L.ptr(self.rank), L.ptr(w), L.stream())

    def count(self) -> int:
        return int((self.n_dev if self.hashed else self.rank[-1]).item())       # documented read-back (one host sync)

    def coords(self, n: int) -> torch.Tensor:
        c = torch.empty(n, 4, dtype=torch.int32, device=self.bitmap.device)
        if n and self.hashed:
            L.call('u3d_hash_index_coords', L.ptr(self.ukeys), n, *self.shape, L.ptr(c), L.stream())
        elif n:
            L.call('u3d_index_coords', L.ptr(self.bitmap), L.ptr(self.rank), self.B, *self.shape, L.ptr(c), L.stream())
        return mark_canonical(c)

    def rows_of(self, coords: torch.Tensor) -> torch.Tensor:
        """int32 [n]: the canonical row of every coordinate (int32 [n, 4] = (b, x, y, z)) in this index, -1 for a cell that is absent or
        outside the grid or the batch (u3d_index_rows); no coordinates, no launch"""
        n = coords.shape[0]
        rows = torch.empty(n, dtype=torch.int32, device=coords.device)
        if n:
            L.call('u3d_index_rows', L.ptr(coords), n, *self.table(), self.B, *self.shape, L.ptr(rows), L.stream())
        return rows

    @staticmethod
    def from_coords(coords: torch.Tensor, B: int, shape, shift: int = 0) -> 'OccupancyIndex':
        n = coords.shape[0]

        def mark(bitmap):
            if bitmap is not None:
                return L.call('u3d_index_mark', L.ptr(coords), n, shift, *[int(s) for s in shape], L.ptr(bitmap), L.stream())
            cells = torch.empty(n, dtype=torch.int64, device=coords.device)
            if n:
                L.call('u3d_cells_of_coords', L.ptr(coords), n, shift, B, *[int(s) for s in shape], L.ptr(cells), L.stream())
            return cells
        return OccupancyIndex.from_marks(B, shape, coords.device, mark)


# ----------------------------------------------------------------------------------------
# rulebooks
# ----------------------------------------------------------------------------------------
_PAIR_CACHE: Dict = {}
# rulebook tag (its indice_key) -> the (role, tile height) lists the convolutions asked of that rulebook in earlier steps:
# ``Rulebook.precompute_tiles`` builds them with the rulebook (on the side stream of ``UniDet3D.prefetch``) instead of on first use
# in the middle of the forward / backward pass (34 launches of ~6.6 us on the main stream per step otherwise)
_TILE_HISTORY: Dict = {}
_TILE_PRECOMPUTE = os.environ.get('U3D_TILE_PRECOMPUTE', '1') != '0'


class Rulebook:
    """pair_in / pair_out int32 [K, cap] grouped by offset, ascending inside an offset."""

    def __init__(self, pair_in, pair_out, counts, K, n_in, n_out):
        self.pair_in, self.pair_out, self.counts = pair_in, pair_out, counts
        self.K, self.cap, self.n_in, self.n_out = K, pair_in.shape[1], n_in, n_out
        self._tiles: Dict = {}
        self._total = None
        self.tag = None             # set by ``cached_level`` (indice_key): lets the tile lists follow last step's use
        self.coords = self.index = None      # SubM k=3 / dilation 1 rulebooks ONLY: the level's voxels and occupancy index (tile-stationary kernel's tables)
        self.geom = None            # set by ``cached_level``: the layer geometry it was built for (a shared indice_key must agree)
        self._halo: Dict = {}
        self._nbr: Dict = {}

    def neighbours(self, role: str) -> torch.Tensor:
        """The destination-major view of the pair lists (u3d_pair_table) the pooling kernels walk: int32 [n, K], entry [r, k] = the row
        paired with r at offset k, or -1.  role 'out': n = n_out, each output row's inputs; 'in': n = n_in, each input row's outputs.
        Built once per rulebook and role (4 K n bytes); remembered like the tile lists so that the next step's rulebook builds it ahead."""
        if role not in ('out', 'in'):
            raise L.U3DError(f"Rulebook.neighbours: role must be 'out' or 'in', got {role!r}")
        if self.tag is not None:
            _TILE_HISTORY.setdefault(self.tag, set()).add(('nbr', role))
        return self._neighbours(role)

    def _neighbours(self, role: str) -> torch.Tensor:
        if role not in self._nbr:
            key, val, n, m = (self.pair_out, self.pair_in, self.n_out, self.n_in) if role == 'out' else (self.pair_in, self.pair_out, self.n_in, self.n_out)
            if n and m:
                t = torch.empty(n, self.K, dtype=torch.int32, device=key.device)
                L.call('u3d_pair_table', L.ptr(key), L.ptr(val), L.ptr(self.counts), self.K, self.cap, n, L.ptr(t), L.stream())
            else:           # an empty level on either side: no pairs (the C entry points take n > 0 only)
                t = torch.full((n, self.K), -1, dtype=torch.int32, device=key.device)
            self._nbr[role] = t
        return self._nbr[role]

    def _tile_starts(self, role: str, T: int) -> torch.Tensor:
        key = (role, T)
        if key not in self._tiles:
            rows = self.pair_out if role == 'out' else self.pair_in
            n_dst = self.n_out if role == 'out' else self.n_in
            nt = (n_dst + T - 1) // T
            ts = torch.empty(self.K, nt + 1, dtype=torch.int32, device=rows.device)
            L.call('u3d_tile_starts', L.ptr(rows), L.ptr(self.counts), self.K, self.cap, T, nt, L.ptr(ts), L.stream())
            self._tiles[key] = ts
        return self._tiles[key]

    def tile_starts(self, role: str, T: int, wgrad=None) -> torch.Tensor:
        """``wgrad`` = (C_in, C_out) when T is a weight-gradient tile height: that height follows the row count (u3d_spconv_wgrad_tile_rows),
        so the history remembers the layer shape and the next rulebook recomputes ITS height instead of replaying this one."""
        if self.tag is not None:
            _TILE_HISTORY.setdefault(self.tag, set()).add((role, T) if wgrad is None else (role, 'wgrad', int(wgrad[0]), int(wgrad[1])))
        return self._tile_starts(role, T)

    def halo(self, T: int, H: int):
        """Tables of the tile-stationary SubM kernel (csrc/spconv_ts.hip, u3d_subm_halo) for tiles of T rows and passes of H halo
        rows: (nhalo, halo, loc, pmask).  Built once per rulebook and (T, H); remembered like the tile lists so that the next step's
        rulebook builds them on the side stream."""
        if self.tag is not None:
            _TILE_HISTORY.setdefault(self.tag, set()).add(('halo', int(T), int(H)))
        return self._halo_tables(int(T), int(H))

    def _halo_tables(self, T: int, H: int):
        key = (T, H)
        if key not in self._halo:
            if self.coords is None:
                raise L.U3DError('halo tables need a SubM rulebook built by build_subm_rulebook')
            n, dev = self.n_out, self.coords.device
            nt = (n + T - 1) // T
            pmax = L.lib().u3d_subm_halo_pmax(T, H)
            nhalo = torch.empty(nt, dtype=torch.int32, device=dev)
            halo = torch.empty(nt, 27 * T, dtype=torch.int32, device=dev)
            loc = torch.empty(nt, 27, T, dtype=torch.int16, device=dev)
            pmask = torch.empty(nt, pmax, dtype=torch.int32, device=dev)
            L.call('u3d_subm_halo', L.ptr(self.coords), n, *self.index.table(), self.index.B, *self.index.shape, T, H,
                   L.ptr(nhalo), L.ptr(halo), L.ptr(loc), L.ptr(pmask), L.stream())
            self._halo[key] = (nhalo, halo, loc, pmask)
        return self._halo[key]

    def precompute_tiles(self):
        """Build the tile lists the PREVIOUS rulebook with this tag was asked for: fixed heights (the forward / input-gradient kernels'
        32 / 64 rows) as they were, weight-gradient heights recomputed for THIS rulebook's row count.  Only this step's real requests
        are remembered for the next."""
        if self.tag is None or not _TILE_PRECOMPUTE:
            return
        for key in sorted(_TILE_HISTORY.pop(self.tag, ()), key=str):
            if key[0] == 'halo':
                if self.coords is not None and self.n_out > 0:
                    self._halo_tables(key[1], key[2])
            elif key[0] == 'nbr':
                self._neighbours(key[1])
            elif len(key) == 2:
                self._tile_starts(*key)
            else:
                role, _, cin, cout = key
                n_dy = self.n_out if role == 'out' else self.n_in
                if n_dy > 0:
                    self._tile_starts(role, int(L.lib().u3d_spconv_wgrad_tile_rows(self.K, n_dy, cin, cout)))

    @property
    def total_pairs(self) -> int:
        """Number of rulebook pairs (flops accounting).  Host read-back, cached by geometry so a bench
        that replays the same scenes does not synchronise inside its timed region.  The layer geometry is part of the key: two
        rulebooks of one level (SubM k=3 with dilation 1 and 2) share K and both row counts, not their pairs."""
        if self._total is None:
            key = (self.K, self.n_in, self.n_out, self.geom)
            if key not in _PAIR_CACHE:
                _PAIR_CACHE[key] = int(self.counts.sum().item())
            self._total = _PAIR_CACHE[key]
        return self._total

    def lists(self):
        """Host copy as 27/8 (in_rows, out_rows) arrays -- the canonical rulebook (tests)."""
        c = self.counts.cpu().tolist()
        pi, po = self.pair_in.cpu(), self.pair_out.cpu()
        return [(pi[k, :c[k]].numpy(), po[k, :c[k]].numpy()) for k in range(self.K)]


def build_subm_rulebook(coords: torch.Tensor, index: OccupancyIndex) -> Rulebook:
    n, dev = coords.shape[0], coords.device
    pin = torch.empty(27, n, dtype=torch.int32, device=dev)
    pout = torch.empty(27, n, dtype=torch.int32, device=dev)
    cnt = torch.empty(27, dtype=torch.int32, device=dev)
    w = L.ws(L.lib().u3d_subm_rulebook_ws_bytes(n), dev)
    L.call('u3d_subm_rulebook', L.ptr(coords), n, *index.table(), index.B, *index.shape,
           L.ptr(pin), L.ptr(pout), L.ptr(cnt), L.ptr(w), L.stream())
    rb = Rulebook(pin, pout, cnt, 27, n, n)
    rb.coords, rb.index = coords, index
    return rb


def build_down_rulebook(coords: torch.Tensor, B: int, shape):
    """Returns (out_coords, out_shape, out_index, Rulebook)."""
    n, dev = coords.shape[0], coords.device
    oshape = [int(s) // 2 for s in shape]
    ix2 = OccupancyIndex.from_coords(coords, B, oshape, shift=1)
    n2 = ix2.count()
    oc = ix2.coords(n2)
    pin = torch.empty(8, n, dtype=torch.int32, device=dev)
    pout = torch.empty(8, n, dtype=torch.int32, device=dev)
    cnt = torch.empty(8, dtype=torch.int32, device=dev)
    w = L.ws(L.lib().u3d_down_rulebook_ws_bytes(n), dev)
    L.call('u3d_down_rulebook', L.ptr(coords), n, *ix2.table(), B, *oshape,
           L.ptr(pin), L.ptr(pout), L.ptr(cnt), L.ptr(w), L.stream())
    return oc, oshape, ix2, Rulebook(pin, pout, cnt, 8, n, n2)


def _triple(v, what: str):
    """an integer or a 3-sequence of integers (anything with ``__index__``: Python ints, numpy integer scalars; no bools, no floats)
    -> (a, b, c) of Python ints"""
    def as_int(a):
        if isinstance(a, bool):
            raise TypeError
        return operator.index(a)
    try:
        try:
            a = as_int(v)
            return (a, a, a)
        except TypeError:
            t = tuple(as_int(a) for a in v)
    except TypeError:
        t = ()
    if len(t) != 3:
        raise L.U3DError(f'sparse conv: {what} must be an int or a sequence of three ints, got {v!r}')
    return t


def conv_geometry(kernel_size, stride=1, padding=0, dilation=1):
    """(k0, k1, k2, s0, s1, s2, p0, p1, p2, d0, d1, d2) of a layer, refused where the geometry kernels (csrc/rulebook.hip) have no form
    for it: 1 <= kernel extent <= 3, stride >= 1, padding >= 0, dilation >= 1 on every axis."""
    k, s, p, d = _triple(kernel_size, 'kernel_size'), _triple(stride, 'stride'), _triple(padding, 'padding'), _triple(dilation, 'dilation')
    if not all(1 <= a <= 3 for a in k):
        raise L.U3DError(f'sparse conv: kernel_size {k}: every kernel extent must satisfy 1 <= extent <= 3 (K = 27 offsets at most)')
    if not all(a >= 1 for a in s):
        raise L.U3DError(f'sparse conv: stride {s}: every stride must be >= 1')
    if not all(a >= 0 for a in p):
        raise L.U3DError(f'sparse conv: padding {p}: every padding must be >= 0')
    if not all(a >= 1 for a in d):
        raise L.U3DError(f'sparse conv: dilation {d}: every dilation must be >= 1')
    return (*k, *s, *p, *d)


def layer_geometry(layer, geom):
    """sets what every layer derives from its 12 integers: ``kernel_size`` (the int of a cubic kernel), the triples, K; -> kernel extents"""
    k, layer.geom = geom[:3], geom
    layer.kernel_size = k[0] if k[0] == k[1] == k[2] else k
    layer.stride, layer.padding, layer.dilation = geom[3:6], geom[6:9], geom[9:]
    layer.K = k[0] * k[1] * k[2]
    return k


def _geom_array(geom):
    return (ctypes.c_int * 12)(*geom)


def conv_out_shape(geom, shape):
    """per axis floor((in + 2 p - d (k - 1) - 1) / s) + 1, 0 where that is not positive (u3d_conv_out_shape, host only)"""
    out = (ctypes.c_int * 3)()
    L.call('u3d_conv_out_shape', _geom_array(geom), *[int(s) for s in shape], out)
    return [int(v) for v in out]


def _level_pairs(coords, index, B, shape, geom, new=None, transposed=False):
    """The tail of the two general builders: the rows of the new level ``new`` (its index; one host read, ``count()``; None = submanifold,
    the output rows ARE the input rows) and the [K, cap] pair lists between them and the layer's input rows ``coords`` (extent ``shape``,
    index ``index``).  u3d_conv_rulebook walks the taps of a stationary side and looks the other side up: the output rows against
    ``index``, or -- ``transposed`` -- the input rows against ``new``.  -> (out_coords, n_out, looked-up side's list, stationary side's, counts)"""
    n, dev = coords.shape[0], coords.device
    K = geom[0] * geom[1] * geom[2]
    n2 = n if new is None else new.count()
    oc = coords if new is None else new.coords(n2)
    cap = max(1, min(n, n2))
    pin = torch.empty(K, cap, dtype=torch.int32, device=dev)
    pout = torch.empty(K, cap, dtype=torch.int32, device=dev)
    if n and n2:
        still, n_still, n_looked, looked, extent = (coords, n, n2, new, new.shape) if transposed else (oc, n2, n, index, shape)
        cnt = torch.empty(K, dtype=torch.int32, device=dev)
        w = L.ws(L.lib().u3d_conv_rulebook_ws_bytes(n_still, K), dev)
        L.call('u3d_conv_rulebook', L.ptr(still), n_still, n_looked, *looked.table(), B, *extent, _geom_array(geom), cap,
               L.ptr(pin), L.ptr(pout), L.ptr(cnt), L.ptr(w), L.stream())
    else:               # an empty level on either side: no pairs (the C entry points take n > 0 only)
        cnt = torch.zeros(K, dtype=torch.int32, device=dev)
    return oc, n2, pin, pout, cnt


def _marked_level(coords, B, shape, oshape, geom, entry, *extra):
    """the index of the cells the mark kernel ``entry`` (u3d_conv_mark; u3d_convt_mark with the output padding as ``extra``) reaches from
    ``coords``; the K n cell ids exist in the hashed form only, and an empty level launches nothing"""
    n, K = coords.shape[0], geom[0] * geom[1] * geom[2]

    def mark(bitmap):
        cells = torch.empty(K * n, dtype=torch.int64, device=coords.device) if bitmap is None else None
        if n:
            L.call(entry, L.ptr(coords), n, _geom_array(geom), *extra, B, *shape, L.ptr(bitmap), L.ptr(cells), L.stream())
        return cells
    return OccupancyIndex.from_marks(B, oshape, coords.device, mark)


def build_conv_rulebook(coords: torch.Tensor, index: OccupancyIndex, B: int, shape, geom, subm: bool = False):
    """General geometry (csrc/rulebook.hip, conv_mark_k / conv_count_k / conv_write_k): kernel extents 1..3, any stride / padding /
    dilation, spconv's rule.  ``index``: the occupancy index of the INPUT level ``coords``.  ``subm``: the output set is the input set
    (``geom`` then carries stride 1 and the padding d (k - 1) / 2).  Returns (out_coords, out_shape, out_index, Rulebook).
    The rulebook's lists are [K, cap] with cap = min(n_in, n_out) (at least 1): for a fixed offset the pairs are a monotone partial
    bijection between the two levels, so both columns ascend and neither side has more pairs than rows.  It leaves ``Rulebook.coords`` /
    ``index`` unset: those mean "SubM k=3, dilation 1" to the tile-stationary kernels (``_conv_route``)."""
    shape = [int(s) for s in shape]
    oshape, ix_out, new = shape, index, None
    if not subm:
        oshape = conv_out_shape(geom, shape)
        if min(oshape) <= 0:
            raise L.U3DError(f'sparse conv: spatial shape {shape} is smaller than the reach of kernel {tuple(geom[:3])} with dilation '
                             f'{tuple(geom[9:])} and padding {tuple(geom[6:9])}: the output level would have extent {oshape}')
        ix_out = new = _marked_level(coords, B, shape, oshape, geom, 'u3d_conv_mark')
    oc, n2, pin, pout, cnt = _level_pairs(coords, index, B, shape, geom, new)
    return oc, oshape, ix_out, Rulebook(pin, pout, cnt, pin.shape[0], coords.shape[0], n2)


def output_padding_of(output_padding, geom):
    """(q0, q1, q2) of a transposed layer, under ``_triple``'s rules; refused where torch refuses it: 0 <= q < max(stride, dilation)"""
    q = _triple(output_padding, 'output_padding')
    s, d = geom[3:6], geom[9:]
    if not all(0 <= q[a] < max(s[a], d[a]) for a in range(3)):
        raise L.U3DError(f'sparse conv: output_padding {q}: every output padding must be >= 0 and smaller than max(stride, dilation) = '
                         f'{tuple(max(s[a], d[a]) for a in range(3))}')
    return q


def convt_out_shape(geom, outpad, shape):
    """per axis (in - 1) s - 2 p + d (k - 1) + q + 1, torch's rule (u3d_convt_out_shape, host only); an empty grid is refused there"""
    out = (ctypes.c_int * 3)()
    L.call('u3d_convt_out_shape', _geom_array(geom), (ctypes.c_int * 3)(*outpad), *[int(s) for s in shape], out)
    return [int(v) for v in out]


def build_convt_rulebook(coords: torch.Tensor, B: int, shape, geom, outpad):
    """Transposed convolution (csrc/rulebook.hip convt_mark_k, then the general builder's count / write passes): input cell i pairs with
    output cell o = i s - p + t d.  That is ``build_conv_rulebook``'s relation o' s - p + t d = i' with the two levels swapped, so the
    pair lists are those of "the SparseConv3d of this geometry from the NEW level, restricted to these rows": u3d_conv_rulebook with the
    layer's input rows on its stationary side and the new level's index on its looked-up side.  Returns (out_coords, out_shape,
    out_index, Rulebook) with pair_in = new-level rows, pair_out = layer-input rows (n_in = n_new, n_out = n): the layer runs
    ``sparse_conv(..., mode='inv')``, the path ``SparseInverseConv3d`` takes over a general rulebook.  Both columns ascend inside an offset
    (the same monotone map, read from the other side), cap = min(n_in, n_out) (at least 1); one host read, ``count()``.  It leaves
    ``Rulebook.coords`` / ``index`` unset (``_conv_route``)."""
    shape = [int(s) for s in shape]
    try:
        oshape = convt_out_shape(geom, outpad, shape)
    except L.U3DError as e:
        raise L.U3DError(f'sparse conv transpose: spatial shape {shape} with kernel {tuple(geom[:3])}, stride {tuple(geom[3:6])}, padding '
                         f'{tuple(geom[6:9])}, dilation {tuple(geom[9:])} and output padding {tuple(outpad)} has no output level: {e}') from None
    ix_out = _marked_level(coords, B, shape, oshape, geom, 'u3d_convt_mark', (ctypes.c_int * 3)(*outpad))
    oc, n2, pin, pout, cnt = _level_pairs(coords, None, B, shape, geom, new=ix_out, transposed=True)
    return oc, oshape, ix_out, Rulebook(pin, pout, cnt, pin.shape[0], n2, coords.shape[0])


# ----------------------------------------------------------------------------------------
# levels made from levels: the union of two voxel sets, the rows a mask keeps
# ----------------------------------------------------------------------------------------
class UnionLevel:
    """The union of two levels A and B of one grid.  ``coords`` / ``index`` / ``n``: its rows (canonical order), occupancy index and row
    count; ``rows_a`` / ``rows_b`` int32 [n]: the operand row of every union row, or -1; ``same``: 'a' / 'b' when the union IS that
    operand's level (then ``coords`` and ``index`` are that operand's own objects), else None.  ``into(which)``: int32 [n_operand], the
    union row of every operand row (the backward's map), built on first use."""

    def __init__(self, coords, index, n, rows_a, rows_b, same, a_coords, b_coords):
        self.coords, self.index, self.n, self.rows_a, self.rows_b, self.same = coords, index, n, rows_a, rows_b, same
        self._operand = {'a': a_coords, 'b': b_coords}
        self._into: Dict = {}

    def into(self, which: str) -> torch.Tensor:
        if which not in self._into:      # every operand cell is in the union: no -1, and the map is injective
            self._into[which] = self.index.rows_of(self._operand[which])
        return self._into[which]


def build_union_level(a_coords, a_index: OccupancyIndex, b_coords, b_index: OccupancyIndex, B: int, shape) -> UnionLevel:
    """The level on the union of the rows ``a_coords`` and ``b_coords`` (both canonical, one grid).  The index comes from
    ``OccupancyIndex.from_marks`` like every other: two marks into the one zeroed bitmap (``atomicOr``: the union) and the rank pass, or
    the two cell-id lists concatenated into the hashed build (which drops the duplicates).  One host read, ``count()``.  A union with as
    many rows as an operand IS that operand's level -- canonical order makes "a superset with the same count" the same rows in the same
    order -- and keeps that operand's coordinate tensor and index; otherwise ``coords(n)`` writes the new rows.  The destination-major
    maps are the union's coordinates looked up in each operand's index (``rows_of``)."""
    shape = [int(s) for s in shape]
    na, nb, dev = a_coords.shape[0], b_coords.shape[0], a_coords.device

    def mark(bitmap):
        if bitmap is not None:
            for c in (a_coords, b_coords):
                if c.shape[0]:
                    L.call('u3d_index_mark', L.ptr(c), c.shape[0], 0, *shape, L.ptr(bitmap), L.stream())
            return None
        cells = torch.empty(na + nb, dtype=torch.int64, device=dev)
        for c, out in ((a_coords, cells[:na]), (b_coords, cells[na:])):
            if c.shape[0]:
                L.call('u3d_cells_of_coords', L.ptr(c), c.shape[0], 0, B, *shape, L.ptr(out), L.stream())
        return cells
    ix = OccupancyIndex.from_marks(B, shape, dev, mark)
    n = ix.count()
    same = 'a' if n == na else 'b' if n == nb else None
    if same is not None:
        coords, ix = (a_coords, a_index) if same == 'a' else (b_coords, b_index)
    else:
        coords = ix.coords(n)
    return UnionLevel(coords, ix, n, a_index.rows_of(coords), b_index.rows_of(coords), same, a_coords, b_coords)


def compact_mask(keep: torch.Tensor):
    """(kept int32 [n_keep] ascending, pos int32 [n]: the position of a row in ``kept`` or -1, n_keep) of a torch.bool mask [n] on the
    device (u3d_mask_compact: block counts, scan, ballot prefix; stable, no atomics).  One host read, the count; an empty mask launches
    nothing."""
    n, dev = keep.shape[0], keep.device
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    if not n:
        return kept, pos, 0
    n_dev = torch.empty(1, dtype=torch.int32, device=dev)
    w = L.ws(L.lib().u3d_mask_compact_ws_bytes(n), dev)
    L.call('u3d_mask_compact', L.ptr(keep), n, L.ptr(kept), L.ptr(pos), L.ptr(n_dev), L.ptr(w), L.stream())
    n_keep = int(n_dev.item())             # documented read-back (one host sync), as ``OccupancyIndex.count``
    return kept[:n_keep], pos, n_keep


# ----------------------------------------------------------------------------------------
# levels from dense grids (csrc/sparse_dense.hip): dense cell number of (b, x, y, z) = ((b X + x) Y + y) Z + z
# ----------------------------------------------------------------------------------------
def dense_cells(B: int, shape, what: str) -> int:
    """B X Y Z, refused at 2^31 and above: cell and row numbers are 32-bit (element offsets are not)"""
    n_cells = int(B)
    for s in shape:
        n_cells *= int(s)
    if int(B) < 0 or any(int(s) < 0 for s in shape):
        raise L.U3DError(f'{what}: the grid {int(B)} x {" x ".join(str(int(s)) for s in shape)} has a negative extent')
    if n_cells >= 1 << 31:
        raise L.U3DError(f'{what}: the grid {int(B)} x {" x ".join(str(int(s)) for s in shape)} has {n_cells} cells, 2^31 or more: cell numbers are 32-bit')
    return n_cells


def active_cells(x: torch.Tensor):
    """(kept int32 [n_active] ascending, pos int32 [n_cells], n_active) of a contiguous fp32 channels-last grid [B, X, Y, Z, C] on the
    device: a cell is active iff any of its C values != 0 (u3d_dense_active), the mask goes through ``compact_mask``.  Ascending cell
    number = canonical row order.  One host read, the count; a grid without cells launches nothing."""
    C = x.shape[-1]
    n_cells = x.numel() // C
    mask = torch.empty(n_cells, dtype=torch.bool, device=x.device)
    if n_cells:
        L.call('u3d_dense_active', L.ptr(x), n_cells, C, L.ptr(mask), L.stream())
    return compact_mask(mask)


def cells_coords(cells: torch.Tensor, shape) -> torch.Tensor:
    """int32 [n, 4] = (b, x, y, z) of the dense cell numbers ``cells`` int32 [n] (u3d_cells_coords); no cells, no launch"""
    n = cells.shape[0]
    coords = torch.empty(n, 4, dtype=torch.int32, device=cells.device)
    if n:
        L.call('u3d_cells_coords', L.ptr(cells.contiguous()), n, *[int(s) for s in shape], L.ptr(coords), L.stream())
    return mark_canonical(coords)


# ----------------------------------------------------------------------------------------
# scene ranges (csrc/sparse_scene.hip, include/u3d.h section S3)
# ----------------------------------------------------------------------------------------
# Coordinate rows that this library wrote itself (``OccupancyIndex.coords``, ``cells_coords``, a subset of such rows taken in order) are in
# canonical order by construction: they carry a mark, an attribute of the tensor object as a bf16 shadow is one of its features.  Rows a
# caller hands in carry none until a reader of the order flag has seen it clear (``check_scene_order``).
def mark_canonical(coords: torch.Tensor) -> torch.Tensor:
    coords._u3d_canonical = True
    return coords


def is_canonical(coords: torch.Tensor) -> bool:
    return getattr(coords, '_u3d_canonical', False)


def scene_offsets(indices: torch.Tensor, B: int):
    """(offsets int32 [B + 1], flag int32 [1]) of coordinate rows int32 [n, 4] in canonical order, on their device: offsets[b] = the first
    row whose batch index is >= b, offsets[B] = n (u3d_scene_offsets: thread = row, every entry written once).  flag != 0: a batch index
    descends (bit 0) or lies outside [0, B) (bit 1) -- ``check_scene_order`` turns a flag value into the error.  No host read; no rows
    gives zeros without a launch."""
    if not isinstance(B, int) or isinstance(B, bool) or B < 1:
        raise L.U3DError(f'scene_offsets: batch_size must be an int >= 1, got {B!r}')
    if indices.dim() != 2 or indices.shape[1] != 4 or indices.dtype != torch.int32:
        raise L.U3DError(f'scene_offsets: coordinates must be int32 [n, 4], got {indices.dtype} {tuple(indices.shape)}')
    n, dev = indices.shape[0], indices.device
    if not n:
        buf = torch.zeros(B + 2, dtype=torch.int32, device=dev)
        return buf[:B + 1], buf[B + 1:]
    buf = torch.empty(B + 2, dtype=torch.int32, device=dev)
    offsets, flag = buf[:B + 1], buf[B + 1:]
    L.call('u3d_scene_offsets', L.ptr(indices.contiguous()), n, B, L.ptr(offsets), L.ptr(flag), L.stream())
    return offsets, flag


def check_scene_order(flag: int, what: str, B: int):
    """raise for a non-zero order flag of ``scene_offsets``, naming the first thing that can be said about the violation"""
    if flag & 2:
        raise L.U3DError(f'{what}: a batch index lies outside [0, {B}): the tensor is not in canonical order (ascending ((b X + x) Y + y) Z + z)')
    if flag & 1:
        raise L.U3DError(f'{what}: the batch indices descend: the tensor is not in canonical order (ascending ((b X + x) Y + y) Z + z)')


# ----------------------------------------------------------------------------------------
# the level cache: what lives where in a SparseConvTensor's ``indice_dict``
# ----------------------------------------------------------------------------------------
#   indice_key of a SubM layer, or ('__subm__', id(layer))        -> its Rulebook
#   ('__down__', name) of a strided convolution / pooling layer   -> (out_coords, out_shape, out_index, Rulebook)
#   name itself, for such a layer                                 -> (Rulebook, in_coords, in_shape, in_index): what the inverse layer reads
#   ('__up__', name) of a transposed layer, and name itself       -> one UpLevel (out_coords, out_shape, out_index, Rulebook)
#   ('__index__', shape, address of the rows)                     -> the OccupancyIndex of a tensor built without one
# name = the layer's indice_key; ('__anon__', id(layer)) for a keyless layer, which then has no entry under a plain name.  The U-Net's own
# keyless k = 2 / s = 2 / p = 0 layer keeps the name None, alias included, as it always did.
_DOWN_K2S2 = (2, 2, 2, 2, 2, 2, 0, 0, 0, 1, 1, 1)      # the U-Net's strided layer: the hard-coded parity rulebook (``build_down_rulebook``)


class UpLevel(tuple):
    """(out_coords, out_shape, out_index, Rulebook) of a ``SparseConvTranspose3d``: its ``indice_dict`` entry, under ('__up__', name) and
    under the plain ``indice_key``, where the other layer kinds recognise it by its type"""


# (kind of the layer that asks, kind of the entry that holds its indice_key) -> what the refusal calls the holder; pairs that are not
# here do not collide (same kind: a shared key; a strided layer over a SubM layer's key replaces the plain entry, as it always did)
_TAKEN = {('subm', 'down'): 'strided convolution', ('subm', 'up'): 'SparseConvTranspose3d', ('down', 'up'): 'SparseConvTranspose3d',
          ('up', 'subm'): 'SubMConv3d', ('up', 'down'): 'strided convolution or pooling layer'}


def _agree(layer, rb: Rulebook, mine):
    """a rulebook found under a layer's ``indice_key`` must have been built for that layer's geometry"""
    if rb.geom is not None and rb.geom != mine:
        raise L.U3DError(f'{type(layer).__name__}: indice_key {layer.indice_key!r} holds a rulebook built for geometry {rb.geom}, this layer '
                         f'has {mine}: layers that share an indice_key must share kernel_size, stride, padding and dilation')


def saved_under(indice_dict, name):
    """(kind, entry) under the plain key ``name``: ('subm', Rulebook), ('down', (Rulebook, in_coords, in_shape, in_index)), ('up', UpLevel), (None, None)"""
    entry = indice_dict.get(name)
    kind = None if entry is None else 'subm' if isinstance(entry, Rulebook) else 'up' if isinstance(entry, UpLevel) else 'down'
    return kind, entry


def tensor_index(indice_dict, coords, B, shape) -> OccupancyIndex:
    """the occupancy index of a level that came without one, built once per ``indice_dict``"""
    key = ('__index__', tuple(shape), coords.data_ptr())
    if key not in indice_dict:
        indice_dict[key] = OccupancyIndex.from_coords(coords, B, shape)
    return indice_dict[key]


def cached_level(x, kind: str, layer, geom, build):
    """The geometry of ``layer`` ('subm' / 'down' / 'up') on the sparse tensor ``x``, from ``x.indice_dict`` or built by ``build()`` and
    entered there (layouts above): a Rulebook for 'subm', (out_coords, out_shape, out_index, Rulebook) otherwise.  ``geom``: the identity
    stamped on a new rulebook and compared on a hit (``_agree``).  A keyless layer's entry is ``id``-keyed: no alias, no ``tag``."""
    d, name = x.indice_dict, layer.indice_key
    if name is None and not (kind == 'down' and layer.geom == _DOWN_K2S2):
        name = ('__subm__' if kind == 'subm' else '__anon__', id(layer))
    named = isinstance(name, str) if kind == 'subm' else not isinstance(name, tuple)       # a tag, and for 'down' / 'up' the alias
    key = name if kind == 'subm' else ('__down__' if kind == 'down' else '__up__', name)
    hit = d.get(key)
    if hit is not None and (kind != 'subm' or isinstance(hit, Rulebook)):
        _agree(layer, hit if kind == 'subm' else hit[3], geom)
        return hit
    if kind != 'up' or named:
        holder = saved_under(d, name)[0]
        if kind == 'up' and holder != 'subm' and (name in d or ('__down__', name) in d):
            holder = 'down'              # whatever else holds a transposed layer's key: the strided kinds' message, as always
        if (kind, holder) in _TAKEN:
            who = {'subm': 'SubMConv3d', 'up': 'SparseConvTranspose3d'}.get(kind, type(layer).__name__)
            raise L.U3DError(f'{who}: indice_key {name!r} is taken by a {_TAKEN[kind, holder]}')
    level = build()
    rb = level if kind == 'subm' else level[3]
    rb.geom, rb.tag = geom, None if not named else ('subm', key) if kind == 'subm' else key
    d[key] = level if kind == 'subm' else UpLevel(level) if kind == 'up' else tuple(level)
    if named and kind != 'subm':          # ``_index``, not ``index``: the inverse layer may never need one built
        d[name] = d[key] if kind == 'up' else (rb, x.indices, x.spatial_shape, x._index)
    return d[key]


def strided_geometry(layer, x):
    """(out_coords, out_shape, out_index, Rulebook) of a layer that moves to a new level -- ``SparseConv3d`` and the pooling layers, which
    consume the same ``layer.geom`` and ``layer.indice_key``, so a pool and a convolution that share both share one rulebook (``cached_level``)"""
    def build():
        if layer.geom != _DOWN_K2S2:
            return build_conv_rulebook(x.indices, x.index, x.batch_size, x.spatial_shape, layer.geom)
        return build_down_rulebook(x.indices, x.batch_size, x.spatial_shape)
    return cached_level(x, 'down', layer, ('conv', *layer.geom), build)
