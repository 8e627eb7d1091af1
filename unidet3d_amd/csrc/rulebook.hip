// R2 / R3 rulebooks on gfx950.
// Replaces spconv's indice-pair generation for SubMConv3d(k=3) and SparseConv3d(k=2,s=2)
// (reference call sites unidet3d/spconv_unet.py:43-56,148-154,178-183; unidet3d/unidet3d.py:97-103), and, for every other layer
// shape with kernel extents up to 3 (stride, padding, dilation), the general builder further down (conv_mark_k / conv_count_k / conv_write_k).
// Neighbour lookup goes through the occupancy bitmap + popcount rank (u3d_common.h) --
// the key -> row map is a direct-address table, so rows come out in canonical (sorted-key)
// order by construction and the pair lists are bit-exact against the CPU oracle.
// Pair lists are produced by a two-pass stable compaction: per-block counts (ballot/popcount),
// a per-offset scan of block counts, then a wave-64 ballot prefix inside each block.
#include "rb_compact.h"      // RB_T, rb_scan_k, rb_block_rank: shared with sparse_sets.hip

namespace u3d {

// val[k*n + i] = parent row if offset(i) == k (and the parent is inside the halved grid) else -1
__global__ __launch_bounds__(RB_T) void down_nbr_k(const int32_t* __restrict__ coords, int64_t n, Index ix2, int32_t* val) {
    const int64_t i = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    if (i >= n) return;
    const int4 c = *reinterpret_cast<const int4*>(coords + i * 4);
    const int k = ((c.y & 1) << 2) | ((c.z & 1) << 1) | (c.w & 1);
    const int prow = index_lookup(ix2, c.x, c.y >> 1, c.z >> 1, c.w >> 1);
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) val[(int64_t)kk * n + i] = (kk == k) ? prow : -1;
}

__global__ __launch_bounds__(RB_T) void index_mark_k(const int32_t* __restrict__ coords, int64_t n, int shift, int X2, int Y2, int Z2,
                                                     int Zw2, unsigned long long* bitmap2) {
    const int64_t i = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    if (i >= n) return;
    const int4 c = *reinterpret_cast<const int4*>(coords + i * 4);
    const int x = c.y >> shift, y = c.z >> shift, z = c.w >> shift;
    if ((unsigned)x >= (unsigned)X2 || (unsigned)y >= (unsigned)Y2 || (unsigned)z >= (unsigned)Z2) return;   // odd extent: edge voxel dropped
    const int64_t w = ((int64_t)(c.x * X2 + x) * Y2 + y) * Zw2 + (z >> 6);
    atomicOr(&bitmap2[w], 1ull << (z & 63));
}

// grid (nblk, K)
__global__ __launch_bounds__(RB_T) void rb_count_k(const int32_t* __restrict__ val, int64_t n, int nblk, int32_t* block_cnt) {
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    const int k = blockIdx.y;
    const bool ok = r < n && val[(int64_t)k * n + r] >= 0;
    const int c = __syncthreads_count(ok);
    if (threadIdx.x == 0) block_cnt[(int64_t)k * nblk + blockIdx.x] = c;
}

// stable compaction: list_row[k][pos] = r, list_val[k][pos] = val[k][r]   grid (nblk, K)
__global__ __launch_bounds__(RB_T) void rb_write_k(const int32_t* __restrict__ val, int64_t n, int nblk, const int32_t* __restrict__ block_base,
                                                   int64_t cap, int32_t* list_row, int32_t* list_val) {
    __shared__ int s_w[RB_T / 64];
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    const int k = blockIdx.y;
    const int v = r < n ? val[(int64_t)k * n + r] : -1;
    const bool ok = v >= 0;
    const int rank = rb_block_rank(ok, s_w);
    if (ok) {
        const int64_t pos = (int64_t)k * cap + block_base[(int64_t)k * nblk + blockIdx.x] + rank;
        list_row[pos] = (int)r;
        list_val[pos] = v;
    }
}

// ---- SubM rulebook without the dense neighbour matrix -------------------------------------------------------------------
// Rounds 1-2 stored nbr[27][n] (subm_nbr_k) and read it back in the count and the write pass: 3 x 27 n 4 B = 115 MB of traffic at
// level 1 of cfg2 for 34 MB of pairs.  The lookup is a bitmap word + a rank word (L2-resident), so both passes now redo it.
__device__ __forceinline__ int subm_lookup(const int32_t* __restrict__ coords, int64_t o, int k, const Index& ix) {
    const int dx = k / 9 - 1, dy = (k / 3) % 3 - 1, dz = k % 3 - 1;
    const int4 c = *reinterpret_cast<const int4*>(coords + o * 4);
    return index_lookup(ix, c.x, c.y + dx, c.z + dy, c.w + dz);
}

// grid (nblk, 27)
__global__ __launch_bounds__(RB_T) void subm_count_k(const int32_t* __restrict__ coords, int64_t n, Index ix, int nblk, int32_t* block_cnt) {
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    const int k = blockIdx.y;
    const bool ok = r < n && subm_lookup(coords, r, k, ix) >= 0;
    const int c = __syncthreads_count(ok);
    if (threadIdx.x == 0) block_cnt[(int64_t)k * nblk + blockIdx.x] = c;
}

// stable compaction, as rb_write_k: list_row[k][pos] = output row, list_val[k][pos] = its neighbour's row    grid (nblk, 27)
__global__ __launch_bounds__(RB_T) void subm_write_k(const int32_t* __restrict__ coords, int64_t n, Index ix, int nblk,
                                                     const int32_t* __restrict__ block_base, int64_t cap, int32_t* list_row, int32_t* list_val) {
    __shared__ int s_w[RB_T / 64];
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    const int k = blockIdx.y;
    const int v = r < n ? subm_lookup(coords, r, k, ix) : -1;
    const bool ok = v >= 0;
    const int rank = rb_block_rank(ok, s_w);
    if (ok) {
        const int64_t pos = (int64_t)k * cap + block_base[(int64_t)k * nblk + blockIdx.x] + rank;
        list_row[pos] = (int)r;
        list_val[pos] = v;
    }
}

// ---- general convolution geometry: kernel extents 1..3 per axis, any stride / padding / dilation ------------------------------
// spconv's rule, per axis: out_dim = floor((in_dim + 2 p - d (k - 1) - 1) / s) + 1, and output cell o is active iff an active input i and
// a tap t in [0, k) satisfy i + p = o s + t d on all three axes with 0 <= o < out_dim.  Offset index = (t0 k1 + t1) k2 + t2, the order of
// the weight layout [C_out, k0, k1, k2, C_in].  SparseConv3d(k=2, s=2) (out = in >> 1, edge drop) and SubMConv3d(k=3) (p = 1, output set
// = input set) are special cases and come out of these kernels with the same lists as down_nbr_k / subm_lookup above.
//
// The rulebook pass is output-stationary like the SubM builder: thread = output row r, grid.y = offset, value = the row of the input cell
// o s - p + t d in the INPUT level's index, looked up again in the count and in the write pass (same traffic argument as above).
// Both columns of an offset's list ascend and no row repeats: for a fixed tap the map o -> o s - p + t d is, axis by axis, strictly
// increasing, so it is injective and keeps the lexicographic order of (b, x, y, z), which is the canonical order of either level.  Walking
// the output rows in order therefore emits the input rows in order, and an offset has at most min(n_in, n_out) pairs.
struct ConvGeom {
    int k[3], s[3], p[3], d[3];
    int out[3];                 // output extents
    int K;                      // k[0] k[1] k[2]
};

__device__ __forceinline__ void conv_taps(const ConvGeom& g, int k, int t[3]) {
    t[2] = k % g.k[2];
    t[1] = (k / g.k[2]) % g.k[1];
    t[0] = k / (g.k[2] * g.k[1]);
}

// output cell of input cell `c` under tap `t` on one axis, or -1
__device__ __forceinline__ int conv_out_of_in(int c, int t, int s, int p, int d, int out_dim) {
    const int v = c + p - t * d;
    if (v < 0) return -1;
    // the stride is uniform over the launch: strides 1 and 2 (nearly every layer) take no integer division, one scalar branch instead
    const int o = s == 1 ? v : (s == 2 ? v >> 1 : v / s);
    return (o * s == v && o < out_dim) ? o : -1;
}

// grid (nblk, K): marks the output cell of (input row, tap) where there is one.  bitmap != nullptr: sets its bit (bitmap zeroed by the
// caller); else cells[k n + i] = the cell id, CELL_NONE for none (the hashed index sorts and uniques them)
__global__ __launch_bounds__(RB_T) void conv_mark_k(const int32_t* __restrict__ coords, int64_t n, ConvGeom g, int B, int Zw, unsigned long long* bitmap,
                                                    int64_t* __restrict__ cells) {
    const int64_t i = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    if (i >= n) return;
    const int k = blockIdx.y;
    int t[3];
    conv_taps(g, k, t);
    const int4 c = *reinterpret_cast<const int4*>(coords + i * 4);
    const int x = conv_out_of_in(c.y, t[0], g.s[0], g.p[0], g.d[0], g.out[0]);
    const int y = conv_out_of_in(c.z, t[1], g.s[1], g.p[1], g.d[1], g.out[1]);
    const int z = conv_out_of_in(c.w, t[2], g.s[2], g.p[2], g.d[2], g.out[2]);
    const bool ok = (x | y | z) >= 0 && (unsigned)c.x < (unsigned)B;
    const int64_t w = (((int64_t)c.x * g.out[0] + x) * g.out[1] + y) * Zw + (z >> 6);
    if (bitmap) {
        if (ok) atomicOr(&bitmap[w], 1ull << (z & 63));
    } else {
        cells[(int64_t)k * n + i] = ok ? w * 64 + (z & 63) : 0x7fffffffffffffffLL;
    }
}

// Transposed convolution (SparseConvTranspose3d): the output cell of (input row, tap) is o = i s - p + t d -- no division, no stride
// branch, only the range test against the output extent (g.out holds the TRANSPOSED layer's output extents here, convt_geom).  Same
// launch shape and the same two output forms as conv_mark_k.  The relation is conv_lookup's o' s - p + t d = i' with the two levels
// swapped, so the pair lists come from conv_count_k / conv_write_k run over the layer's INPUT rows against the new level's index, and
// the ascending-columns argument above holds read from the other side: for a fixed tap i -> i s - p + t d is strictly increasing on
// every axis, hence injective and order-preserving from the layer's input level into the new level; walking the input rows in
// canonical order emits the new level's rows in canonical order, no row repeats, and an offset has at most min(n_in, n_out) pairs.
__global__ __launch_bounds__(RB_T) void convt_mark_k(const int32_t* __restrict__ coords, int64_t n, ConvGeom g, int B, int Zw, unsigned long long* bitmap,
                                                     int64_t* __restrict__ cells) {
    const int64_t i = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    if (i >= n) return;
    const int k = blockIdx.y;
    int t[3];
    conv_taps(g, k, t);
    const int4 c = *reinterpret_cast<const int4*>(coords + i * 4);
    const int x = c.y * g.s[0] - g.p[0] + t[0] * g.d[0];
    const int y = c.z * g.s[1] - g.p[1] + t[1] * g.d[1];
    const int z = c.w * g.s[2] - g.p[2] + t[2] * g.d[2];
    const bool ok = (unsigned)x < (unsigned)g.out[0] && (unsigned)y < (unsigned)g.out[1] && (unsigned)z < (unsigned)g.out[2] &&
                    (unsigned)c.x < (unsigned)B;
    const int64_t w = (((int64_t)c.x * g.out[0] + x) * g.out[1] + y) * Zw + (z >> 6);
    if (bitmap) {
        if (ok) atomicOr(&bitmap[w], 1ull << (z & 63));
    } else {
        cells[(int64_t)k * n + i] = ok ? w * 64 + (z & 63) : 0x7fffffffffffffffLL;
    }
}

__device__ __forceinline__ int conv_lookup(const int32_t* __restrict__ out_coords, int64_t r, int k, const ConvGeom& g, const Index& ix) {
    int t[3];
    conv_taps(g, k, t);
    const int4 c = *reinterpret_cast<const int4*>(out_coords + r * 4);
    return index_lookup(ix, c.x, c.y * g.s[0] - g.p[0] + t[0] * g.d[0], c.z * g.s[1] - g.p[1] + t[1] * g.d[1], c.w * g.s[2] - g.p[2] + t[2] * g.d[2]);
}

// grid (nblk, K)
__global__ __launch_bounds__(RB_T) void conv_count_k(const int32_t* __restrict__ out_coords, int64_t n, ConvGeom g, Index ix, int nblk,
                                                     int32_t* block_cnt) {
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    const int k = blockIdx.y;
    const bool ok = r < n && conv_lookup(out_coords, r, k, g, ix) >= 0;
    const int c = __syncthreads_count(ok);
    if (threadIdx.x == 0) block_cnt[(int64_t)k * nblk + blockIdx.x] = c;
}

// stable compaction, as subm_write_k: list_row[k][pos] = output row, list_val[k][pos] = its input row    grid (nblk, K)
__global__ __launch_bounds__(RB_T) void conv_write_k(const int32_t* __restrict__ out_coords, int64_t n, ConvGeom g, Index ix, int nblk,
                                                     const int32_t* __restrict__ block_base, int64_t cap, int32_t* list_row, int32_t* list_val) {
    __shared__ int s_w[RB_T / 64];
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    const int k = blockIdx.y;
    const int v = r < n ? conv_lookup(out_coords, r, k, g, ix) : -1;
    const bool ok = v >= 0;
    const int64_t at = (int64_t)block_base[(int64_t)k * nblk + blockIdx.x] + rb_block_rank(ok, s_w);
    if (ok && at < cap) {       // (at < cap always holds for cap >= min(n_in, n_out), which the entry point checks)
        list_row[(int64_t)k * cap + at] = (int)r;
        list_val[(int64_t)k * cap + at] = v;
    }
}

// geom = kernel[3], stride[3], padding[3], dilation[3] (host) -> ConvGeom for input extents (X, Y, Z); U3D_OK, or the code with the text set.
// Output extents may come out <= 0 (an input smaller than the kernel's reach): they are reported as 0, an empty level.
static int conv_geom(const int32_t* geom, int X, int Y, int Z, ConvGeom* g) {
    if (!geom || X <= 0 || Y <= 0 || Z <= 0) { set_error("conv geometry: null geometry or non-positive extent %d x %d x %d", X, Y, Z); return U3D_EINVAL; }
    const int in[3] = {X, Y, Z};
    g->K = 1;
    for (int a = 0; a < 3; ++a) {
        const int k = geom[a], s = geom[3 + a], p = geom[6 + a], d = geom[9 + a];
        if (k < 1 || k > 3) { set_error("conv geometry: kernel extent %d on axis %d is outside 1..3", k, a); return U3D_EUNSUPPORTED; }
        if (s < 1 || d < 1 || p < 0) { set_error("conv geometry: stride %d / dilation %d must be >= 1 and padding %d >= 0 (axis %d)", s, d, p, a); return U3D_EINVAL; }
        // every coordinate the kernels form lies in [-(p + 2 d), in + 2 p + 2 d]: keep that inside int32
        if ((int64_t)in[a] + 2 * (int64_t)p + 2 * (int64_t)d >= 0x7fffffffLL) {
            set_error("conv geometry: extent %d + 2 * padding %d + 2 * dilation %d overflows 32-bit coordinates (axis %d)", in[a], p, d, a);
            return U3D_EUNSUPPORTED;
        }
        const int64_t span = (int64_t)in[a] + 2 * (int64_t)p - (int64_t)d * (k - 1) - 1;
        g->k[a] = k; g->s[a] = s; g->p[a] = p; g->d[a] = d;
        g->out[a] = span < 0 ? 0 : (int)(span / s) + 1;
        g->K *= k;
    }
    return U3D_OK;
}

// The transposed layer of `geom` with output padding outpad[3] on INPUT extents (X, Y, Z): conv_geom's validation of k / s / p / d, then
// torch's rule per axis, out = (in - 1) s - 2 p + d (k - 1) + q + 1, formed in int64; g->out receives it.  U3D_OK, or the code with
// the text set -- all before any HIP call.
static int convt_geom(const int32_t* geom, const int32_t* outpad, int X, int Y, int Z, ConvGeom* g) {
    const int rc = conv_geom(geom, X, Y, Z, g);
    if (rc != U3D_OK) return rc;
    if (!outpad) { set_error("conv transpose geometry: null output padding"); return U3D_EINVAL; }
    const int in[3] = {X, Y, Z};
    for (int a = 0; a < 3; ++a) {
        const int q = outpad[a], lim = g->s[a] > g->d[a] ? g->s[a] : g->d[a];
        if (q < 0 || q >= lim) {
            set_error("conv transpose geometry: output padding %d must be >= 0 and smaller than max(stride %d, dilation %d) (axis %d)", q, g->s[a], g->d[a], a);
            return U3D_EINVAL;
        }
        const int64_t out = ((int64_t)in[a] - 1) * g->s[a] - 2 * (int64_t)g->p[a] + (int64_t)g->d[a] * (g->k[a] - 1) + q + 1;
        if (out <= 0) {
            set_error("conv transpose geometry: the output grid is empty: extent %lld on axis %d (input %d, padding %d beyond the reach)", (long long)out, a, in[a], g->p[a]);
            return U3D_EINVAL;
        }
        // every coordinate the kernels form lies in [-p, out + 2 p): keep that, and what conv_geom asks of the new level, inside int32
        if (out + 2 * (int64_t)g->p[a] + 2 * (int64_t)g->d[a] >= 0x7fffffffLL) {
            set_error("conv transpose geometry: output extent %lld + 2 * padding %d + 2 * dilation %d overflows 32-bit coordinates (axis %d)", (long long)out, g->p[a], g->d[a], a);
            return U3D_EUNSUPPORTED;
        }
        g->out[a] = (int)out;
    }
    return U3D_OK;
}

// tile_starts[k][t] = lower_bound(rows[k][0..counts[k]), t*T)
__global__ __launch_bounds__(256) void tile_starts_k(const int32_t* __restrict__ rows, const int32_t* __restrict__ counts, int64_t cap,
                                                     int T, int64_t n_tiles, int32_t* out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (t > n_tiles) return;
    const int32_t* a = rows + (int64_t)k * cap;
    const int64_t target = t * T;
    int lo = 0, hi = counts[k];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)a[mid] < target) lo = mid + 1; else hi = mid;
    }
    out[(int64_t)k * (n_tiles + 1) + t] = lo;
}

static int compact(const int32_t* val, int64_t n, int K, int64_t cap, int32_t* list_row, int32_t* list_val,
                   int32_t* counts, int32_t* block_cnt, int32_t* block_base, hipStream_t s) {
    const int nblk = (int)ceil_div(n, RB_T);
    hipLaunchKernelGGL(rb_count_k, dim3(nblk, K), dim3(RB_T), 0, s, val, n, nblk, block_cnt);
    hipLaunchKernelGGL(rb_scan_k, dim3(K), dim3(RB_T), 0, s, (const int32_t*)block_cnt, nblk, block_base, counts);
    hipLaunchKernelGGL(rb_write_k, dim3(nblk, K), dim3(RB_T), 0, s, val, n, nblk, (const int32_t*)block_base, cap, list_row, list_val);
    return check_launch("rulebook compact");
}

static int64_t rb_ws_bytes(int64_t n, int K) {
    const int64_t nblk = ceil_div(n, RB_T);
    return (K * n + 2 * K * nblk + 64) * 4;
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int64_t u3d_subm_rulebook_ws_bytes(int64_t n) { return (2 * 27 * ceil_div(n, RB_T) + 64) * 4; }      // block counts + bases only
int64_t u3d_down_rulebook_ws_bytes(int64_t n) { return rb_ws_bytes(n, 8); }

int u3d_subm_rulebook(const int32_t* coords, int64_t n, const uint64_t* bitmap, const int32_t* word_rank, int64_t hash_slots, int B,
                      int X, int Y, int Z, int32_t* pair_in, int32_t* pair_out, int32_t* counts, void* ws,
                      u3d_stream_t stream) {
    if (!coords || !bitmap || !word_rank || !pair_in || !pair_out || !counts || !ws || n <= 0) return U3D_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    const Index ix = make_index(bitmap, word_rank, B, X, Y, Z, hash_slots);
    const int nblk = (int)ceil_div(n, RB_T);
    int32_t* bc = (int32_t*)ws;
    int32_t* bb = bc + (int64_t)27 * nblk;
    // rows = output voxel, value = input (neighbour) row; count -> per-offset scan of the block counts -> stable write
    hipLaunchKernelGGL(subm_count_k, dim3(nblk, 27), dim3(RB_T), 0, s, coords, n, ix, nblk, bc);
    hipLaunchKernelGGL(rb_scan_k, dim3(27), dim3(RB_T), 0, s, (const int32_t*)bc, nblk, bb, counts);
    hipLaunchKernelGGL(subm_write_k, dim3(nblk, 27), dim3(RB_T), 0, s, coords, n, ix, nblk, (const int32_t*)bb, n, pair_out, pair_in);
    return check_launch("subm rulebook");
}

int u3d_index_mark(const int32_t* coords, int64_t n, int shift, int X2, int Y2, int Z2, uint64_t* bitmap2, u3d_stream_t stream) {
    if (!coords || !bitmap2 || n <= 0 || X2 <= 0 || Y2 <= 0 || Z2 <= 0 || shift < 0 || shift > 8) return U3D_EINVAL;
    hipLaunchKernelGGL(index_mark_k, dim3((unsigned)ceil_div(n, RB_T)), dim3(RB_T), 0, (hipStream_t)stream, coords, n, shift, X2,
                       Y2, Z2, (Z2 + 63) / 64, (unsigned long long*)bitmap2);
    return check_launch("index_mark");
}

int u3d_down_rulebook(const int32_t* coords, int64_t n, const uint64_t* bitmap2, const int32_t* word_rank2, int64_t hash_slots, int B,
                      int X2, int Y2, int Z2, int32_t* pair_in, int32_t* pair_out, int32_t* counts, void* ws,
                      u3d_stream_t stream) {
    if (!coords || !bitmap2 || !word_rank2 || !pair_in || !pair_out || !counts || !ws || n <= 0) return U3D_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    const Index ix = make_index(bitmap2, word_rank2, B, X2, Y2, Z2, hash_slots);
    const int nblk = (int)ceil_div(n, RB_T);
    int32_t* val = (int32_t*)ws;
    int32_t* bc = val + 8 * n;
    int32_t* bb = bc + (int64_t)8 * nblk;
    hipLaunchKernelGGL(down_nbr_k, dim3(nblk), dim3(RB_T), 0, s, coords, n, ix, val);
    // rows = input (child) voxel, value = output (parent) row
    return compact(val, n, 8, n, pair_in, pair_out, counts, bc, bb, s);
}

int u3d_conv_out_shape(const int32_t* geom, int X, int Y, int Z, int32_t* out_shape) {
    ConvGeom g;
    if (!out_shape) return U3D_EINVAL;
    const int rc = conv_geom(geom, X, Y, Z, &g);
    if (rc != U3D_OK) return rc;
    for (int a = 0; a < 3; ++a) out_shape[a] = g.out[a];
    return U3D_OK;
}

int u3d_conv_mark(const int32_t* coords, int64_t n, const int32_t* geom, int B, int X, int Y, int Z, uint64_t* bitmap_out, int64_t* cells_out,
                  u3d_stream_t stream) {
    ConvGeom g;
    const int rc = conv_geom(geom, X, Y, Z, &g);
    if (rc != U3D_OK) return rc;
    if (!coords || n <= 0 || B <= 0 || (bitmap_out != nullptr) == (cells_out != nullptr)) {
        set_error("conv_mark: needs rows, a batch size and exactly one of bitmap_out / cells_out");
        return U3D_EINVAL;
    }
    if (g.out[0] <= 0 || g.out[1] <= 0 || g.out[2] <= 0) { set_error("conv_mark: the output level is empty (%d x %d x %d)", g.out[0], g.out[1], g.out[2]); return U3D_EINVAL; }
    const int64_t zw = (g.out[2] + 63) / 64;
    const long double words = (long double)B * g.out[0] * g.out[1] * zw;
    if (bitmap_out ? words > (long double)U3D_INDEX_MAX_WORDS : words * 64 >= 4.0e18L) {
        set_error("conv_mark: output grid %d x %d x %d x %d is too large for the %s index", B, g.out[0], g.out[1], g.out[2], bitmap_out ? "direct-address" : "hashed");
        return U3D_EUNSUPPORTED;
    }
    if (n >= 0x7fffffffLL / g.K) { set_error("conv_mark: %lld rows x %d offsets exceed 32-bit counts", (long long)n, g.K); return U3D_EUNSUPPORTED; }
    hipLaunchKernelGGL(conv_mark_k, dim3((unsigned)ceil_div(n, RB_T), g.K), dim3(RB_T), 0, (hipStream_t)stream, coords, n, g, B, (int)zw,
                       (unsigned long long*)bitmap_out, cells_out);
    return check_launch("conv_mark");
}

int u3d_convt_out_shape(const int32_t* geom, const int32_t* outpad, int X, int Y, int Z, int32_t* out_shape) {
    ConvGeom g;
    if (!out_shape) { set_error("convt_out_shape: null out_shape"); return U3D_EINVAL; }
    const int rc = convt_geom(geom, outpad, X, Y, Z, &g);
    if (rc != U3D_OK) return rc;
    for (int a = 0; a < 3; ++a) out_shape[a] = g.out[a];
    return U3D_OK;
}

int u3d_convt_mark(const int32_t* coords, int64_t n, const int32_t* geom, const int32_t* outpad, int B, int X, int Y, int Z, uint64_t* bitmap_out,
                   int64_t* cells_out, u3d_stream_t stream) {
    ConvGeom g;
    const int rc = convt_geom(geom, outpad, X, Y, Z, &g);
    if (rc != U3D_OK) return rc;
    if (!coords || n <= 0 || B <= 0 || (bitmap_out != nullptr) == (cells_out != nullptr)) {
        set_error("convt_mark: needs rows, a batch size and exactly one of bitmap_out / cells_out");
        return U3D_EINVAL;
    }
    const int64_t zw = (g.out[2] + 63) / 64;
    const long double words = (long double)B * g.out[0] * g.out[1] * zw;
    if (bitmap_out ? words > (long double)U3D_INDEX_MAX_WORDS : words * 64 >= 4.0e18L) {
        set_error("convt_mark: output grid %d x %d x %d x %d is too large for the %s index", B, g.out[0], g.out[1], g.out[2], bitmap_out ? "direct-address" : "hashed");
        return U3D_EUNSUPPORTED;
    }
    if (n >= 0x7fffffffLL / g.K) { set_error("convt_mark: %lld rows x %d offsets exceed 32-bit counts", (long long)n, g.K); return U3D_EUNSUPPORTED; }
    hipLaunchKernelGGL(convt_mark_k, dim3((unsigned)ceil_div(n, RB_T), g.K), dim3(RB_T), 0, (hipStream_t)stream, coords, n, g, B, (int)zw,
                       (unsigned long long*)bitmap_out, cells_out);
    return check_launch("convt_mark");
}

int64_t u3d_conv_rulebook_ws_bytes(int64_t n_out, int K) {
    if (n_out <= 0 || K <= 0 || K > 27) return 0;
    return (2 * K * ceil_div(n_out, RB_T) + 64) * 4;      // block counts + bases
}

int u3d_conv_rulebook(const int32_t* out_coords, int64_t n_out, int64_t n_in, const uint64_t* bitmap_in, const int32_t* word_rank_in,
                      int64_t hash_slots, int B, int X, int Y, int Z, const int32_t* geom, int64_t cap, int32_t* pair_in, int32_t* pair_out,
                      int32_t* counts, void* ws, u3d_stream_t stream) {
    ConvGeom g;
    const int rc = conv_geom(geom, X, Y, Z, &g);
    if (rc != U3D_OK) return rc;
    if (!out_coords || !bitmap_in || !word_rank_in || !pair_in || !pair_out || !counts || !ws || n_out <= 0 || n_in <= 0 || B <= 0 || hash_slots < 0) {
        set_error("conv_rulebook: null argument or non-positive row count");
        return U3D_EINVAL;
    }
    if (cap < (n_in < n_out ? n_in : n_out)) {
        set_error("conv_rulebook: cap %lld is below min(n_in %lld, n_out %lld)", (long long)cap, (long long)n_in, (long long)n_out);
        return U3D_EINVAL;
    }
    if (n_out >= 0x7fffffffLL || n_in >= 0x7fffffffLL) { set_error("conv_rulebook: row counts exceed int32"); return U3D_EUNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    const Index ix = make_index(bitmap_in, word_rank_in, B, X, Y, Z, hash_slots);
    const int nblk = (int)ceil_div(n_out, RB_T);
    int32_t* bc = (int32_t*)ws;
    int32_t* bb = bc + (int64_t)g.K * nblk;
    hipLaunchKernelGGL(conv_count_k, dim3(nblk, g.K), dim3(RB_T), 0, s, out_coords, n_out, g, ix, nblk, bc);
    hipLaunchKernelGGL(rb_scan_k, dim3(g.K), dim3(RB_T), 0, s, (const int32_t*)bc, nblk, bb, counts);
    hipLaunchKernelGGL(conv_write_k, dim3(nblk, g.K), dim3(RB_T), 0, s, out_coords, n_out, g, ix, nblk, (const int32_t*)bb, cap, pair_out, pair_in);
    return check_launch("conv rulebook");
}

int u3d_tile_starts(const int32_t* rows, const int32_t* counts, int K, int64_t cap, int tile_rows, int64_t n_tiles,
                    int32_t* tile_starts, u3d_stream_t stream) {
    if (!rows || !counts || !tile_starts || K <= 0 || tile_rows <= 0 || n_tiles <= 0) return U3D_EINVAL;
    hipLaunchKernelGGL(tile_starts_k, dim3((unsigned)ceil_div(n_tiles + 1, 256), K), dim3(256), 0, (hipStream_t)stream, rows,
                       counts, cap, tile_rows, n_tiles, tile_starts);
    return check_launch("tile_starts");
}

}  // extern "C"
