// Sparse tensors on different voxel sets (include/u3d.h section S1): the row of every coordinate in an occupancy index, the stable
// compaction of a row mask, and the two row movers behind `sparse_add` (join of two operands on the union of their sets) and `prune`.
// Row movers, the lane shape of sparse_pool.hip: a group of lanes owns a destination row and 16-byte column slices, narrow rows share a
// wave, rows wider than a wave's 256 columns take a column loop, ROWS destination rows of a group are in flight at once.  Every
// destination element is written exactly once: no LDS, no atomics, no memset of the destination.  The row lists ascend (canonical
// order on both sides), so the reads are near-streaming.  A row value outside [0, n_src) is an absent row, whatever it is: a wrong map
// never reads outside a tensor.
#include "rb_compact.h"

// the one addition of this file rounds on its own whatever the command line says (there is no product to contract today; said here so
// that it stays true)
#pragma clang fp contract(off)

namespace u3d {

// thread = row
__global__ __launch_bounds__(RB_T) void index_rows_k(const int32_t* __restrict__ coords, int64_t n, Index ix, int32_t* __restrict__ rows_out) {
    const int64_t i = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    if (i >= n) return;
    const int4 c = *reinterpret_cast<const int4*>(coords + i * 4);
    // (index_lookup tests the three grid axes; the batch test comes first: a wrong batch must not form a word address)
    rows_out[i] = (unsigned)c.x < (unsigned)ix.B ? index_lookup(ix, c.x, c.y, c.z, c.w) : -1;
}

// ---- mask compaction: block counts -> rb_scan_k -> ballot prefix -> stable write (rb_compact.h), one list --------------------------
__global__ __launch_bounds__(RB_T) void mask_count_k(const uint8_t* __restrict__ mask, int64_t n, int32_t* block_cnt) {
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    const bool ok = r < n && mask[r] != 0;
    const int c = __syncthreads_count(ok);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = c;
}

// kept[position] = r for the set rows, pos[r] = position or -1 for every row
__global__ __launch_bounds__(RB_T) void mask_write_k(const uint8_t* __restrict__ mask, int64_t n, const int32_t* __restrict__ block_base,
                                                     int32_t* __restrict__ kept, int32_t* __restrict__ pos) {
    __shared__ int s_w[RB_T / 64];
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    const bool ok = r < n && mask[r] != 0;
    const int at = block_base[blockIdx.x] + rb_block_rank(ok, s_w);
    if (r < n) pos[r] = ok ? at : -1;
    if (ok) kept[at] = (int)r;       // (at < n: at counts the set rows before r)
}

// ---- row movers -----------------------------------------------------------------------------------------------------------------------
constexpr int ROWS = 4;         // destination rows (= row loads per operand) of one group in flight

// lg = log2(lanes per row); group g of the grid serves the destination rows g, g + G, g + 2 G, g + 3 G (G = groups: neighbouring groups
// write neighbouring rows), lane l of it the columns 4 l + 256 i
__global__ __launch_bounds__(256) void rows_take_k(const uint4* __restrict__ x, const int32_t* __restrict__ rows, int64_t n_out, int64_t n_src,
                                                   int64_t G, int C4, int lg, uint4* __restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = t >> lg;
    const int c0 = (int)(t & ((1 << lg) - 1));
    if (g >= G) return;
    int r[ROWS];
#pragma unroll
    for (int u = 0; u < ROWS; ++u) r[u] = g + u * G < n_out ? rows[g + u * G] : -1;
    for (int c = c0; c < C4; c += 1 << lg) {
        uint4 v[ROWS];
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if ((uint64_t)(int64_t)r[u] < (uint64_t)n_src) v[u] = x[(int64_t)r[u] * C4 + c];
        }
#pragma unroll
        for (int u = 0; u < ROWS; ++u)
            if (g + u * G < n_out) y[(g + u * G) * C4 + c] = v[u];
    }
}

// one element of the join: the fp32 sum where both rows are present, the bits of the present one otherwise (+0.0 where neither is)
__device__ __forceinline__ float join(bool pa, bool pb, float a, float b) { return pa && pb ? a + b : (pa ? a : b); }

__global__ __launch_bounds__(256) void rows_take2_k(const float4* __restrict__ a, const int32_t* __restrict__ rows_a, int64_t n_a,
                                                    const float4* __restrict__ b, const int32_t* __restrict__ rows_b, int64_t n_b,
                                                    int64_t n_out, int64_t G, int C4, int lg, float4* __restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = t >> lg;
    const int c0 = (int)(t & ((1 << lg) - 1));
    if (g >= G) return;
    int ra[ROWS], rb[ROWS];
#pragma unroll
    for (int u = 0; u < ROWS; ++u) {
        const bool in = g + u * G < n_out;
        ra[u] = in ? rows_a[g + u * G] : -1;
        rb[u] = in ? rows_b[g + u * G] : -1;
    }
    for (int c = c0; c < C4; c += 1 << lg) {
        float4 va[ROWS], vb[ROWS];
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            va[u] = vb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((uint64_t)(int64_t)ra[u] < (uint64_t)n_a) va[u] = a[(int64_t)ra[u] * C4 + c];
            if ((uint64_t)(int64_t)rb[u] < (uint64_t)n_b) vb[u] = b[(int64_t)rb[u] * C4 + c];
        }
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            if (g + u * G >= n_out) continue;
            const bool pa = (uint64_t)(int64_t)ra[u] < (uint64_t)n_a, pb = (uint64_t)(int64_t)rb[u] < (uint64_t)n_b;
            y[(g + u * G) * C4 + c] = make_float4(join(pa, pb, va[u].x, vb[u].x), join(pa, pb, va[u].y, vb[u].y),
                                                  join(pa, pb, va[u].z, vb[u].z), join(pa, pb, va[u].w, vb[u].w));
        }
    }
}

// lanes per row: the power of two that covers C / 4, one wave at most (sparse_pool.hip's rule)
static int lanes_log2(int C) {
    int lg = 0;
    while (lg < 6 && (4 << lg) < C) ++lg;
    return lg;
}

// the contract the two row movers share, checked before any HIP call
static int check_rows(const char* what, bool null, int64_t n_out, int64_t n_src0, int64_t n_src1, int C) {
    if (null || n_out <= 0 || n_src0 < 0 || n_src1 < 0) {
        set_error("%s: NULL pointer, no destination rows (n_out = %lld) or a negative source row count", what, (long long)n_out);
        return U3D_EINVAL;
    }
    if (C < 4 || C > 512 || C % 4) { set_error("%s: width %d unsupported (a multiple of 4 in 4..512)", what, C); return U3D_EUNSUPPORTED; }
    if (n_out >= 0x80000000LL || n_src0 >= 0x80000000LL || n_src1 >= 0x80000000LL) {
        set_error("%s: row counts (%lld destination, %lld / %lld source) exceed 32-bit row numbers", what, (long long)n_out, (long long)n_src0,
                  (long long)n_src1);
        return U3D_EUNSUPPORTED;
    }
    return U3D_OK;
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int u3d_index_rows(const int32_t* coords, int64_t n, const uint64_t* bitmap, const int32_t* word_rank, int64_t hash_slots, int B, int X, int Y,
                   int Z, int32_t* rows_out, u3d_stream_t stream) {
    if (!coords || !bitmap || !word_rank || !rows_out || n <= 0 || B <= 0 || X <= 0 || Y <= 0 || Z <= 0 || hash_slots < 0) {
        set_error("index_rows: NULL pointer, no rows (n = %lld), an empty grid %d x %d x %d x %d or negative hash_slots", (long long)n, B, X, Y, Z);
        return U3D_EINVAL;
    }
    if (n >= 0x80000000LL) { set_error("index_rows: %lld rows exceed 32-bit row numbers", (long long)n); return U3D_EUNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    const Index ix = make_index(bitmap, word_rank, B, X, Y, Z, hash_slots);
    hipLaunchKernelGGL(index_rows_k, dim3((unsigned)ceil_div(n, RB_T)), dim3(RB_T), 0, s, coords, n, ix, rows_out);
    return check_launch("index_rows");
}

int64_t u3d_mask_compact_ws_bytes(int64_t n) {
    if (n <= 0) return 0;
    return (2 * ceil_div(n, RB_T) + 64) * 4;      // block counts + bases
}

int u3d_mask_compact(const uint8_t* mask, int64_t n, int32_t* kept, int32_t* pos, int32_t* n_kept, void* ws, u3d_stream_t stream) {
    if (!mask || !kept || !pos || !n_kept || !ws || n <= 0) {
        set_error("mask_compact: NULL pointer or no rows (n = %lld)", (long long)n);
        return U3D_EINVAL;
    }
    if (n >= 0x80000000LL) { set_error("mask_compact: %lld rows exceed 32-bit row numbers", (long long)n); return U3D_EUNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    const int nblk = (int)ceil_div(n, RB_T);
    int32_t* bc = (int32_t*)ws;
    int32_t* bb = bc + nblk;
    hipLaunchKernelGGL(mask_count_k, dim3(nblk), dim3(RB_T), 0, s, mask, n, bc);
    hipLaunchKernelGGL(rb_scan_k, dim3(1), dim3(RB_T), 0, s, (const int32_t*)bc, nblk, bb, n_kept);
    hipLaunchKernelGGL(mask_write_k, dim3(nblk), dim3(RB_T), 0, s, mask, n, (const int32_t*)bb, kept, pos);
    return check_launch("mask_compact");
}

int u3d_rows_take(const float* x, const int32_t* rows, int64_t n_out, int64_t n_src, int C, float* y, u3d_stream_t stream) {
    const int rc = check_rows("rows_take", !x || !rows || !y, n_out, n_src, 0, C);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_POOL, s, 0.0);
    const int lg = lanes_log2(C);
    const int64_t G = ceil_div(n_out, ROWS);
    hipLaunchKernelGGL(rows_take_k, dim3((unsigned)ceil_div(G << lg, 256)), dim3(256), 0, s, reinterpret_cast<const uint4*>(x), rows, n_out, n_src,
                       G, C / 4, lg, reinterpret_cast<uint4*>(y));
    return check_launch("rows_take");
}

int u3d_rows_take2(const float* a, const int32_t* rows_a, int64_t n_a, const float* b, const int32_t* rows_b, int64_t n_b, int64_t n_out, int C,
                   float* y, u3d_stream_t stream) {
    const int rc = check_rows("rows_take2", !a || !rows_a || !b || !rows_b || !y, n_out, n_a, n_b, C);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_POOL, s, 0.0);
    const int lg = lanes_log2(C);
    const int64_t G = ceil_div(n_out, ROWS);
    hipLaunchKernelGGL(rows_take2_k, dim3((unsigned)ceil_div(G << lg, 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(a), rows_a, n_a,
                       reinterpret_cast<const float4*>(b), rows_b, n_b, n_out, G, C / 4, lg, reinterpret_cast<float4*>(y));
    return check_launch("rows_take2");
}

}  // extern "C"
