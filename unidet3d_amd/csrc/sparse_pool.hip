// Sparse max / average pooling over a convolution rulebook (spconv's SparseMaxPool3d / SparseAvgPool3d; include/u3d.h section P1).
// Gather form on a DESTINATION-MAJOR view of the pair lists: table[row][k] = the row paired with `row` at offset k, or -1
// (u3d_pair_table).  A group of lanes owns one destination row and a 16-byte column slice, walks the K entries of its row in ascending
// offset order, loads the present rows only (16-byte loads, four entries in flight) and writes every destination element exactly once:
// no atomics, no memset of the destination, one summation order.  Narrow rows share a wave (64 / lanes-per-row rows), rows wider
// than a wave's 256 columns take a column loop.  No LDS: nothing is reused inside a workgroup.
#include "u3d_common.h"

// every product and every sum of this file rounds on its own (the effect of -ffp-contract=off, said here so that the file carries it
// whatever its command line): dy * (1 / count) + acc must not become one fused operation
#pragma clang fp contract(off)

namespace u3d {

__global__ __launch_bounds__(256) void pair_table_k(const int32_t* __restrict__ key, const int32_t* __restrict__ val,
                                                    const int32_t* __restrict__ counts, int K, int64_t cap, int64_t n,
                                                    int32_t* __restrict__ table) {
    const int k = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || i >= counts[k]) return;
    const int r = key[k * cap + i];
    if ((uint64_t)r < (uint64_t)n) table[(int64_t)r * K + k] = val[k * cap + i];      // (for a fixed k no row repeats: race-free)
}

constexpr int ENTRIES = 4;      // table entries (= row loads) of one group in flight

// the selection rule of the maximum: the held element gives way only to a strictly larger one, or to a NaN while it is none itself
__device__ __forceinline__ void take_max(float& h, unsigned& a, float v, unsigned k, bool first) {
    const bool rep = first || v > h || (v != v && h == h);
    h = rep ? v : h;
    a = rep ? k : a;
}

// lg = log2(lanes per row); thread t of the grid serves row t >> lg, columns 4 (t & (lanes - 1)) + 256 i
template <int MODE>
__global__ __launch_bounds__(256) void sparse_pool_fwd_k(const float* __restrict__ x, const int32_t* __restrict__ table, int64_t n_out, int K,
                                                         int C, int lg, float* __restrict__ y, uint8_t* __restrict__ arg,
                                                         int32_t* __restrict__ count) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j = t >> lg;
    const int c0 = (int)(t & ((1 << lg) - 1)) * 4;
    if (j >= n_out) return;
    const int32_t* tj = table + j * K;
    for (int c = c0; c < C; c += 4 << lg) {
        float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
        unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        int m = 0;
        for (int k0 = 0; k0 < K; k0 += ENTRIES) {
            int r[ENTRIES];
            float4 v[ENTRIES];
#pragma unroll
            for (int u = 0; u < ENTRIES; ++u) r[u] = k0 + u < K ? tj[k0 + u] : -1;
#pragma unroll
            for (int u = 0; u < ENTRIES; ++u) {
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r[u] >= 0) v[u] = *reinterpret_cast<const float4*>(x + (int64_t)r[u] * C + c);
            }
#pragma unroll
            for (int u = 0; u < ENTRIES; ++u) {
                if (r[u] < 0) continue;
                if (MODE == U3D_POOL_MAX) {
                    const unsigned k = k0 + u;
                    take_max(h.x, a0, v[u].x, k, m == 0); take_max(h.y, a1, v[u].y, k, m == 0);
                    take_max(h.z, a2, v[u].z, k, m == 0); take_max(h.w, a3, v[u].w, k, m == 0);
                } else {
                    h.x += v[u].x; h.y += v[u].y; h.z += v[u].z; h.w += v[u].w;
                }
                ++m;
            }
        }
        if (MODE == U3D_POOL_MAX) {
            *reinterpret_cast<unsigned*>(arg + j * C + c) = a0 | a1 << 8 | a2 << 16 | a3 << 24;
        } else {
            const float d = (float)(m > 0 ? m : 1);
            h.x /= d; h.y /= d; h.z /= d; h.w /= d;
            if (c == 0) count[j] = m;
        }
        *reinterpret_cast<float4*>(y + j * C + c) = h;
    }
}

// table: the INPUT row's outputs; max: dx = the dy of the outputs that selected this row's element, avg: dy / count of every output
template <int MODE>
__global__ __launch_bounds__(256) void sparse_pool_bwd_k(const float* __restrict__ dy, const int32_t* __restrict__ table, int64_t n_in, int K,
                                                         int C, int lg, const uint8_t* __restrict__ arg, const int32_t* __restrict__ count,
                                                         float* __restrict__ dx) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t >> lg;
    const int c0 = (int)(t & ((1 << lg) - 1)) * 4;
    if (i >= n_in) return;
    const int32_t* ti = table + i * K;
    for (int c = c0; c < C; c += 4 << lg) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        bool s0 = false, s1 = false, s2 = false, s3 = false;      // a first term is taken as it is: the sum of one term has its bits
        for (int k0 = 0; k0 < K; k0 += ENTRIES) {
            int r[ENTRIES];
            float4 g[ENTRIES];
            unsigned w[ENTRIES];          // max: the four selected offsets; avg: the pair count of the output row
#pragma unroll
            for (int u = 0; u < ENTRIES; ++u) r[u] = k0 + u < K ? ti[k0 + u] : -1;
#pragma unroll
            for (int u = 0; u < ENTRIES; ++u) {
                g[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                w[u] = 0;
                if (r[u] >= 0) {
                    g[u] = *reinterpret_cast<const float4*>(dy + (int64_t)r[u] * C + c);
                    w[u] = MODE == U3D_POOL_MAX ? *reinterpret_cast<const unsigned*>(arg + (int64_t)r[u] * C + c) : (unsigned)count[r[u]];
                }
            }
#pragma unroll
            for (int u = 0; u < ENTRIES; ++u) {
                if (r[u] < 0) continue;
                const unsigned k = k0 + u;
                bool p0 = true, p1 = true, p2 = true, p3 = true;
                float4 q = g[u];
                if (MODE == U3D_POOL_MAX) {
                    p0 = (w[u] & 255u) == k; p1 = (w[u] >> 8 & 255u) == k; p2 = (w[u] >> 16 & 255u) == k; p3 = (w[u] >> 24) == k;
                } else {
                    const float inv = 1.0f / (float)(w[u] > 0u ? w[u] : 1u);
                    q.x *= inv; q.y *= inv; q.z *= inv; q.w *= inv;
                }
                if (p0) { acc.x = s0 ? acc.x + q.x : q.x; s0 = true; }
                if (p1) { acc.y = s1 ? acc.y + q.y : q.y; s1 = true; }
                if (p2) { acc.z = s2 ? acc.z + q.z : q.z; s2 = true; }
                if (p3) { acc.w = s3 ? acc.w + q.w : q.w; s3 = true; }
            }
        }
        *reinterpret_cast<float4*>(dx + i * C + c) = acc;
    }
}

// lanes per row: the power of two that covers C / 4, one wave at most
static int lanes_log2(int C) {
    int lg = 0;
    while (lg < 6 && (4 << lg) < C) ++lg;
    return lg;
}

// the contract both directions share, checked before any HIP call
static int check_pool(const char* what, const void* a, const void* table, const void* out, const void* aux, int64_t n, int K, int C, int mode) {
    if (!a || !table || !out || !aux || n <= 0) { set_error("%s: NULL pointer or no rows (n = %lld)", what, (long long)n); return U3D_EINVAL; }
    if (mode != U3D_POOL_MAX && mode != U3D_POOL_AVG) { set_error("%s: mode %d is neither U3D_POOL_MAX nor U3D_POOL_AVG", what, mode); return U3D_EINVAL; }
    if (K < 1 || K > 27) { set_error("%s: K = %d offsets unsupported (1..27)", what, K); return U3D_EUNSUPPORTED; }
    if (C < 4 || C > 512 || C % 4) { set_error("%s: width %d unsupported (a multiple of 4 in 4..512)", what, C); return U3D_EUNSUPPORTED; }
    if (n * (int64_t)(C > K ? C : K) > 0x7fffffffLL) {
        set_error("%s: %lld rows of %d channels / %d offsets exceed 32-bit element addressing", what, (long long)n, C, K);
        return U3D_EUNSUPPORTED;
    }
    return U3D_OK;
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int u3d_pair_table(const int32_t* pair_key, const int32_t* pair_val, const int32_t* counts, int K, int64_t cap, int64_t n, int32_t* table,
                   u3d_stream_t stream) {
    if (!pair_key || !pair_val || !counts || !table || n <= 0 || cap <= 0) {
        set_error("pair_table: NULL pointer, no rows (n = %lld) or no list capacity (cap = %lld)", (long long)n, (long long)cap);
        return U3D_EINVAL;
    }
    if (K < 1 || K > 27) { set_error("pair_table: K = %d offsets unsupported (1..27)", K); return U3D_EUNSUPPORTED; }
    if (n * K > 0x7fffffffLL || cap > 0x7fffffffLL) {
        set_error("pair_table: %lld rows x %d offsets (cap %lld) exceed 32-bit element addressing", (long long)n, K, (long long)cap);
        return U3D_EUNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    if (hipMemsetAsync(table, 0xff, (size_t)n * K * sizeof(int32_t), s) != hipSuccess) return check_launch("pair_table (fill)");
    hipLaunchKernelGGL(pair_table_k, dim3((unsigned)ceil_div(cap, 256), (unsigned)K), dim3(256), 0, s, pair_key, pair_val, counts, K, cap, n, table);
    return check_launch("pair_table");
}

int u3d_sparse_pool_fwd(const float* x, const int32_t* table_out, int64_t n_out, int K, int C, int mode, float* y, uint8_t* arg,
                        int32_t* count, u3d_stream_t stream) {
    const int rc = check_pool("sparse_pool_fwd", x, table_out, y, mode == U3D_POOL_AVG ? (const void*)count : (const void*)arg, n_out, K, C, mode);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_POOL, s, 0.0);
    const int lg = lanes_log2(C);
    const dim3 grid((unsigned)ceil_div(n_out << lg, 256));
    if (mode == U3D_POOL_MAX)
        hipLaunchKernelGGL((sparse_pool_fwd_k<U3D_POOL_MAX>), grid, dim3(256), 0, s, x, table_out, n_out, K, C, lg, y, arg, count);
    else
        hipLaunchKernelGGL((sparse_pool_fwd_k<U3D_POOL_AVG>), grid, dim3(256), 0, s, x, table_out, n_out, K, C, lg, y, arg, count);
    return check_launch("sparse_pool_fwd");
}

int u3d_sparse_pool_bwd(const float* dy, const int32_t* table_in, int64_t n_in, int K, int C, int mode, const uint8_t* arg,
                        const int32_t* count, float* dx, u3d_stream_t stream) {
    const int rc = check_pool("sparse_pool_bwd", dy, table_in, dx, mode == U3D_POOL_AVG ? (const void*)count : (const void*)arg, n_in, K, C, mode);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_POOL, s, 0.0);
    const int lg = lanes_log2(C);
    const dim3 grid((unsigned)ceil_div(n_in << lg, 256));
    if (mode == U3D_POOL_MAX)
        hipLaunchKernelGGL((sparse_pool_bwd_k<U3D_POOL_MAX>), grid, dim3(256), 0, s, dy, table_in, n_in, K, C, lg, arg, count, dx);
    else
        hipLaunchKernelGGL((sparse_pool_bwd_k<U3D_POOL_AVG>), grid, dim3(256), 0, s, dy, table_in, n_in, K, C, lg, arg, count, dx);
    return check_launch("sparse_pool_bwd");
}

}  // extern "C"
