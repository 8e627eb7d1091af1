// K-tgt: the distance targets of every `target_by_distance` scene of a batch (unidet3d/unidet3d.py:371-409, get_targets) in two launches.
//   d(s, g)  = ((cx - px)^2 + (cy - py)^2) + (cz - pz)^2 in fp32, in this order (this file is built with -ffp-contract=off)
//   kth[g]   = the min(topk + 1, S_b)-th smallest d(., g) over the scene's superpoints           -- phase 1, one workgroup per (scene, box)
//   mask[g, s] = g is the box with the smallest d(s, g) among those with d(s, g) < kth[g] (strictly; lowest g on ties; none if there
//              is no such box or the distance reaches the reference's 1e8 "no box" value)         -- phase 2, one thread per superpoint
// Phase 1 never sorts a scene: every lane keeps the 16 smallest distances of its strided share in registers (a compare-exchange
// chain per element), then the workgroup pops the global minimum topk + 1 times -- a DPP / swizzle min inside each wave, four values
// through LDS across the waves, and the lane that owns the minimum shifts its list.  Distances are non-negative, so their bit
// patterns order like the values and the reduction runs on unsigned integers.  Phase 2 writes the whole [G_b, S_b] block of its scene,
// zeros included: the output needs no memset.  No atomics; the result does not depend on scheduling.
#include "u3d_common.h"

namespace u3d {

constexpr int TGT_K = 16;                 // list length per lane: topk + 1 <= 16
constexpr unsigned TGT_SENT = 0xffffffffu;
constexpr int TGT_TILE = 64;              // boxes per LDS tile of phase 2
constexpr float TGT_FLOAT_MAX = 1e8f;     // the reference's float_max

template <int CTRL>
__device__ __forceinline__ unsigned tgt_dpp(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}

// minimum over the 64 lanes of a wave, the same value in every lane
__device__ __forceinline__ unsigned tgt_wave_min(unsigned v) {
    v = min(v, tgt_dpp<0xB1>(v));                                          // quad_perm [1, 0, 3, 2]
    v = min(v, tgt_dpp<0x4E>(v));                                          // quad_perm [2, 3, 0, 1]
    v = min(v, tgt_dpp<0x124>(v));                                         // row_ror 4
    v = min(v, tgt_dpp<0x128>(v));                                         // row_ror 8: every lane holds its row's minimum
    v = min(v, (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x401F));     // lane ^ 16
    return min((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 32));
}

__device__ __forceinline__ float tgt_dist(float cx, float cy, float cz, float px, float py, float pz) {
    const float dx = cx - px, dy = cy - py, dz = cz - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(256) void tgt_kth_k(const float* __restrict__ centers, int64_t n_sp, const int64_t* __restrict__ sp_off,
                                                 const float* __restrict__ boxc, int64_t box_ld, int64_t n_boxes,
                                                 const int64_t* __restrict__ box_off, int topk, float* __restrict__ kth) {
    __shared__ unsigned wmin[2][4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g0 = box_off[b], G = box_off[b + 1] - g0;
    if ((int64_t)blockIdx.x >= G) return;                                   // (every exit up to the loop is uniform over the workgroup)
    const int64_t g = g0 + blockIdx.x;
    const int64_t s0 = sp_off[b], S = sp_off[b + 1] - s0;
    if (g0 < 0 || g >= n_boxes || s0 < 0 || S < 0 || s0 + S > n_sp) return;
    if (S == 0) { if (threadIdx.x == 0) kth[g] = 0.f; return; }
    const int K = (int64_t)(topk + 1) < S ? topk + 1 : (int)S;
    const float cx = boxc[g * box_ld], cy = boxc[g * box_ld + 1], cz = boxc[g * box_ld + 2];
    unsigned a[TGT_K];
#pragma unroll
    for (int j = 0; j < TGT_K; ++j) a[j] = TGT_SENT;
    for (int64_t l = threadIdx.x; l < S; l += 256) {
        const float* p = centers + (s0 + l) * 3;
        unsigned v = __float_as_uint(tgt_dist(cx, cy, cz, p[0], p[1], p[2]));
#pragma unroll
        for (int j = 0; j < TGT_K; ++j) {                                   // a stays ascending, v carries the displaced value on
            const unsigned lo = min(a[j], v);
            v = max(a[j], v);
            a[j] = lo;
        }
    }
    unsigned m = 0;
    for (int r = 0; r < K; ++r) {
        const unsigned wm = tgt_wave_min(a[0]);
        if (lane == 0) wmin[r & 1][w] = wm;
        __syncthreads();                                                    // (the other buffer is still being read by slower waves)
        const unsigned w0 = wmin[r & 1][0], w1 = wmin[r & 1][1], w2 = wmin[r & 1][2], w3 = wmin[r & 1][3];
        m = min(min(w0, w1), min(w2, w3));
        const int owner = w0 == m ? 0 : (w1 == m ? 1 : (w2 == m ? 2 : 3));
        if (w == owner) {
            const unsigned long long bal = __ballot(a[0] == m);
            if (lane == __ffsll((long long)bal) - 1) {                      // one element leaves per round: equal values count one by one
#pragma unroll
                for (int j = 0; j + 1 < TGT_K; ++j) a[j] = a[j + 1];
                a[TGT_K - 1] = TGT_SENT;
            }
        }
    }
    if (threadIdx.x == 0) kth[g] = __uint_as_float(m);
}

__global__ __launch_bounds__(256) void tgt_assign_k(const float* __restrict__ centers, int64_t n_sp, const int64_t* __restrict__ sp_off,
                                                    const float* __restrict__ boxc, int64_t box_ld, int64_t n_boxes,
                                                    const int64_t* __restrict__ box_off, const int64_t* __restrict__ mask_off,
                                                    int64_t mask_entries, const float* __restrict__ kth, uint8_t* __restrict__ out) {
    __shared__ float4 tile[TGT_TILE];
    const int b = blockIdx.y;
    const int64_t s0 = sp_off[b], S = sp_off[b + 1] - s0;
    const int64_t g0 = box_off[b], G = box_off[b + 1] - g0;
    const int64_t m0 = mask_off[b], m1 = mask_off[b + 1];
    const int64_t start = (int64_t)blockIdx.x * 256;
    if (start >= S || G <= 0) return;                                       // uniform, like the range checks below
    if (s0 < 0 || s0 + S > n_sp || g0 < 0 || g0 + G > n_boxes || m0 < 0 || m1 > mask_entries || m1 - m0 < G * S) return;
    const int64_t l = start + threadIdx.x;
    const bool active = l < S;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (active) { const float* p = centers + (s0 + l) * 3; px = p[0]; py = p[1]; pz = p[2]; }
    float bd = TGT_FLOAT_MAX;
    int64_t best = -1;
    for (int64_t t0 = 0; t0 < G; t0 += TGT_TILE) {
        __syncthreads();
        if (threadIdx.x < TGT_TILE && t0 + threadIdx.x < G) {
            const int64_t gg = g0 + t0 + threadIdx.x;
            tile[threadIdx.x] = make_float4(boxc[gg * box_ld], boxc[gg * box_ld + 1], boxc[gg * box_ld + 2], kth[gg]);
        }
        __syncthreads();
        const int nt = G - t0 < TGT_TILE ? (int)(G - t0) : TGT_TILE;
        for (int j = 0; j < nt; ++j) {
            const float4 c = tile[j];
            const float d = tgt_dist(c.x, c.y, c.z, px, py, pz);
            if (d < c.w && d < bd) { bd = d; best = t0 + j; }               // strictly closer: the lowest box index wins a tie
        }
    }
    if (active)
        for (int64_t g = 0; g < G; ++g) out[m0 + g * S + l] = g == best ? 1 : 0;
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int64_t u3d_targets_by_distance_ws_bytes(int64_t n_boxes) { return n_boxes < 0 ? -1 : (n_boxes * 4 + 255) / 256 * 256; }

int u3d_targets_by_distance(const float* centers, int64_t n_sp, const int64_t* sp_offsets, const float* box_centers, int64_t box_ld,
                            int64_t n_boxes, const int64_t* box_offsets, const int64_t* mask_offsets, int64_t mask_entries, int B,
                            int64_t max_boxes, int64_t max_sp, int topk, uint8_t* masks, void* ws, u3d_stream_t stream) {
    if (B < 0 || n_sp < 0 || n_boxes < 0 || mask_entries < 0 || max_boxes < 0 || max_sp < 0 || topk < 0) return U3D_EINVAL;
    if (topk + 1 > TGT_K) { set_error("targets_by_distance: topk + 1 = %d exceeds %d", topk + 1, TGT_K); return U3D_EUNSUPPORTED; }
    if (B == 0 || max_boxes == 0 || max_sp == 0 || mask_entries == 0) return U3D_OK;      // every block is [0, S] or [G, 0]
    if (!centers || !sp_offsets || !box_centers || !box_offsets || !mask_offsets || !masks || !ws || box_ld < 3) return U3D_EINVAL;
    if (B > 65535 || max_boxes > 0x7fffffff || ceil_div(max_sp, 256) > 0x7fffffff) { set_error("targets_by_distance: batch too large"); return U3D_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    float* kth = static_cast<float*>(ws);
    hipLaunchKernelGGL(tgt_kth_k, dim3((unsigned)max_boxes, B), dim3(256), 0, s, centers, n_sp, sp_offsets, box_centers, box_ld, n_boxes, box_offsets,
                       topk, kth);
    hipLaunchKernelGGL(tgt_assign_k, dim3((unsigned)ceil_div(max_sp, 256), B), dim3(256), 0, s, centers, n_sp, sp_offsets, box_centers, box_ld,
                       n_boxes, box_offsets, mask_offsets, mask_entries, kth, masks);
    return check_launch("targets_by_distance");
}

}  // extern "C"
