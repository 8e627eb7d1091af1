// Shared by the attention kernels of attn.hip (native fp32 MFMA) and attn_x3.hip (bf16 planes): the work decode, the delta
// kernel of the backward pass, and the host bodies behind the u3d_attn_varlen_* entry points (with and without dropout).
#pragma once
#include "dropout.h"
#include "u3d_common.h"

namespace u3d {

// 1-D launch decode: workgroup b runs on XCD b % 8 (private L2).  XCD x takes the (scene, head) pairs x, x+8, ...
// and all their tiles (64 rows; attn_x3.hip: 16 rows per wave of the workgroup, attn_tiles) back to back, so the K/V (or Q/dO) rows of one (scene, head) stay in that XCD's
// L2 while its tiles stream them (PMC before: 321 MB fetched per forward launch for 49 MB of qkv).
struct AttnWork { int b, h, tile; };
__device__ __forceinline__ AttnWork attn_decode(int H, int B, int n_tiles) {
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int hb = (j / n_tiles) * 8 + x;
    AttnWork w;
    w.tile = j % n_tiles;
    w.h = hb % H;
    w.b = hb / H;          // >= B for the padding workgroups of the last group
    return w;
}
static inline int attn_tiles(int max_len, int tile_rows) { return (max_len + tile_rows - 1) / tile_rows; }
static inline unsigned attn_grid(int H, int B, int n_tiles) { return (unsigned)(((H * B + 7) / 8) * 8 * n_tiles); }

// delta[h][i] = sum_d dO[i][h*HD+d] * O[i][h*HD+d]; T = float, or __bf16 for bf16 tensors (products and sum in fp32)
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_delta_k(const T* __restrict__ o, const T* __restrict__ dout, int64_t n, int H, float* delta) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * H) return;
    const int64_t i = idx / H;
    const int h = (int)(idx % H);
    float s = 0.f;
    if constexpr (sizeof(T) == 4) {
        const float4* a = reinterpret_cast<const float4*>(o + i * H * HD + h * HD);
        const float4* b = reinterpret_cast<const float4*>(dout + i * H * HD + h * HD);
#pragma unroll
        for (int j = 0; j < HD / 4; ++j) {
            const float4 x = a[j], y = b[j];
            s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
        }
    } else {
        const u32x4* a = reinterpret_cast<const u32x4*>(o + i * H * HD + h * HD);
        const u32x4* b = reinterpret_cast<const u32x4*>(dout + i * H * HD + h * HD);
#pragma unroll
        for (int j = 0; j < HD / 8; ++j) {
            const u32x4 x = a[j], y = b[j];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                s += bf16_bits_to_f32((unsigned short)x[c]) * bf16_bits_to_f32((unsigned short)y[c]) +
                     __builtin_bit_cast(float, x[c] & 0xffff0000u) * __builtin_bit_cast(float, y[c] & 0xffff0000u);
        }
    }
    delta[(int64_t)h * n + i] = s;
}

// what the tensors of a call hold and which kernels run it
enum AttnMode {
    ATTN_NATIVE,        // fp32 tensors, fp32 MFMA (attn.hip; U3D_FP32_MATH=mfma)
    ATTN_X3,            // fp32 tensors, three bf16 planes per operand (the default)
    ATTN_BF16_OPS,      // fp32 tensors, one bf16 plane per operand
    ATTN_B16,           // bf16 tensors (qkv / out / dout / dqkv), one plane
};

// attn_x3.hip: the plane kernels of every mode but ATTN_NATIVE, hd 32 or 64 (the backward launcher expects delta_ws filled);
// `dr` non-null: the DROP = true instantiations with that key (csrc/dropout.h)
void attn_fwd_x3_launch(AttnMode mode, const void* qkv, const int32_t* cu, int B, int max_len, int64_t n_total, int H, int hd, float scale, void* out,
                        float* lse, hipStream_t s, const DropArgs* dr = nullptr);
void attn_bwd_x3_launch(AttnMode mode, const void* qkv, const void* dout, const float* lse, const int32_t* cu, int B, int max_len,
                        int64_t n_total, int H, int hd, float scale, void* dqkv, const float* delta, hipStream_t s, const DropArgs* dr = nullptr);

// attn.hip: the bodies of the u3d_attn_varlen_{fwd,bwd}{,_bf16,_b16} entry points -- validation, timing scope, dispatch, launch check
int attn_fwd(AttnMode mode, const void* qkv, const int32_t* cu, int B, int max_len, int64_t n_total, int H, int hd, float scale, void* out,
             float* lse, double flops_hint, u3d_stream_t stream, const DropArgs* dr = nullptr);
int attn_bwd(AttnMode mode, const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* cu, int B, int max_len,
             int64_t n_total, int H, int hd, float scale, void* dqkv, float* delta_ws, double flops_hint, u3d_stream_t stream, const DropArgs* dr = nullptr);
// the bodies of the u3d_attn_varlen_{fwd,bwd}_drop{,_bf16,_b16} entry points: p outside [0, 1) is U3D_EINVAL, ATTN_NATIVE with p > 0
// U3D_EUNSUPPORTED, both before the first HIP call; p == 0 is the call without dropout
int attn_fwd_drop(AttnMode mode, const void* qkv, const int32_t* cu, int B, int max_len, int64_t n_total, int H, int hd, float scale, void* out,
                  float* lse, double flops_hint, u3d_stream_t stream, double p, uint64_t seed, uint64_t offset);
int attn_bwd_drop(AttnMode mode, const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* cu, int B, int max_len,
                  int64_t n_total, int H, int hd, float scale, void* dqkv, float* delta_ws, double flops_hint, u3d_stream_t stream, double p,
                  uint64_t seed, uint64_t offset);

}  // namespace u3d
