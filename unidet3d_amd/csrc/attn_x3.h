// Shared by the plane kernels of attn_x3.hip (head_dim 32) and attn_x3_hd64.h (head_dim 64): the MFMA wrapper, the running-sum
// product with its separate low-order accumulators, the plane split of rows and of C fragments, and the launchers of the 64-wide forms.
#pragma once
#include "attn_common.h"

namespace u3d {

constexpr float X_LOG2E = 1.44269504088896340736f, X_LN2 = 0.69314718055994530942f;
#define U3D_MFMA_X(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

// c += a . b with both operands in three planes takes h.l, m.m, l.h, h.m, m.h, h.h (smallest terms first).
// A bf16 MFMA truncates its 32 products at the exponent of its C operand, always towards zero: plane products 2^-8 .. 2^-16 below
// a running sum lose their low bits every time -- a coherent bias (tools/bias_probe.py: -1.2e-8 mean error after 8 blocks, zero
// for fp32 MFMAs) that reductions over thousands of rows downstream do not average out.  So chains that start from zero (S, dP)
// run smallest terms first, and the running sums O / dQ / dK / dV keep the low-order products in accumulators of their own.
//
// running sums: the h.h product goes to (c0, c1), the five low-order plane products to their own accumulators (l0, l1), joined
// once at the end of the kernel (NP = 1, bf16 operands: the one product goes to (c0, c1))
template <int NP>
__device__ __forceinline__ void mfma_x3_2b(const bf16x8 (&a)[NP], const bf16x8 (&b0)[NP], const bf16x8 (&b1)[NP], f32x4& c0, f32x4& c1,
                                           f32x4& l0, f32x4& l1) {
#pragma unroll
    for (int o = NP - 1; o >= 1; --o)
#pragma unroll
        for (int qa = 0; qa <= o; ++qa) {
            l0 = U3D_MFMA_X(a[qa], b0[o - qa], l0);
            l1 = U3D_MFMA_X(a[qa], b1[o - qa], l1);
        }
    c0 = U3D_MFMA_X(a[0], b0[0], c0);
    c1 = U3D_MFMA_X(a[0], b1[0], c1);
}

// NP planes of a pair / of eight values: NP = 3 the exact split (u3d_common.h), NP = 1 one bf16 value rounded to nearest even
// (bf16 operands, BASELINE configs[2])
template <int NP>
__device__ __forceinline__ void planes_pair(float a, float b, unsigned (&w)[NP]) {
    if constexpr (NP == 3) split3_pair(a, b, w[0], w[1], w[2]);
    else w[0] = pack_bf16(a, b);
}
template <int NP>
__device__ __forceinline__ void planes_x8(const f32x4& lo, const f32x4& hi, bf16x8 (&out)[NP]) {
    if constexpr (NP == 3) split3_x8(lo, hi, out);
    else out[0] = bf16x8{(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3], (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
}

// own row -> B operand of a bf16 tensor: 8 consecutive dims of row `ptr` (nullptr: zeros), the tensor's own values
__device__ __forceinline__ void row_frag_x16(const __bf16* ptr, bf16x8 (&out)[1]) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (ptr) v = *reinterpret_cast<const u32x4*>(ptr);
    out[0] = __builtin_bit_cast(bf16x8, v);
}

// own row -> B operand planes: 8 consecutive dims of row `ptr` (nullptr: zeros), scaled
template <int NP>
__device__ __forceinline__ void row_frag_x3(const float* ptr, float scale, bf16x8 (&out)[NP]) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
    if (ptr) { a = *reinterpret_cast<const f32x4*>(ptr); b = *reinterpret_cast<const f32x4*>(ptr + 4); }
    a *= scale;
    b *= scale;
    planes_x8<NP>(a, b, out);
}

// A operand planes from two C fragments: k = 8g + e <-> row 16 (e >> 2) + 4g + (e & 3) of the 32-row block
template <int NP>
__device__ __forceinline__ void pair_frag_x3(const float (&lo)[4], const float (&hi)[4], bf16x8 (&out)[NP]) {
    planes_x8<NP>(f32x4{lo[0], lo[1], lo[2], lo[3]}, f32x4{hi[0], hi[1], hi[2], hi[3]}, out);
}

// attn_x3_hd64.h: the 64-wide forms behind attn_fwd_x3_launch / attn_bwd_x3_launch (dQ on `sq`, dK / dV on `s`)
void attn_fwd_x3_hd64_launch(AttnMode mode, const void* qkv, const int32_t* cu, int B, int n_tiles, int64_t n_total, int H, float scale, void* out,
                             float* lse, hipStream_t s);
void attn_bwd_x3_hd64_launch(AttnMode mode, const void* qkv, const void* dout, const float* lse, const int32_t* cu, int B, int n_tiles,
                             int64_t n_total, int H, float scale, void* dqkv, const float* delta, hipStream_t sq, hipStream_t s);

}  // namespace u3d
