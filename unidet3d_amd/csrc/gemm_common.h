// The pieces gemm.hip and gemm_b16.hip share, each written once: the tile constants, the fp32 NT epilogue, the host-side plan
// helpers (tile table, split clamp, 32-bit offset guards, grids) and the launchers that cross the two files (the library is linked
// without relocatable device code: a host function crosses the files, a kernel does not).  Internal, not part of the C ABI.
// What is NOT here: the workgroup frames (tile / split decode + descriptors), the accumulator zeroing, the 32 x 32 partial store and
// the column-sum tail of the kernels.  Written as a struct or an inlined function, each of them changed the instruction stream of
// every kernel that used it (tools/isa_compare.py against the text in place: other register allocation, other address arithmetic),
// so the kernels keep that text; for the same reason gemm_nt_b16_k's fp32-result branch repeats nt_epilogue for EPI 0 / 1 / 3 / 5 (its GELU epilogues, new, call it).
#pragma once
#include "u3d_common.h"

namespace u3d {

constexpr int GT = 128;        // macro tile (both dims)
constexpr int GK = 16;         // K-step of the native fp32 kernels
constexpr int GKH = 32;        // K-step of the bf16-MFMA NT kernels (one and three planes)
constexpr int GLH = GKH + 8;   // their padded LDS row (halves): 80-byte rows keep the 16-byte reads of 32 consecutive rows conflict-free
constexpr int TKH = 32;        // rows per stage of the bf16-operand TN kernel
constexpr int TLH = GT + 32;   // its padded LDS row (halves): the four rows a half-wave reads lie on four different 64-byte bank groups

// eight fp32 values rounded to bf16 (RNE)
__device__ __forceinline__ bf16x8 cvt8(const f32x4& lo, const f32x4& hi) {
    return bf16x8{(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3], (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
}

// fp32 epilogue of the NT kernels (EPI: see gemm.hip).  D layout of 32x32 MFMAs (dtype independent): col = lane & 31,
// row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).  The stores go through a bounds-checked descriptor (row offset scalar, column
// offset per lane, out-of-range lanes dropped); rows / columns of `aux` outside the tile read as 0 the same way.
template <int TN, int EPI, int TM = GT>
__device__ __forceinline__ void nt_epilogue(const f32x16 (&acc)[TM / 64][TN / 64], float* __restrict__ C, const float* __restrict__ bias,
                                            const float* __restrict__ aux, float* __restrict__ pre, int64_t m0, int n0, int rows_a, int N,
                                            int wr, int wc, int i32, int kh) {
    constexpr int NB = TN / 64, TA = TM / 64;
    const __amdgpu_buffer_rsrc_t rs_c = make_rsrc(C + m0 * N, (int64_t)rows_a * N * 4);
    const __amdgpu_buffer_rsrc_t rs_x = make_rsrc((EPI == 2 ? (const float*)pre : aux) + (EPI >= 2 ? m0 * N : 0), (int64_t)rows_a * N * 4);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int n = n0 + wc * (TN / 2) + b * 32 + i32;
        const float bv = (bias && n < N) ? bias[n] : 0.f;
        const int vc = n < N ? (4 * kh * N + n) * 4 : 0x7fffffff;        // columns past N: dropped by the bounds check
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wr * (TM / 2) + a * 32 + (r & 3) + 8 * (r >> 2);
                float v = acc[a][b][r] + bv;
                if constexpr (EPI == 1) v = fmaxf(v, 0.f);
                if constexpr (EPI == 2) {
                    float h = v;
                    asm volatile("" : "+v"(h));
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, h), rs_x, vc, row * N * 4, 0);
                    v = gelu_f(v);
                }
                if constexpr (EPI == 3 || EPI == 4 || EPI == 5) {
                    const float x = __builtin_bit_cast(float, bload32(rs_x, vc, row * N * 4));
                    v = EPI == 3 ? (x > 0.f ? v : 0.f) : (EPI == 4 ? v * gelu_grad_f(x) : v + x);
                }
                // the element goes through an opaque VGPR copy: handed a vector element directly, this compiler's buffer-store
                // builtin stores element 0 of the accumulator sixteen times (seen in the ISA, caught by the parity test)
                asm volatile("" : "+v"(v));
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs_c, vc, row * N * 4, 0);
            }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// the three NT tiles, largest first
constexpr int NT_TM[3] = {128, 128, 64}, NT_TN[3] = {128, 64, 64};
inline dim3 nt_grid(int64_t M, int N, int tile) { return dim3((unsigned)(ceil_div(M, NT_TM[tile]) * ceil_div(N, NT_TN[tile]))); }
// an NT kernel forms its tile offsets in 32 bits
inline bool nt_offsets_ok(const char* who, int N, int K) {
    if ((int64_t)GT * K * 4 < 0x7fffffffLL && (int64_t)GT * N * 4 < 0x7fffffffLL) return true;
    set_error("%s: N=%d / K=%d too large for 32-bit tile offsets", who, N, K);
    return false;
}
// row splits of a TN product: `wanted`, at least 4 trips of `trip` rows each, 1 .. 256
inline int tn_clamp_splits(int64_t wanted, int64_t M, int trip) {
    const int64_t max_s = ceil_div(M, 4 * trip);
    if (wanted > max_s) wanted = max_s;
    return (int)(wanted < 1 ? 1 : (wanted > 256 ? 256 : wanted));
}
// a TN kernel forms its offsets inside a split in 32 bits (two 32-row trips of look-ahead past the split's rows)
inline bool tn_offsets_ok(const char* who, int64_t M, int N, int K, int64_t rows_per_split) {
    const int64_t r = rows_per_split + 2 * TKH;
    if (r * N * 4 < 0x7fffffffLL && r * K * 4 < 0x7fffffffLL && (int64_t)N * K * 4 < 0x7fffffffLL) return true;
    set_error("%s: M=%lld N=%d K=%d too large for 32-bit split offsets", who, (long long)M, N, K);
    return false;
}
// 1-D grid of the TN kernels, padded to whole groups of 8 splits (a workgroup whose split is >= S returns)
inline unsigned tn_grid(int S, int N, int K, int ta, int tb) { return (unsigned)(ceil_div(S, 8) * 8 * ceil_div(N, ta) * ceil_div(K, tb)); }
// What a launch does, decided in ONE host function per dispatcher (gemm.hip nt_plan / tn_plan, gemm_b16.hip nt16_plan / tn16_plan)
// that the launch path and the u3d_gemm_*_plan queries both call: kernel family (U3D_GEMM_* of include/u3d.h), tile, row splits.
struct NtPlan { int kernel, tile; };                                  // tile: index into NT_TM / NT_TN
struct TnPlan { int kernel, ta, tb, splits; int64_t rows_per_split; };  // ta x tb: output rows (columns of A) x output columns (columns of B)
// C [N*K] (and colsum [N], nullable) = the S blocks of `ws` summed in a fixed order (gemm.hip)
void launch_tn_reduce(const float* ws, int S, int N, int K, float* C, float* colsum, hipStream_t s);
// gemm_b16.hip's gemm_nt_b16_k<.., A16 = false, C16 = false> on tile `tile` of the table above, for gemm.hip's U3D_BF16_OPERANDS route
// (every instantiation of that kernel stays in its file): epi 0 .. 5; `pre` is written by epi 2, `aux` read by epi 3 .. 5
void launch_nt_b16_f32(int epi, int tile, const float* A, const float* W, const float* bias, float* C, int64_t M, int N, int K, const float* aux,
                       float* pre, hipStream_t s);

}  // namespace u3d
