// Channel-blocked weight gradient of the sparse convolutions for the layer shapes spconv_wgrad_k (spconv.hip) has no instantiation
// for: any Cs in {16} u {32, 64, ..., 512}, Cd in {32, 64, ..., 512}.
//   dW_k[n][c] = sum_p dy[rows_dy[k][p]][n] * x[rows_x[k][p]][c]
// spconv_wgrad_k keeps the whole Cd x Cs block of an offset in the accumulators of one workgroup (at most 128 16x16 blocks); here a
// WAVE owns one (Cd-block, Cs-block) of one offset and one row range, BD x BS channels with BD, BS in {64, 32} (BS = 16 for the
// 16-channel input convolution): at most 16 accumulator blocks, so 320 x 320 is 25 waves per (offset, range) instead of one
// impossible workgroup.  The walk itself is spconv_wgrad_k's: the pair index is the MFMA reduction dimension (16 pairs per trip of
// four v_mfma_f32_16x16x4_f32, or 32 pairs per v_mfma_f32_16x16x32_bf16 with the row parts rounded to bf16 as the operands are
// formed), channel blocks are strided inside the wave's block (lane i16 reads the NGW / NXW consecutive floats at block + N * i16 of
// its pair's row, so a load instruction fetches whole contiguous row pieces), rows are read with their TRUE stride (Cd, Cs are
// run-time values), no LDS, no barrier.
// Waves are numbered (range, offset, block) with the block fastest and the numbering is laid over the XCDs in contiguous chunks
// (xcd_swizzle): the waves that re-read the rows of a range for its other channel blocks and offsets run on the same L2.
// Partials are NATURAL-order blocks partial[k][range][co][ci] (the buffer u3d_spconv_wgrad_ws_bytes sizes: K * ranges * Cd * Cs
// floats); wgrad_blk_reduce_k adds the ranges in a fixed order into dW[co][k][ci].  No floating-point atomics anywhere: the result
// is bit-reproducible from run to run.
#include "u3d_common.h"
#include "spconv_gmm.h"

namespace u3d {

// index of the partial block of (offset k, row range) in the workspace
__host__ __device__ inline int64_t item_offset(int k, int range, int n_tiles) { return (int64_t)k * n_tiles + range; }

// N consecutive floats of a row at byte offset voff (16-byte loads where the piece is a multiple of 16 bytes, dwords otherwise)
template <int N>
__device__ __forceinline__ void blk_row_part(float (&v)[N], __amdgpu_buffer_rsrc_t r, int voff) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int s = 0; s < N; s += 4) {
            const f32x4 t = bload128(r, voff + s * 4, 0);
            v[s] = t[0]; v[s + 1] = t[1]; v[s + 2] = t[2]; v[s + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int s = 0; s < N; ++s) v[s] = __builtin_bit_cast(float, bload32(r, voff + s * 4, 0));
    }
}

// NGW / NXW: 16-channel groups of the wave's dy / x block (block = 16 NGW x 16 NXW channels)
template <int NGW, int NXW, bool BF>
__global__ __launch_bounds__(256) void spconv_wgrad_blk_k(WgBlkParams p) {
    const int tid = threadIdx.x, lane = tid & 63, i16 = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: range bounds and block offsets stay in SGPRs
    const int nbs = p.Cs / (16 * NXW), nblk = (p.Cd / (16 * NGW)) * nbs;
    const int64_t wid = xcd_swizzle(blockIdx.x, gridDim.x) * 4 + wave;
    const int64_t item = wid / nblk;                                // (range, offset)
    const int blk = (int)(wid % nblk);
    if (item >= (int64_t)p.n_tiles * p.K) return;                   // wave-uniform; the kernel has no barrier
    const int range = (int)(item / p.K), k = (int)(item % p.K);
    const int cd0 = (blk / nbs) * (16 * NGW), cs0 = (blk % nbs) * (16 * NXW);
    const int lo = p.ts[(int64_t)k * (p.n_tiles + 1) + range];
    const int hi = p.ts[(int64_t)k * (p.n_tiles + 1) + range + 1];

    const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(p.x, p.n_rows_x * p.Cs * 4), rs_g = make_rsrc(p.dy, p.n_rows_dy * p.Cd * 4);
    const __amdgpu_buffer_rsrc_t rs_rx = make_rsrc(p.rows_x, (int64_t)p.K * p.cap * 4), rs_rg = make_rsrc(p.rows_dy, (int64_t)p.K * p.cap * 4);
    const int ksoff = (int)(k * p.cap) * 4;
    const int cd4 = p.Cd * 4, cs4 = p.Cs * 4;                       // row strides in bytes
    const int gvo = (cd0 + NGW * i16) * 4, xvo = (cs0 + NXW * i16) * 4;

    f32x4 acc[NGW][NXW];
#pragma unroll
    for (int a = 0; a < NGW; ++a)
#pragma unroll
        for (int b = 0; b < NXW; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    int base = lo;
    if constexpr (BF) {
        const int q32 = q * 32;
        for (; base < hi; base += 32) {              // 32 pairs per trip (lane group q: pairs 8q .. 8q+7); the last trip clamps its
            const bool full = base + 32 <= hi;       // indices into the range and masks dy (wave-uniform)
            float gv[8][NGW], xv[8][NXW];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int io, ix;
                if (full) {
                    io = bload32(rs_rg, q32 + u * 4, ksoff + base * 4);
                    ix = bload32(rs_rx, q32 + u * 4, ksoff + base * 4);
                } else {
                    const int pi = min(base + 8 * q + u, hi - 1);
                    io = bload32(rs_rg, pi * 4, ksoff);
                    ix = bload32(rs_rx, pi * 4, ksoff);
                }
                blk_row_part<NGW>(gv[u], rs_g, (int)__umul24(io, cd4) + gvo);
                blk_row_part<NXW>(xv[u], rs_x, (int)__umul24(ix, cs4) + xvo);
                if (!full && base + 8 * q + u >= hi) {          // pairs past the end contribute exact zeros
#pragma unroll
                    for (int a = 0; a < NGW; ++a) gv[u][a] = 0.f;
                }
            }
            bf16x8 xb[NXW];
#pragma unroll
            for (int b = 0; b < NXW; ++b)
                xb[b] = bf16x8{(__bf16)xv[0][b], (__bf16)xv[1][b], (__bf16)xv[2][b], (__bf16)xv[3][b], (__bf16)xv[4][b], (__bf16)xv[5][b], (__bf16)xv[6][b], (__bf16)xv[7][b]};
#pragma unroll
            for (int a = 0; a < NGW; ++a) {
                const bf16x8 ga = bf16x8{(__bf16)gv[0][a], (__bf16)gv[1][a], (__bf16)gv[2][a], (__bf16)gv[3][a], (__bf16)gv[4][a], (__bf16)gv[5][a], (__bf16)gv[6][a], (__bf16)gv[7][a]};
#pragma unroll
                for (int b = 0; b < NXW; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga, xb[b], acc[a][b], 0, 0, 0);
            }
        }
    } else {
        const int q16 = q * 16;
        for (; base + 16 <= hi; base += 16) {        // full trips: 16 pairs = 4 MFMA K-steps (lane group q: pairs 4q .. 4q+3), loads up front
            int io[4], ix[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                io[u] = bload32(rs_rg, q16 + u * 4, ksoff + base * 4);
                ix[u] = bload32(rs_rx, q16 + u * 4, ksoff + base * 4);
            }
            float gv[4][NGW], xv[4][NXW];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                blk_row_part<NGW>(gv[u], rs_g, (int)__umul24(io[u], cd4) + gvo);
                blk_row_part<NXW>(xv[u], rs_x, (int)__umul24(ix[u], cs4) + xvo);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int a = 0; a < NGW; ++a)
#pragma unroll
                    for (int b = 0; b < NXW; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[u][a], xv[u][b], acc[a][b], 0, 0, 0);
        }
        if (base < hi) {                             // last, partial trip: indices clamped into the range, masked dy
            float gv[4][NGW], xv[4][NXW];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pi = min(base + 4 * q + u, hi - 1);
                const int io = bload32(rs_rg, pi * 4, ksoff), ix = bload32(rs_rx, pi * 4, ksoff);
                blk_row_part<NGW>(gv[u], rs_g, (int)__umul24(io, cd4) + gvo);
                blk_row_part<NXW>(xv[u], rs_x, (int)__umul24(ix, cs4) + xvo);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool ok = base + 4 * q + u < hi;        // pairs past the end contribute exact zeros
#pragma unroll
                for (int a = 0; a < NGW; ++a) {
                    const float ga = ok ? gv[u][a] : 0.f;
#pragma unroll
                    for (int b = 0; b < NXW; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, xv[u][b], acc[a][b], 0, 0, 0);
                }
            }
        }
    }
    // accumulator element (a, b, r) of lane (i16, q) is dW_k[cd0 + NGW (4q + r) + a][cs0 + NXW i16 + b]: for fixed (a, r) a lane
    // holds NXW consecutive input channels, written as one vector
    float* out = p.partial + (item_offset(k, range, p.n_tiles) * p.Cd + cd0) * p.Cs + cs0 + NXW * i16;
#pragma unroll
    for (int a = 0; a < NGW; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* o = out + (int64_t)(NGW * (4 * q + r) + a) * p.Cs;
            if constexpr (NXW == 4) {
                *reinterpret_cast<float4*>(o) = make_float4(acc[a][0][r], acc[a][1][r], acc[a][2][r], acc[a][3][r]);
            } else if constexpr (NXW == 2) {
                *reinterpret_cast<float2*>(o) = make_float2(acc[a][0][r], acc[a][1][r]);
            } else {
                o[0] = acc[a][0][r];
            }
        }
}

// dW[co][k][ci] = sum over the row ranges of offset k, four interleaved running sums combined in a fixed order (overwrites dW)
__global__ __launch_bounds__(256) void wgrad_blk_reduce_k(const float* __restrict__ partial, int n_tiles, int K, int Cs, int E, float* __restrict__ dW) {
    const int k = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float* src = partial + item_offset(k, 0, n_tiles) * E + e;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    int r = 0;
    for (; r + 4 <= n_tiles; r += 4) {
        v0 += src[(int64_t)r * E];
        v1 += src[(int64_t)(r + 1) * E];
        v2 += src[(int64_t)(r + 2) * E];
        v3 += src[(int64_t)(r + 3) * E];
    }
    for (; r < n_tiles; ++r) v0 += src[(int64_t)r * E];
    const int co = e / Cs, ci = e % Cs;
    dW[((int64_t)co * K + k) * Cs + ci] = (v0 + v1) + (v2 + v3);
}

// widest block side the channel count divides: 64 or 32 channels (16 for the padded input convolution's Cs)
static int blk_groups(int C) { return C % 64 == 0 ? 4 : (C % 32 == 0 ? 2 : 1); }

bool wgrad_blk_supported(int Cs, int Cd) {
    return (Cs == 16 || (Cs > 0 && Cs % 32 == 0 && Cs <= 512)) && Cd > 0 && Cd % 32 == 0 && Cd <= 512;
}

template <int NGW, int NXW>
static void launch_blk(const WgBlkParams& p, bool bf16, unsigned grid, hipStream_t s) {
    if (bf16) hipLaunchKernelGGL((spconv_wgrad_blk_k<NGW, NXW, true>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((spconv_wgrad_blk_k<NGW, NXW, false>), dim3(grid), dim3(256), 0, s, p);
}

int launch_wgrad_blk(const WgBlkParams& p, bool bf16, float* dW, hipStream_t s) {
    if (!wgrad_blk_supported(p.Cs, p.Cd)) { set_error("spconv_wgrad: no kernel for Cs=%d Cd=%d", p.Cs, p.Cd); return U3D_EUNSUPPORTED; }
    const int ngw = blk_groups(p.Cd), nxw = blk_groups(p.Cs);
    const int64_t waves = (int64_t)p.n_tiles * p.K * (p.Cd / (16 * ngw)) * (p.Cs / (16 * nxw));
    const int64_t grid = ceil_div(waves, 4);
    if (grid >= 0x7fffffffLL) { set_error("spconv_wgrad: %lld workgroups exceed the grid limit", (long long)grid); return U3D_EUNSUPPORTED; }
    const unsigned g = (unsigned)grid;
    if (ngw == 4) { if (nxw == 4) launch_blk<4, 4>(p, bf16, g, s); else if (nxw == 2) launch_blk<4, 2>(p, bf16, g, s); else launch_blk<4, 1>(p, bf16, g, s); }
    else { if (nxw == 4) launch_blk<2, 4>(p, bf16, g, s); else if (nxw == 2) launch_blk<2, 2>(p, bf16, g, s); else launch_blk<2, 1>(p, bf16, g, s); }
    const int E = p.Cd * p.Cs;
    hipLaunchKernelGGL(wgrad_blk_reduce_k, dim3((unsigned)ceil_div(E, 256), p.K), dim3(256), 0, s, (const float*)p.partial, p.n_tiles, p.K, p.Cs, E, dW);
    return check_launch("spconv_wgrad_blk");
}

}  // namespace u3d
