// K13 at head_dim 64: the plane kernels of attn_x3.hip (varlen flash attention, every product from bf16 planes on
// v_mfma_f32_16x16x32_bf16; NP = 3 exact planes for fp32 math, NP = 1 for bf16 operands / bf16 tensors) for rows of 64 dims.  The
// data flow, the work decode, the 64-row tiles and the online softmax are those of attn_x3.hip (read its head comment first); attn_x3.h
// holds what the two files share.  What the wider row changes:
//   reduction   the instruction reduces over 32 elements, so S^T = K . Q^T and dP^T = V . dO^T are KK = 2 chained instructions per plane
//               product (dims 32 kk + 8g .. of the row).  The chain still starts from zero and still runs smallest terms first: all the
//               products of one order of BOTH halves before the next larger order (mfma_x3_2a / _2c).
//   outputs     O, dQ, dK, dV are CB = 4 blocks of 16 columns; the running sums keep their separate low-order accumulators (attn_x3.h
//               mfma_x3_2b, called per pair of column blocks with the same P / dS operand planes).
//   staging     a thread holds dims 4c .. 4c+3 (c = tid & 15) of the four rows 4p .. 4p+3 (p = tid >> 4): 16 lanes cover a row's 256 bytes.
//   LDS         a natural plane row is 128 bytes = 8 chunks of 16 bytes, two rows per 256-byte bank row (row & 1 picks the half), and
//               the chunk XOR of the 64-byte rows, (row >> 1) & 3, no longer serves both kinds of read.  With u = (row >> 1) & 7 (bits
//               u2 u1 u0) the chunk index is XORed with  v(u) = (u1 ^ u2) << 2 | u0 << 1 | u2  (xswz; a bijection of u, equal for rows
//               r and r + 16).  The bank of byte a is (a / 4) % 64 for both reads:
//     ds_read_b128, rows 16 kb + i, logical chunk 4 kk + g: one 16-lane bank group of the instruction holds all sixteen i -- those with
//               u2 ^ u1 = 0 (i in 0..3, 12..15) with one g, those with u2 ^ u1 = 1 (i in 4..11) with g ^ 1.  Bit 2 of v is u1 ^ u2, so
//               the first set lands on the four chunks whose bit 2 is that of the logical chunk and the second on the four others, whatever
//               bit 0 of the logical chunk is; inside a set (v1, v0) = (u0, u2) tells the four u apart.  Eight even rows take the eight
//               chunks of one half, eight odd rows those of the other: 16 distinct 16-byte slots, conflict-free.
//     ds_read_b64_tr_b16, dims 16 cb ..: a 32-lane half takes the aligned rows 8n .. 8n+7, 32 bytes (chunks 2 cb, 2 cb + 1) of each.  u2 is
//               fixed there and (u1, u0) counts the four even (odd) rows, so bits 2..1 of v = (u1 ^ u2, u0) send the four rows to the four
//               distinct chunk PAIRS of their half (v0 only swaps the two chunks inside a pair): 8 x 32 = 256 distinct bytes,
//               conflict-free.  (The straight generalisation (row >> 1) & 7 serves the row reads and leaves these reads 2-way.)
//   registers   DESIGN 4.2 "head_dim 64": no instantiation uses scratch; dK / dV with three planes runs two workgroups per CU.
// Included by attn_x3.hip, once, at its end: one translation unit, so these kernels are compiled with that file's code generation options
// (csrc/build.py EXTRA); the names of attn_x3.hip they redefine at the wider row live in a namespace of their own.
#pragma once
#include "attn_x3.h"

namespace u3d {
namespace hd64 {          // the names of attn_x3.hip (StageRegs, IoT, nat_frag_x3, the kernels ...) at the wider row

constexpr int HD = 64;                       // halves per row of a natural plane, unpadded
constexpr int XN = 64 * HD;                  // halves per natural plane
__device__ __forceinline__ int xswz(int row) { return ((((row >> 2) ^ (row >> 3)) & 1) << 2) | (row & 2) | ((row >> 3) & 1); }

// c += a . b over KK chained 32-deep reduction blocks, two independent accumulators side by side: the plane products smallest terms
// first (attn_x3.h), every block's products of one order before the next larger order
template <int NP, int KK>
__device__ __forceinline__ void mfma_x3_2a(const bf16x8 (&a0)[KK][NP], const bf16x8 (&a1)[KK][NP], const bf16x8 (&b)[KK][NP], f32x4& c0, f32x4& c1) {
#pragma unroll
    for (int o = NP - 1; o >= 0; --o)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
#pragma unroll
            for (int qa = 0; qa <= o; ++qa) {
                c0 = U3D_MFMA_X(a0[kk][qa], b[kk][o - qa], c0);
                c1 = U3D_MFMA_X(a1[kk][qa], b[kk][o - qa], c1);
            }
}
// one chain pair sharing nothing: s += a . b, d += c . e (S and dP of the backward kernels)
template <int NP, int KK>
__device__ __forceinline__ void mfma_x3_2c(const bf16x8 (&a)[KK][NP], const bf16x8 (&b)[KK][NP], const bf16x8 (&c)[KK][NP], const bf16x8 (&e)[KK][NP], f32x4& s, f32x4& d) {
#pragma unroll
    for (int o = NP - 1; o >= 0; --o)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
#pragma unroll
            for (int qa = 0; qa <= o; ++qa) {
                s = U3D_MFMA_X(a[kk][qa], b[kk][o - qa], s);
                d = U3D_MFMA_X(c[kk][qa], e[kk][o - qa], d);
            }
}

// Stage 64 rows x 64 floats of `base` (rows >= len are zero, values scaled before the split): thread (p = tid >> 4, c = tid & 15)
// holds dims 4c .. 4c+3 of the R = 4 rows 4p .. 4p+3; load_x3 issues the global loads (one tile ahead of their use: the
// compute phase of the tile before covers their latency), store_x3 splits and writes the natural planes nat[NP][64][HD] halves.
struct StageRegs { f32x4 v[HD / 16]; };
__device__ __forceinline__ StageRegs load_x3(const float* __restrict__ base, int ld, int row0, int len, int tid) {
    constexpr int R = HD / 16;
    const int p = tid / (HD / 4), c = tid % (HD / 4);
    const int r0 = row0 + R * p;
    StageRegs r;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        r.v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r0 + j < len) r.v[j] = *reinterpret_cast<const f32x4*>(base + (int64_t)(r0 + j) * ld + c * 4);
    }
    return r;
}
template <int NP>
__device__ __forceinline__ void store_x3(StageRegs r, float scale, __bf16* nat, int tid) {
    constexpr int R = HD / 16;
    const int p = tid / (HD / 4), c = tid % (HD / 4);
    unsigned w[R][2][NP];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const f32x4 a = r.v[j] * scale;
        planes_pair<NP>(a[0], a[1], w[j][0]);
        planes_pair<NP>(a[2], a[3], w[j][1]);
    }
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int row = R * p + j;
            *reinterpret_cast<uint2*>(nat + q * XN + row * HD + (((c >> 1) ^ xswz(row)) * 8) + (c & 1) * 4) = make_uint2(w[j][0][q], w[j][1][q]);
        }
}

// bf16 tensors in HBM (IO16; one plane, include/u3d.h u3d_attn_varlen_*_b16): the same staging map with 8-byte loads and no arithmetic --
// the staged values are the tensor's own, so a scale cannot be folded in here (the kernels apply it to the scores / to dK instead)
struct StageRegs16 { uint2 v[HD / 16]; };
__device__ __forceinline__ StageRegs16 load_x16(const __bf16* __restrict__ base, int ld, int row0, int len, int tid) {
    constexpr int R = HD / 16;
    const int p = tid / (HD / 4), c = tid % (HD / 4);
    const int r0 = row0 + R * p;
    StageRegs16 r;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        r.v[j] = make_uint2(0u, 0u);
        if (r0 + j < len) r.v[j] = *reinterpret_cast<const uint2*>(base + (int64_t)(r0 + j) * ld + c * 4);
    }
    return r;
}
__device__ __forceinline__ void store_x16(StageRegs16 r, __bf16* nat, int tid) {
    constexpr int R = HD / 16;
    const int p = tid / (HD / 4), c = tid % (HD / 4);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int row = R * p + j;
        *reinterpret_cast<uint2*>(nat + row * HD + (((c >> 1) ^ xswz(row)) * 8) + (c & 1) * 4) = r.v[j];
    }
}
template <bool IO16> struct IoT { typedef float t; typedef StageRegs regs; };
template <> struct IoT<true> { typedef __bf16 t; typedef StageRegs16 regs; };
template <bool IO16> using io_of = typename IoT<IO16>::t;          // the tensors' element type
template <bool IO16>
__device__ __forceinline__ typename IoT<IO16>::regs load_io(const io_of<IO16>* __restrict__ base, int ld, int row0, int len, int tid) {
    if constexpr (IO16) return load_x16(base, ld, row0, len, tid);
    else return load_x3(base, ld, row0, len, tid);
}
template <int NP, bool IO16>
__device__ __forceinline__ void store_io(typename IoT<IO16>::regs r, float scale, __bf16* nat, int tid) {
    if constexpr (IO16) store_x16(r, nat, tid);
    else store_x3<NP>(r, scale, nat, tid);
}
template <bool IO16>
__device__ __forceinline__ void put_io(io_of<IO16>* p, float v) {
    if constexpr (IO16) *p = (__bf16)v;
    else *p = v;
}

// natural planes: rows 16 kb + i, dims 32 kk + 8g .. 32 kk + 8g+7, kk < HD / 32
template <int NP>
__device__ __forceinline__ void nat_frag_x3(const __bf16* nat, int kb, int i16, int g, bf16x8 (&out)[HD / 32][NP]) {
#pragma unroll
    for (int kk = 0; kk < HD / 32; ++kk)
#pragma unroll
        for (int q = 0; q < NP; ++q)
            out[kk][q] = *reinterpret_cast<const bf16x8*>(nat + q * XN + (kb * 16 + i16) * HD + (((4 * kk + g) ^ xswz(i16)) * 8));      // xswz(16 kb + i) = xswz(i)
}

// natural planes read by COLUMN: dim 16 cb + i16 over rows {4g..4g+3} and {16+4g..16+4g+3} of the 32-row block t (the k order of
// pair_frag_x3).  ds_read_b64_tr_b16: lane i16 of a 16-lane group passes the address of 4 halves -- row (i16 >> 2) of the group's four,
// dims 16 cb + 4 (i16 & 3) .. -- and receives dim 16 cb + i16 of the four rows.
template <int NP>
__device__ __forceinline__ void tr_col_frag_x3(const __bf16* nat, int t, int g, int i16, int cb, bf16x8 (&out)[NP]) {
    const int row = 32 * t + 4 * g + (i16 >> 2), pc = i16 & 3;
    const __bf16* s = nat + row * HD + (((2 * cb + (pc >> 1)) ^ xswz(row)) * 8) + 4 * (pc & 1);      // row + 16 has the same chunk XOR
#pragma unroll
    for (int q = 0; q < NP; ++q) out[q] = tr16_pair(s + q * XN, s + q * XN + 16 * HD);
}

template <int NP, bool IO16 = false>
__global__ __launch_bounds__(256) void attn_fwd_x3_k(const io_of<IO16>* __restrict__ qkv, const int32_t* __restrict__ cu, int H, float scale,
                                                     io_of<IO16>* __restrict__ out, float* __restrict__ lse, int64_t n_total, int B, int n_tiles) {
    static_assert(!IO16 || NP == 1, "bf16 tensors carry one plane");
    typedef io_of<IO16> io_t;
    constexpr int KK = HD / 32, CB = HD / 16;          // 32-deep reduction blocks of a row | 16-column blocks of an output row
    __shared__ __attribute__((aligned(16))) __bf16 Kn[NP * XN];
    __shared__ __attribute__((aligned(16))) __bf16 Vn[NP * XN];
    const AttnWork wk_ = attn_decode(H, B, n_tiles);
    const int b = wk_.b, h = wk_.h;
    if (b >= B) return;
    const int start = cu[b], len = cu[b + 1] - start;
    const int q0 = wk_.tile * 64;
    if (q0 >= len) return;
    const int D = H * HD, ld = 3 * D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
    const io_t* base = qkv + (int64_t)start * ld + h * HD;
    const int qrow = q0 + wave * 16 + i16;
    bf16x8 qf[KK][NP];                            // scores in log2 units: q carries scale * log2(e) -- or, IO16, the scores are scaled
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        if constexpr (IO16) row_frag_x16(qrow < len ? base + (int64_t)qrow * ld + 32 * kk + g * 8 : nullptr, qf[kk]);
        else row_frag_x3(qrow < len ? base + (int64_t)qrow * ld + 32 * kk + g * 8 : nullptr, scale * X_LOG2E, qf[kk]);
    }
    const float sc_ = IO16 ? scale * X_LOG2E : 1.f;
    float m = -INFINITY, l = 0.f;
    f32x4 o[CB], ol[CB];          // h.h | low-order products
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) o[cb] = ol[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (len + 63) >> 6;
    typename IoT<IO16>::regs rk = load_io<IO16>(base + D, ld, 0, len, tid), rv = load_io<IO16>(base + 2 * D, ld, 0, len, tid);
    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();
        store_io<NP, IO16>(rk, 1.f, Kn, tid);
        store_io<NP, IO16>(rv, 1.f, Vn, tid);
        if (kt + 1 < ntiles) {
            rk = load_io<IO16>(base + D, ld, kt * 64 + 64, len, tid);
            rv = load_io<IO16>(base + 2 * D, ld, kt * 64 + 64, len, tid);
        }
        __syncthreads();
        float st[4][4];
#pragma unroll
        for (int kb = 0; kb < 4; kb += 2) {
            bf16x8 a0[KK][NP], a1[KK][NP];
            nat_frag_x3<NP>(Kn, kb, i16, g, a0);
            nat_frag_x3<NP>(Kn, kb + 1, i16, g, a1);
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
            mfma_x3_2a<NP, KK>(a0, a1, qf, s0, s1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (IO16) { st[kb][r] = s0[r] * sc_; st[kb + 1][r] = s1[r] * sc_; }
                else { st[kb][r] = s0[r]; st[kb + 1][r] = s1[r]; }
            }
        }
        if (kt == ntiles - 1 && (len & 63)) {          // only the last tile can hold keys past the end (wave-uniform)
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt * 64 + kb * 16 + g * 4 + r >= len) st[kb][r] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[kb][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);
        float ps = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(st[kb][r] - m_new);
                st[kb][r] = p;
                ps += p;
            }
        ps += __shfl_xor(ps, 16, 64);
        ps += __shfl_xor(ps, 32, 64);
        l = l * alpha + ps;
        m = m_new;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ar = __shfl(alpha, g * 4 + r, 64);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) o[cb][r] *= ar;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) ol[cb][r] *= ar;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            bf16x8 pa[NP], v0[NP], v1[NP];
            pair_frag_x3(st[2 * t], st[2 * t + 1], pa);
#pragma unroll
            for (int cb = 0; cb < CB; cb += 2) {
                tr_col_frag_x3<NP>(Vn, t, g, i16, cb, v0);
                tr_col_frag_x3<NP>(Vn, t, g, i16, cb + 1, v1);
                mfma_x3_2b(pa, v0, v1, o[cb], o[cb + 1], ol[cb], ol[cb + 1]);
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) o[cb] += ol[cb];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float lr = __shfl(l, g * 4 + r, 64);
        const int row = q0 + wave * 16 + g * 4 + r;
        if (row < len) {
            const float inv = 1.f / lr;
            io_t* op = out + (int64_t)(start + row) * D + h * HD + i16;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) put_io<IO16>(op + 16 * cb, o[cb][r] * inv);
        }
    }
    if (g == 0 && qrow < len) lse[(int64_t)h * n_total + start + qrow] = m * X_LN2 + __logf(l);      // natural-log units
}

// dQ: one workgroup per 64-query tile, keys streamed.  K is read by rows for S and by columns for dQ += dS . K.
template <int NP, bool IO16 = false>
__global__ __launch_bounds__(256) void attn_bwd_dq_x3_k(const io_of<IO16>* __restrict__ qkv, const io_of<IO16>* __restrict__ dout, const float* __restrict__ lse,
                                                        const float* __restrict__ delta, const int32_t* __restrict__ cu, int H, float scale,
                                                        io_of<IO16>* __restrict__ dqkv, int64_t n_total, int B, int n_tiles) {
    static_assert(!IO16 || NP == 1, "bf16 tensors carry one plane");
    typedef io_of<IO16> io_t;
    constexpr int KK = HD / 32, CB = HD / 16;          // 32-deep reduction blocks of a row | 16-column blocks of an output row
    __shared__ __attribute__((aligned(16))) __bf16 Kn[NP * XN];
    __shared__ __attribute__((aligned(16))) __bf16 Vn[NP * XN];
    const AttnWork wk_ = attn_decode(H, B, n_tiles);
    const int b = wk_.b, h = wk_.h;
    if (b >= B) return;
    const int start = cu[b], len = cu[b + 1] - start;
    const int q0 = wk_.tile * 64;
    if (q0 >= len) return;
    const int D = H * HD, ld = 3 * D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
    const io_t* base = qkv + (int64_t)start * ld + h * HD;
    const int qrow = q0 + wave * 16 + i16;
    const bool qok = qrow < len;
    bf16x8 qf[KK][NP], dof[KK][NP];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        if constexpr (IO16) {
            row_frag_x16(qok ? base + (int64_t)qrow * ld + 32 * kk + g * 8 : nullptr, qf[kk]);
            row_frag_x16(qok ? dout + (int64_t)(start + qrow) * D + h * HD + 32 * kk + g * 8 : nullptr, dof[kk]);
        } else {
            row_frag_x3(qok ? base + (int64_t)qrow * ld + 32 * kk + g * 8 : nullptr, scale * X_LOG2E, qf[kk]);
            row_frag_x3(qok ? dout + (int64_t)(start + qrow) * D + h * HD + 32 * kk + g * 8 : nullptr, 1.f, dof[kk]);
        }
    }
    const float sc_ = IO16 ? scale * X_LOG2E : 1.f;
    // log2 units; rows past the end get +inf so that exp2(s - lse) = 0 masks them without a select per element
    const float lse_q = qok ? lse[(int64_t)h * n_total + start + qrow] * X_LOG2E : INFINITY;
    const float del_q = qok ? delta[(int64_t)h * n_total + start + qrow] : 0.f;
    f32x4 dq[CB], dql[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) dq[cb] = dql[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (len + 63) >> 6;
    typename IoT<IO16>::regs rk = load_io<IO16>(base + D, ld, 0, len, tid), rv = load_io<IO16>(base + 2 * D, ld, 0, len, tid);
    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();
        store_io<NP, IO16>(rk, 1.f, Kn, tid);
        store_io<NP, IO16>(rv, 1.f, Vn, tid);
        if (kt + 1 < ntiles) {
            rk = load_io<IO16>(base + D, ld, kt * 64 + 64, len, tid);
            rv = load_io<IO16>(base + 2 * D, ld, kt * 64 + 64, len, tid);
        }
        __syncthreads();
        const bool last = kt == ntiles - 1 && (len & 63);          // wave-uniform
        float ds[4][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            bf16x8 ak[KK][NP], av[KK][NP];
            nat_frag_x3<NP>(Kn, kb, i16, g, ak);
            nat_frag_x3<NP>(Vn, kb, i16, g, av);
            f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, dp4 = s4;
            mfma_x3_2c<NP, KK>(ak, qf, av, dof, s4, dp4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p = __builtin_amdgcn_exp2f(IO16 ? s4[r] * sc_ - lse_q : s4[r] - lse_q);
                if (last && kt * 64 + kb * 16 + g * 4 + r >= len) p = 0.f;        // zero-padded keys of the last tile
                ds[kb][r] = p * (dp4[r] - del_q);
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            bf16x8 da[NP], k0[NP], k1[NP];
            pair_frag_x3(ds[2 * t], ds[2 * t + 1], da);
#pragma unroll
            for (int cb = 0; cb < CB; cb += 2) {
                tr_col_frag_x3<NP>(Kn, t, g, i16, cb, k0);
                tr_col_frag_x3<NP>(Kn, t, g, i16, cb + 1, k1);
                mfma_x3_2b(da, k0, k1, dq[cb], dq[cb + 1], dql[cb], dql[cb + 1]);
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) dq[cb] += dql[cb];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = q0 + wave * 16 + g * 4 + r;
        if (row < len) {
            io_t* op = dqkv + (int64_t)(start + row) * ld + h * HD + i16;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) put_io<IO16>(op + 16 * cb, dq[cb][r] * scale);
        }
    }
}

// dK, dV: one workgroup per 64-key tile, queries streamed.  Q and dO are read by rows (S, dP) and by columns (dK, dV).
// (HD = 32, three planes: three workgroups per CU -- the compiler settles at 178 VGPRs without the bound and 166, no spills, with it.
// HD = 64: the accumulators and the register-resident K / V planes double; DKV_WAVES asks for what leaves no scratch -- DESIGN 4.2)
template <int NP> constexpr int DKV_WAVES = NP == 3 ? 2 : 1;
template <int NP, bool IO16 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DKV_WAVES<NP>))) void attn_bwd_dkv_x3_k(const io_of<IO16>* __restrict__ qkv, const io_of<IO16>* __restrict__ dout, const float* __restrict__ lse,
                                                         const float* __restrict__ delta, const int32_t* __restrict__ cu, int H, float scale,
                                                         io_of<IO16>* __restrict__ dqkv, int64_t n_total, int B, int n_tiles) {
    static_assert(!IO16 || NP == 1, "bf16 tensors carry one plane");
    typedef io_of<IO16> io_t;
    constexpr int KK = HD / 32, CB = HD / 16;          // 32-deep reduction blocks of a row | 16-column blocks of an output row
    __shared__ __attribute__((aligned(16))) __bf16 Qn[NP * XN];
    __shared__ __attribute__((aligned(16))) __bf16 On[NP * XN];
    __shared__ float lse_s[64], del_s[64];
    const AttnWork wk_ = attn_decode(H, B, n_tiles);
    const int b = wk_.b, h = wk_.h;
    if (b >= B) return;
    const int start = cu[b], len = cu[b + 1] - start;
    const int k0 = wk_.tile * 64;
    if (k0 >= len) return;
    const int D = H * HD, ld = 3 * D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
    const io_t* base = qkv + (int64_t)start * ld + h * HD;
    const io_t* dobase = dout + (int64_t)start * D + h * HD;
    const int krow = k0 + wave * 16 + i16;
    bf16x8 kf[KK][NP], vf[KK][NP];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        if constexpr (IO16) {
            row_frag_x16(krow < len ? base + (int64_t)krow * ld + D + 32 * kk + g * 8 : nullptr, kf[kk]);
            row_frag_x16(krow < len ? base + (int64_t)krow * ld + 2 * D + 32 * kk + g * 8 : nullptr, vf[kk]);
        } else {
            row_frag_x3(krow < len ? base + (int64_t)krow * ld + D + 32 * kk + g * 8 : nullptr, 1.f, kf[kk]);
            row_frag_x3(krow < len ? base + (int64_t)krow * ld + 2 * D + 32 * kk + g * 8 : nullptr, 1.f, vf[kk]);
        }
    }
    const float sc_ = IO16 ? scale * X_LOG2E : 1.f;
    f32x4 dk[CB], dv[CB], dkl[CB], dvl[CB];       // dkl, dvl: low-order plane products
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) dk[cb] = dv[cb] = dkl[cb] = dvl[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (len + 63) >> 6;
    typename IoT<IO16>::regs rq = load_io<IO16>(base, ld, 0, len, tid), ro = load_io<IO16>(dobase, D, 0, len, tid);
    for (int qt = 0; qt < ntiles; ++qt) {
        __syncthreads();
        store_io<NP, IO16>(rq, scale * X_LOG2E, Qn, tid);  // log2 units; dK is rescaled by ln 2 at the end (IO16: Q as it is, scores scaled, dK by `scale`)
        store_io<NP, IO16>(ro, 1.f, On, tid);
        if (qt + 1 < ntiles) {
            rq = load_io<IO16>(base, ld, qt * 64 + 64, len, tid);
            ro = load_io<IO16>(dobase, D, qt * 64 + 64, len, tid);
        }
        if (tid < 64) {
            const int q = qt * 64 + tid;
            lse_s[tid] = q < len ? lse[(int64_t)h * n_total + start + q] * X_LOG2E : INFINITY;   // exp2(s - inf) = 0 masks the row
            del_s[tid] = q < len ? delta[(int64_t)h * n_total + start + q] : 0.f;
        }
        __syncthreads();
        #pragma unroll
        for (int t = 0; t < 2; ++t) {
            float p[2][4], ds[2][4];          // 32 queries at a time: S / dP of two 16-query blocks, then their dV / dK products
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int qb = 2 * t + u;
                bf16x8 aq[KK][NP], ao[KK][NP];
                nat_frag_x3<NP>(Qn, qb, i16, g, aq);
                nat_frag_x3<NP>(On, qb, i16, g, ao);
                f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, dp4 = s4;
                mfma_x3_2c<NP, KK>(aq, kf, ao, vf, s4, dp4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qq = qb * 16 + g * 4 + r;
                    p[u][r] = __builtin_amdgcn_exp2f(IO16 ? s4[r] * sc_ - lse_s[qq] : s4[r] - lse_s[qq]);
                    ds[u][r] = p[u][r] * (dp4[r] - del_s[qq]);
                }
            }
            bf16x8 pa[NP], da[NP], f0[NP], f1[NP];
            pair_frag_x3(p[0], p[1], pa);
#pragma unroll
            for (int cb = 0; cb < CB; cb += 2) {
                tr_col_frag_x3<NP>(On, t, g, i16, cb, f0);
                tr_col_frag_x3<NP>(On, t, g, i16, cb + 1, f1);
                mfma_x3_2b(pa, f0, f1, dv[cb], dv[cb + 1], dvl[cb], dvl[cb + 1]);
            }
            pair_frag_x3(ds[0], ds[1], da);
#pragma unroll
            for (int cb = 0; cb < CB; cb += 2) {
                tr_col_frag_x3<NP>(Qn, t, g, i16, cb, f0);
                tr_col_frag_x3<NP>(Qn, t, g, i16, cb + 1, f1);
                mfma_x3_2b(da, f0, f1, dk[cb], dk[cb + 1], dkl[cb], dkl[cb + 1]);
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) { dv[cb] += dvl[cb]; dk[cb] += dkl[cb]; }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = k0 + wave * 16 + g * 4 + r;
        if (row < len) {
            io_t* op = dqkv + (int64_t)(start + row) * ld + h * HD + i16;
            const float ks = IO16 ? scale : X_LN2;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) put_io<IO16>(op + D + 16 * cb, dk[cb][r] * ks);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) put_io<IO16>(op + 2 * D + 16 * cb, dv[cb][r]);
        }
    }
}

}  // namespace hd64

// launchers, called from attn_x3.hip's attn_fwd_x3_launch / attn_bwd_x3_launch when hd == 64 (which own the tile count and the dQ fork)
void attn_fwd_x3_hd64_launch(AttnMode mode, const void* qkv, const int32_t* cu, int B, int n_tiles, int64_t n_total, int H, float scale, void* out,
                             float* lse, hipStream_t s) {
    const dim3 grid(attn_grid(H, B, n_tiles));
    if (mode == ATTN_B16) hipLaunchKernelGGL((hd64::attn_fwd_x3_k<1, true>), grid, dim3(256), 0, s, (const __bf16*)qkv, cu, H, scale, (__bf16*)out, lse, n_total, B, n_tiles);
    else if (mode == ATTN_BF16_OPS) hipLaunchKernelGGL((hd64::attn_fwd_x3_k<1, false>), grid, dim3(256), 0, s, (const float*)qkv, cu, H, scale, (float*)out, lse, n_total, B, n_tiles);
    else hipLaunchKernelGGL((hd64::attn_fwd_x3_k<3, false>), grid, dim3(256), 0, s, (const float*)qkv, cu, H, scale, (float*)out, lse, n_total, B, n_tiles);
}

void attn_bwd_x3_hd64_launch(AttnMode mode, const void* qkv, const void* dout, const float* lse, const int32_t* cu, int B, int n_tiles,
                             int64_t n_total, int H, float scale, void* dqkv, const float* delta, hipStream_t sq, hipStream_t s) {
    const dim3 grid(attn_grid(H, B, n_tiles));
    if (mode == ATTN_B16) {
        hipLaunchKernelGGL((hd64::attn_bwd_dq_x3_k<1, true>), grid, dim3(256), 0, sq, (const __bf16*)qkv, (const __bf16*)dout, lse, delta, cu, H, scale, (__bf16*)dqkv, n_total, B, n_tiles);
        hipLaunchKernelGGL((hd64::attn_bwd_dkv_x3_k<1, true>), grid, dim3(256), 0, s, (const __bf16*)qkv, (const __bf16*)dout, lse, delta, cu, H, scale, (__bf16*)dqkv, n_total, B, n_tiles);
    } else if (mode == ATTN_BF16_OPS) {
        hipLaunchKernelGGL((hd64::attn_bwd_dq_x3_k<1, false>), grid, dim3(256), 0, sq, (const float*)qkv, (const float*)dout, lse, delta, cu, H, scale, (float*)dqkv, n_total, B, n_tiles);
        hipLaunchKernelGGL((hd64::attn_bwd_dkv_x3_k<1, false>), grid, dim3(256), 0, s, (const float*)qkv, (const float*)dout, lse, delta, cu, H, scale, (float*)dqkv, n_total, B, n_tiles);
    } else {
        hipLaunchKernelGGL((hd64::attn_bwd_dq_x3_k<3, false>), grid, dim3(256), 0, sq, (const float*)qkv, (const float*)dout, lse, delta, cu, H, scale, (float*)dqkv, n_total, B, n_tiles);
        hipLaunchKernelGGL((hd64::attn_bwd_dkv_x3_k<3, false>), grid, dim3(256), 0, s, (const float*)qkv, (const float*)dout, lse, delta, cu, H, scale, (float*)dqkv, n_total, B, n_tiles);
    }
}

}  // namespace u3d
