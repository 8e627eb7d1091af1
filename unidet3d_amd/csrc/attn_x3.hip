// K13 (fp32 math on the bf16 matrix pipe, u3d_common.h "bf16x3"): the varlen flash attention of attn.hip with every fp32
// operand split exactly into three bf16 planes and every product formed from six v_mfma_f32_16x16x32_bf16 -- the error of an
// fp32 FMA chain at 6 x 16 instead of 8 x 32 matrix-pipe cycles per 16 x 16 x 32 block.  The default path of
// u3d_attn_varlen_fwd / _bwd (reference: nn.MultiheadAttention inside unidet3d/encoder.py:19-21,55-61; oracle/model.py);
// U3D_FP32_MATH=mfma selects the native fp32 MFMA kernels of attn.hip.
//
// v_mfma_f32_16x16x32_bf16: lane (i = lane & 15, g = lane >> 4) holds the 8 reduction elements k = 8g .. 8g+7 of row i (A) /
// column i (B).
//   S^T (16 keys x 16 queries) = K_tile . Q^T       A = K rows, natural [key][dim] planes in LDS (one 16-byte read per plane),
//                                                   B = own Q rows, split once into registers
//   O (16 queries x 16 dims) += P . V               A = two C fragments (keys {4g..4g+3} of two 16-key tiles), split in registers,
//                                                   B = a COLUMN of the natural V planes: the fragment k = 8g + e <-> key
//       32t + 16 (e >> 2) + 4g + (e & 3) of dim i is two ds_read_b64_tr_b16 per plane -- a 16-lane group hands in the [4 keys][16 dims]
//       block of its lane group (lane t the 8 bytes at key t >> 2, dims 4 (t & 3) ..) and lane t receives dim t over the four keys.
//       (Rounds 2-3 staged such tensors a second time in a "pair" layout -- two keys per dword, [dim][key-pair slot] -- read with
//       ds_read_b128; the transpose read makes that copy unnecessary: half the LDS per staged tensor, no second packing and no
//       dword stores in the staging threads.)
// The backward kernels read their staged tiles in both orientations the same way: rows with ds_read_b128, columns with transpose reads.
// The kernels are templates over the head dim and the number of planes: NP = 3 is the fp32 path above, NP = 1 the bf16-operand form of
// BASELINE configs[2] (one bf16 value per operand, rounded to nearest even; u3d_attn_varlen_*_bf16 at the end of the file).
//
// HD = 32 is one instruction's reduction depth and two 16-column output blocks; what a row of HD = 64 dims changes is counted, not coded:
//   reduction   S^T = K . Q^T and dP^T = V . dO^T are KK = HD / 32 chained instructions per plane product (dims 32 kk + 8g .. of the
//               row).  The chain still starts from zero and still runs smallest terms first: all the products of one order of EVERY
//               reduction block before the next larger order (mfma_x3_2a / _2c).
//   outputs     O, dQ, dK, dV are CB = HD / 16 blocks of 16 columns; the running sums keep their separate low-order accumulators
//               (mfma_x3_2b, called per pair of column blocks with the same P / dS operand planes).
//   staging     a thread holds dims 4c .. 4c+3 (c = tid % (HD / 4)) of the R = HD / 16 rows R p .. R p + R-1 (p = tid / (HD / 4)): 8 (16)
//               lanes cover a row's 128 (256) bytes.  (Four waves per workgroup; with eight, half the rows per thread: "tile waves" below.)
//   LDS         the chunk XOR of the unpadded natural planes, xswz<HD> -- the one place where the two widths differ in logic.
//   registers   DESIGN 4.2 "head_dim 64": no instantiation uses scratch; dK / dV with three planes runs three (HD = 64: two) workgroups
//               per CU (DKV_WAVES).
#include <mutex>
#include <stdlib.h>
#include <type_traits>

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

// Natural planes are [64 rows][HD halves], unpadded; the 16-byte chunk index of a row is XORed with xswz<HD>(row), equal for rows r
// and r + 16.  The bank of byte a is (a / 4) % 64 for both kinds of read.
// HD = 32: a row is 64 bytes = 4 chunks and the XOR is (row >> 1) & 3.
//     ds_read_b128, lane -> (row = lane & 15, chunk = lane >> 4): conflict-free.
//     ds_read_b64_tr_b16: rows 4g + j and 4 (g + 1) + j of a plane differ by 2 in the chunk XOR, so the 32 lanes of a read cover 256
//               consecutive-bank bytes: conflict-free.
// HD = 64: a row is 128 bytes = 8 chunks, two rows per 256-byte bank row (row & 1 picks the half), and (row >> 1) & 3 no longer serves
//     both kinds of read.  With u = (row >> 1) & 7 (bits u2 u1 u0) the XOR is  v(u) = (u1 ^ u2) << 2 | u0 << 1 | u2  (a bijection of u).
//     ds_read_b128, rows 16 kb + i, logical chunk 4 kk + g: one 16-lane bank group of the instruction holds all sixteen i -- those with
//               u2 ^ u1 = 0 (i in 0..3, 12..15) with one g, those with u2 ^ u1 = 1 (i in 4..11) with g ^ 1.  Bit 2 of v is u1 ^ u2, so
//               the first set lands on the four chunks whose bit 2 is that of the logical chunk and the second on the four others, whatever
//               bit 0 of the logical chunk is; inside a set (v1, v0) = (u0, u2) tells the four u apart.  Eight even rows take the eight
//               chunks of one half, eight odd rows those of the other: 16 distinct 16-byte slots, conflict-free.
//     ds_read_b64_tr_b16, dims 16 cb ..: a 32-lane half takes the aligned rows 8n .. 8n+7, 32 bytes (chunks 2 cb, 2 cb + 1) of each.  u2 is
//               fixed there and (u1, u0) counts the four even (odd) rows, so bits 2..1 of v = (u1 ^ u2, u0) send the four rows to the four
//               distinct chunk PAIRS of their half (v0 only swaps the two chunks inside a pair): 8 x 32 = 256 distinct bytes,
//               conflict-free.  (The straight generalisation (row >> 1) & 7 serves the row reads and leaves these reads 2-way.)
template <int HD>
__device__ __forceinline__ int xswz(int row) {
    static_assert(HD == 32 || HD == 64, "head_dim 32 or 64");
    if constexpr (HD == 32) return (row >> 1) & 3;
    else return ((((row >> 2) ^ (row >> 3)) & 1) << 2) | (row & 2) | ((row >> 3) & 1);
}
template <int HD> constexpr int XN = 64 * HD;          // halves per natural plane

// c += a . b over KK chained 32-deep reduction blocks, two independent accumulators side by side: the plane products smallest terms
// first (mfma_x3_2b above), every block's products of one order before the next larger order
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

// Stage 64 rows x HD floats of `base` (rows >= len are zero, values scaled before the split).  A workgroup of NW waves (16 NW query / key
// rows of its own, DESIGN 4.2 "tile waves") stages every 64-row tile ONCE for all of them: its 64 NW threads share the tile, thread
// (p = tid / (HD / 4), c = tid % (HD / 4)) holding dims 4c .. 4c+3 of the R = STG_R rows R p .. R p + R-1 -- HD / 16 rows at NW = 4, HD / 32
// at NW = 8.  load_x3 issues the global loads (one tile ahead of their use: the compute phase of the tile before covers their latency),
// store_x3 splits and writes the natural planes nat[NP][64][HD] halves.  The LDS image does not depend on NW.
// The loads are raw buffer loads through a descriptor over the tile's rows below `len` (tile_rsrc): a row past the end of the scene reads
// zeros in the range check of the load itself -- no branch, no zero fill, no 64-bit address per row -- and the descriptor is rebuilt per
// tile from wave-uniform values, so a thread's byte offset (tile_voff, the same for every tile, plus a scalar row offset) stays below 64 rows whatever `len` is.
template <int HD, int NW> constexpr int STG_R = HD / (4 * NW);
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const T* __restrict__ base, int ld, int row0, int len) {
    const int rows = len - row0 < 64 ? len - row0 : 64;
    return make_rsrc(base + (int64_t)row0 * ld, rows > 0 ? (int64_t)rows * ld * (int)sizeof(T) : 0);
}
template <int HD, int NW, typename T>
__device__ __forceinline__ int tile_voff(int ld, int tid) {          // of the thread's first row; row j of its R: + j * ld elements, a scalar offset
    const int p = tid / (HD / 4), c = tid % (HD / 4);
    return (STG_R<HD, NW> * p * ld + c * 4) * (int)sizeof(T);
}
template <int HD, int NW> struct StageRegs { f32x4 v[STG_R<HD, NW>]; };
template <int HD, int NW>
__device__ __forceinline__ StageRegs<HD, NW> load_x3(const float* __restrict__ base, int ld, int row0, int len, int tid) {
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(base, ld, row0, len);
    StageRegs<HD, NW> r;
#pragma unroll
    for (int j = 0; j < STG_R<HD, NW>; ++j) r.v[j] = bload128(rs, tile_voff<HD, NW, float>(ld, tid), j * ld * (int)sizeof(float));
    return r;
}
template <int HD, int NP, int NW>
__device__ __forceinline__ void store_x3(StageRegs<HD, NW> r, float scale, __bf16* nat, int tid) {
    constexpr int R = STG_R<HD, NW>;
    const int p = tid / (HD / 4), c = tid % (HD / 4);
    unsigned w[R][2][NP];
#pragma unroll
    for (int j = 0; j < R; ++j) r.v[j] *= scale;
#pragma unroll
    for (int h = 0; h < 2; ++h)          // the first halves of every row, then the second: the order the kernels were timed with
#pragma unroll
        for (int j = 0; j < R; ++j) planes_pair<NP>(r.v[j][2 * h], r.v[j][2 * h + 1], w[j][h]);
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int row = R * p + j;
            *reinterpret_cast<uint2*>(nat + q * XN<HD> + row * HD + (((c >> 1) ^ xswz<HD>(row)) * 8) + (c & 1) * 4) = make_uint2(w[j][0][q], w[j][1][q]);
        }
}

// bf16 tensors in HBM (IO16; one plane, include/u3d.h u3d_attn_varlen_*_b16): the same staging map with 8-byte loads and no arithmetic --
// the staged values are the tensor's own, so a scale cannot be folded in here (the kernels apply it to the scores / to dK instead)
template <int HD, int NW> struct StageRegs16 { uint2 v[STG_R<HD, NW>]; };
template <int HD, int NW>
__device__ __forceinline__ StageRegs16<HD, NW> load_x16(const __bf16* __restrict__ base, int ld, int row0, int len, int tid) {
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(base, ld, row0, len);
    StageRegs16<HD, NW> r;
#pragma unroll
    for (int j = 0; j < STG_R<HD, NW>; ++j) r.v[j] = bload64(rs, tile_voff<HD, NW, __bf16>(ld, tid), j * ld * (int)sizeof(__bf16));
    return r;
}
template <int HD, int NW>
__device__ __forceinline__ void store_x16(StageRegs16<HD, NW> r, __bf16* nat, int tid) {
    constexpr int R = STG_R<HD, NW>;
    const int p = tid / (HD / 4), c = tid % (HD / 4);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int row = R * p + j;
        *reinterpret_cast<uint2*>(nat + row * HD + (((c >> 1) ^ xswz<HD>(row)) * 8) + (c & 1) * 4) = r.v[j];
    }
}
template <bool IO16> struct IoT { typedef float t; template <int HD, int NW> using regs = StageRegs<HD, NW>; };
template <> struct IoT<true> { typedef __bf16 t; template <int HD, int NW> using regs = StageRegs16<HD, NW>; };
template <bool IO16> using io_of = typename IoT<IO16>::t;                                        // the tensors' element type
template <int HD, bool IO16, int NW> using io_regs = typename IoT<IO16>::template regs<HD, NW>;   // a thread's share of a staged tile
template <int HD, bool IO16, int NW>
__device__ __forceinline__ io_regs<HD, IO16, NW> load_io(const io_of<IO16>* __restrict__ base, int ld, int row0, int len, int tid) {
    if constexpr (IO16) return load_x16<HD, NW>(base, ld, row0, len, tid);
    else return load_x3<HD, NW>(base, ld, row0, len, tid);
}
template <int HD, int NP, bool IO16, int NW>
__device__ __forceinline__ void store_io(io_regs<HD, IO16, NW> r, float scale, __bf16* nat, int tid) {
    if constexpr (IO16) store_x16<HD, NW>(r, nat, tid);
    else store_x3<HD, NP, NW>(r, scale, nat, tid);
}
template <bool IO16>
__device__ __forceinline__ void put_io(io_of<IO16>* p, float v) {
    if constexpr (IO16) *p = (__bf16)v;
    else *p = v;
}

// natural planes: rows 16 kb + i, dims 32 kk + 8g .. 32 kk + 8g+7 of the reduction blocks kk < HD / 32
template <int HD, int NP>
__device__ __forceinline__ void nat_frag_x3(const __bf16* nat, int kb, int i16, int g, bf16x8 (&out)[HD / 32][NP]) {
#pragma unroll
    for (int kk = 0; kk < HD / 32; ++kk)
#pragma unroll
        for (int q = 0; q < NP; ++q)
            out[kk][q] = *reinterpret_cast<const bf16x8*>(nat + q * XN<HD> + (kb * 16 + i16) * HD + (((4 * kk + g) ^ xswz<HD>(i16)) * 8));      // xswz<HD>(16 kb + i) = xswz<HD>(i)
}

// natural planes read by COLUMN: dim 16 cb + i16 over rows {4g..4g+3} and {16+4g..16+4g+3} of the 32-row block t (the k order of
// pair_frag_x3).  ds_read_b64_tr_b16: lane i16 of a 16-lane group passes the address of 4 halves -- row (i16 >> 2) of the group's four,
// dims 16 cb + 4 (i16 & 3) .. -- and receives dim 16 cb + i16 of the four rows.
template <int HD, int NP>
__device__ __forceinline__ void tr_col_frag_x3(const __bf16* nat, int t, int g, int i16, int cb, bf16x8 (&out)[NP]) {
    const int row = 32 * t + 4 * g + (i16 >> 2), pc = i16 & 3;
    const __bf16* s = nat + row * HD + (((2 * cb + (pc >> 1)) ^ xswz<HD>(row)) * 8) + 4 * (pc & 1);      // row + 16 has the same chunk XOR
#pragma unroll
    for (int q = 0; q < NP; ++q) out[q] = tr16_pair(s + q * XN<HD>, s + q * XN<HD> + 16 * HD);
}

// DROP: dropout on the probabilities, the mask regenerated per element by csrc/dropout.h from (head, packed query row, packed
// key row) -- l, m and lse come from the undropped probabilities, O = (P . M) V / (1 - p) with the factor folded into the final scaling.
// The switch is the kernel's trailing argument pack: <HD, NP, IO16> is the kernel without dropout, argument list and all; <HD, NP, IO16,
// DropArgs> takes the key and has DROP = true.
struct DropNone {};
__device__ __forceinline__ DropNone drop_of() { return DropNone{}; }
__device__ __forceinline__ DropArgs drop_of(DropArgs a) { return a; }
template <typename... DR> constexpr bool DROP_ON = sizeof...(DR) == 1;

template <int HD, int NP, bool IO16, int NW, typename... DR>
__global__ __launch_bounds__(64 * NW) void attn_fwd_x3_k(const io_of<IO16>* __restrict__ qkv, const int32_t* __restrict__ cu, int H, float scale,
                                                     io_of<IO16>* __restrict__ out, float* __restrict__ lse, int64_t n_total, int B, int n_tiles,
                                                     DR... dr_) {
    static_assert(!IO16 || NP == 1, "bf16 tensors carry one plane");
    constexpr bool DROP = DROP_ON<DR...>;
    const auto dr = drop_of(dr_...);
    typedef io_of<IO16> io_t;
    constexpr int KK = HD / 32, CB = HD / 16;          // 32-deep reduction blocks of a row | 16-column blocks of an output row
    __shared__ __attribute__((aligned(16))) __bf16 Kn[NP * XN<HD>];
    __shared__ __attribute__((aligned(16))) __bf16 Vn[NP * XN<HD>];
    const AttnWork wk_ = attn_decode(H, B, n_tiles);
    const int b = wk_.b, h = wk_.h;
    if (b >= B) return;
    const int start = cu[b], len = cu[b + 1] - start;
    const int q0 = wk_.tile * (16 * NW);
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
    DropRow drw = {0u, 0u};                       // this lane's query row of the mask; a lane's keys are c = start + 64 kt + 16 kb + 4g + r
    if constexpr (DROP) drw = drop_row(drop_key(dr.seed, dr.offset, (uint32_t)h), (uint32_t)(start + qrow));
    float m = -INFINITY, l = 0.f;
    f32x4 o[CB], ol[CB];          // h.h | low-order products
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) o[cb] = ol[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (len + 63) >> 6;
    io_regs<HD, IO16, NW> rk = load_io<HD, IO16, NW>(base + D, ld, 0, len, tid), rv = load_io<HD, IO16, NW>(base + 2 * D, ld, 0, len, tid);
    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();
        store_io<HD, NP, IO16, NW>(rk, 1.f, Kn, tid);
        store_io<HD, NP, IO16, NW>(rv, 1.f, Vn, tid);
        if (kt + 1 < ntiles) {
            rk = load_io<HD, IO16, NW>(base + D, ld, kt * 64 + 64, len, tid);
            rv = load_io<HD, IO16, NW>(base + 2 * D, ld, kt * 64 + 64, len, tid);
        }
        __syncthreads();
        float st[4][4];
#pragma unroll
        for (int kb = 0; kb < 4; kb += 2) {
            bf16x8 a0[KK][NP], a1[KK][NP];
            nat_frag_x3<HD, NP>(Kn, kb, i16, g, a0);
            nat_frag_x3<HD, NP>(Kn, kb + 1, i16, g, a1);
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
        if constexpr (DROP) {                     // after the row sum, before the planes of P are formed
            const DropRow rt = {drw.x + (uint32_t)(start + kt * 64 + g * 4), drw.y};
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (drop_hash32(rt, (uint32_t)(kb * 16 + r)) < dr.thr) st[kb][r] = 0.f;
        }
        f32x4 ar;          // alpha of the rows 4g .. 4g+3 whose sums this lane holds; all four fetched before the first is used -- fetched
                           // row by row beside the scaling, two of the four shuffles no longer overlap (DESIGN 4.2 "head_dim 64")
#pragma unroll
        for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, g * 4 + r, 64);
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            o[cb] *= ar;
            ol[cb] *= ar;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            bf16x8 pa[NP], v0[NP], v1[NP];
            pair_frag_x3(st[2 * t], st[2 * t + 1], pa);
#pragma unroll
            for (int cb = 0; cb < CB; cb += 2) {
                tr_col_frag_x3<HD, NP>(Vn, t, g, i16, cb, v0);
                tr_col_frag_x3<HD, NP>(Vn, t, g, i16, cb + 1, v1);
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
            float inv = 1.f / lr;
            if constexpr (DROP) inv *= dr.rinv;
            io_t* op = out + (int64_t)(start + row) * D + h * HD + i16;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) put_io<IO16>(op + 16 * cb, o[cb][r] * inv);
        }
    }
    if (g == 0 && qrow < len) lse[(int64_t)h * n_total + start + qrow] = m * X_LN2 + __logf(l);      // natural-log units
}

// dQ: one workgroup per 64-query tile, keys streamed.  K is read by rows for S and by columns for dQ += dS . K.
// DROP: dS = P . (M . dP' / (1 - p) - delta); the lane's query and keys are those of the forward kernel
template <int HD, int NP, bool IO16, int NW, typename... DR>
__global__ __launch_bounds__(64 * NW) void attn_bwd_dq_x3_k(const io_of<IO16>* __restrict__ qkv, const io_of<IO16>* __restrict__ dout, const float* __restrict__ lse,
                                                        const float* __restrict__ delta, const int32_t* __restrict__ cu, int H, float scale,
                                                        io_of<IO16>* __restrict__ dqkv, int64_t n_total, int B, int n_tiles, DR... dr_) {
    static_assert(!IO16 || NP == 1, "bf16 tensors carry one plane");
    constexpr bool DROP = DROP_ON<DR...>;
    const auto dr = drop_of(dr_...);
    typedef io_of<IO16> io_t;
    constexpr int KK = HD / 32, CB = HD / 16;          // 32-deep reduction blocks of a row | 16-column blocks of an output row
    __shared__ __attribute__((aligned(16))) __bf16 Kn[NP * XN<HD>];
    __shared__ __attribute__((aligned(16))) __bf16 Vn[NP * XN<HD>];
    const AttnWork wk_ = attn_decode(H, B, n_tiles);
    const int b = wk_.b, h = wk_.h;
    if (b >= B) return;
    const int start = cu[b], len = cu[b + 1] - start;
    const int q0 = wk_.tile * (16 * NW);
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
    DropRow drw = {0u, 0u};
    if constexpr (DROP) drw = drop_row(drop_key(dr.seed, dr.offset, (uint32_t)h), (uint32_t)(start + qrow));
    f32x4 dq[CB], dql[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) dq[cb] = dql[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (len + 63) >> 6;
    io_regs<HD, IO16, NW> rk = load_io<HD, IO16, NW>(base + D, ld, 0, len, tid), rv = load_io<HD, IO16, NW>(base + 2 * D, ld, 0, len, tid);
    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();
        store_io<HD, NP, IO16, NW>(rk, 1.f, Kn, tid);
        store_io<HD, NP, IO16, NW>(rv, 1.f, Vn, tid);
        if (kt + 1 < ntiles) {
            rk = load_io<HD, IO16, NW>(base + D, ld, kt * 64 + 64, len, tid);
            rv = load_io<HD, IO16, NW>(base + 2 * D, ld, kt * 64 + 64, len, tid);
        }
        __syncthreads();
        const bool last = kt == ntiles - 1 && (len & 63);          // wave-uniform
        float ds[4][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            bf16x8 ak[KK][NP], av[KK][NP];
            nat_frag_x3<HD, NP>(Kn, kb, i16, g, ak);
            nat_frag_x3<HD, NP>(Vn, kb, i16, g, av);
            f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, dp4 = s4;
            mfma_x3_2c<NP, KK>(ak, qf, av, dof, s4, dp4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p = __builtin_amdgcn_exp2f(IO16 ? s4[r] * sc_ - lse_q : s4[r] - lse_q);
                if (last && kt * 64 + kb * 16 + g * 4 + r >= len) p = 0.f;        // zero-padded keys of the last tile
                if constexpr (DROP) {
                    const bool keep = drop_hash32(DropRow{drw.x + (uint32_t)(start + kt * 64 + g * 4), drw.y}, (uint32_t)(kb * 16 + r)) >= dr.thr;
                    ds[kb][r] = p * ((keep ? dp4[r] * dr.rinv : 0.f) - del_q);
                } else {
                    ds[kb][r] = p * (dp4[r] - del_q);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            bf16x8 da[NP], k0[NP], k1[NP];
            pair_frag_x3(ds[2 * t], ds[2 * t + 1], da);
#pragma unroll
            for (int cb = 0; cb < CB; cb += 2) {
                tr_col_frag_x3<HD, NP>(Kn, t, g, i16, cb, k0);
                tr_col_frag_x3<HD, NP>(Kn, t, g, i16, cb + 1, k1);
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
// HD = 64: the accumulators and the register-resident K / V planes double; DKV_WAVES asks for what leaves no scratch -- DESIGN 4.2.
// DROP: the keep mask and the hash temporaries take HD = 32 with three planes from 154 to over 168 registers -- two workgroups per CU there, no scratch.
// NW = 8: a workgroup is two waves per SIMD, so three per SIMD cannot be had: two it is -- four costs 52 bytes of scratch at 128 registers
// and measured 467 us against 428 us of NW = 4, DESIGN 4.2 "tile waves")
template <int HD, int NP, bool DROP, int NW> constexpr int DKV_WAVES = NP == 3 ? (HD == 32 && !DROP && NW != 8 ? 3 : 2) : 1;
// DROP: dV += (P . M)^T dO / (1 - p) (the factor at the end), dS = P . (M . dP' / (1 - p) - delta).  Here a lane holds ONE key (c = start +
// krow) and four consecutive queries (b = start + 64 qt + 16 qb + 4g + r): the row stage of the hash runs per element.
template <int HD, int NP, bool IO16, int NW, typename... DR>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(DKV_WAVES<HD, NP, DROP_ON<DR...>, NW>))) void attn_bwd_dkv_x3_k(const io_of<IO16>* __restrict__ qkv, const io_of<IO16>* __restrict__ dout, const float* __restrict__ lse,
                                                         const float* __restrict__ delta, const int32_t* __restrict__ cu, int H, float scale,
                                                         io_of<IO16>* __restrict__ dqkv, int64_t n_total, int B, int n_tiles, DR... dr_) {
    static_assert(!IO16 || NP == 1, "bf16 tensors carry one plane");
    constexpr bool DROP = DROP_ON<DR...>;
    const auto dr = drop_of(dr_...);
    typedef io_of<IO16> io_t;
    constexpr int KK = HD / 32, CB = HD / 16;          // 32-deep reduction blocks of a row | 16-column blocks of an output row
    __shared__ __attribute__((aligned(16))) __bf16 Qn[NP * XN<HD>];
    __shared__ __attribute__((aligned(16))) __bf16 On[NP * XN<HD>];
    __shared__ float lse_s[64], del_s[64];
    const AttnWork wk_ = attn_decode(H, B, n_tiles);
    const int b = wk_.b, h = wk_.h;
    if (b >= B) return;
    const int start = cu[b], len = cu[b + 1] - start;
    const int k0 = wk_.tile * (16 * NW);
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
    DropKey dkey = {0u, 0u};
    if constexpr (DROP) dkey = drop_key(dr.seed, dr.offset, (uint32_t)h);
    f32x4 dk[CB], dv[CB], dkl[CB], dvl[CB];       // dkl, dvl: low-order plane products
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) dk[cb] = dv[cb] = dkl[cb] = dvl[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (len + 63) >> 6;
    io_regs<HD, IO16, NW> rq = load_io<HD, IO16, NW>(base, ld, 0, len, tid), ro = load_io<HD, IO16, NW>(dobase, D, 0, len, tid);
    for (int qt = 0; qt < ntiles; ++qt) {
        __syncthreads();
        store_io<HD, NP, IO16, NW>(rq, scale * X_LOG2E, Qn, tid);  // log2 units; dK is rescaled by ln 2 at the end (IO16: Q as it is, scores scaled, dK by `scale`)
        store_io<HD, NP, IO16, NW>(ro, 1.f, On, tid);
        if (qt + 1 < ntiles) {
            rq = load_io<HD, IO16, NW>(base, ld, qt * 64 + 64, len, tid);
            ro = load_io<HD, IO16, NW>(dobase, D, qt * 64 + 64, len, tid);
        }
        if (tid < 64) {
            const int q = qt * 64 + tid;
            lse_s[tid] = q < len ? lse[(int64_t)h * n_total + start + q] * X_LOG2E : INFINITY;   // exp2(s - inf) = 0 masks the row
            del_s[tid] = q < len ? delta[(int64_t)h * n_total + start + q] : 0.f;
        }
        __syncthreads();
        unsigned km = 0u;          // DROP: bit 4 qb + r = keep (query 16 qb + 4g + r of this tile, this lane's key), made here in one register:
                                   // hashed where the probabilities are formed, the sixteen hashes' temporaries stay live across the MFMA chains
        if constexpr (DROP) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int qq = (e >> 2) * 16 + g * 4 + (e & 3);
                if (drop_hash32(drop_row(dkey, (uint32_t)(start + qt * 64 + qq)), (uint32_t)(start + krow)) >= dr.thr) km |= 1u << e;
            }
        }
        #pragma unroll
        for (int t = 0; t < 2; ++t) {
            float p[2][4], ds[2][4];          // 32 queries at a time: S / dP of two 16-query blocks, then their dV / dK products
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int qb = 2 * t + u;
                bf16x8 aq[KK][NP], ao[KK][NP];
                nat_frag_x3<HD, NP>(Qn, qb, i16, g, aq);
                nat_frag_x3<HD, NP>(On, qb, i16, g, ao);
                f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, dp4 = s4;
                mfma_x3_2c<NP, KK>(aq, kf, ao, vf, s4, dp4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qq = qb * 16 + g * 4 + r;
                    p[u][r] = __builtin_amdgcn_exp2f(IO16 ? s4[r] * sc_ - lse_s[qq] : s4[r] - lse_s[qq]);
                    if constexpr (DROP) {
                        const bool keep = (km >> (4 * qb + r)) & 1u;
                        ds[u][r] = p[u][r] * ((keep ? dp4[r] * dr.rinv : 0.f) - del_s[qq]);
                        if (!keep) p[u][r] = 0.f;
                    } else {
                        ds[u][r] = p[u][r] * (dp4[r] - del_s[qq]);
                    }
                }
            }
            bf16x8 pa[NP], da[NP], f0[NP], f1[NP];
            pair_frag_x3(p[0], p[1], pa);
#pragma unroll
            for (int cb = 0; cb < CB; cb += 2) {
                tr_col_frag_x3<HD, NP>(On, t, g, i16, cb, f0);
                tr_col_frag_x3<HD, NP>(On, t, g, i16, cb + 1, f1);
                mfma_x3_2b(pa, f0, f1, dv[cb], dv[cb + 1], dvl[cb], dvl[cb + 1]);
            }
            pair_frag_x3(ds[0], ds[1], da);
#pragma unroll
            for (int cb = 0; cb < CB; cb += 2) {
                tr_col_frag_x3<HD, NP>(Qn, t, g, i16, cb, f0);
                tr_col_frag_x3<HD, NP>(Qn, t, g, i16, cb + 1, f1);
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
            for (int cb = 0; cb < CB; ++cb) {
                if constexpr (DROP) put_io<IO16>(op + 2 * D + 16 * cb, dv[cb][r] * dr.rinv);
                else put_io<IO16>(op + 2 * D + 16 * cb, dv[cb][r]);
            }
        }
    }
}

// (hd, mode) -> the instantiation (HD, NP, IO16) that runs it; `f` receives it as a tag type
template <int HD_, int NP_, bool IO16_> struct X3Form {
    static constexpr int HD = HD_, NP = NP_;
    static constexpr bool IO16 = IO16_;
    typedef io_of<IO16_> io_t;
};
template <int HD, typename F>
static void attn_x3_by_mode(AttnMode mode, F&& f) {
    if (mode == ATTN_B16) f(X3Form<HD, 1, true>());
    else if (mode == ATTN_BF16_OPS) f(X3Form<HD, 1, false>());
    else f(X3Form<HD, 3, false>());
}
template <typename F>
static void attn_x3_dispatch(int hd, AttnMode mode, F&& f) {
    if (hd == 64) attn_x3_by_mode<64>(mode, f);
    else attn_x3_by_mode<32>(mode, f);
}

// ---- tile waves: how many waves -- 16 query (dK / dV: key) rows each -- share one workgroup and with it every staged tile ----
// The per-wave program does not depend on NW, so every form gives the same bits; the plan holds, per kernel, what measured ahead of
// NW = 4 (profiles/attn_tile_waves_time.txt), and u3d_attn_tile_waves (include/u3d.h) forces one form for tests and A/B runs.
enum AttnKernel { ATTN_K_FWD, ATTN_K_DQ, ATTN_K_DKV };
static int attn_plan_waves(AttnKernel k, AttnMode mode, int hd, bool drop) {
    const int forced = u3d_attn_tile_waves(-1);
    if (forced) return forced;
    // Eight waves win where the staging they halve is largest and the registers they free raise the occupancy: three planes at head_dim 32,
    // forward (120 -> 107 VGPRs, four waves per SIMD either way: 257.6 -> 252.7 us at 8 x 2125 queries) and dQ (164 -> 116, three -> four
    // waves: 334.0 -> 322.4 us).  dK / dV needs 136 registers -- one 8-wave workgroup per CU instead of three 4-wave ones: 427.8 -> 499.9 us.
    // One plane, head_dim 64 and the dropout forms measured level or behind at that size (ahead only at 3000 queries) and stay on four.
    if (mode == ATTN_X3 && hd == 32 && !drop && (k == ATTN_K_FWD || k == ATTN_K_DQ)) return 8;
    return 4;
}
template <typename F>
static void attn_x3_by_waves(int nw, F&& f) {
    if (nw == 8) f(std::integral_constant<int, 8>());
    else f(std::integral_constant<int, 4>());
}
struct AttnGrid { dim3 grid; int n_tiles; };
static AttnGrid attn_x3_grid(int H, int B, int max_len, int nw) {
    const int n_tiles = attn_tiles(max_len, 16 * nw);
    return {dim3(attn_grid(H, B, n_tiles)), n_tiles};
}

// launchers, called from attn.hip's attn_fwd / attn_bwd for every mode but ATTN_NATIVE (arguments already validated there: hd is 32 or 64)
void attn_fwd_x3_launch(AttnMode mode, const void* qkv, const int32_t* cu, int B, int max_len, int64_t n_total, int H, int hd, float scale, void* out,
                        float* lse, hipStream_t s, const DropArgs* dr) {
    attn_x3_dispatch(hd, mode, [&](auto form) {
        typedef decltype(form) F;
        typedef typename F::io_t T;
        attn_x3_by_waves(attn_plan_waves(ATTN_K_FWD, mode, hd, dr != nullptr), [&](auto nw) {
            constexpr int NW = decltype(nw)::value;
            const AttnGrid g = attn_x3_grid(H, B, max_len, NW);
            if (dr) hipLaunchKernelGGL((attn_fwd_x3_k<F::HD, F::NP, F::IO16, NW, DropArgs>), g.grid, dim3(64 * NW), 0, s, (const T*)qkv, cu, H, scale, (T*)out, lse, n_total, B, g.n_tiles, *dr);
            else hipLaunchKernelGGL((attn_fwd_x3_k<F::HD, F::NP, F::IO16, NW>), g.grid, dim3(64 * NW), 0, s, (const T*)qkv, cu, H, scale, (T*)out, lse, n_total, B, g.n_tiles);
        });
    });
}

// dQ and dK / dV are independent given delta: with U3D_ATTN_FORK=1 the dQ kernel is forked onto a per-device side stream and joined
// before the call hands `s` back (events only; nothing blocks the host).  Each of the two grids leaves the last of its ~2.8 waves of
// workgroups a quarter full; side by side they fill each other's tail: attention backward 4.88 / 4.95 -> 4.75 / 4.76 ms per step
// alone -- and the training step got SLOWER (302.3 / 301.2 -> 297.8 / 296.8 scenes/s, same box, round 5): the fork competes with the
// weight-gradient chain that already runs beside the decoder's backward (sparse.set_wgrad_overlap(2)).  OFF by default.
struct AttnFork {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
static AttnFork* attn_fork_of_device() {
    static AttnFork forks[64];
    static std::mutex mu;
    static const bool on = [] { const char* e = getenv("U3D_ATTN_FORK"); return e && atoi(e) != 0; }();
    if (!on) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if ((unsigned)dev >= 64u) return nullptr;        // as DeviceOnce: an ordinal past the table gets no fork instead of another device's
    AttnFork& f = forks[dev];
    std::lock_guard<std::mutex> lk(mu);
    if (!f.side) {
        if (hipStreamCreateWithFlags(&f.side, hipStreamNonBlocking) != hipSuccess) { f.side = nullptr; return nullptr; }
        hipEventCreateWithFlags(&f.fork, hipEventDisableTiming);
        hipEventCreateWithFlags(&f.join, hipEventDisableTiming);
    }
    return &f;
}

void attn_bwd_x3_launch(AttnMode mode, const void* qkv, const void* dout, const float* lse, const int32_t* cu, int B, int max_len,
                        int64_t n_total, int H, int hd, float scale, void* dqkv, const float* delta, hipStream_t s, const DropArgs* dr) {
    AttnFork* f = attn_fork_of_device();
    hipStream_t sq = s;
    if (f) {
        hipEventRecord(f->fork, s);
        hipStreamWaitEvent(f->side, f->fork, 0);
        sq = f->side;
    }
    attn_x3_dispatch(hd, mode, [&](auto form) {
        typedef decltype(form) F;
        typedef typename F::io_t T;
        attn_x3_by_waves(attn_plan_waves(ATTN_K_DQ, mode, hd, dr != nullptr), [&](auto nw) {
            constexpr int NW = decltype(nw)::value;
            const AttnGrid g = attn_x3_grid(H, B, max_len, NW);
            if (dr) hipLaunchKernelGGL((attn_bwd_dq_x3_k<F::HD, F::NP, F::IO16, NW, DropArgs>), g.grid, dim3(64 * NW), 0, sq, (const T*)qkv, (const T*)dout, lse, delta, cu, H, scale, (T*)dqkv, n_total, B, g.n_tiles, *dr);
            else hipLaunchKernelGGL((attn_bwd_dq_x3_k<F::HD, F::NP, F::IO16, NW>), g.grid, dim3(64 * NW), 0, sq, (const T*)qkv, (const T*)dout, lse, delta, cu, H, scale, (T*)dqkv, n_total, B, g.n_tiles);
        });
        attn_x3_by_waves(attn_plan_waves(ATTN_K_DKV, mode, hd, dr != nullptr), [&](auto nw) {
            constexpr int NW = decltype(nw)::value;
            const AttnGrid g = attn_x3_grid(H, B, max_len, NW);
            if (dr) hipLaunchKernelGGL((attn_bwd_dkv_x3_k<F::HD, F::NP, F::IO16, NW, DropArgs>), g.grid, dim3(64 * NW), 0, s, (const T*)qkv, (const T*)dout, lse, delta, cu, H, scale, (T*)dqkv, n_total, B, g.n_tiles, *dr);
            else hipLaunchKernelGGL((attn_bwd_dkv_x3_k<F::HD, F::NP, F::IO16, NW>), g.grid, dim3(64 * NW), 0, s, (const T*)qkv, (const T*)dout, lse, delta, cu, H, scale, (T*)dqkv, n_total, B, g.n_tiles);
        });
    });
    if (f) {
        hipEventRecord(f->join, f->side);
        hipStreamWaitEvent(s, f->join, 0);
    }
}

}  // namespace u3d

using namespace u3d;

extern "C" {

// bf16-operand form (BASELINE configs[2]; the reference's `--amp` run through nn.MultiheadAttention, tools/train.py:86-99): the
// same kernels with ONE plane per operand, rounded to nearest even where the three-plane form splits; qkv / out / gradients stay
// fp32 in HBM, accumulation and softmax stay fp32.
int u3d_attn_varlen_fwd_bf16(const float* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                             float scale, float* out, float* lse, double flops_hint, u3d_stream_t stream) {
    return attn_fwd(ATTN_BF16_OPS, qkv, cu_seqlens, B, max_len, n_total, H, hd, scale, out, lse, flops_hint, stream);
}

int u3d_attn_varlen_bwd_bf16(const float* qkv, const float* out, const float* dout, const float* lse, const int32_t* cu_seqlens,
                             int B, int max_len, int64_t n_total, int H, int hd, float scale, float* dqkv, float* delta_ws,
                             double flops_hint, u3d_stream_t stream) {
    return attn_bwd(ATTN_BF16_OPS, qkv, out, dout, lse, cu_seqlens, B, max_len, n_total, H, hd, scale, dqkv, delta_ws, flops_hint, stream);
}

// bf16 TENSORS (include/u3d.h K14b): qkv / out / dout / dqkv are bf16 in HBM -- what the reference's autocast hands to and takes from
// nn.MultiheadAttention (tools/train.py:86-99, unidet3d/encoder.py:19-21); lse / delta, softmax and all accumulators fp32.
int u3d_attn_varlen_fwd_b16(const void* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                            float scale, void* out, float* lse, double flops_hint, u3d_stream_t stream) {
    return attn_fwd(ATTN_B16, qkv, cu_seqlens, B, max_len, n_total, H, hd, scale, out, lse, flops_hint, stream);
}

int u3d_attn_varlen_bwd_b16(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* cu_seqlens,
                            int B, int max_len, int64_t n_total, int H, int hd, float scale, void* dqkv, float* delta_ws,
                            double flops_hint, u3d_stream_t stream) {
    return attn_bwd(ATTN_B16, qkv, out, dout, lse, cu_seqlens, B, max_len, n_total, H, hd, scale, dqkv, delta_ws, flops_hint, stream);
}

// dropout forms of the four entry points above (include/u3d.h "dropout"): the same arguments plus (p, seed, offset)
int u3d_attn_varlen_fwd_drop_bf16(const float* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                                  float scale, float* out, float* lse, double flops_hint, u3d_stream_t stream, double p, uint64_t seed, uint64_t offset) {
    return attn_fwd_drop(ATTN_BF16_OPS, qkv, cu_seqlens, B, max_len, n_total, H, hd, scale, out, lse, flops_hint, stream, p, seed, offset);
}

int u3d_attn_varlen_bwd_drop_bf16(const float* qkv, const float* out, const float* dout, const float* lse, const int32_t* cu_seqlens,
                                  int B, int max_len, int64_t n_total, int H, int hd, float scale, float* dqkv, float* delta_ws,
                                  double flops_hint, u3d_stream_t stream, double p, uint64_t seed, uint64_t offset) {
    return attn_bwd_drop(ATTN_BF16_OPS, qkv, out, dout, lse, cu_seqlens, B, max_len, n_total, H, hd, scale, dqkv, delta_ws, flops_hint, stream, p, seed, offset);
}

int u3d_attn_varlen_fwd_drop_b16(const void* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                                 float scale, void* out, float* lse, double flops_hint, u3d_stream_t stream, double p, uint64_t seed, uint64_t offset) {
    return attn_fwd_drop(ATTN_B16, qkv, cu_seqlens, B, max_len, n_total, H, hd, scale, out, lse, flops_hint, stream, p, seed, offset);
}

int u3d_attn_varlen_bwd_drop_b16(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* cu_seqlens,
                                 int B, int max_len, int64_t n_total, int H, int hd, float scale, void* dqkv, float* delta_ws,
                                 double flops_hint, u3d_stream_t stream, double p, uint64_t seed, uint64_t offset) {
    return attn_bwd_drop(ATTN_B16, qkv, out, dout, lse, cu_seqlens, B, max_len, n_total, H, hd, scale, dqkv, delta_ws, flops_hint, stream, p, seed, offset);
}

}  // extern "C"
