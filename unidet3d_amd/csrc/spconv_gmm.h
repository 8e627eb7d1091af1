// Shared between the two output-stationary sparse-convolution kernels (spconv.hip: wave-private tiles, spconv_wg.hip:
// workgroup tiles with the weights of an offset shared through LDS).  Internal, not part of the C ABI.
#pragma once
#include "u3d_common.h"

namespace u3d {

// Output epilogue of the forward launches (u3d_spconv_gmm_ep, fused inference): where the rows of dst go as they leave the LDS
// accumulator tile (or gmm_reduce_ep_k's registers when the offsets are split over groups).  x = the fp32 value the plain launch stores.
//   raw (nullable): x itself, into columns [raw_col, raw_col + Cd) of a buffer with leading dimension raw_ld;
//   act[j], j < n_act <= 2: x * scale[j][c] + shift[j][c] (+ ReLU), c = the column of act[j] the value lands in (act_col[j] + dst column):
//   a norm over a wider tensor (the U-Net's concat) is applied to its column blocks by the convolutions that produce them.
// All leading dimensions and column offsets are multiples of 4 floats: every store is a 16-byte vector store.
// relu[j] is the flag word of the C ABI: U3D_EP_RELU (1) = ReLU follows, U3D_EP_BF16_ROWS (2) = act[j] is a bf16-row buffer -- the shadow
// u3d_bn_apply writes (u3d_common.h store_shadow: same rounding, same fragment order), act_ld / act_col then count bf16 elements in
// multiples of 32: one 8-byte store per 16-byte fp32 piece.  (The two halves c4 / c4 + 4 of a 16-byte shadow quad sit on lanes l and
// l + 4 of the write-out loops: pairing them would cost a cross-lane move per piece, so they stay two stores.)
struct GmmEpilogue {
    float* raw;
    float* act[2];
    const float* scale[2];
    const float* shift[2];
    int raw_ld, raw_col;
    int act_ld[2], act_col[2], relu[2];
    int n_act;
};

// one 16-byte piece of dst (row, dst columns col .. col + 3) through the epilogue
__device__ __forceinline__ void gmm_write_out(const GmmEpilogue& ep, int64_t row, int col, const float4& v) {
    if (ep.raw) *reinterpret_cast<float4*>(ep.raw + row * ep.raw_ld + ep.raw_col + col) = v;
#pragma unroll
    for (int j = 0; j < 2; ++j) {        // constant indices into the kernel argument: no private copy of the struct
        if (j < ep.n_act) {
            const int c = ep.act_col[j] + col;
            const float4 sc = *reinterpret_cast<const float4*>(ep.scale[j] + c), sf = *reinterpret_cast<const float4*>(ep.shift[j] + c);
            const float4 o = bn_affine_relu(v, sc, sf, ep.relu[j] & U3D_EP_RELU);
            if (ep.relu[j] & U3D_EP_BF16_ROWS) store_shadow(reinterpret_cast<__bf16*>(ep.act[j]), row, ep.act_ld[j] >> 2, ep.act_col[j] >> 2, col >> 2, o);
            else *reinterpret_cast<float4*>(ep.act[j] + row * ep.act_ld[j] + c) = o;
        }
    }
}

struct GmmParams {
    const float* src;
    const float* w;
    const int32_t* gather;
    const int32_t* scatter;
    const int32_t* ts;
    const float* addend;
    float* out;          // dst, or the partial buffer [G][n_dst][Cd] when G > 1
    float* stats;        // nullable (G == 1 only): per-tile column sums of dst for the batch norm behind this convolution,
                         // float [n_sub][2][Cd] = sum x | sum x^2 over the tile's rows
    int K;
    int64_t cap;
    int Cs, Cd;
    int64_t n_dst;
    int64_t n_src;
    int64_t n_sub;
    int n_slices;
    int G;
    int kper;
};

// Argument of the EP = true instantiations of the two kernels (fused inference; G == 1 and stats == nullptr: with offset groups the
// plain kernels write partials as always and the epilogue runs in gmm_reduce_ep_k).  The epilogue is a TEMPLATE parameter, not a
// branch: one kernel with a wave-uniform `if (ep.on)` in front of its write-out measured 0.1 - 0.2 ms per training step behind the
// parent on bench.py (25.54 / 25.56 -> 25.65 / 25.63 ms and 25.65 / 25.77 -> 25.85 / 25.86 ms, two sessions: outside the parent's
// spread) -- the descriptor's 22 dwords are loaded ahead of the main loop and held in SGPRs through it, and the register allocation
// of the whole kernel moves.  The EP = false kernels are the parent's, instruction for instruction.
struct GmmParamsEp : GmmParams {
    GmmEpilogue ep;
};
template <bool EP> struct GmmArg { using type = GmmParams; };
template <> struct GmmArg<true> { using type = GmmParamsEp; };

constexpr int GMM_CDS = 32;            // output columns per wave
// Accumulator tile of a wave in LDS: R rows x 32 floats.  Default layout (round 3): 128-byte rows, the eight 16-byte quads of
// row r stored at quad ^ (r & 7) -- the XOR spreads the random-row 16-byte accesses of the MFMA read-modify-write over the
// banks like the padded 160-byte rows of rounds 1-2 did, without their 25 % padding, and the scratch row for lanes past the
// end of a range aliases the head of the staging image (dead at that point of a unit) instead of being a 65th row:
// 10 KB per wave instead of 12.4 -> FOUR workgroups (16 waves) per CU instead of three for the 64-row kernels.
// -DU3D_GMM_ALD40 builds the old layout (A/B measurements).
#ifdef U3D_GMM_ALD40
constexpr bool GMM_SWZ = false;
constexpr int GMM_ALD = 40;
#else
constexpr bool GMM_SWZ = true;
constexpr int GMM_ALD = 32;
#endif

// workgroup-tile kernel (spconv_wg.hip): pr = 1 bf16 operands, 2 three bf16 planes, 3 bf16 source rows (p.src points at bf16 [n_src][Cs]); p.n_sub counts R-row tiles
int launch_gmm_wg(const GmmParams& p, int cs16, int R, int pr, hipStream_t s, const GmmEpilogue* ep = nullptr);      // ep: the EP = true kernels
bool gmm_wg_supported(int cs16, int R, int pr);

// channel-blocked weight gradient (spconv_wgrad_blk.hip): every (Cs, Cd) pair of the C ABI contract that spconv_wgrad_k (spconv.hip) has
// no instantiation for.  Same pair lists, tile_starts and workspace size as that kernel; partial = [K][n_tiles][Cd][Cs] floats.
struct WgBlkParams {
    const float* x;
    const float* dy;
    const int32_t* rows_x;
    const int32_t* rows_dy;
    const int32_t* ts;        // tile_starts [K][n_tiles+1] over the dy-side rows
    float* partial;
    int K;
    int64_t cap;
    int n_tiles;
    int Cs, Cd;
    int64_t n_rows_x, n_rows_dy;
};
bool wgrad_blk_supported(int Cs, int Cd);       // Cs in {16} u {32, 64, ..., 512}, Cd in {32, 64, ..., 512}
int launch_wgrad_blk(const WgBlkParams& p, bool bf16, float* dW, hipStream_t s);

}  // namespace u3d
